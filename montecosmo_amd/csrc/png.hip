// Local primordial non-Gaussianity of the initial field (montecosmo/bricks.py:108-141, add_png) and its VJP:
//   u = safe_div(lin, t(|k|)),  phi = irfftn(u),  psi = phi + fNL (phi^2 - <phi^2>),  out = t(|k|) rfftn(psi)
// t = the phi -> delta transfer function, linearly interpolated from a 256-point DEVICE float64 table inside the k-space kernels
// (interp_zero of tables_dev.h at the |k| of kmode_dev.h's decoder: no mesh-sized table exists anywhere).  <phi^2> and the two sums of the adjoint
// are grid reductions in float64 with the fixed-order fold of reduce_dev.h; the cotangent of the table entries is scattered to the
// two bracketing nodes with the interpolation weights and summed as integers (the scheme of lightcone_tables_vjp_kernel,
// observe.hip), so every output is bitwise the same call after call.
#include "mcpm_internal.h"
#include "reduce_dev.h"
#include "tables_dev.h"
#include "kmode_dev.h"

namespace {

// ---- forward ---------------------------------------------------------------------------------------------------------------
// out = scale * safe_div(in, t)      (scale = 1 / M: the C2R behind it is unnormalised);  lap: times -|k|^2 (the Laplacian of phi)
__global__ __launch_bounds__(256) void png_div_kernel(KGeom kg, Table tt, float scale, int lap,
                                                      const float2 *__restrict__ in, float2 *__restrict__ out, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    const float t = (float)interp_zero(m.kn, tt).t;
    if (lap) scale *= -(float)(m.kn * m.kn);
    const float2 v = in[idx];
    out[idx] = t == 0.f ? make_float2(0.f, 0.f) : make_float2(scale * (v.x / t), scale * (v.y / t));
}

// in place: io *= t
__global__ __launch_bounds__(256) void png_mult_kernel(KGeom kg, Table tt, float2 *__restrict__ io, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    const float t = (float)interp_zero(m.kn, tt).t;
    const float2 v = io[idx];
    io[idx] = make_float2(t * v.x, t * v.y);
}

// per-workgroup partials of sum phi^2
__global__ __launch_bounds__(256) void png_moment_kernel(const float *__restrict__ phi, int64_t M, double *__restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[1] = {0.};
    if (i < M) {
        const double x = (double)phi[i];
        v[0] = x * x;
    }
    block_partial<1>(v, part, gridDim.x, blockIdx.x);
}

// psi = phi + fNL (phi^2 - <phi^2>)
__global__ __launch_bounds__(256) void png_quad_kernel(const float *__restrict__ phi, float fnl, const double *__restrict__ mean, int64_t M,
                                                       float *__restrict__ psi) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float x = phi[i], m = (float)*mean;
    psi[i] = x + fnl * (x * x - m);
}

// ---- adjoint ---------------------------------------------------------------------------------------------------------------
// cotangent of Psi = rfftn(psi) from the cotangent of out, ready for the unnormalised C2R that is the adjoint of rfftn under the
// real-pair convention: the doubly counted modes are halved first (the C2R applies irfftn's multiplicity weights)
__global__ __launch_bounds__(256) void png_vjp_in_kernel(KGeom kg, Table tt, const float2 *__restrict__ ob,
                                                         float2 *__restrict__ out, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    const float t = (float)interp_zero(m.kn, tt).t * (m.zw == 2.f ? 0.5f : 1.f);
    const float2 v = ob[idx];
    out[idx] = make_float2(t * v.x, t * v.y);
}

// per-workgroup partials of S0 = sum psi_bar and S1 = sum psi_bar phi^2
__global__ __launch_bounds__(256) void png_vjp_sums_kernel(const float *__restrict__ phi, const float *__restrict__ psib, int64_t M,
                                                           double *__restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[2] = {0., 0.};
    if (i < M) {
        const double x = (double)phi[i], b = (double)psib[i];
        v[0] = b;
        v[1] = b * x * x;
    }
    block_partial<2>(v, part, gridDim.x, blockIdx.x);
}

// in place: psi_bar -> phi_bar = psi_bar (1 + 2 fNL phi) - 2 fNL phi <psi_bar>   (the second term is the adjoint of the mean: every
// cell feeds <phi^2>, whose cotangent is -fNL S0);  fNL_bar = S1 - <phi^2> S0
__global__ __launch_bounds__(256) void png_quad_vjp_kernel(const float *__restrict__ phi, float fnl, const double *__restrict__ mean,
                                                           const double *__restrict__ sums, int64_t M, const float *__restrict__ add,
                                                           float *__restrict__ io, double *__restrict__ fnl_bar) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *fnl_bar = sums[1] - *mean * sums[0];
    if (i >= M) return;
    const float x = phi[i], mb = (float)(sums[0] / (double)M);
    io[i] = io[i] * (1.f + 2.f * fnl * x) - 2.f * fnl * x * mb + (add ? add[i] : 0.f);      // add: phi's cotangent from its other readers
}

// u_bar = zw / M * (R2C(phi_bar) - k^2 R2C(lap_phi_bar))  ->  lin_bar = safe_div(u_bar, t), and the per-mode cotangent of t from both of its uses:
//   multiply  out = t Psi:  Re(conj(out_bar) Psi),  Psi = out / t;      divide  u = lin / t:  -Re(conj(u_bar) lin) / t^2
__global__ __launch_bounds__(256) void png_vjp_out_kernel(KGeom kg, Table tt, float scale, const float2 *__restrict__ lin,
                                                          const float2 *__restrict__ out, const float2 *__restrict__ ob,
                                                          const float2 *__restrict__ spec, const float2 *__restrict__ spec2,
                                                          float2 *__restrict__ lin_bar, double *__restrict__ tbar, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    const float t = (float)interp_zero(m.kn, tt).t;
    float2 s = spec[idx];
    if (spec2) {      // u also feeds lap phi = irfftn(-k^2 u): both cotangents meet here, before the single divide by t
        const float k2 = (float)(m.kn * m.kn);
        const float2 s2 = spec2[idx];
        s.x -= k2 * s2.x, s.y -= k2 * s2.y;
    }
    const float ux = scale * m.zw * s.x, uy = scale * m.zw * s.y;
    if (t == 0.f) {
        lin_bar[idx] = make_float2(0.f, 0.f);
        tbar[idx] = 0.;
        return;
    }
    lin_bar[idx] = make_float2(ux / t, uy / t);
    const float2 l = lin[idx];
    const double td = (double)t;
    double tb = -((double)ux * l.x + (double)uy * l.y) / (td * td);
    if (ob) {      // (no cotangent of out: only the divide uses t)
        const float2 o = out[idx], b = ob[idx];
        tb += ((double)b.x * o.x + (double)b.y * o.y) / td;
    }
    tbar[idx] = tb;
}

// table cotangent: tbar[k] goes to the nodes (lo, lo + 1) of its bracket with the weights (1 - w, w), summed as integers so that the result
// does not depend on the order (tables_dev.h, ORDER-INDEPENDENT SUMS; one kind).  A non-finite contribution makes the whole table NaN.
template <int PASS>
__global__ __launch_bounds__(256) void png_table_vjp_kernel(KGeom kg, Table tt, const double *__restrict__ tbar, int64_t Mh,
                                                            unsigned *__restrict__ mxbits, unsigned long long *__restrict__ acc) {
    extern __shared__ unsigned long long png_sh[];
    Acc<1> A;
    acc_begin(A, png_sh, tt.n, mxbits, PASS);
    bool bad = false;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < Mh; idx += (int64_t)gridDim.x * 256) {
        const KMode m = kdecode(kg, (uint32_t)idx);
        const TNode b = interp_zero(m.kn, tt);
        if (b.lo < 0) continue;
        const double v = tbar[idx];
        bad = bad || !(v == v);
        acc_add<PASS>(A, 0, 0, b.lo, v * (1. - b.w));
        acc_add<PASS>(A, 0, 0, b.lo + 1, v * b.w);
    }
    acc_end<PASS>(A, tt.n, mxbits, acc, bad);
}

// ---- PNG terms of the Lagrangian bias weights (montecosmo/bricks.py:413-441) -----------------------------------------------------
// per particle: g growth, d = dr g, D2 = d^2 - <d^2>, S2 = s2r g^2 - 2/3 <d^2> (the renormalised quantities of bias_weights_kernel),
// ph = phi, lp = lap phi;   w += bp ph + bpd (ph d - <ph d>) + bpd2 (ph D2 - 2 <ph d> d) + bps2 ph S2 + bn2p lp
struct Png5 {
    float bp, bpd, bpd2, bps2, bn2p;
};

// per-workgroup partials of sum d^2 (the sum of bias_moment_kernel, same order: the same <d^2> to the bit) and sum ph d
__global__ __launch_bounds__(256) void png_w_moment_kernel(const float *__restrict__ dr, const float *__restrict__ ph, const float *__restrict__ gp,
                                                           float gs, int64_t n, double *part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[2] = {0., 0.};
    if (i < n) {
        const float d = dr[i] * (gp ? gp[i] : gs);
        v[0] = (double)d * (double)d;
        v[1] = (double)ph[i] * (double)d;
    }
    block_partial<2>(v, part, gridDim.x, blockIdx.x);
}

struct PngTerms {
    float d, D2, S2, t[5];
};
__device__ __forceinline__ PngTerms png_terms(float draw, float s2raw, float ph, float lp, float g, float sig, float spd) {
    PngTerms r;
    r.d = draw * g;
    r.D2 = r.d * r.d - sig;
    r.S2 = s2raw * g * g - (2.f / 3.f) * sig;
    r.t[0] = ph;
    r.t[1] = ph * r.d - spd;
    r.t[2] = ph * r.D2 - 2.f * spd * r.d;
    r.t[3] = ph * r.S2;
    r.t[4] = lp;
    return r;
}

__global__ __launch_bounds__(256) void png_weights_kernel(const float *__restrict__ dr, const float *__restrict__ s2r, const float *__restrict__ ph,
                                                          const float *__restrict__ lp, const float *__restrict__ gp, float gs, Png5 B,
                                                          const double *__restrict__ mom, int64_t n, float *__restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PngTerms T = png_terms(dr[i], s2r[i], ph[i], lp[i], gp ? gp[i] : gs, (float)mom[0], (float)mom[1]);
    w[i] += B.bp * T.t[0] + B.bpd * T.t[1] + B.bpd2 * T.t[2] + B.bps2 * T.t[3] + B.bn2p * T.t[4];
}

// pass 1 of the VJP: the five coefficient cotangents, <ph d>_bar and <d^2>_bar (rows 0..6 of per-workgroup partials)
__global__ __launch_bounds__(256) void png_w_vjp_reduce_kernel(const float *__restrict__ dr, const float *__restrict__ s2r,
                                                               const float *__restrict__ ph, const float *__restrict__ lp,
                                                               const float *__restrict__ gp, float gs, Png5 B, const double *__restrict__ mom,
                                                               const float *__restrict__ wb, int64_t n, double *part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[7] = {0., 0., 0., 0., 0., 0., 0.};
    if (i < n) {
        const float x = ph[i], w = wb[i];
        const PngTerms T = png_terms(dr[i], s2r[i], x, lp[i], gp ? gp[i] : gs, (float)mom[0], (float)mom[1]);
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = (double)w * (double)T.t[k];
        v[5] = (double)(w * (-B.bpd - 2.f * B.bpd2 * T.d));                       // <ph d> enters terms 1 and 2
        v[6] = (double)(w * x * (-B.bpd2 - (2.f / 3.f) * B.bps2));                // <d^2> enters D2 and S2
    }
    block_partial<7>(v, part, gridDim.x, blockIdx.x);
}

// pass 2: per-particle cotangents.  The two means couple all particles: each one receives mean_bar / n times its own factor.
// drb, s2rb, gbar (may be NULL) are ADDED to (they hold the Gaussian terms' cotangents); phb, lpb are written.
__global__ __launch_bounds__(256) void png_w_vjp_particles_kernel(const float *__restrict__ dr, const float *__restrict__ s2r,
                                                                  const float *__restrict__ ph, const float *__restrict__ lp,
                                                                  const float *__restrict__ gp, float gs, Png5 B, const double *__restrict__ mom,
                                                                  const double *__restrict__ mbar, const float *__restrict__ wb, int64_t n,
                                                                  float *__restrict__ drb, float *__restrict__ s2rb, float *__restrict__ phb,
                                                                  float *__restrict__ lpb, float *__restrict__ gbar, double *part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[1] = {0.};
    if (i < n) {
        const float g = gp ? gp[i] : gs, x = ph[i], w = wb[i], draw = dr[i], s2raw = s2r[i];
        const float spd = (float)mom[1], spdb = (float)(mbar[0] / (double)n), sigb = (float)(mbar[1] / (double)n);
        const PngTerms T = png_terms(draw, s2raw, x, lp[i], g, (float)mom[0], spd);
        phb[i] = w * (B.bp + B.bpd * T.d + B.bpd2 * T.D2 + B.bps2 * T.S2) + spdb * T.d;
        lpb[i] = w * B.bn2p;
        const float dbar = w * (B.bpd * x + 2.f * B.bpd2 * (x * T.d - spd)) + spdb * x + sigb * 2.f * T.d;
        const float s2b = w * B.bps2 * x;
        drb[i] += dbar * g;
        s2rb[i] += s2b * g * g;
        const float gb = dbar * draw + s2b * 2.f * g * s2raw;
        if (gbar) gbar[i] += gb;
        v[0] = (double)gb;
    }
    block_partial<1>(v, part, gridDim.x, blockIdx.x);
}

}  // namespace

extern "C" {

// phi = irfftn(safe_div(lin, t)) and lap_phi = irfftn(-k^2 safe_div(lin, t)) (bricks.py:415, :439): two transforms
int mcpm_png_phi_f32(mcpm_plan *p, const float *lin_mesh, float kpx, float kpy, float kpz, const double *ks, const double *trans, int ntab,
                     float *phi, float *lap_phi) {
    if (!p) return MCPM_E_ARG;
    KGeom kg;
    Table tt;
    MCPM_REQUIRE(p, lin_mesh && phi && lap_phi, MCPM_E_ARG, "mcpm_png_phi_f32: bad argument");
    MCPM_TRY(table_arg(p, "mcpm_png_phi_f32", ks, trans, ntab, &tt));
    MCPM_TRY(kgeom_arg(p, "mcpm_png_phi_f32", kpx, kpy, kpz, &kg));
    const int64_t Mh = p->Mh;
    const unsigned nbk = (unsigned)((Mh + 255) / 256);
    for (int lap = 0; lap < 2; ++lap) {
        {
            StageTimer st_(p, ST_KSPACE, 16.0 * Mh);
            png_div_kernel<<<nbk, 256, 0, p->stream>>>(kg, tt, 1.f / (float)p->M, lap, (const float2 *)lin_mesh,
                                                       (float2 *)p->spec1, Mh);
            MCPM_LAUNCH_CHECK(p, "png_div_kernel");
        }
        MCPM_TRY(mcpm_fft_c2r(p, p->spec1, lap ? lap_phi : phi, 1));
    }
    return MCPM_OK;
}

// out = scale * safe_div(in, t(|k|)) on the half-spectrum (the PNG term of the Kaiser boost, bricks.py:181-183; real, self-adjoint)
int mcpm_png_div_f32(mcpm_plan *p, const float *in, float kpx, float kpy, float kpz, const double *ks, const double *trans, int ntab, float scale,
                     float *out) {
    if (!p) return MCPM_E_ARG;
    KGeom kg;
    Table tt;
    MCPM_REQUIRE(p, in && out, MCPM_E_ARG, "mcpm_png_div_f32: bad argument");
    MCPM_TRY(table_arg(p, "mcpm_png_div_f32", ks, trans, ntab, &tt));
    MCPM_TRY(kgeom_arg(p, "mcpm_png_div_f32", kpx, kpy, kpz, &kg));
    StageTimer st_(p, ST_KSPACE, 16.0 * p->Mh);
    png_div_kernel<<<(unsigned)((p->Mh + 255) / 256), 256, 0, p->stream>>>(kg, tt, scale, 0, (const float2 *)in,
                                                                          (float2 *)out, p->Mh);
    MCPM_LAUNCH_CHECK(p, "png_div_kernel");
    return MCPM_OK;
}

// weights += the five PNG terms.  dr, s2r: raw reads of delta and s^2 (as mcpm_bias_weights_f32 takes them); ph, lp: reads of phi and
// lap phi; png5 = {fNL_bp, fNL_bpd, fNL_bpd2, fNL_bps2, fNL_bn2p} (host).  moments_out (device, 2 doubles, may be NULL): <d^2>, <ph d>.
int mcpm_png_weights_f32(mcpm_plan *p, int64_t n, const float *dr, const float *s2r, const float *ph, const float *lp, const float *growth,
                         float growth_scalar, const float *png5, float *weights, double *moments_out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n > 0 && dr && s2r && ph && lp && png5 && weights, MCPM_E_ARG, "mcpm_png_weights_f32: bad argument");
    const Png5 B{png5[0], png5[1], png5[2], png5[3], png5[4]};
    double *mom = p->reduce + MCPM_RED_SCALARS;
    DetSum s;
    const unsigned nb = (unsigned)((n + 255) / 256);
    StageTimer st_(p, ST_LPT, 40.0 * n);
    MCPM_TRY(mcpm_det_begin(p, 2, nb, &s));
    png_w_moment_kernel<<<nb, 256, 0, p->stream>>>(dr, ph, growth, growth_scalar, n, s.P);
    MCPM_LAUNCH_CHECK(p, "png_w_moment_kernel");
    MCPM_TRY(mcpm_det_fold(p, s, 2, 1.0 / (double)n, det_outs_row(DET_STORE, mom, 2)));
    png_weights_kernel<<<nb, 256, 0, p->stream>>>(dr, s2r, ph, lp, growth, growth_scalar, B, mom, n, weights);
    MCPM_LAUNCH_CHECK(p, "png_weights_kernel");
    if (moments_out) MCPM_HIP(p, hipMemcpyAsync(moments_out, mom, 2 * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    return MCPM_OK;
}

// VJP: weights_bar -> drb, s2rb, growth_bar (ADDED to; growth_bar may be NULL), phb, lpb (written), and scalars_out (device, 10 doubles):
// [0..4] cotangents of png5, [5] <ph d>_bar, [6] <d^2>_bar, [7] the summed growth cotangent, [8] <d^2>, [9] <ph d>.
int mcpm_png_weights_vjp_f32(mcpm_plan *p, int64_t n, const float *dr, const float *s2r, const float *ph, const float *lp, const float *growth,
                             float growth_scalar, const float *png5, const float *weights_bar, float *drb, float *s2rb, float *phb, float *lpb,
                             float *growth_bar, double *scalars_out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n > 0 && dr && s2r && ph && lp && png5 && weights_bar && drb && s2rb && phb && lpb && scalars_out, MCPM_E_ARG,
                 "mcpm_png_weights_vjp_f32: bad argument");
    const Png5 B{png5[0], png5[1], png5[2], png5[3], png5[4]};
    double *mom = scalars_out + 8;
    DetSum s;
    const unsigned nb = (unsigned)((n + 255) / 256);
    StageTimer st_(p, ST_LPT, 80.0 * n);
    MCPM_TRY(mcpm_det_begin(p, 7, nb, &s));
    png_w_moment_kernel<<<nb, 256, 0, p->stream>>>(dr, ph, growth, growth_scalar, n, s.P);
    MCPM_LAUNCH_CHECK(p, "png_w_moment_kernel");
    MCPM_TRY(mcpm_det_fold(p, s, 2, 1.0 / (double)n, det_outs_row(DET_STORE, mom, 2)));
    png_w_vjp_reduce_kernel<<<nb, 256, 0, p->stream>>>(dr, s2r, ph, lp, growth, growth_scalar, B, mom, weights_bar, n, s.P);
    MCPM_LAUNCH_CHECK(p, "png_w_vjp_reduce_kernel");
    MCPM_TRY(mcpm_det_fold(p, s, 7, 1.0, det_outs_row(DET_STORE, scalars_out, 7)));
    png_w_vjp_particles_kernel<<<nb, 256, 0, p->stream>>>(dr, s2r, ph, lp, growth, growth_scalar, B, mom, scalars_out + 5, weights_bar, n, drb, s2rb,
                                                          phb, lpb, growth_bar, s.P);
    MCPM_LAUNCH_CHECK(p, "png_w_vjp_particles_kernel");
    return mcpm_det_fold(p, s, 1, 1.0, det_outs_ptrs(DET_STORE, scalars_out + 7));
}

int mcpm_png_add_f32(mcpm_plan *p, const float *lin_mesh, float kpx, float kpy, float kpz, const double *ks, const double *trans, int ntab,
                     float fnl, int phi_given, float *phi, float *out, double *mean_out) {
    if (!p) return MCPM_E_ARG;
    KGeom kg;
    Table tt;
    MCPM_REQUIRE(p, lin_mesh && phi && out, MCPM_E_ARG, "mcpm_png_add_f32: bad argument");
    MCPM_TRY(table_arg(p, "mcpm_png_add_f32", ks, trans, ntab, &tt));
    MCPM_TRY(kgeom_arg(p, "mcpm_png_add_f32", kpx, kpy, kpz, &kg));
    const int64_t M = p->M, Mh = p->Mh;
    const unsigned nbk = (unsigned)((Mh + 255) / 256), nbr = (unsigned)((M + 255) / 256);
    if (!phi_given) {
        {
            StageTimer st_(p, ST_KSPACE, 16.0 * Mh);
            png_div_kernel<<<nbk, 256, 0, p->stream>>>(kg, tt, 1.f / (float)M, 0, (const float2 *)lin_mesh,
                                                       (float2 *)p->spec1, Mh);
            MCPM_LAUNCH_CHECK(p, "png_div_kernel");
        }
        MCPM_TRY(mcpm_fft_c2r(p, p->spec1, phi, 1));
    }
    double *mean = p->reduce + MCPM_RED_SCALARS;
    DetSum s;
    MCPM_TRY(mcpm_det_begin(p, 1, nbr, &s));
    {
        StageTimer st_(p, ST_LPT, 12.0 * M);
        png_moment_kernel<<<nbr, 256, 0, p->stream>>>(phi, M, s.P);
        MCPM_LAUNCH_CHECK(p, "png_moment_kernel");
        MCPM_TRY(mcpm_det_fold(p, s, 1, 1.0 / (double)M, det_outs_ptrs(DET_STORE, mean)));
        png_quad_kernel<<<nbr, 256, 0, p->stream>>>(phi, fnl, mean, M, p->rho);
        MCPM_LAUNCH_CHECK(p, "png_quad_kernel");
    }
    if (mean_out) MCPM_HIP(p, hipMemcpyAsync(mean_out, mean, sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    MCPM_TRY(mcpm_fft_r2c(p, p->rho, out, 1));
    StageTimer st_(p, ST_KSPACE, 16.0 * Mh);
    png_mult_kernel<<<nbk, 256, 0, p->stream>>>(kg, tt, (float2 *)out, Mh);
    MCPM_LAUNCH_CHECK(p, "png_mult_kernel");
    return MCPM_OK;
}

int mcpm_png_add_vjp_f32(mcpm_plan *p, const float *lin_mesh, const float *out, const float *phi, const double *mean, float kpx, float kpy,
                         float kpz, const double *ks, const double *trans, int ntab, float fnl, const float *out_bar, const float *phi_bar,
                         const float *lap_phi_bar, float *lin_mesh_bar, double *fnl_bar, double *trans_bar) {
    if (!p) return MCPM_E_ARG;
    KGeom kg;
    Table tt;
    MCPM_REQUIRE(p, lin_mesh && lin_mesh_bar && fnl_bar && trans_bar, MCPM_E_ARG, "mcpm_png_add_vjp_f32: bad argument");
    MCPM_TRY(table_arg(p, "mcpm_png_add_vjp_f32", ks, trans, ntab, &tt));
    MCPM_REQUIRE(p, out_bar ? (out && phi && mean) : (phi_bar != nullptr), MCPM_E_ARG,
                 "mcpm_png_add_vjp_f32: out_bar needs out, phi and mean; without out_bar, phi_bar is the cotangent to pull back");
    MCPM_TRY(kgeom_arg(p, "mcpm_png_add_vjp_f32", kpx, kpy, kpz, &kg));
    const int64_t M = p->M, Mh = p->Mh;
    const unsigned nbk = (unsigned)((Mh + 255) / 256), nbr = (unsigned)((M + 255) / 256);
    // the table cotangent's accumulators, cleared here so that an oversized table is refused before anything is written.  They lie behind the
    // plan scalars S0, S1 of this call (the map in mcpm_internal.h): NOTHING between here and png_table_vjp_kernel may touch plan->reduce beyond
    // MCPM_RED_SCALARS (the det sums keep their partials in plan->part, the transforms use no reduction scratch)
    TabSum t;
    MCPM_TRY(mcpm_tab_begin(p, "mcpm_png_add_vjp_f32", MCPM_RED_PNG_ACC, (size_t)ntab, Mh, &t));
    const float *psib = phi_bar;      // without out_bar, phi_bar alone is pulled back: no C2R, no sums, fNL_bar = 0
    if (out_bar) {
        float *pb = p->rho;
        {
            StageTimer st_(p, ST_KSPACE, 16.0 * Mh);
            png_vjp_in_kernel<<<nbk, 256, 0, p->stream>>>(kg, tt, (const float2 *)out_bar, (float2 *)p->spec1, Mh);
            MCPM_LAUNCH_CHECK(p, "png_vjp_in_kernel");
        }
        MCPM_TRY(mcpm_fft_c2r(p, p->spec1, pb, 1));
        double *sums = p->reduce + MCPM_RED_SCALARS;
        DetSum s;
        MCPM_TRY(mcpm_det_begin(p, 2, nbr, &s));
        StageTimer st_(p, ST_LPT, 20.0 * M);
        png_vjp_sums_kernel<<<nbr, 256, 0, p->stream>>>(phi, pb, M, s.P);
        MCPM_LAUNCH_CHECK(p, "png_vjp_sums_kernel");
        MCPM_TRY(mcpm_det_fold(p, s, 2, 1.0, det_outs_row(DET_STORE, sums, 2)));
        png_quad_vjp_kernel<<<nbr, 256, 0, p->stream>>>(phi, fnl, mean, sums, M, phi_bar, pb, fnl_bar);
        MCPM_LAUNCH_CHECK(p, "png_quad_vjp_kernel");
        psib = pb;
    } else {
        MCPM_HIP(p, hipMemsetAsync(fnl_bar, 0, sizeof(double), p->stream));
    }
    MCPM_TRY(mcpm_fft_r2c(p, psib, p->spec1, 1));
    float *spec2 = lap_phi_bar ? p->spec + 2 * Mh : nullptr;      // behind tbar in the six-spectrum scratch
    if (spec2) MCPM_TRY(mcpm_fft_r2c(p, lap_phi_bar, spec2, 1));
    double *tbar = reinterpret_cast<double *>(p->spec);      // Mh doubles of the six-spectrum scratch
    StageTimer st_(p, ST_KSPACE, 56.0 * Mh);
    png_vjp_out_kernel<<<nbk, 256, 0, p->stream>>>(kg, tt, 1.f / (float)M, (const float2 *)lin_mesh,
                                                   (const float2 *)out, (const float2 *)out_bar, (const float2 *)p->spec1,
                                                   (const float2 *)spec2, (float2 *)lin_mesh_bar, tbar, Mh);
    MCPM_LAUNCH_CHECK(p, "png_vjp_out_kernel");
    png_table_vjp_kernel<0><<<t.nb, 256, 0, p->stream>>>(kg, tt, tbar, Mh, t.mx, t.acc);
    MCPM_LAUNCH_CHECK(p, "png_table_vjp_kernel");
    png_table_vjp_kernel<1><<<t.nb, 256, t.lds, p->stream>>>(kg, tt, tbar, Mh, t.mx, t.acc);
    MCPM_LAUNCH_CHECK(p, "png_table_vjp_kernel");
    return mcpm_tab_finish(p, t, &ntab, 1, trans_bar);
}

}  // extern "C"
