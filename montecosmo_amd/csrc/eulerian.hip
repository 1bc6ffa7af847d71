// Eulerian bias expansion on the painted matter field (montecosmo/bricks.py:513-586) and its VJP:
//   w = 1 + b1E d + b2E (d^2 - <d^2>)/2 + bs2 (s2 - 2/3 <d^2>) + bn2 lap(d) [+ bp phi + bpdE (phi d - <phi d>)]
// with d = irfftn(matter_k, zero mode dropped), s2 = the squared traceless tidal shear of d, phi = irfftn(phi_k) the advected Gaussian
// potential (only when phi_k is given), all on the plan's mesh; coef = {b1E, b2E, bs2, bn2, bp, bpdE}.
// Forward: bias_spectra_kernel<0> (bias_dev.h: d and the five Hessians) -> C2R x6, eul_lap_phi_kernel (-k^2 d [, phi]) -> C2R x1|2, all into
// `saved` = {d, h00, h11, h01, h02, h12, lap d [, phi]}; then the two moments and ONE streaming pass that contracts the shear in registers
// and writes w: 7 (8 with phi) floats in, 1 out per cell = 32 (36) bytes; no s2 mesh exists.
// w is affine in the two moments.  They are taken by a moment pass FIRST (eul_moment_kernel reads d [, phi]: 4 (8) bytes per cell) rather
// than by a single pass with a constant-offset fix-up (8 more bytes per cell, w rounded twice).  Measured at 256^3 on one MI355X, moments +
// weights: 140.3 us against 137.0 us for the fix-up form without phi, 154.1 against 153.9 us with phi (profiles/eulerian_bias.txt): no
// difference beyond the spread of repeat runs, so the form that rounds w once and needs no third kernel is the one kept.
// VJP: pass 1 reduces the six coefficient cotangents and the two moment cotangents; pass 2 writes the cotangents of the 7 (8) real meshes
// with the moments' share (moment_bar 2 d / M; moment_bar phi / M and d / M) folded in; R2C x6 -> bias_spectra_vjp_kernel<0>, R2C x1|2 ->
// eul_lap_phi_vjp_kernel.  All sums are float64 per-workgroup partials folded in a fixed order (reduce_dev.h): no floating-point atomic,
// every output bitwise repeatable.
#include "mcpm_internal.h"
#include "reduce_dev.h"
#include "bias_dev.h"

namespace {

struct Coef6 {
    float b1, b2, bs2, bn2, bp, bpd;
};

// out[0] = scale (-k^2) in, out[1] = scale phi (phi may be NULL: one spectrum)
__global__ __launch_bounds__(256) void eul_lap_phi_kernel(KGeom kg, float scale, const float2 *__restrict__ in,
                                                          const float2 *__restrict__ phi, float2 *__restrict__ out, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    float re[7], im[3];
    multipliers(m, true, re, im);
    const float2 v = in[idx];
    out[idx] = make_float2(scale * re[6] * v.x, scale * re[6] * v.y);
    if (phi) {
        const float2 q = phi[idx];
        out[Mh + idx] = make_float2(scale * q.x, scale * q.y);
    }
}

// adjoint: mk_bar += scale zw (-k^2) in[0] (its zero mode set to 0: the forward pass drops that mode), phi_bar = scale zw in[1]
// (kphys arrives as three scalars here: handed over inside KGeom, the compiler pairs other components of k^2 = k0 k0 + k1 k1 + k2 k2 into its
// packed multiply, another product is the one fused into the sum, and mk_bar changes in its last bit)
__global__ __launch_bounds__(256) void eul_lap_phi_vjp_kernel(Geom g, float kx, float ky, float kz, float scale, const float2 *__restrict__ in,
                                                              float2 *__restrict__ mk_bar, float2 *__restrict__ phi_bar, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(KGeom{g, {kx, ky, kz}}, idx);
    float re[7], im[3];
    multipliers(m, false, re, im);
    const float s = scale * m.zw;
    const float2 v = in[idx], o = mk_bar[idx];
    mk_bar[idx] = idx == 0 ? make_float2(0.f, 0.f) : make_float2(o.x + s * re[6] * v.x, o.y + s * re[6] * v.y);
    if (phi_bar) {
        const float2 q = in[Mh + idx];
        phi_bar[idx] = make_float2(s * q.x, s * q.y);
    }
}

// s = {d, h00, h11, h01, h02, h12, lap d, phi}, M apart: the squared traceless shear, c = -(a + b) as shear_combine_kernel (bias.hip)
__device__ __forceinline__ float shear2(const float *__restrict__ s, int64_t M, int64_t i, float d) {
    const float t = d * (1.f / 3.f);
    const float a = s[M + i] - t, b = s[2 * M + i] - t, c = -(a + b);
    const float e0 = s[3 * M + i], e1 = s[4 * M + i], e2 = s[5 * M + i];
    return a * a + b * b + c * c + 2.f * (e0 * e0 + e1 * e1 + e2 * e2);
}

// rows 0, 1: d^2, phi d
template <bool PHI>
__global__ __launch_bounds__(256) void eul_moment_kernel(const float *__restrict__ s, int64_t M, double *part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[2] = {0., 0.};
    if (i < M) {
        const float d = s[i];
        v[0] = (double)d * (double)d;
        if (PHI) v[1] = (double)s[7 * M + i] * (double)d;
    }
    block_partial<2>(v, part, gridDim.x, blockIdx.x);
}

template <bool PHI>
__global__ __launch_bounds__(256) void eul_weights_kernel(const float *__restrict__ s, int64_t M, Coef6 B, const double *__restrict__ mom,
                                                          float *__restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float sig = (float)mom[0];
    const float d = s[i], s2 = shear2(s, M, i, d) - (2.f / 3.f) * sig;
    float wt = 1.f + B.b1 * d;
    wt += B.b2 * (d * d - sig) * 0.5f;
    wt += B.bs2 * s2;
    wt += B.bn2 * s[6 * M + i];
    if (PHI) {
        const float ph = s[7 * M + i];
        wt += B.bp * ph;
        wt += B.bpd * (ph * d - (float)mom[1]);
    }
    w[i] = wt;
}

// pass 1 of the VJP: rows 0..5 the cotangents of coef, 6: <d^2>_bar, 7: <phi d>_bar
template <bool PHI>
__global__ __launch_bounds__(256) void eul_vjp_reduce_kernel(const float *__restrict__ s, int64_t M, Coef6 B, const double *__restrict__ mom,
                                                             const float *__restrict__ wb, double *part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (i < M) {
        const float sig = (float)mom[0];
        const float d = s[i], s2 = shear2(s, M, i, d) - (2.f / 3.f) * sig;
        const float g = wb[i];
        v[0] = (double)(g * d);
        v[1] = (double)(g * (d * d - sig) * 0.5f);
        v[2] = (double)(g * s2);
        v[3] = (double)(g * s[6 * M + i]);
        v[6] = (double)(g * (-0.5f * B.b2 - (2.f / 3.f) * B.bs2));
        if (PHI) {
            const float ph = s[7 * M + i];
            v[4] = (double)(g * ph);
            v[5] = (double)(g * (ph * d - (float)mom[1]));
            v[7] = (double)(-g * B.bpd);
        }
    }
    block_partial<8>(v, part, gridDim.x, blockIdx.x);
}

// pass 2: cotangents of the 7 (8) real meshes into r (same layout as s); mbar = {<d^2>_bar, <phi d>_bar}
template <bool PHI>
__global__ __launch_bounds__(256) void eul_vjp_cells_kernel(const float *__restrict__ s, int64_t M, Coef6 B, const double *__restrict__ mbar,
                                                            const float *__restrict__ wb, float *__restrict__ r) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float sigbar = (float)mbar[0], inv = 1.f / (float)M;
    const float d = s[i], t = d * (1.f / 3.f), g = wb[i];
    const float a = s[M + i] - t, b = s[2 * M + i] - t, c = -(a + b);
    const float w2 = g * B.bs2;
    const float ab = w2 * (2.f * a - 2.f * c), bb = w2 * (2.f * b - 2.f * c);
    float db = g * (B.b1 + B.b2 * d) + sigbar * 2.f * d * inv - (ab + bb) * (1.f / 3.f);
    if (PHI) {
        const float ph = s[7 * M + i], mubar = (float)mbar[1];
        db += g * B.bpd * ph + mubar * ph * inv;
        r[7 * M + i] = g * (B.bp + B.bpd * d) + mubar * d * inv;
    }
    r[i] = db;
    r[M + i] = ab;
    r[2 * M + i] = bb;
    r[3 * M + i] = w2 * 4.f * s[3 * M + i];
    r[4 * M + i] = w2 * 4.f * s[4 * M + i];
    r[5 * M + i] = w2 * 4.f * s[5 * M + i];
    r[6 * M + i] = g * B.bn2;
}

}  // namespace

extern "C" {

// matter_k, phi_k (may be NULL): plain half-spectra of the plan's mesh; coef6 (host) = {b1E, b2E, bs2, bn2, fNL_bp, fNL_bpdE}.
// w: M floats.  saved: 7 M floats (8 M with phi_k), receives {d, h00, h11, h01, h02, h12, lap d [, phi]} for the adjoint.
// moments (device, 2 doubles): <d^2>, <phi d> (0 without phi_k).
int mcpm_eulerian_bias_f32(mcpm_plan *p, const float *matter_k, const float *phi_k, float kpx, float kpy, float kpz, const float *coef6,
                           float *w, float *saved, double *moments) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, matter_k && coef6 && w && saved && moments, MCPM_E_ARG, "mcpm_eulerian_bias_f32: null buffer");
    KGeom kg;
    MCPM_TRY(kgeom_arg(p, "mcpm_eulerian_bias_f32", kpx, kpy, kpz, &kg));
    const int64_t M = p->M, Mh = p->Mh;
    const unsigned nbh = (unsigned)((Mh + 255) / 256), nb = (unsigned)((M + 255) / 256);
    const float scale = 1.f / (float)M;
    const Coef6 B{coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
    float *spec = p->spec;
    bias_spectra_kernel<0><<<nbh, 256, 0, p->stream>>>(kg, scale, (const float2 *)matter_k, (float2 *)spec, Mh);
    MCPM_LAUNCH_CHECK(p, "bias_spectra_kernel");
    MCPM_HIP(p, hipMemsetAsync(spec, 0, sizeof(float2), p->stream));      // the zero mode of d (the Hessian multipliers vanish there already)
    MCPM_TRY(mcpm_fft_c2r(p, spec, saved, 6));
    eul_lap_phi_kernel<<<nbh, 256, 0, p->stream>>>(kg, scale, (const float2 *)matter_k, (const float2 *)phi_k, (float2 *)spec, Mh);
    MCPM_LAUNCH_CHECK(p, "eul_lap_phi_kernel");
    MCPM_TRY(mcpm_fft_c2r(p, spec, saved + 6 * M, phi_k ? 2 : 1));
    DetSum s;
    MCPM_TRY(mcpm_det_begin(p, 2, nb, &s));
    StageTimer st_(p, ST_LPT, (phi_k ? 44.0 : 36.0) * M);      // moments: 1 (2) floats in; weights: 7 (8) in, 1 out
    if (phi_k) eul_moment_kernel<true><<<nb, 256, 0, p->stream>>>(saved, M, s.P);
    else eul_moment_kernel<false><<<nb, 256, 0, p->stream>>>(saved, M, s.P);
    MCPM_LAUNCH_CHECK(p, "eul_moment_kernel");
    MCPM_TRY(mcpm_det_fold(p, s, 2, 1.0 / (double)M, det_outs_row(DET_STORE, moments, 2)));
    if (phi_k) eul_weights_kernel<true><<<nb, 256, 0, p->stream>>>(saved, M, B, moments, w);
    else eul_weights_kernel<false><<<nb, 256, 0, p->stream>>>(saved, M, B, moments, w);
    MCPM_LAUNCH_CHECK(p, "eul_weights_kernel");
    return MCPM_OK;
}

// saved, moments: what the forward call left (has_phi: it was given a phi_k); w_bar: M floats -> matter_k_bar (real-pair convention, irfftn
// multiplicity weights, zero mode 0), phi_k_bar (required with has_phi), coef_bar (device, 6 doubles; [4], [5] = 0 without phi).
int mcpm_eulerian_bias_vjp_f32(mcpm_plan *p, const float *saved, const double *moments, int has_phi, float kpx, float kpy, float kpz,
                               const float *coef6, const float *w_bar, float *matter_k_bar, float *phi_k_bar, double *coef_bar) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, saved && moments && coef6 && w_bar && matter_k_bar && coef_bar && (!has_phi || phi_k_bar), MCPM_E_ARG,
                 "mcpm_eulerian_bias_vjp_f32: null buffer");
    KGeom kg;
    MCPM_TRY(kgeom_arg(p, "mcpm_eulerian_bias_vjp_f32", kpx, kpy, kpz, &kg));
    const int64_t M = p->M, Mh = p->Mh;
    const unsigned nbh = (unsigned)((Mh + 255) / 256), nb = (unsigned)((M + 255) / 256);
    const float scale = 1.f / (float)M;
    const Coef6 B{coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
    float *spec = p->spec, *r = p->fmesh;      // scratch: up to 6 plain spectra, 8 of the 9 real meshes
    double *mbar = p->reduce + MCPM_RED_SCALARS;
    DetSum s;
    MCPM_TRY(mcpm_det_begin(p, 8, nb, &s));
    DetOuts o8 = det_outs_row(DET_STORE, coef_bar, 6);
    o8.p[6] = mbar;
    o8.p[7] = mbar + 1;
    {
        StageTimer st_(p, ST_LPT, (has_phi ? 100.0 : 88.0) * M);      // pass 1: 8 (9) floats in; pass 2: 7 (8) in, 7 (8) out
        if (has_phi) eul_vjp_reduce_kernel<true><<<nb, 256, 0, p->stream>>>(saved, M, B, moments, w_bar, s.P);
        else eul_vjp_reduce_kernel<false><<<nb, 256, 0, p->stream>>>(saved, M, B, moments, w_bar, s.P);
        MCPM_LAUNCH_CHECK(p, "eul_vjp_reduce_kernel");
        MCPM_TRY(mcpm_det_fold(p, s, 8, 1.0, o8));
        if (has_phi) eul_vjp_cells_kernel<true><<<nb, 256, 0, p->stream>>>(saved, M, B, mbar, w_bar, r);
        else eul_vjp_cells_kernel<false><<<nb, 256, 0, p->stream>>>(saved, M, B, mbar, w_bar, r);
        MCPM_LAUNCH_CHECK(p, "eul_vjp_cells_kernel");
    }
    MCPM_TRY(mcpm_fft_r2c(p, r, spec, 6));
    bias_spectra_vjp_kernel<0><<<nbh, 256, 0, p->stream>>>(kg, scale, (const float2 *)spec, (float2 *)matter_k_bar, Mh, 0);
    MCPM_LAUNCH_CHECK(p, "bias_spectra_vjp_kernel");
    MCPM_TRY(mcpm_fft_r2c(p, r + 6 * M, spec, has_phi ? 2 : 1));
    eul_lap_phi_vjp_kernel<<<nbh, 256, 0, p->stream>>>(p->g, kpx, kpy, kpz, scale, (const float2 *)spec, (float2 *)matter_k_bar,
                                                       (float2 *)(has_phi ? phi_k_bar : nullptr), Mh);
    MCPM_LAUNCH_CHECK(p, "eul_lap_phi_vjp_kernel");
    return MCPM_OK;
}

}  // extern "C"
