// N-body state on the light cone: every particle takes the Euler solution at its OWN growth time g_p = a2g(a_p), by linear
// interpolation between the step states (diffrax's dense output, as nbody.py's `_snapshots` restates it for whole snapshots).
//
//   s = (g_p - g0) / dg,  i = clamp(floor(s), 0, K - 1),  theta = clamp(s - i, 0, 1)
//   disp_p = (1 - theta) x_i[p] + theta x_{i+1}[p],   vel_p likewise
//
// with the step states (x_i, v_i) as displacements from the lattice: x_i = x'_i - v_i dg / 2 from the checkpoint arrays 2 i, 2 i + 1 for
// i < K, and state K the run's returned (pos_out, vel_out).  Particles earlier than the start take the LPT start state, later than the end
// the final state.  Three kernels, all one streaming pass with one particle per lane:
//   lc_select_kernel   the forward selection;
//   lc_gbar_kernel     the cotangent of g_p and the three f64 sums of the reverse sweep (deterministic grid sums, reduce_dev.h);
//   lc_inject_kernel   the adjoint of the selection for ONE state j: the K + 1 launches of a sweep read g_p and touch a particle's
//                      cotangents only for its two states.
// The loop that calls them is mcpm_nbody_bf_lc_vjp_f32 (composite.hip).
#include "mcpm_internal.h"
#include "particles_dev.h"
#include "reduce_dev.h"

namespace {

// Interval and weight of one particle.  s is formed in double from the float32 g_p; the index is chosen by comparisons BEFORE any
// conversion to int, so that no g_p (NaN, +-Inf, huge) can give an index outside [0, K - 1]: a NaN fails `s >= 0` and maps to interval 0
// with theta = NaN.  `inside`: theta was not clamped (the only case with a derivative with respect to g_p).
struct LcSel {
    int i;
    float th;
    bool inside;
};
__device__ __forceinline__ LcSel lc_locate(float gp, double g0, double inv_dg, int K) {
    const double s = ((double)gp - g0) * inv_dg;
    LcSel r;
    r.i = (s >= 0.) ? (s < (double)K ? (int)s : K - 1) : 0;
    double th = s - (double)r.i;
    r.inside = th >= 0. && th <= 1.;
    if (th < 0.) th = 0.;      // (comparisons: a NaN stays a NaN)
    if (th > 1.) th = 1.;
    r.th = (float)th;
    return r;
}

// step state j of particle p as displacements: (x'_j - v_j dg/2, v_j) for j < K, (pos_out, vel_out) for j = K.  Offsets in 64 bits.
__device__ __forceinline__ void lc_state(const float *__restrict__ ckpt, int64_t pitch, int K, const float *__restrict__ xK,
                                         const float *__restrict__ vK, int j, int64_t p, float hd, P3 &x, P3 &v) {
    if (j < K) {
        const P3 xp = load3(ckpt + (int64_t)(2 * j) * pitch, p);
        v = load3(ckpt + (int64_t)(2 * j + 1) * pitch, p);
        x = P3{__builtin_fmaf(-hd, v.x, xp.x), __builtin_fmaf(-hd, v.y, xp.y), __builtin_fmaf(-hd, v.z, xp.z)};
    } else {
        x = load3(xK, p);
        v = load3(vK, p);
    }
}

// the convex form: theta = 0 and theta = 1 return a state bit for bit
__device__ __forceinline__ float lc_mix(float a, float b, float th) { return (1.f - th) * a + th * b; }

__global__ __launch_bounds__(256) void lc_select_kernel(const float *__restrict__ ckpt, int64_t pitch, int K, int64_t N, double g0, double inv_dg,
                                                        float hd, const float *__restrict__ xK, const float *__restrict__ vK,
                                                        const float *__restrict__ gp, float *__restrict__ disp, float *__restrict__ vel) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const LcSel s = lc_locate(gp[p], g0, inv_dg, K);
    // neighbours share an interval except at shell boundaries: the two loads are the same arrays across a wave nearly everywhere, and a
    // boundary costs a wave two array pairs, not a loop
    P3 x0, v0, x1, v1;
    lc_state(ckpt, pitch, K, xK, vK, s.i, p, hd, x0, v0);
    lc_state(ckpt, pitch, K, xK, vK, s.i + 1, p, hd, x1, v1);
    store3(disp, p, P3{lc_mix(x0.x, x1.x, s.th), lc_mix(x0.y, x1.y, s.th), lc_mix(x0.z, x1.z, s.th)});
    store3(vel, p, P3{lc_mix(v0.x, v1.x, s.th), lc_mix(v0.y, v1.y, s.th), lc_mix(v0.z, v1.z, s.th)});
}

// g_bar_p = (Xb . (x_{i+1} - x_i) + Vb . (v_{i+1} - v_i)) / dg where theta was not clamped, else 0; partial sums of
//   [0] g_bar_p, [1] g_bar_p (g_p - g0) / dg + Xb . ((1 - theta) v_i + [i + 1 < K] theta v_{i+1}) / 2
__global__ __launch_bounds__(256) void lc_gbar_kernel(const float *__restrict__ ckpt, int64_t pitch, int K, int64_t N, double g0, double inv_dg,
                                                      float hd, const float *__restrict__ xK, const float *__restrict__ vK,
                                                      const float *__restrict__ gp, const float *__restrict__ Xb, const float *__restrict__ Vb,
                                                      float *__restrict__ gbar, double *__restrict__ P) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double r[2] = {0., 0.};
    if (p < N) {
        const float g = gp[p];
        const LcSel s = lc_locate(g, g0, inv_dg, K);
        P3 x0, v0, x1, v1;
        lc_state(ckpt, pitch, K, xK, vK, s.i, p, hd, x0, v0);
        lc_state(ckpt, pitch, K, xK, vK, s.i + 1, p, hd, x1, v1);
        const P3 xb = load3(Xb, p), vb = load3(Vb, p);
        float gb = 0.f;
        if (s.inside) {
            const double d = (double)xb.x * ((double)x1.x - x0.x) + (double)xb.y * ((double)x1.y - x0.y) + (double)xb.z * ((double)x1.z - x0.z) +
                             (double)vb.x * ((double)v1.x - v0.x) + (double)vb.y * ((double)v1.y - v0.y) + (double)vb.z * ((double)v1.z - v0.z);
            gb = (float)(d * inv_dg);
            r[0] = gb;
            r[1] = (double)gb * (((double)g - g0) * inv_dg);
        }
        gbar[p] = gb;
        const double w0 = 1. - (double)s.th, w1 = s.i + 1 < K ? (double)s.th : 0.;
        // (a zero weight drops its term: a clamped theta = NaN cannot occur with w = 0, and 0 * v of a finite v is 0 anyway)
        r[1] += 0.5 * (w0 * ((double)xb.x * v0.x + (double)xb.y * v0.y + (double)xb.z * v0.z) +
                       (w1 != 0. ? w1 * ((double)xb.x * v1.x + (double)xb.y * v1.y + (double)xb.z * v1.z) : 0.));
    }
    block_partial<2>(r, P, gridDim.x, blockIdx.x);
}

// Injection of state j.  Weight w = 1 - theta if i_p == j, theta if i_p == j - 1, else 0.
//   init (state K, opens the sweep): xb = w Xb, vb = w Vb for every particle;
//   else: pos_bar += w Xb, vel_bar += w (Vb + cu Xb) for the particles with w != 0 -- predicated, the others are not touched.
// cu = -dg/2 when vel_bar holds the true v_bar (x_j = x'_j - v_j dg/2), and tau' - dg/2 when it holds the carried u = v_bar + tau' x_bar
// of a chained sweep: u is linear in (x_bar, v_bar), so adding w Xb to x_bar and w (Vb - dg/2 Xb) to v_bar adds w (Vb + (tau' - dg/2) Xb) to u.
__global__ __launch_bounds__(256) void lc_inject_kernel(int j, int K, int64_t N, double g0, double inv_dg, const float *__restrict__ gp,
                                                        const float *__restrict__ Xb, const float *__restrict__ Vb, float cu, int init,
                                                        float *__restrict__ xb, float *__restrict__ vb) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const LcSel s = lc_locate(gp[p], g0, inv_dg, K);
    const float w = s.i == j ? 1.f - s.th : (s.i == j - 1 ? s.th : 0.f);
    if (init) {
        P3 X = {0.f, 0.f, 0.f}, V = {0.f, 0.f, 0.f};
        if (w != 0.f) {
            const P3 a = load3(Xb, p), b = load3(Vb, p);
            X = P3{w * a.x, w * a.y, w * a.z};
            V = P3{w * b.x, w * b.y, w * b.z};
        }
        store3(xb, p, X);
        store3(vb, p, V);
        return;
    }
    if (w == 0.f) return;      // (a NaN weight is not zero: it is injected, as the forward pass gave NaN there)
    const P3 a = load3(Xb, p), b = load3(Vb, p);
    P3 X = load3(xb, p), V = load3(vb, p);
    X = P3{__builtin_fmaf(w, a.x, X.x), __builtin_fmaf(w, a.y, X.y), __builtin_fmaf(w, a.z, X.z)};
    V = P3{__builtin_fmaf(w, __builtin_fmaf(cu, a.x, b.x), V.x), __builtin_fmaf(w, __builtin_fmaf(cu, a.y, b.y), V.y),
           __builtin_fmaf(w, __builtin_fmaf(cu, a.z, b.z), V.z)};
    store3(xb, p, X);
    store3(vb, p, V);
}

inline unsigned lc_blocks(int64_t N) { return (unsigned)((N + 255) / 256); }

}  // namespace

int mcpm_lc_inject(mcpm_plan *p, int j, int n_steps, double dg, double g0, const float *g_p, const float *Xb, const float *Vb, float cu,
                   int init, float *xb, float *vb) {
    const int64_t N = p->Np;
    // K launches read g_p (4 N); a particle's cotangents (Xb, Vb, x_bar, v_bar in, x_bar, v_bar out: 72 B) move for two states of the sweep
    StageTimer st_(p, ST_AXPY, 4.0 * N + (init ? 48.0 * N : 0.0));
    lc_inject_kernel<<<lc_blocks(N), 256, 0, p->stream>>>(j, n_steps, N, g0, 1.0 / dg, g_p, Xb, Vb, cu, init, xb, vb);
    MCPM_LAUNCH_CHECK(p, "lc_inject_kernel");
    return MCPM_OK;
}

// g_bar_p to the caller's array; into the DEVICE doubles: *g_bar -= row 0, *dg_bar -= row 1 of the kernel's sums
int mcpm_lc_gbar(mcpm_plan *p, const float *ckpt, int n_steps, double dg, double g0, const float *pos_out, const float *vel_out,
                 const float *g_p, const float *Xb, const float *Vb, float *g_bar_p, double *g_bar, double *dg_bar) {
    const int64_t N = p->Np;
    const unsigned nb = lc_blocks(N);
    StageTimer st_(p, ST_AXPY, 80.0 * N);
    DetSum s;
    MCPM_TRY(mcpm_det_begin(p, 2, nb, &s));
    lc_gbar_kernel<<<nb, 256, 0, p->stream>>>(ckpt, mcpm_pitch(p), n_steps, N, g0, 1.0 / dg, (float)(dg / 2), pos_out, vel_out, g_p, Xb, Vb,
                                              g_bar_p, s.P);
    MCPM_LAUNCH_CHECK(p, "lc_gbar_kernel");
    return mcpm_det_fold(p, s, 2, -1.0, det_outs_ptrs(DET_ACCUMULATE, g_bar, dg_bar));
}

extern "C" int mcpm_nbody_lightcone_f32(mcpm_plan *p, const float *ckpt, int n_steps, double dg, double g0, const float *pos_out,
                                        const float *vel_out, const float *g_p, float *disp, float *vel) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, ckpt && pos_out && vel_out && g_p && disp && vel, MCPM_E_ARG, "mcpm_nbody_lightcone_f32: null buffer");
    MCPM_REQUIRE(p, n_steps >= 1, MCPM_E_ARG, "mcpm_nbody_lightcone_f32: n_steps must be >= 1");
    MCPM_REQUIRE(p, dg != 0. && dg == dg && g0 == g0, MCPM_E_ARG, "mcpm_nbody_lightcone_f32: dg must be non-zero, dg and g0 numbers");
    const int64_t N = p->Np;
    StageTimer st_(p, ST_AXPY, 76.0 * N);      // g_p, two states (48) in; disp, vel (24) out
    lc_select_kernel<<<lc_blocks(N), 256, 0, p->stream>>>(ckpt, mcpm_pitch(p), n_steps, N, g0, 1.0 / dg, (float)(dg / 2), pos_out, vel_out, g_p,
                                                          disp, vel);
    MCPM_LAUNCH_CHECK(p, "lc_select_kernel");
    return MCPM_OK;
}
