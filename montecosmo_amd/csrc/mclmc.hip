// Isokinetic (MCLMC / MAMS) integrator passes over one flat float32 state vector (samplers.py: the 'hip' back end).  Plain streaming
// kernels: two passes per velocity update, the three sums between them stay on the device as fixed-order float64 sums (reduce_dev.h).
#include <algorithm>
#include <cmath>

#include "mcpm_internal.h"
#include "reduce_dev.h"

namespace {

constexpr unsigned MCLMC_MAX_BLOCKS = 2048;      // 8 workgroups of 256 on each of 256 compute units; beyond that the grid strides

__device__ __forceinline__ void sums_add(double (&v)[3], float u, float g, float s) {
    const double gt = (double)s * (double)g, ud = (double)u;      // (the product of two float32 is exact in float64)
    v[0] += gt * gt, v[1] += ud * gt, v[2] += ud * ud;
}

// Pass 1.  P: [sum (s g)^2 : nblk] [sum u s g : nblk] [sum u^2 : nblk].  VEC: every pointer is 16-byte aligned, lanes take float4;
// the last d % 4 elements go to the first lanes of workgroup 0.
template <bool VEC>
__global__ __launch_bounds__(256) void mclmc_sums_kernel(const float *__restrict__ u, const float *__restrict__ g, const float *__restrict__ s,
                                                         int64_t d, double *__restrict__ P) {
    double v[3] = {0., 0., 0.};
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t d4 = d >> 2;
        const float4 *u4 = reinterpret_cast<const float4 *>(u), *g4 = reinterpret_cast<const float4 *>(g), *s4 = reinterpret_cast<const float4 *>(s);
        for (int64_t i = t0; i < d4; i += stride) {
            const float4 a = u4[i], b = g4[i], c = s ? s4[i] : make_float4(1.f, 1.f, 1.f, 1.f);
            sums_add(v, a.x, b.x, c.x), sums_add(v, a.y, b.y, c.y), sums_add(v, a.z, b.z, c.z), sums_add(v, a.w, b.w, c.w);
        }
        const int64_t j = (d4 << 2) + t0;
        if (t0 < 4 && j < d) sums_add(v, u[j], g[j], s ? s[j] : 1.f);
    } else {
        for (int64_t i = t0; i < d; i += stride) sums_add(v, u[i], g[i], s ? s[i] : 1.f);
    }
    block_partial<3>(v, P, gridDim.x, blockIdx.x);
}

// The two coefficients of u' = ca s g + cb u, and the kinetic energy change, from the three sums (mcpm.h: the formulas).
struct KickCoef {
    double ca, cb, dK;
};
__device__ __forceinline__ KickCoef kick_coef(const double *__restrict__ stats, int64_t d, double eps_kick) {
    const double gg = stats[0], ug = stats[1], uu = stats[2];
    const double n = sqrt(uu);
    KickCoef k;
    if (!(gg > 0.)) {      // no force: the velocity is only normalised
        k.ca = 0., k.cb = 1. / n, k.dK = 0.;
        return k;
    }
    const double gam = sqrt(gg), c = ug / (gam * n), dm1 = (double)(d - 1);
    const double delta = eps_kick * gam / dm1, z = exp(-delta);
    const double D = fmax((1. + c) + (1. - c) * z * z, 1e-300);
    k.ca = (1. - z) * (1. + z + c * (1. - z)) / (gam * D);
    k.cb = 2. * z / (n * D);
    k.dK = dm1 * (delta - 0.6931471805599453094 + log(D));
    return k;
}

__device__ __forceinline__ void kick_one(const KickCoef &k, double eps_drift, float &u, float &q, float g, float s, bool drift) {
    const double gt = (double)s * (double)g;
    u = (float)(k.ca * gt + k.cb * (double)u);
    if (drift) q = (float)((double)q + eps_drift * ((double)s * (double)u));
}

// Pass 2: u <- u', q += eps_drift s u' (q may be NULL), stats[3] += dK (one lane).  Reads stats[0..2], which the fold of pass 1 wrote.
template <bool VEC>
__global__ __launch_bounds__(256) void mclmc_update_kernel(float *__restrict__ u, float *__restrict__ q, const float *__restrict__ g,
                                                           const float *__restrict__ s, int64_t d, double eps_kick, double eps_drift,
                                                           double *__restrict__ stats) {
    const KickCoef k = kick_coef(stats, d, eps_kick);
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const bool drift = q != nullptr;
    if (VEC) {
        const int64_t d4 = d >> 2;
        float4 *u4 = reinterpret_cast<float4 *>(u), *q4 = reinterpret_cast<float4 *>(q);
        const float4 *g4 = reinterpret_cast<const float4 *>(g), *s4 = reinterpret_cast<const float4 *>(s);
        for (int64_t i = t0; i < d4; i += stride) {
            float4 a = u4[i], x = drift ? q4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 b = g4[i], c = s ? s4[i] : make_float4(1.f, 1.f, 1.f, 1.f);
            kick_one(k, eps_drift, a.x, x.x, b.x, c.x, drift), kick_one(k, eps_drift, a.y, x.y, b.y, c.y, drift);
            kick_one(k, eps_drift, a.z, x.z, b.z, c.z, drift), kick_one(k, eps_drift, a.w, x.w, b.w, c.w, drift);
            u4[i] = a;
            if (drift) q4[i] = x;
        }
        const int64_t j = (d4 << 2) + t0;
        if (t0 < 4 && j < d) {
            float a = u[j], x = drift ? q[j] : 0.f;
            kick_one(k, eps_drift, a, x, g[j], s ? s[j] : 1.f, drift);
            u[j] = a;
            if (drift) q[j] = x;
        }
    } else {
        for (int64_t i = t0; i < d; i += stride) {
            float a = u[i], x = drift ? q[i] : 0.f;
            kick_one(k, eps_drift, a, x, g[i], s ? s[i] : 1.f, drift);
            u[i] = a;
            if (drift) q[i] = x;
        }
    }
    if (t0 == 0) stats[3] += k.dK;
}

// xavg = gamma xavg + w q, x2avg = gamma x2avg + w q^2: every product and sum rounded on its own (no contraction), so that the result is
// the float64 expression as written.
__device__ __forceinline__ void moments_one(double gamma, double w, float qf, double &xa, double &x2a) {
#pragma clang fp contract(off)
    const double q = (double)qf;
    const double a = gamma * xa, b = w * q, c = gamma * x2a, e = w * (q * q);
    xa = a + b;
    x2a = c + e;
}

template <bool VEC>
__global__ __launch_bounds__(256) void mclmc_moments_kernel(const float *__restrict__ q, int64_t d, double gamma, double w,
                                                            double *__restrict__ xavg, double *__restrict__ x2avg) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t d4 = d >> 2;
        const float4 *q4 = reinterpret_cast<const float4 *>(q);
        double2 *x2 = reinterpret_cast<double2 *>(xavg), *y2 = reinterpret_cast<double2 *>(x2avg);
        for (int64_t i = t0; i < d4; i += stride) {
            const float4 a = q4[i];
            double2 x0 = x2[2 * i], x1 = x2[2 * i + 1], y0 = y2[2 * i], y1 = y2[2 * i + 1];
            moments_one(gamma, w, a.x, x0.x, y0.x), moments_one(gamma, w, a.y, x0.y, y0.y);
            moments_one(gamma, w, a.z, x1.x, y1.x), moments_one(gamma, w, a.w, x1.y, y1.y);
            x2[2 * i] = x0, x2[2 * i + 1] = x1, y2[2 * i] = y0, y2[2 * i + 1] = y1;
        }
        const int64_t j = (d4 << 2) + t0;
        if (t0 < 4 && j < d) moments_one(gamma, w, q[j], xavg[j], x2avg[j]);
    } else {
        for (int64_t i = t0; i < d; i += stride) moments_one(gamma, w, q[i], xavg[i], x2avg[i]);
    }
}

inline unsigned mclmc_blocks(int64_t d, bool vec) {
    const int64_t work = vec ? std::max<int64_t>(d >> 2, 1) : d;
    return (unsigned)std::min<int64_t>((work + 255) / 256, MCLMC_MAX_BLOCKS);
}

}  // namespace

extern "C" {

int mcpm_mclmc_kick_drift_f32(mcpm_plan *p, float *u, float *q, const float *g, const float *s, int64_t d, double eps_kick,
                              double eps_drift, double *stats) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, d >= 2 && u && g && stats, MCPM_E_ARG, "mcpm_mclmc_kick_drift_f32: bad argument");
    const bool vec = mcpm_aligned(u) && mcpm_aligned(q) && mcpm_aligned(g) && mcpm_aligned(s);
    const unsigned nb = mclmc_blocks(d, vec);
    DetSum sum;
    StageTimer st_(p, ST_AXPY, ((s ? 24.0 : 20.0) + (q ? 8.0 : 0.0)) * d);
    MCPM_TRY(mcpm_det_begin(p, 3, nb, &sum));
    if (vec) mclmc_sums_kernel<true><<<nb, 256, 0, p->stream>>>(u, g, s, d, sum.P);
    else mclmc_sums_kernel<false><<<nb, 256, 0, p->stream>>>(u, g, s, d, sum.P);
    MCPM_LAUNCH_CHECK(p, "mclmc_sums_kernel");
    MCPM_TRY(mcpm_det_fold(p, sum, 3, 1.0, det_outs_row(DET_STORE, stats, 3)));
    if (vec) mclmc_update_kernel<true><<<nb, 256, 0, p->stream>>>(u, q, g, s, d, eps_kick, eps_drift, stats);
    else mclmc_update_kernel<false><<<nb, 256, 0, p->stream>>>(u, q, g, s, d, eps_kick, eps_drift, stats);
    MCPM_LAUNCH_CHECK(p, "mclmc_update_kernel");
    return MCPM_OK;
}

int mcpm_mclmc_moments_f64(mcpm_plan *p, const float *q, int64_t d, double gamma, double w, double *xavg, double *x2avg) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, d >= 1 && q && xavg && x2avg, MCPM_E_ARG, "mcpm_mclmc_moments_f64: bad argument");
    const bool vec = mcpm_aligned(q) && mcpm_aligned(xavg) && mcpm_aligned(x2avg);
    StageTimer st_(p, ST_AXPY, 36.0 * d);
    if (vec) mclmc_moments_kernel<true><<<mclmc_blocks(d, true), 256, 0, p->stream>>>(q, d, gamma, w, xavg, x2avg);
    else mclmc_moments_kernel<false><<<mclmc_blocks(d, false), 256, 0, p->stream>>>(q, d, gamma, w, xavg, x2avg);
    MCPM_LAUNCH_CHECK(p, "mclmc_moments_kernel");
    return MCPM_OK;
}

}  // extern "C"
