// MAP optimisation and Laplace approximation passes over flat vectors (samplers.optimize, lapprox.py: the 'hip' back end).  Plain streaming
// kernels in the style of mclmc.hip: grid-stride loops, 64-bit indices, 16-byte accesses where every pointer allows them, every value formed
// in float64 and rounded once, the Schur sums in a fixed order (reduce_dev.h).  The Rademacher probes are never stored: each kernel
// regenerates r_i from (seed, probe, i) by the splitmix64 hash that mcpm.h states.
#include <algorithm>
#include <cstdint>

#include "mcpm_internal.h"
#include "reduce_dev.h"

namespace {

constexpr unsigned LAP_MAX_BLOCKS = 2048;      // as mclmc.hip: beyond that the grid strides
constexpr int SCHUR_MAXM = 16;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
inline uint64_t probe_key(uint64_t seed, uint64_t probe) { return splitmix64(seed ^ splitmix64(probe)); }
// r_i: +1 / -1 on start <= i < stop by the top bit of the hash, 0 elsewhere
__device__ __forceinline__ double rademacher(uint64_t key, int64_t i, int64_t start, int64_t stop) {
    if (i < start || i >= stop) return 0.;
    return (splitmix64((uint64_t)i ^ key) >> 63) ? -1. : 1.;
}

// ---- Adam ---------------------------------------------------------------------------------------------------------------------------
struct AdamCoef {
    double lr, b1, b2, eps, c1, c2;
};
// Every product and sum rounded on its own (no contraction): the aligned and the unaligned path, and the float64 restatement, agree.
__device__ __forceinline__ void adam_one(const AdamCoef &a, float &q, float &m, float &v, float g) {
#pragma clang fp contract(off)
    const double gu = -(double)g;
    const double m1 = (1. - a.b1) * gu, m2 = a.b1 * (double)m, md = m1 + m2;
    const double v1 = (1. - a.b2) * (gu * gu), v2 = a.b2 * (double)v, vd = v1 + v2;
    const double num = a.lr * (md * a.c1), den = sqrt(vd * a.c2) + a.eps;
    q = (float)((double)q - num / den);
    m = (float)md;
    v = (float)vd;
}

template <bool VEC>
__global__ __launch_bounds__(256) void adam_step_kernel(float *__restrict__ q, float *__restrict__ m, float *__restrict__ v,
                                                        const float *__restrict__ g, int64_t d, AdamCoef a) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t d4 = d >> 2;
        float4 *q4 = reinterpret_cast<float4 *>(q), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
        const float4 *g4 = reinterpret_cast<const float4 *>(g);
        for (int64_t i = t0; i < d4; i += stride) {
            float4 x = q4[i], y = m4[i], z = v4[i];
            const float4 b = g4[i];
            adam_one(a, x.x, y.x, z.x, b.x), adam_one(a, x.y, y.y, z.y, b.y), adam_one(a, x.z, y.z, z.z, b.z), adam_one(a, x.w, y.w, z.w, b.w);
            q4[i] = x, m4[i] = y, v4[i] = z;
        }
        const int64_t j = (d4 << 2) + t0;
        if (t0 < 4 && j < d) adam_one(a, q[j], m[j], v[j], g[j]);
    } else {
        for (int64_t i = t0; i < d; i += stride) adam_one(a, q[i], m[i], v[i], g[i]);
    }
}

// ---- probes -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float shift_one(float q, double er) { return (float)((double)q + er); }

template <bool VEC>
__global__ __launch_bounds__(256) void probe_shift_kernel(const float *__restrict__ q, int64_t d, int64_t start, int64_t stop, uint64_t key,
                                                          double eps, float *__restrict__ qp, float *__restrict__ qm) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t d4 = d >> 2;
        const float4 *q4 = reinterpret_cast<const float4 *>(q);
        float4 *p4 = reinterpret_cast<float4 *>(qp), *m4 = reinterpret_cast<float4 *>(qm);
        for (int64_t i = t0; i < d4; i += stride) {
            const float4 x = q4[i];
            const double e0 = eps * rademacher(key, 4 * i, start, stop), e1 = eps * rademacher(key, 4 * i + 1, start, stop);
            const double e2 = eps * rademacher(key, 4 * i + 2, start, stop), e3 = eps * rademacher(key, 4 * i + 3, start, stop);
            if (qp) p4[i] = make_float4(shift_one(x.x, e0), shift_one(x.y, e1), shift_one(x.z, e2), shift_one(x.w, e3));
            if (qm) m4[i] = make_float4(shift_one(x.x, -e0), shift_one(x.y, -e1), shift_one(x.z, -e2), shift_one(x.w, -e3));
        }
        const int64_t j = (d4 << 2) + t0;
        if (t0 < 4 && j < d) {
            const double e = eps * rademacher(key, j, start, stop);
            if (qp) qp[j] = shift_one(q[j], e);
            if (qm) qm[j] = shift_one(q[j], -e);
        }
    } else {
        for (int64_t i = t0; i < d; i += stride) {
            const double e = eps * rademacher(key, i, start, stop);
            if (qp) qp[i] = shift_one(q[i], e);
            if (qm) qm[i] = shift_one(q[i], -e);
        }
    }
}

// diag += coef r (g+ - g-): the difference, the product and the sum each rounded on their own (r only sets a sign)
__device__ __forceinline__ void accum_one(double coef, double r, float gp, float gm, double &diag) {
#pragma clang fp contract(off)
    const double diff = (double)gp - (double)gm;
    const double t = coef * (r * diff);
    diag = diag + t;
}

// Elements outside start .. stop are neither read nor written.
template <bool VEC>
__global__ __launch_bounds__(256) void hutchinson_accum_kernel(const float *__restrict__ gp, const float *__restrict__ gm, int64_t d,
                                                               int64_t start, int64_t stop, uint64_t key, double coef,
                                                               double *__restrict__ diag) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t d4 = d >> 2;
        const float4 *p4 = reinterpret_cast<const float4 *>(gp), *m4 = reinterpret_cast<const float4 *>(gm);
        double2 *x2 = reinterpret_cast<double2 *>(diag);
        // whole groups of four inside the range take 16-byte accesses, the (at most two) groups that straddle an end go element by element
        for (int64_t i = t0; i < d4; i += stride) {
            const int64_t e = 4 * i;
            if (e + 4 <= start || e >= stop) continue;
            if (e >= start && e + 4 <= stop) {
                const float4 a = p4[i], b = m4[i];
                double2 x0 = x2[2 * i], x1 = x2[2 * i + 1];
                accum_one(coef, rademacher(key, e, start, stop), a.x, b.x, x0.x), accum_one(coef, rademacher(key, e + 1, start, stop), a.y, b.y, x0.y);
                accum_one(coef, rademacher(key, e + 2, start, stop), a.z, b.z, x1.x), accum_one(coef, rademacher(key, e + 3, start, stop), a.w, b.w, x1.y);
                x2[2 * i] = x0, x2[2 * i + 1] = x1;
            } else {
                for (int64_t j = e > start ? e : start; j < e + 4 && j < stop; ++j)
                    accum_one(coef, rademacher(key, j, start, stop), gp[j], gm[j], diag[j]);
            }
        }
        const int64_t j = (d4 << 2) + t0;
        if (t0 < 4 && j < d && j >= start && j < stop) accum_one(coef, rademacher(key, j, start, stop), gp[j], gm[j], diag[j]);
    } else {
        for (int64_t i = start + t0; i < stop; i += stride) accum_one(coef, rademacher(key, i, start, stop), gp[i], gm[i], diag[i]);
    }
}

// ---- Schur sums ---------------------------------------------------------------------------------------------------------------------
// One launch adds up to DET_MAXK pairs (i <= j) of rows: v[p] = sum_k B[i_p, k] B[j_p, k] / (D[k] + eps_diag).  The product of two float32
// is exact in float64; the quotient and the sum round.  Unused slots stay zero.
struct SchurPairs {
    int n;
    unsigned char i[DET_MAXK], j[DET_MAXK];
};

__global__ __launch_bounds__(256) void schur_sums_kernel(const float *__restrict__ B, int64_t n, int64_t ldb, const double *__restrict__ D,
                                                         double eps_diag, SchurPairs pr, double *__restrict__ P) {
    double v[DET_MAXK];
#pragma unroll
    for (int p = 0; p < DET_MAXK; ++p) v[p] = 0.;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t k = t0; k < n; k += stride) {
        const double w = 1. / (D[k] + eps_diag);
#pragma unroll
        for (int p = 0; p < DET_MAXK; ++p)
            if (p < pr.n) v[p] += ((double)B[(int64_t)pr.i[p] * ldb + k] * (double)B[(int64_t)pr.j[p] * ldb + k]) * w;
    }
    block_partial<DET_MAXK>(v, P, gridDim.x, blockIdx.x);
}

// out[j, i] = out[i, j] for i < j: the matrix is exactly symmetric
__global__ void schur_mirror_kernel(double *__restrict__ out, int m) {
    const int i = threadIdx.x / m, j = threadIdx.x % m;
    if (i < m && i < j) out[j * m + i] = out[i * m + j];
}

inline unsigned lap_blocks(int64_t work) { return (unsigned)std::min<int64_t>((std::max<int64_t>(work, 1) + 255) / 256, LAP_MAX_BLOCKS); }
inline unsigned lap_blocks(int64_t d, bool vec) { return lap_blocks(vec ? d >> 2 : d); }

}  // namespace

extern "C" {

int mcpm_adam_step_f32(mcpm_plan *p, float *q, float *m, float *v, const float *g, int64_t d, double lr, double b1, double b2, double eps,
                       double c1, double c2) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, d >= 1 && q && m && v && g, MCPM_E_ARG, "mcpm_adam_step_f32: bad argument");
    const bool vec = mcpm_aligned(q) && mcpm_aligned(m) && mcpm_aligned(v) && mcpm_aligned(g);
    const AdamCoef a{lr, b1, b2, eps, c1, c2};
    StageTimer st_(p, ST_AXPY, 28.0 * d);
    if (vec) adam_step_kernel<true><<<lap_blocks(d, true), 256, 0, p->stream>>>(q, m, v, g, d, a);
    else adam_step_kernel<false><<<lap_blocks(d, false), 256, 0, p->stream>>>(q, m, v, g, d, a);
    MCPM_LAUNCH_CHECK(p, "adam_step_kernel");
    return MCPM_OK;
}

int mcpm_probe_shift_f32(mcpm_plan *p, const float *q, int64_t d, int64_t start, int64_t stop, uint64_t seed, uint64_t probe, double eps,
                         float *q_plus, float *q_minus) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, d >= 1 && q && 0 <= start && start <= stop && stop <= d, MCPM_E_ARG, "mcpm_probe_shift_f32: bad argument");
    if (!q_plus && !q_minus) return MCPM_OK;
    const bool vec = mcpm_aligned(q) && mcpm_aligned(q_plus) && mcpm_aligned(q_minus);
    const uint64_t key = probe_key(seed, probe);
    StageTimer st_(p, ST_AXPY, (4.0 + (q_plus ? 4.0 : 0.0) + (q_minus ? 4.0 : 0.0)) * d);
    if (vec) probe_shift_kernel<true><<<lap_blocks(d, true), 256, 0, p->stream>>>(q, d, start, stop, key, eps, q_plus, q_minus);
    else probe_shift_kernel<false><<<lap_blocks(d, false), 256, 0, p->stream>>>(q, d, start, stop, key, eps, q_plus, q_minus);
    MCPM_LAUNCH_CHECK(p, "probe_shift_kernel");
    return MCPM_OK;
}

int mcpm_hutchinson_accum_f64(mcpm_plan *p, const float *g_plus, const float *g_minus, int64_t d, int64_t start, int64_t stop,
                              uint64_t seed, uint64_t probe, double coef, double *diag) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, d >= 1 && g_plus && g_minus && diag && 0 <= start && start <= stop && stop <= d, MCPM_E_ARG,
                 "mcpm_hutchinson_accum_f64: bad argument");
    if (start == stop) return MCPM_OK;
    const bool vec = mcpm_aligned(g_plus) && mcpm_aligned(g_minus) && mcpm_aligned(diag);
    const uint64_t key = probe_key(seed, probe);
    StageTimer st_(p, ST_AXPY, 24.0 * (stop - start));
    if (vec) hutchinson_accum_kernel<true><<<lap_blocks(d, true), 256, 0, p->stream>>>(g_plus, g_minus, d, start, stop, key, coef, diag);
    else hutchinson_accum_kernel<false><<<lap_blocks(stop - start), 256, 0, p->stream>>>(g_plus, g_minus, d, start, stop, key, coef, diag);
    MCPM_LAUNCH_CHECK(p, "hutchinson_accum_kernel");
    return MCPM_OK;
}

int mcpm_schur_f64(mcpm_plan *p, const float *B, int m, int64_t n, int64_t ldb, const double *D, double eps_diag, double *out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, m >= 1 && m <= SCHUR_MAXM, MCPM_E_ARG, "mcpm_schur_f64: 1 <= m <= 16");
    MCPM_REQUIRE(p, n >= 1 && ldb >= n && B && D && out, MCPM_E_ARG, "mcpm_schur_f64: bad argument");
    const unsigned nb = lap_blocks(n);
    const int npair = m * (m + 1) / 2;
    StageTimer st_(p, ST_AXPY, (8.0 * DET_MAXK + 8.0) * n * ((npair + DET_MAXK - 1) / DET_MAXK));
    SchurPairs pr{};
    DetOuts outs{};
    for (int i = 0, done = 0; i < m; ++i) {
        for (int j = i; j < m; ++j) {
            pr.i[pr.n] = (unsigned char)i, pr.j[pr.n] = (unsigned char)j;
            outs.p[pr.n++] = out + (int64_t)i * m + j;
            ++done;
            if (pr.n == DET_MAXK || done == npair) {      // DET_MAXK pairs to a launch, the rest to the last one
                DetSum sum;
                MCPM_TRY(mcpm_det_begin(p, DET_MAXK, nb, &sum));
                schur_sums_kernel<<<nb, 256, 0, p->stream>>>(B, n, ldb, D, eps_diag, pr, sum.P);
                MCPM_LAUNCH_CHECK(p, "schur_sums_kernel");
                outs.accumulate = DET_STORE;
                MCPM_TRY(mcpm_det_fold(p, sum, pr.n, 1.0, outs));
                pr = SchurPairs{};
                outs = DetOuts{};
            }
        }
    }
    schur_mirror_kernel<<<1, 256, 0, p->stream>>>(out, m);
    MCPM_LAUNCH_CHECK(p, "schur_mirror_kernel");
    return MCPM_OK;
}

}  // extern "C"
