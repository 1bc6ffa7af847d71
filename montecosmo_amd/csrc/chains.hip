// Chain diagnostics: per-dimension moments and integrated autocorrelation time of MCMC draws x[c, t, d], the device half of
// numpyro.diagnostics' effective_sample_size / gelman_rubin as montecosmo/metrics.py:562-579 uses them (chains.py holds the formulas).
//
// Addressing.  Element (c, p, t, d) is x[offset0 + c stride_chain + p stride_part + t stride_draw + d], strides in elements, d contiguous;
// a SEGMENT is a pair (c, p), numbered c n_part + p.  Whole chains are n_part = 1, the halves of split R-hat n_part = 2, the blocks of
// `thin` n_part = number of blocks.  Every index is 64-bit.
//
// Layout of the work.  One lane owns one dimension d; consecutive lanes hold consecutive d, so every load of a wave is one contiguous run.
// Everything is float64 from the float32 input (the cast is exact).  A dimension's result is formed by its lane alone, in an order fixed
// by (n_seg, n_draw, bias): no atomics, no LDS, no cross-lane sum.  So every output is bitwise reproducible and does not depend on n_dim,
// on where the dimension sits, on the alignment of x or on what the neighbouring lanes hold.
//
// Moments: two sweeps over the draws of a segment, as numpy.var makes them: the mean, then the centred sum of squares.
//
// tau: the autocovariance sums S(k) = sum_seg sum_t y[t] y[t + k] (y = x - mean of the segment) are made TAU_K lags per sweep.  A sweep
// walks u = k0 .. N - 1 and keeps the window w[i] = y[u - k0 - i], i < TAU_K (zero before the start of the segment), so S(k0 + i) += w[i] y[u]
// receives its products in the order t = 0, 1, ..: the products with the zero padding add +-0 to a sum that starts at +0 and never show.
// The window and the accumulators are plain arrays under full unrolling (static indices: registers, no scratch).  After a sweep the lane
// turns its TAU_K / 2 pair sums P_j = rho(2j) + rho(2j+1) into Geyer's initial monotone sequence; a lane that meets P_j <= 0 (j >= 1) freezes its
// tau and its count of lags.  The sweeps go on while a ballot finds an unfinished lane in the wave, and never past the N_even / 2 pairs
// that exist: a NaN compares false forever and runs to that bound.  A frozen lane's later sums are never read, so neither TAU_K nor the
// point of the vote shows in any output bit.
#include "mcpm_internal.h"

namespace {

constexpr int TAU_K = 16;       // lags per sweep (even: pairs do not straddle sweeps)
constexpr int CH_BLOCK = 256;

struct ChainArgs {
    const float *x;
    long long offset0, n_dim, stride_chain, stride_part, stride_draw, n_draw;
    int n_chain, n_part;
};

__device__ __forceinline__ const float *segment_base(const ChainArgs &a, int seg) {
    const long long c = seg / a.n_part, p = seg - c * a.n_part;
    return a.x + a.offset0 + c * a.stride_chain + p * a.stride_part;
}

__global__ __launch_bounds__(CH_BLOCK) void chain_moments_kernel(ChainArgs a, double *__restrict__ mean, double *__restrict__ m2) {
    const long long d = (long long)blockIdx.x * CH_BLOCK + threadIdx.x;
    if (d >= a.n_dim) return;
    const int seg = blockIdx.y;
    const float *p = segment_base(a, seg) + d;
    const long long n = a.n_draw, sd = a.stride_draw;
    double s = 0.;
#pragma unroll 8
    for (long long t = 0; t < n; ++t) s += (double)p[t * sd];
    const double m = s / (double)n;
    double q = 0.;
#pragma unroll 8
    for (long long t = 0; t < n; ++t) {
        const double y = (double)p[t * sd] - m;
        q += y * y;
    }
    mean[(long long)seg * a.n_dim + d] = m;
    m2[(long long)seg * a.n_dim + d] = q;
}

__global__ __launch_bounds__(CH_BLOCK) void chain_tau_kernel(ChainArgs a, const double *__restrict__ mean, const double *__restrict__ m2,
                                                             int bias, double *__restrict__ tau, int *__restrict__ n_lags) {
    const long long d0 = (long long)blockIdx.x * CH_BLOCK + threadIdx.x;
    const bool live = d0 < a.n_dim;
    const long long d = live ? d0 : a.n_dim - 1;      // idle lanes of the last wave redo its last dimension and store nothing
    const int n_seg = a.n_chain * a.n_part;
    const long long N = a.n_draw, sd = a.stride_draw;
    const long long n_even = N - (N & 1);

    // W = mean of the segments' variances, V = W (N - 1) / N + the variance of their means (ddof 1); one segment: W = V
    double sv = 0., sm = 0.;
    for (int s = 0; s < n_seg; ++s) {
        sv += m2[(long long)s * a.n_dim + d] / (double)(N - 1);
        sm += mean[(long long)s * a.n_dim + d];
    }
    double W = sv / (double)n_seg, V = W * (double)(N - 1) / (double)N;
    if (n_seg > 1) {
        const double mm = sm / (double)n_seg;
        double b = 0.;
        for (int s = 0; s < n_seg; ++s) {
            const double e = mean[(long long)s * a.n_dim + d] - mm;
            b += e * e;
        }
        V += b / (double)(n_seg - 1);
    } else {
        W = V;
    }

    double sum = 0., run_min = 0.;      // sum of the pair terms so far; the running minimum of max(P_j, 0), j >= 1
    long long lags = n_even;            // lags summed: 2 (j_stop + 1), or all of them
    bool done = false;

    for (long long k0 = 0; k0 < n_even; k0 += TAU_K) {
        double acc[TAU_K];
#pragma unroll
        for (int i = 0; i < TAU_K; ++i) acc[i] = 0.;
        for (int s = 0; s < n_seg; ++s) {
            const float *p = segment_base(a, s) + d;
            const double m = mean[(long long)s * a.n_dim + d];
            double w[TAU_K];
#pragma unroll
            for (int i = 0; i < TAU_K; ++i) w[i] = 0.;
            long long u = k0;
            for (; u + TAU_K <= N; u += TAU_K) {      // TAU_K steps at once: the shifts become register names
                double z[TAU_K], wn[TAU_K];
#pragma unroll
                for (int r = 0; r < TAU_K; ++r) {
                    z[r] = (double)p[(u + r) * sd] - m;
                    wn[r] = (double)p[(u + r - k0) * sd] - m;
                }
#pragma unroll
                for (int r = 0; r < TAU_K; ++r) {
#pragma unroll
                    for (int i = TAU_K - 1; i > 0; --i) w[i] = w[i - 1];
                    w[0] = wn[r];
#pragma unroll
                    for (int i = 0; i < TAU_K; ++i) acc[i] += w[i] * z[r];
                }
            }
            for (; u < N; ++u) {
                const double z = (double)p[u * sd] - m, wn = (double)p[(u - k0) * sd] - m;
#pragma unroll
                for (int i = TAU_K - 1; i > 0; --i) w[i] = w[i - 1];
                w[0] = wn;
#pragma unroll
                for (int i = 0; i < TAU_K; ++i) acc[i] += w[i] * z;
            }
        }
        // the pairs of this sweep
#pragma unroll
        for (int i = 0; i < TAU_K; i += 2) {
            const long long k = k0 + i, j = k >> 1;
            if (k < n_even && !done) {
                const double n0 = bias ? (double)N : (double)(N - k), n1 = bias ? (double)N : (double)(N - k - 1);
                const double g0 = acc[i] / ((double)n_seg * n0), g1 = acc[i + 1] / ((double)n_seg * n1);
                const double r0 = k == 0 ? 1. : 1. - (W - g0) / V, r1 = 1. - (W - g1) / V;
                const double P = r0 + r1;
                if (j == 0) {
                    sum = P;
                } else if (P <= 0.) {
                    done = true;
                    lags = 2 * (j + 1);
                } else {      // (a NaN comes here, and stays)
                    run_min = (j == 1 || P < run_min || P != P) ? P : run_min;
                    sum += run_min;
                }
            }
        }
        if (__ballot(live && !done) == 0ull) break;
    }
    if (live) {
        tau[d] = -1. + 2. * sum;
        n_lags[d] = (int)(lags < n_even ? lags : n_even);
    }
}

int chain_args(const char *who, const float *x, int64_t offset0, int64_t n_dim, int n_chain, int64_t stride_chain, int n_part,
               int64_t stride_part, int64_t n_draw, int64_t stride_draw, ChainArgs *a) {
    const std::string w(who);
    if (!x) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": null pointer");
    if (n_dim < 1 || n_chain < 1 || n_part < 1 || n_draw < 1) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": need n_dim, n_chain, n_part, n_draw >= 1");
    if ((int64_t)n_chain * n_part > 65535) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": at most 65535 segments");
    if (n_dim > (int64_t)CH_BLOCK * 0x7fffffff) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": n_dim out of range");
    if (offset0 < 0 || stride_chain < 0 || stride_part < 0 || stride_draw < 0) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": negative offset or stride");
    a->x = x;
    a->offset0 = offset0;
    a->n_dim = n_dim;
    a->stride_chain = stride_chain;
    a->stride_part = stride_part;
    a->stride_draw = stride_draw;
    a->n_draw = n_draw;
    a->n_chain = n_chain;
    a->n_part = n_part;
    return MCPM_OK;
}

}  // namespace

extern "C" {

int mcpm_chain_moments_f32(void *stream, const float *x, int64_t offset0, int64_t n_dim, int n_chain, int64_t stride_chain, int n_part,
                           int64_t stride_part, int64_t n_draw, int64_t stride_draw, double *mean, double *m2) {
    ChainArgs a;
    MCPM_TRY(chain_args("mcpm_chain_moments_f32", x, offset0, n_dim, n_chain, stride_chain, n_part, stride_part, n_draw, stride_draw, &a));
    if (!mean || !m2) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_chain_moments_f32: null pointer");
    const dim3 grid((unsigned)((n_dim + CH_BLOCK - 1) / CH_BLOCK), (unsigned)(n_chain * n_part));
    chain_moments_kernel<<<grid, CH_BLOCK, 0, (hipStream_t)stream>>>(a, mean, m2);
    MCPM_LAUNCH_CHECK(nullptr, "chain_moments_kernel");
    return MCPM_OK;
}

int mcpm_chain_tau_f32(void *stream, const float *x, int64_t offset0, int64_t n_dim, int n_chain, int64_t stride_chain, int n_part,
                       int64_t stride_part, int64_t n_draw, int64_t stride_draw, const double *mean, const double *m2, int bias, double *tau,
                       unsigned *n_lags) {
    ChainArgs a;
    MCPM_TRY(chain_args("mcpm_chain_tau_f32", x, offset0, n_dim, n_chain, stride_chain, n_part, stride_part, n_draw, stride_draw, &a));
    if (!mean || !m2 || !tau || !n_lags) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_chain_tau_f32: null pointer");
    if (n_draw < 2) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_chain_tau_f32: need n_draw >= 2");
    if (n_draw > 0x3fffffff) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_chain_tau_f32: n_draw out of range");
    const unsigned grid = (unsigned)((n_dim + CH_BLOCK - 1) / CH_BLOCK);
    chain_tau_kernel<<<grid, CH_BLOCK, 0, (hipStream_t)stream>>>(a, mean, m2, bias, tau, (int *)n_lags);
    MCPM_LAUNCH_CHECK(nullptr, "chain_tau_kernel");
    return MCPM_OK;
}

}  // extern "C"
