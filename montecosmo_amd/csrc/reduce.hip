// Second stages kept in one place: the fold of the deterministic f64 grid sums (first stage: reduce_dev.h) with its scratch and launcher, the
// fold of the binned statistics' workgroup partials (first stages: spectrum.hip, binned.hip, bispectrum.hip), and the host side of the
// order-independent integer table sums (device side: tables_dev.h) with its scale kernel.
//
// The two folds.  mcpm_det_begin / mcpm_det_fold add up at most DET_MAXK values per call: scratch that grows with the plan, ONE launch whose
// last workgroup (a ticket) finishes the sum, a scale and an accumulate flag on the way out.  mcpm_fold_partials adds up many outputs per
// group (a histogram per batch row): no plan and no ticket, the caller's workspace holds P and Q, and two launches with one lane per output
// walk the workgroups in increasing order, so an output is a fixed-order sum whatever the batch.
#include <algorithm>

#include "mcpm_internal.h"
#include "reduce_dev.h"

constexpr unsigned DET_MAXR = 128;      // most workgroups a fold is launched with

// plan->part: [ticket (one unsigned in a double's slot, zero between launches)] [Q: K * DET_MAXR second-level sums] [P: K * nblk partials]
static unsigned *det_ticket(const mcpm_plan *p) { return reinterpret_cast<unsigned *>(p->part); }
static double *det_Q(const mcpm_plan *p) { return p->part + 1; }
// Workgroups of the fold.  Few: each ends with one atomic on the shared ticket, and those serialise at ~27 ns apiece (1024 of them:
// 34 us per fold at 512^3, against 23 us with 256); 128 workgroups still pull 12.6 MB of partials in a few microseconds.
static unsigned det_R(unsigned nblk) { return std::max(1u, std::min(DET_MAXR, (nblk + 511u) / 512u)); }

// R workgroups each sum a contiguous range of every row of P into Q[k * R + r]; the last one to finish (the ticket) sums Q and writes the
// outputs, then zeroes the ticket for the next launch (which is what lets a captured graph replay a fold).  K <= DET_MAXK,
// R <= DET_MAXR.
// (The last workgroup's sum over Q is a fixed TREE over 256 lanes, not a serial loop: 256 dependent-latency loads by one lane cost
// 43 us at 256^3 and 55 us at 512^3 -- `profiles/r04_kernel_stats_*.csv` of the first version -- against 5 us for everything else.)
__global__ __launch_bounds__(256) void det_fold_kernel(const double *__restrict__ P, unsigned nblk, int K, double *Q, unsigned *ticket, double scale,
                                                       DetOuts o) {
    const unsigned R = gridDim.x, r = blockIdx.x, C = (nblk + R - 1) / R, lo = r * C, hi = min(lo + C, nblk);
    __shared__ double sh[DET_MAXK][4];
    __shared__ int last;
    for (int k = 0; k < K; ++k) {
        // eight independent loads in flight per lane, added in a fixed pattern (one load per iteration is a chain of memory latencies:
        // 29 us per fold at 512^3, 16 iterations x 3 rows)
        const double *Pk = P + (size_t)k * nblk;
        double t = 0.;
        for (unsigned i = lo + threadIdx.x; i < hi; i += 256 * 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = i + 256u * j < hi ? Pk[i + 256u * j] : 0.;
            t += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
        t = wave_sum(t);
        if ((threadIdx.x & 63) == 63) sh[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) Q[(size_t)threadIdx.x * R + r] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(ticket, 1u) == R - 1u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    for (int k = 0; k < K; ++k) {      // lane i holds Q[k][i] (+ Q[k][i + 256] ..., in that order); the same DPP tree and wave order as above
        double t = 0.;
        for (unsigned i = threadIdx.x; i < R; i += 256) t += __hip_atomic_load(Q + (size_t)k * R + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = wave_sum(t);
        if ((threadIdx.x & 63) == 63) sh[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const double t = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
        double *dst = o.p[threadIdx.x];
        if (dst) *dst = (o.accumulate ? *dst : 0.) + scale * t;
    }
    if (threadIdx.x == 0) *ticket = 0u;
}

int mcpm_det_begin(mcpm_plan *p, int K, unsigned nblk, DetSum *s) {
    MCPM_REQUIRE(p, K >= 1 && K <= DET_MAXK, MCPM_E_ARG, "deterministic sum: bad row count");
    const int64_t need = 1 + (int64_t)K * DET_MAXR + (int64_t)K * nblk;
    if (p->part_n < need) {
        if (p->part) {
            MCPM_HIP(p, hipStreamSynchronize(p->stream));
            (void)hipFree(p->part);
            p->part = nullptr;
            p->part_n = 0;
        }
        const int64_t n = need + need / 4;
        if (hipMalloc((void **)&p->part, sizeof(double) * n) != hipSuccess) return mcpm_fail(p, MCPM_E_NOMEM, "reduction scratch");
        p->part_n = n;
        p->det_stale = 1;      // fresh memory: the ticket starts at zero
    }
    if (p->det_stale) {      // a HIP error since the last sum (mcpm_fail): a fold may have stopped short of resetting its ticket
        MCPM_HIP(p, hipMemsetAsync(det_ticket(p), 0, sizeof(unsigned), p->stream));
        p->det_stale = 0;
    }
    s->P = det_Q(p) + (int64_t)K * DET_MAXR;
    s->nblk = nblk;
    return MCPM_OK;
}

int mcpm_det_fold(mcpm_plan *p, const DetSum &s, int K, double scale, const DetOuts &outs) {
    det_fold_kernel<<<det_R(s.nblk), 256, 0, p->stream>>>(s.P, s.nblk, K, det_Q(p), det_ticket(p), scale, outs);
    MCPM_LAUNCH_CHECK(p, "det_fold_kernel");      // on failure mcpm_fail marks the ticket stale
    return MCPM_OK;
}

// ---- the fold of workgroup partials P[group][nblk][nout] (mcpm_internal.h: mcpm_fold_partials) -----------------------------------------
// First level: Q[g][r][o] = sum over workgroups [r C, min((r + 1) C, nblk)) of P[g][i][o], C = ceil(nblk / MCPM_FOLD_R), from 0. in
// increasing i (an empty chunk leaves +0.0).
__global__ __launch_bounds__(256) void partial_fold_kernel(const double *__restrict__ P, unsigned nblk, int nout, double *__restrict__ Q) {
    const int o = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, g = blockIdx.z;
    if (o >= nout) return;
    const unsigned C = (nblk + MCPM_FOLD_R - 1) / MCPM_FOLD_R, lo = r * C, hi = min(lo + C, nblk);
    const double *Pg = P + (size_t)g * nblk * nout + o;
    double t = 0.;
    for (unsigned i = lo; i < hi; ++i) t += Pg[(size_t)i * nout];
    Q[((size_t)g * MCPM_FOLD_R + r) * nout + o] = t;
}

// Second level: the sum over r of Q[g][r][o], from 0. in increasing r, written where `f` says (FoldOut).  In the binned form every group
// holds the same bits in accumulators 0 and 1 (count and sum of values), and a short last group holds copies of the last row: both are dropped.
__global__ __launch_bounds__(256) void partial_fold2_kernel(const double *__restrict__ Q, int nout, FoldOut f) {
    const int o = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (o >= nout) return;
    const double *Qg = Q + (size_t)g * MCPM_FOLD_R * nout + o;
    double t = 0.;
    for (int r = 0; r < MCPM_FOLD_R; ++r) t += Qg[(size_t)r * nout];
    if (f.n_bins == 0) {
        f.out[(size_t)g * nout + o] = t;
        return;
    }
    const int acc = o / f.n_bins, j = o - acc * f.n_bins;
    if (acc < 2) {
        if (g == 0) f.out[(size_t)acc * f.n_bins + j] = t;
    } else {
        const int row = g * f.rb + acc - 2;
        if (row < f.batch) f.out[(size_t)(2 + row) * f.n_bins + j] = t;
    }
}

int mcpm_fold_partials(hipStream_t s, const double *P, int groups, unsigned nblk, int nout, double *Q, const FoldOut &o) {
    const unsigned nx = (unsigned)((nout + 255) / 256);
    partial_fold_kernel<<<dim3(nx, MCPM_FOLD_R, groups), 256, 0, s>>>(P, nblk, nout, Q);
    MCPM_LAUNCH_CHECK(nullptr, "partial_fold_kernel");
    partial_fold2_kernel<<<dim3(nx, groups), 256, 0, s>>>(Q, nout, o);
    MCPM_LAUNCH_CHECK(nullptr, "partial_fold2_kernel");
    return MCPM_OK;
}

// ---- the order-independent integer table sums (the rule: tables_dev.h, ORDER-INDEPENDENT SUMS) ----------------------------------------
// out[i] = integer sum scaled back by its kind's 2^(e - 30); e0 .. e3: one past the last entry of kinds 0 .. 3 (ntot for a kind the sum
// does not have).  A non-finite maximum makes the whole kind NaN.
__global__ void tab_scale_kernel(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ mxbits, int ntot, int e0, int e1,
                                 int e2, int e3, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntot) return;
    const int k = i < e0 ? 0 : (i < e1 ? 1 : (i < e2 ? 2 : (i < e3 ? 3 : 4)));
    const int be = (int)(mxbits[k] >> 23);
    if (be >= 255) { out[i] = __longlong_as_double(0x7ff8000000000000ll); return; }
    out[i] = be == 0 ? 0. : (double)(long long)acc[i] * __longlong_as_double((long long)(1023 - 30 + (be - 126)) << 52);
}

int mcpm_tab_begin(mcpm_plan *p, const char *who, int region, size_t ntot, int64_t nelem, TabSum *t) {
    const bool png = region == MCPM_RED_PNG_ACC;
    MCPM_REQUIRE(p, png || region == MCPM_RED_TABLES, MCPM_E_ARG, std::string(who) + ": not a region of the table sums");
    const size_t cap = png ? MCPM_RED_PNG_NTAB : MCPM_RED_TABLES_END - MCPM_RED_TABLES - MCPM_RED_TAB_TAIL;
    MCPM_REQUIRE(p, ntot <= cap, MCPM_E_ARG, std::string(who) + (png ? ": table exceeds the accumulators" : ": tables exceed the accumulators"));
    // the plan's reduction scratch is free between the model-side calls (the map in mcpm_internal.h)
    t->acc = reinterpret_cast<unsigned long long *>(p->reduce + region);
    t->mx = reinterpret_cast<unsigned *>(t->acc + ntot);
    t->ntot = (int)ntot;
    t->nb = (unsigned)std::min<int64_t>((nelem + 255) / 256, 2048);
    t->lds = ntot * sizeof(unsigned long long);
    MCPM_HIP(p, hipMemsetAsync(t->acc, 0, (ntot + MCPM_RED_TAB_TAIL) * sizeof(double), p->stream));
    return MCPM_OK;
}

int mcpm_tab_finish(mcpm_plan *p, const TabSum &t, const int *kind_end, int nkinds, double *out) {
    static_assert(MCPM_TAB_KINDS == 5, "tab_scale_kernel takes the four inner boundaries of five kinds");
    MCPM_REQUIRE(p, nkinds >= 1 && nkinds <= MCPM_TAB_KINDS && kind_end[nkinds - 1] == t.ntot, MCPM_E_ARG, "table sum: bad kind boundaries");
    int e[MCPM_TAB_KINDS - 1];
    for (int k = 0; k < MCPM_TAB_KINDS - 1; ++k) e[k] = k < nkinds ? kind_end[k] : t.ntot;
    tab_scale_kernel<<<(unsigned)((t.ntot + 255) / 256), 256, 0, p->stream>>>(t.acc, t.mx, t.ntot, e[0], e[1], e[2], e[3], out);
    MCPM_LAUNCH_CHECK(p, "tab_scale_kernel");
    return MCPM_OK;
}
