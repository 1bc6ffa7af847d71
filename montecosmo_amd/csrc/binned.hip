// Binned real-space sums: the np.digitize / np.bincount of montecosmo/metrics.py:bin_and_aggregate (:214-256) in one streaming pass
// over flat arrays of n cells, float64 sums, bitwise reproducible (no floating-point atomics).  Per interior bin: the count, the
// sum of the binning values and, for every batch row, the sum of a target: t0 (plain mode) or (t0 - t1)^2 scale (squared-error mode).
//
// Layout of the work.  A wave owns a contiguous range of cells (a multiple of 256) and walks it in steps of 256 cells = four rounds of
// 64 consecutive cells, lane l of round j holding cell base + 64 j + l (consecutive cells are neighbours along z, so a round of radial
// shells holds few distinct bins).  When every pointer is 16-byte aligned a whole step is loaded with one 16-byte load per lane and
// array (cells base + 4 l .. 4 l + 3) and transposed across the wave (pick4); otherwise, and for the last cells of a range, every
// lane loads its four cells one by one.  Both leave THE SAME cells in the same lanes, so the sums do not know which path ran.
// Neither radii nor cell values are monotone along a row, so the lanes of one bin are scattered over the round and spectrum.hip's
// segmented scan (contiguous segments) does not apply.  Instead a round looks at its distinct bins one after the other: the bin of
// the first unserved lane is read into a scalar register and a ballot finds the lanes that hold it.  A CROWDED bin (BIN_TREE_MIN lanes
// or more: radial shells across the line of sight) is summed at once: its lanes contribute their terms to reduce_dev.h's wave_sum and
// the others +0.0, and lane 63 adds the sums to the wave's own LDS histogram with a plain read-modify-write.  A THIN bin (shells along
// the line of sight, quantile bins of a random field: tens of distinct bins in a round) only has its lanes numbered; after the loop the
// thin bins are served together, step s letting the s-th lane of each add its own terms to the histogram: the lanes of a step hold
// distinct bins, so their read-modify-writes do not meet, and a bin receives its terms in lane order.  Which way a bin goes depends on
// the round's cells alone.  Rounds follow in program order, so every histogram cell is a fixed-order sum whichever load path ran.  The
// four waves' histograms are added in a fixed tree, the workgroup writes its partials P[g][blk][acc][bin] (reduce_dev.h: hist4_partials),
// and mcpm_fold_partials (reduce.hip) adds the workgroups in a fixed order, as for spectrum.hip, and scatters a group's accumulators to
// out[2 + batch][n_bins] (fold_binned).
//
// The ranges depend on n and on the number of edges only.  A workgroup takes up to BIN_ROWS batch rows through the rounds together
// (they share the bins, the ballots, the count and the sum of values); a row's own sums see the same terms in the same order whether
// it runs alone or with others, so a batch row is bitwise the single call.
//
// Bin assignment is np.digitize(values, edges) (right=False) restated exactly: the value goes to double (exact for float32), the bin
// is the count of edges <= value by bisection over the edges in LDS; counts 0 and n_edges are dropped, a NaN compares false with every
// edge and is dropped with count 0.  Edges may repeat (an empty bin).  No arithmetic feeds a comparison, so there is nothing to contract.
#include <algorithm>
#include <cmath>

#include "mcpm_internal.h"
#include "reduce_dev.h"

namespace {

constexpr int BIN_WAVES = 4;            // waves per workgroup, one LDS histogram each
constexpr int BIN_ROWS = 4;             // batch rows a workgroup takes together (1 when the batch has one or two rows)
constexpr int BIN_HIST_DOUBLES = 4096;  // 32 KB of histograms per workgroup: BIN_WAVES * n_acc * bins-per-tile <= this; the edges take up to 32 KB more
constexpr int BIN_STEP = 256;           // cells a wave takes per step (4 per lane)
constexpr int BIN_TREE_MIN = 16;        // lanes of a round in one bin from which the bin is tree-summed (at most 4 such bins in a round)

struct BinArgs {
    const void *values;         // [n] float or double
    const float *t0, *t1;       // [B][n] targets; t1 NULL: plain mode
    long long st0, st1;         // batch strides in elements (0: the same array for every row)
    const unsigned char *mask;  // [n] or NULL; 0 = skip the cell
    const double *edges;        // [n_edges] device
    double scale;
    long long n, cells_per_wave;
    int n_edges, n_bins, batch;
    int n_acc, bt;              // accumulators of a workgroup (2 + rows); bins per tile (gridDim.z tiles)
    unsigned nblk;
    double *P;                  // [groups][nblk][n_acc][n_bins]
};

// count of edges <= v (np.digitize, right=False); NaN -> 0
__device__ __forceinline__ int digitize(const double *ed, int n_edges, double v) {
    int lo = 0, len = n_edges;
    while (len > 0) {
        const int half = len >> 1;
        if (ed[lo + half] <= v) lo += half + 1, len -= half + 1;
        else len = half;
    }
    return lo;
}

// Component k of the four values that lane `src` holds (the transposition after a 16-byte load: four ds_bpermute and three selects).
template <typename T>
__device__ __forceinline__ T pick4(const T (&c)[4], int src, int k) {
    const T a0 = __shfl(c[0], src), a1 = __shfl(c[1], src), a2 = __shfl(c[2], src), a3 = __shfl(c[3], src);
    return k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
}

template <typename VT, int RB, bool VEC>
__global__ __launch_bounds__(64 * BIN_WAVES) void binned_sums_kernel(BinArgs a) {
    extern __shared__ double lds[];      // edges [n_edges], then hist [BIN_WAVES][n_acc][bt]
    double *ed = lds, *hist = lds + a.n_edges;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned blk = blockIdx.x;
    const int g = blockIdx.y, tile0 = blockIdx.z * a.bt, nbt = min(a.bt, a.n_bins - tile0);
    const int hsz = a.n_acc * a.bt;
    for (int i = threadIdx.x; i < a.n_edges; i += blockDim.x) ed[i] = a.edges[i];
    for (int i = threadIdx.x; i < BIN_WAVES * hsz; i += blockDim.x) hist[i] = 0.;
    __syncthreads();
    double *h = hist + wave * hsz;
    const VT *val = static_cast<const VT *>(a.values);
    const bool sq = a.t1 != nullptr;
    const float *p0[RB], *p1[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int row = min(g * RB + r, a.batch - 1);      // a short last group repeats the last row; the fold drops the copies
        p0[r] = a.t0 + row * a.st0;
        p1[r] = sq ? a.t1 + row * a.st1 : nullptr;
    }
    const long long c0 = ((long long)blk * BIN_WAVES + wave) * a.cells_per_wave;
    const long long c1 = min(c0 + a.cells_per_wave, a.n);

    for (long long base = c0; base < c1; base += BIN_STEP) {
        // what round j needs in this lane: cell base + 64 j + lane
        double v[4];
        float x0[RB][4], x1[RB][4];
        unsigned on = 0;      // bit j: that cell exists and is not masked out
        if (VEC && base + BIN_STEP <= c1) {      // a whole step: 16-byte loads of cells base + 4 lane .. + 3, handed to their rounds' lanes
            const long long i0 = base + 4 * lane;
            VT lv[4];
            float l0[RB][4], l1[RB][4];
            if constexpr (sizeof(VT) == 8) {
                const double2 lo = reinterpret_cast<const double2 *>(val + i0)[0], hi = reinterpret_cast<const double2 *>(val + i0)[1];
                lv[0] = lo.x, lv[1] = lo.y, lv[2] = hi.x, lv[3] = hi.y;
            } else {
                const float4 f = *reinterpret_cast<const float4 *>(val + i0);
                lv[0] = f.x, lv[1] = f.y, lv[2] = f.z, lv[3] = f.w;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float4 f = *reinterpret_cast<const float4 *>(p0[r] + i0);
                l0[r][0] = f.x, l0[r][1] = f.y, l0[r][2] = f.z, l0[r][3] = f.w;
                const float4 e = sq ? *reinterpret_cast<const float4 *>(p1[r] + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
                l1[r][0] = e.x, l1[r][1] = e.y, l1[r][2] = e.z, l1[r][3] = e.w;
            }
            const unsigned lm = a.mask ? *reinterpret_cast<const unsigned *>(a.mask + i0) : 0x01010101u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int src = 16 * j + (lane >> 2), k = lane & 3;      // cell 64 j + lane of the step sits in lane src, component k
                v[j] = (double)pick4(lv, src, k);
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    x0[r][j] = pick4(l0[r], src, k);
                    x1[r][j] = sq ? pick4(l1[r], src, k) : 0.f;
                }
                if ((__shfl(lm, src) >> (8 * k)) & 0xffu) on |= 1u << j;
            }
        } else {      // unaligned pointers, or the last cells of the range: one load per cell
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long i = base + 64 * j + lane;
                const bool in = i < c1;
                v[j] = in ? (double)val[i] : 0.;
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    x0[r][j] = in ? p0[r][i] : 0.f;
                    x1[r][j] = in && sq ? p1[r][i] : 0.f;
                }
                if (in && (!a.mask || a.mask[i])) on |= 1u << j;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool live = (on >> j) & 1u;
            const int key = live ? digitize(ed, a.n_edges, v[j]) - 1 : -1;      // bin index; -1 and n_bins: outside the edges
            const int tk = key >= tile0 && key < tile0 + nbt ? key - tile0 : -1;      // bin within this tile, or -1: dropped
            double term[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const double d = (double)x0[r][j] - (double)x1[r][j];
                term[r] = sq ? (d * d) * a.scale : (double)x0[r][j];
            }
            unsigned long long pend = __ballot(tk >= 0);
            int rank = -1, cnt = 0, steps = 0;      // of a lane whose bin is served lane by lane: its place among the bin's lanes, their number
            while (pend) {      // once per distinct bin of the round; `pend` is a ballot, so the branches are uniform and every lane stays active
                const int kb = __builtin_amdgcn_readlane(tk, __ffsll((long long)pend) - 1);
                const bool mine = tk == kb;
                const unsigned long long mm = __ballot(mine);
                const int c = __popcll(mm);
                if (c >= BIN_TREE_MIN) {      // a crowded bin: one tree sum per accumulator, one lane adds it
                    const double sv = wave_sum(mine ? v[j] : 0.);
                    double st[RB];
#pragma unroll
                    for (int r = 0; r < RB; ++r) st[r] = wave_sum(mine ? term[r] : 0.);
                    if (lane == 63) {
                        h[kb] += (double)c;
                        h[a.bt + kb] += sv;
#pragma unroll
                        for (int r = 0; r < RB; ++r) h[(2 + r) * a.bt + kb] += st[r];
                    }
                } else {      // a thin bin: only note each lane's place; the bins are served together below
                    if (mine) rank = __popcll(mm & ((1ull << lane) - 1ull)), cnt = c;
                    steps = max(steps, c);
                }
                pend &= ~mm;
            }
            // thin bins, all at once: in step s the s-th lane of every such bin adds its own terms.  The lanes of a step hold distinct
            // bins, so the read-modify-writes do not meet, and a bin's terms arrive in lane order.
            for (int s = 0; s < steps; ++s)
                if (rank == s) {
                    if (s == 0) h[tk] += (double)cnt;
                    h[a.bt + tk] += v[j];
#pragma unroll
                    for (int r = 0; r < RB; ++r) h[(2 + r) * a.bt + tk] += term[r];
                }
        }
    }
    __syncthreads();
    hist4_partials(hist, hsz, a.n_acc, a.bt, tile0, nbt, a.P, g, a.nblk, blk, a.n_bins);
}

struct BinLayout {
    int rb, groups, n_acc, n_bins, bt, tiles;
    long long cells_per_wave;
    unsigned nblk;
    size_t off_edges, off_P, off_Q, bytes;
};

int bin_layout(int64_t n, int n_edges, int batch, BinLayout *L) {
    if (n < 1) return mcpm_fail(nullptr, MCPM_E_SHAPE, "mcpm_binned: need n >= 1 cells");
    if (n_edges < 2 || n_edges > MCPM_BINNED_MAX_EDGES) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_binned: need 2 .. MCPM_BINNED_MAX_EDGES edges");
    MCPM_TRY(mcpm_check_batch("mcpm_binned", batch));
    L->rb = batch >= 3 ? BIN_ROWS : 1;
    L->groups = (batch + L->rb - 1) / L->rb;
    L->n_acc = 2 + L->rb;
    L->n_bins = n_edges - 1;
    mcpm_hist_tiles(L->n_bins, BIN_HIST_DOUBLES, BIN_WAVES, L->n_acc, &L->bt, &L->tiles);
    // workgroups and cell ranges from n and n_edges alone (never the batch): fewer when a row's partials would pass 32 MB
    const int64_t per = (int64_t)BIN_WAVES * BIN_STEP;
    const int64_t nblk = mcpm_fold_nblk((int64_t)1 << 22, 3 * (int64_t)L->n_bins, (n + per - 1) / per);
    int64_t cpw = (n + nblk * BIN_WAVES - 1) / (nblk * BIN_WAVES);
    cpw = (cpw + BIN_STEP - 1) / BIN_STEP * BIN_STEP;
    L->cells_per_wave = cpw;
    L->nblk = (unsigned)((n + cpw * BIN_WAVES - 1) / (cpw * BIN_WAVES));
    Carve c;
    L->off_edges = c.take((size_t)n_edges * 8);
    mcpm_fold_carve(c, L->groups, L->nblk, (size_t)L->n_acc * L->n_bins, &L->off_P, &L->off_Q);
    L->bytes = c.bytes;
    return MCPM_OK;
}

template <typename VT, int RB>
void launch_bins(const BinArgs &a, const BinLayout &L, bool vec, hipStream_t s) {
    const dim3 grid(L.nblk, L.groups, L.tiles);
    const size_t lds = ((size_t)a.n_edges + (size_t)BIN_WAVES * L.n_acc * L.bt) * 8;
    if (vec)
        binned_sums_kernel<VT, RB, true><<<grid, 64 * BIN_WAVES, lds, s>>>(a);
    else
        binned_sums_kernel<VT, RB, false><<<grid, 64 * BIN_WAVES, lds, s>>>(a);
}

}  // namespace

extern "C" {

int mcpm_binned_workspace(int64_t n, int n_edges, int batch, int64_t *bytes) {
    if (!bytes) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_binned_workspace: null output");
    BinLayout L;
    MCPM_TRY(bin_layout(n, n_edges, batch, &L));
    *bytes = (int64_t)L.bytes;
    return MCPM_OK;
}

int mcpm_binned_sums_f32(void *stream, int64_t n, const void *values, int values_f64, const float *t0, int64_t stride0, const float *t1,
                         int64_t stride1, double scale, const unsigned char *mask, int batch, const double *edges, int n_edges, void *work,
                         int64_t work_bytes, double *out) {
    BinLayout L;
    MCPM_TRY(bin_layout(n, n_edges, batch, &L));
    if (!values || !t0 || !edges || !work || !out) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_binned_sums_f32: null pointer");
    if (work_bytes < (int64_t)L.bytes) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_binned_sums_f32: workspace too small");
    if (stride0 < 0 || stride1 < 0) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_binned_sums_f32: negative stride");
    MCPM_TRY(mcpm_check_edges("mcpm_binned_sums_f32", edges, n_edges, false));
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)work;
    double *dev_edges = (double *)(ws + L.off_edges);
    MCPM_HIP(nullptr, hipMemcpyAsync(dev_edges, edges, (size_t)n_edges * 8, hipMemcpyHostToDevice, s));
    MCPM_HIP(nullptr, hipStreamSynchronize(s));      // the caller's edges may die on return

    BinArgs a{};
    a.values = values;
    a.t0 = t0;
    a.t1 = t1;
    a.st0 = stride0;
    a.st1 = t1 ? stride1 : 0;
    a.mask = mask;
    a.edges = dev_edges;
    a.scale = scale;
    a.n = n;
    a.cells_per_wave = L.cells_per_wave;
    a.n_edges = n_edges;
    a.n_bins = L.n_bins;
    a.batch = batch;
    a.n_acc = L.n_acc;
    a.bt = L.bt;
    a.nblk = L.nblk;
    a.P = (double *)(ws + L.off_P);
    // 16-byte loads when every pointer (and every batch row) allows; the order of the sums is the same on either path
    const bool vec = mcpm_aligned(values) && mcpm_aligned(t0) && mcpm_aligned(t1) && mcpm_aligned(mask, 4) && stride0 % 4 == 0 && a.st1 % 4 == 0;
    if (values_f64) {
        if (L.rb == 1) launch_bins<double, 1>(a, L, vec, s);
        else launch_bins<double, BIN_ROWS>(a, L, vec, s);
    } else {
        if (L.rb == 1) launch_bins<float, 1>(a, L, vec, s);
        else launch_bins<float, BIN_ROWS>(a, L, vec, s);
    }
    MCPM_LAUNCH_CHECK(nullptr, "binned_sums_kernel");
    return mcpm_fold_partials(s, a.P, L.groups, L.nblk, L.n_acc * L.n_bins, (double *)(ws + L.off_Q), fold_binned(out, L.n_bins, L.rb, batch));
}

}  // extern "C"
