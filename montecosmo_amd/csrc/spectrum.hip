// Binned power spectra of half-spectra: the bincount of montecosmo/metrics.py:_spectrum (:113-171) in one pass over one or two
// complex64 spectra, float64 sums, bitwise reproducible (no floating-point atomics).
//
// Layout of the work.  A wave owns a contiguous range of (x, y) rows of the half-spectrum and walks each row in rounds of 64
// consecutive kz (lane = kz).  Along a row |k| never decreases with kz, so the lanes of one round that fall into one k bin are
// CONTIGUOUS: a segmented inclusive scan across the wave (DPP row_shr 1/2/4/8, then row_bcast 15/31 -- the tree of reduce_dev.h's
// wave_sum, cut at segment heads) leaves every segment's sum in its last lane, and those lanes hold DISTINCT bins, so they add it to
// the wave's own LDS histogram with a plain read-modify-write.  Rounds follow in program order, so every histogram cell is a
// fixed-order sum.  At the end the four waves' histograms are added in a fixed tree and the workgroup writes its partials
// P[b][blk][acc][bin] (reduce_dev.h: hist4_partials); mcpm_fold_partials (reduce.hip) adds the workgroups up in a fixed order.
// The decomposition depends on the geometry, the number of accumulators and of edges only, never on the batch, so a batched row is
// bitwise the single call.
//
// Bin assignment is np.digitize(|k|, edges) (right=False) restated exactly: |k|^2 = (kx^2 + ky^2) + kz^2 and mu = ((kx lx + ky ly) +
// kz lz) / |k| with contraction OFF (hipcc would fuse them into v_fmac_f64 and move modes that sit on an edge), a correctly rounded
// sqrt and division.  The bin itself comes from kbin_dev.h (shared with bispectrum.hip).
#include <algorithm>
#include <cmath>

#include "mcpm_internal.h"
#include "kbin_dev.h"
#include "reduce_dev.h"

namespace {

constexpr int SPEC_WAVES = 4;          // waves per workgroup, one LDS histogram each
constexpr int SPEC_LDS_DOUBLES = 8192; // 64 KB per workgroup: SPEC_WAVES * n_acc * bins-per-tile <= this

struct SpecArgs {
    const float2 *s0, *s1;  // [B][nx][ny][nzh]; s1 NULL: auto spectrum of s0 only
    long long st0, st1;     // batch strides in complex elements (0: the same spectrum for every batch row)
    const double *kx, *ky, *kz;         // per-axis |k| tables (caller's units)
    const double *dc0, *dc1;            // per-axis deconvolution factors [nx | ny | nzh] per input, or NULL
    const double *dz0, *dz1;            // their kz parts (dc + nx + ny)
    KBinTable kb;                       // edges [n_edges] and their lookup table
    int n_bins;
    double los[3];
    unsigned long long ells;            // 4 bits per multipole, in request order
    int n_ells, lmax, two;
    int nx, ny, nzh;
    int rows, rows_per_wave, rounds_per_row;
    int n_acc, bt;          // accumulators; bins per tile (gridDim.z tiles)
    unsigned nblk;
    double *P;              // [B][nblk][n_acc][n_bins]
};

// Segmented inclusive scan step: v[l] += v[l - s] when lane l - s is in l's segment.  `tm` holds the six step conditions as bits
// (seg_mask); testing them per step keeps them out of long-lived SGPR masks.
template <int CTRL, int ROWMASK, int BIT>
__device__ __forceinline__ double seg_step(double v, int tm) {
    const double s = dpp_shift_d<CTRL, ROWMASK>(v);
    return (tm >> BIT) & 1 ? v + s : v;
}
__device__ __forceinline__ int seg_mask(int lane, int seg) {     // seg = first lane of the lane's segment
    const int r = lane & 15;
    return (r >= 1 && lane - 1 >= seg) | (r >= 2 && lane - 2 >= seg) << 1 | (r >= 4 && lane - 4 >= seg) << 2 |
           (r >= 8 && lane - 8 >= seg) << 3 | (((lane >> 4) & 1) && seg <= (lane & ~15) - 1) << 4 |   // rows 1, 3 <- lane 15, 47
           (lane >= 32 && seg <= 31) << 5;                                                          // rows 2, 3 <- lane 31
}
__device__ __forceinline__ double seg_scan(double v, int tm) {
    v = seg_step<0x111, 0xf, 0>(v, tm);
    v = seg_step<0x112, 0xf, 1>(v, tm);
    v = seg_step<0x114, 0xf, 2>(v, tm);
    v = seg_step<0x118, 0xf, 3>(v, tm);
    v = seg_step<0x142, 0xa, 4>(v, tm);
    v = seg_step<0x143, 0xc, 5>(v, tm);
    return v;
}

// Legendre polynomial P_l(mu) (Bonnet's recurrence; l is uniform across the wave).
__device__ __forceinline__ double legendre(double mu, int l) {
    double p0 = 1., p1 = mu;
    if (l == 0) return p0;
    for (int n = 1; n < l; ++n) {
        const double p2 = ((2 * n + 1) * mu * p1 - n * p0) / (n + 1);
        p0 = p1;
        p1 = p2;
    }
    return p1;
}

template <bool TWO>
__global__ __launch_bounds__(64 * SPEC_WAVES) void spectrum_bins_kernel(SpecArgs a) {
    extern __shared__ double hist[];      // [SPEC_WAVES][n_acc][bt]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned blk = blockIdx.x;
    const int b = blockIdx.y, t0 = blockIdx.z * a.bt, nbt = min(a.bt, a.n_bins - t0);
    const int hsz = a.n_acc * a.bt;
    for (int i = threadIdx.x; i < SPEC_WAVES * hsz; i += blockDim.x) hist[i] = 0.;
    __syncthreads();
    double *h = hist + wave * hsz;
    const float2 *s0 = a.s0 + b * a.st0;
    const float2 *s1 = TWO ? a.s1 + b * a.st1 : nullptr;
    const int row0 = (blk * SPEC_WAVES + wave) * a.rows_per_wave;
    const int row1 = min(row0 + a.rows_per_wave, a.rows);
    const int nacc = a.n_acc;

    // Flat walk over the wave's rounds (row, q), two rounds loaded ahead: one load per lane and spectrum per round is too little
    // in flight to cover the HBM latency.
    struct Rd {
        float2 v0, v1;
        double kz;
    };
    const int rpr = a.rounds_per_row, nround = max(row1 - row0, 0) * rpr;
    auto load = [&](int R) {
        Rd d{make_float2(0.f, 0.f), make_float2(0.f, 0.f), 0.};
        if (R < nround) {
            const int row = row0 + R / rpr, z = (R - (R / rpr) * rpr) * 64 + lane;
            if (z < a.nzh) {
                d.v0 = s0[(size_t)row * a.nzh + z];
                if (TWO) d.v1 = s1[(size_t)row * a.nzh + z];
                d.kz = a.kz[z];
            }
        }
        return d;
    };
    Rd d1 = load(0), d2 = load(1);
    for (int R = 0; R < nround; ++R) {
        const Rd cur = d1;
        d1 = d2;
        d2 = load(R + 2);
        const int row = row0 + R / rpr, q = R - (R / rpr) * rpr;
        const int x = row / a.ny, y = row - x * a.ny;
        const double kx = a.kx[x], ky = a.ky[y];
        double dx0 = 1., dx1 = 1.;
        if (a.dc0) dx0 = a.dc0[x] * a.dc0[a.nx + y];
        if (TWO && a.dc1) dx1 = a.dc1[x] * a.dc1[a.nx + y];
        double kp2, mu_xy;
        {
#pragma clang fp contract(off)
            kp2 = kx * kx + ky * ky;
            mu_xy = kx * a.los[0] + ky * a.los[1];
        }
        {
            const int z = q * 64 + lane;
            const bool in = z < a.nzh;
            const float2 v0 = cur.v0, v1 = cur.v1;
            const double kz = cur.kz;
            double k2, mu_num;
            {
#pragma clang fp contract(off)
                k2 = kp2 + kz * kz;
                mu_num = mu_xy + kz * a.los[2];
            }
            const double k = __dsqrt_rn(k2);
            const double mu = k == 0. ? 0. : __ddiv_rn(mu_num, k);
            int key = in ? digitize(a.kb, k) - 1 : -1;                 // bin index, or -1: dropped
            if (key >= a.n_bins) key = -1;
            const int tk = key >= t0 && key < t0 + nbt ? key - t0 : -1;   // bin within this tile
            // segments: lanes with equal tk are contiguous (|k| non-decreasing along the row)
            const int prev = __shfl_up(tk, 1);
            const unsigned long long heads = __ballot(lane == 0 || prev != tk);
            const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
            const int seg = 63 - __clzll(heads & upto);
            const int tm = seg_mask(lane, seg);
            const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            const bool live = in && tk >= 0;
            if (__ballot(live) == 0ull) continue;

            const double w = live ? (z == 0 || z == a.nzh - 1 ? 1. : 2.) : 0.;
            double d0 = 1., d1 = 1.;
            if (a.dc0) d0 = dx0 * a.dz0[in ? z : 0];
            if (TWO && a.dc1) d1 = dx1 * a.dz1[in ? z : 0];
            const double re0 = (double)v0.x * d0, im0 = (double)v0.y * d0;
            const double re1 = (double)v1.x * d1, im1 = (double)v1.y * d1;
            const double p00 = re0 * re0 + im0 * im0;
            const double p11 = re1 * re1 + im1 * im1;
            const double cre = re0 * re1 + im0 * im1, cim = im0 * re1 - re0 * im1;

            auto put = [&](int acc, double val) {
                const double s = seg_scan(val, tm);
                if (tail && live) h[acc * a.bt + tk] += s;
            };
            put(0, w);
            put(1, w * k);
            for (int j = 0; j < a.n_ells; ++j) {
                const int l = (int)((a.ells >> (4 * j)) & 15);
                const double c = legendre(mu, l) * (w * (2 * l + 1));
                if (TWO) {
                    put(2 + 4 * j, c * p00);
                    put(3 + 4 * j, c * p11);
                    put(4 + 4 * j, c * cre);
                    put(5 + 4 * j, c * cim);
                } else {
                    put(2 + j, c * p00);
                }
            }
        }
    }
    __syncthreads();
    hist4_partials(hist, hsz, nacc, a.bt, t0, nbt, a.P, b, a.nblk, blk, a.n_bins);
}

struct SpecLayout {
    int n_acc, n_bins, bt, tiles, rows, rows_per_wave;
    unsigned nblk;
    size_t off_tab, off_lut, off_P, off_Q, bytes;
};

int spec_layout(int nx, int ny, int nz, int n_edges, int n_ells, int two, int batch, SpecLayout *L) {
    if (nx < 1 || ny < 1 || nz < 2 || (nz & 1)) return mcpm_fail(nullptr, MCPM_E_SHAPE, "mcpm_spectrum: bad mesh shape (nz must be even)");
    if (n_edges < 2 || n_edges > MCPM_SPECTRUM_MAX_EDGES)
        return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum: need 2 .. MCPM_SPECTRUM_MAX_EDGES edges");
    if (n_ells < 1 || n_ells > 9) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum: 1 .. 9 multipoles");
    MCPM_TRY(mcpm_check_batch("mcpm_spectrum", batch));
    const int nzh = nz / 2 + 1;
    L->n_acc = 2 + n_ells * (two ? 4 : 1);
    L->n_bins = n_edges - 1;
    mcpm_hist_tiles(L->n_bins, SPEC_LDS_DOUBLES, SPEC_WAVES, L->n_acc, &L->bt, &L->tiles);
    L->rows = nx * ny;
    const int64_t nout = (int64_t)L->n_acc * L->n_bins;
    // workgroups: fewer when the partials would pass 32 MB per spectrum
    const int64_t nblk = mcpm_fold_nblk((int64_t)1 << 22, nout, (L->rows + SPEC_WAVES - 1) / SPEC_WAVES);
    L->rows_per_wave = (int)((L->rows + nblk * SPEC_WAVES - 1) / (nblk * SPEC_WAVES));
    L->nblk = (unsigned)((L->rows + (int64_t)L->rows_per_wave * SPEC_WAVES - 1) / ((int64_t)L->rows_per_wave * SPEC_WAVES));
    Carve c;
    L->off_tab = c.take(((size_t)(nx + ny + nzh) * 3 + n_edges) * 8);
    L->off_lut = c.take((size_t)kbin_nlut(n_edges) * 4);
    mcpm_fold_carve(c, batch, L->nblk, (size_t)nout, &L->off_P, &L->off_Q);
    L->bytes = c.bytes;
    return MCPM_OK;
}

}  // namespace

extern "C" {

int mcpm_spectrum_workspace(int nx, int ny, int nz, int n_edges, int n_ells, int two, int batch, int64_t *bytes) {
    if (!bytes) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum_workspace: null output");
    SpecLayout L;
    MCPM_TRY(spec_layout(nx, ny, nz, n_edges, n_ells, two, batch, &L));
    *bytes = (int64_t)L.bytes;
    return MCPM_OK;
}

int mcpm_spectrum_bins_c64(void *stream, int nx, int ny, int nz, const float *spec0, int64_t stride0, const float *spec1,
                           int64_t stride1, int batch, const double *ktab, const double *deconv0, const double *deconv1,
                           const double *edges, int n_edges, const double *los, const int *ells, int n_ells, void *work,
                           int64_t work_bytes, double *out) {
    const int two = spec1 != nullptr;
    SpecLayout L;
    MCPM_TRY(spec_layout(nx, ny, nz, n_edges, n_ells, two, batch, &L));
    if (!spec0 || !ktab || !edges || !los || !ells || !work || !out)
        return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum_bins_c64: null pointer");
    if (work_bytes < (int64_t)L.bytes) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum_bins_c64: workspace too small");
    if (stride0 < 0 || stride1 < 0) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum_bins_c64: negative stride");
    MCPM_TRY(mcpm_check_edges("mcpm_spectrum_bins_c64", edges, n_edges, true));
    int lmax = 0;
    for (int j = 0; j < n_ells; ++j) {
        if (ells[j] < 0 || ells[j] > 8) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_spectrum_bins_c64: multipoles 0 .. 8");
        lmax = std::max(lmax, ells[j]);
    }
    hipStream_t s = (hipStream_t)stream;
    const int nzh = nz / 2 + 1, nk = nx + ny + nzh;
    // tables into the workspace: k [nk], deconv0 [nk], deconv1 [nk], edges
    char *ws = (char *)work;
    double *tab = (double *)(ws + L.off_tab);
    std::vector<double> host((size_t)3 * nk + n_edges, 1.);
    std::copy(ktab, ktab + nk, host.begin());
    if (deconv0) std::copy(deconv0, deconv0 + nk, host.begin() + nk);
    if (deconv1) std::copy(deconv1, deconv1 + nk, host.begin() + 2 * nk);
    std::copy(edges, edges + n_edges, host.begin() + 3 * nk);
    MCPM_HIP(nullptr, hipMemcpyAsync(tab, host.data(), host.size() * 8, hipMemcpyHostToDevice, s));
    MCPM_HIP(nullptr, hipStreamSynchronize(s));      // `host` dies on return

    SpecArgs a{};
    a.s0 = (const float2 *)spec0;
    a.s1 = (const float2 *)spec1;
    a.st0 = stride0;
    a.st1 = stride1;
    a.kx = tab;
    a.ky = tab + nx;
    a.kz = tab + nx + ny;
    a.dc0 = deconv0 ? tab + nk : nullptr;
    a.dc1 = deconv1 && two ? tab + 2 * nk : nullptr;
    a.dz0 = a.dc0 ? a.dc0 + nx + ny : nullptr;
    a.dz1 = a.dc1 ? a.dc1 + nx + ny : nullptr;
    a.n_bins = L.n_bins;
    for (int i = 0; i < 3; ++i) a.los[i] = los[i];
    for (int j = 0; j < n_ells; ++j) a.ells |= (unsigned long long)ells[j] << (4 * j);
    a.n_ells = n_ells;
    a.lmax = lmax;
    a.two = two;
    a.nx = nx;
    a.ny = ny;
    a.nzh = nzh;
    a.rows = L.rows;
    a.rows_per_wave = L.rows_per_wave;
    a.rounds_per_row = (nzh + 63) / 64;
    a.n_acc = L.n_acc;
    a.bt = L.bt;
    a.nblk = L.nblk;
    a.P = (double *)(ws + L.off_P);

    a.kb = kbin_table(edges, n_edges, tab + 3 * nk, (int *)(ws + L.off_lut), s);
    MCPM_LAUNCH_CHECK(nullptr, "kbin_lut_kernel");
    const dim3 grid(L.nblk, batch, L.tiles);
    const size_t lds = (size_t)SPEC_WAVES * L.n_acc * L.bt * 8;
    if (two)
        spectrum_bins_kernel<true><<<grid, 64 * SPEC_WAVES, lds, s>>>(a);
    else
        spectrum_bins_kernel<false><<<grid, 64 * SPEC_WAVES, lds, s>>>(a);
    MCPM_LAUNCH_CHECK(nullptr, "spectrum_bins_kernel");
    return mcpm_fold_partials(s, a.P, batch, L.nblk, L.n_acc * L.n_bins, (double *)(ws + L.off_Q), fold_dense(out));
}

}  // extern "C"
