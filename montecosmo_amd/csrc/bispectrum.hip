// Binned bispectrum of meshes, the FFT (Scoccimarro) estimator: B_ijl ~ sum_x F_i F_j F_l / sum_x I_i I_j I_l, where F_b is the
// inverse transform of the half-spectrum with every mode outside k bin b set to zero and I_b the same of the unit spectrum.  Two
// passes live here; the batched C2R between them is the caller's (mcpm_fft_c2r).
//
// Shell split (bispectrum_split_kernel): one streaming pass, a lane per mode of the half-spectrum.  The lane finds the mode's bin with
// the |k| and the digitize of spectrum.hip (kbin_dev.h), and writes the (deconvolved) mode to that bin's spectrum and zero to every
// other: every element of the output is written, eight bytes per lane and consecutive lanes on consecutive kz.
//
// Triple sums (bispectrum_sums_kernel): T products over M cells.  A workgroup stages a chunk of BISP_CHUNK cells of all n_bins fields
// into LDS as float64 [n_bins][BISP_PITCH], converted once on the way in (a walk over float32 rows that converted every value it read,
// three v_cvt_f64_f32 per product, took 21.8 ms where this takes 16.6 ms at 256^3, 27 bins, 2276 triangles).  The pitch is odd in 8-byte
// words, so the up to 32 rows start in different bank pairs of ds_read_b64 (bank = dword address mod 64).  Lanes own TRIANGLES, not
// cells: lane t reads its three rows once and walks the chunk's cells; the lanes of a wave read the same cell, so equal rows broadcast
// and different rows fall in different banks.  Each lane forms (F_i F_j) F_l in float64 and adds it to its own float64 accumulator,
// which stays in a register over the workgroup's contiguous range of chunks: no cross-lane reduction, no atomics, a fixed order.  A
// workgroup holds up to BISP_RT * 256 triangles (blockIdx.y walks further tiles of the list).  With 128 triangles or fewer the lanes
// split into 256 / tp groups (tp = T rounded up to a power of two, at least 2), group g takes the cells g, g + G, ... of every chunk,
// and the groups are added in order at the end.  Every workgroup writes one partial per triangle; mcpm_fold_partials (reduce.hip) adds the
// workgroups up in a fixed order.  The decomposition follows from n_cells, n_bins and n_tri only, so a batch row is bitwise the single call.
#include <algorithm>
#include <cmath>

#include "mcpm_internal.h"
#include "kbin_dev.h"

namespace {

constexpr int BISP_THREADS = 256;
constexpr int BISP_CHUNK = 128;             // cells per staged chunk (a power of two, at least the largest number of lane groups)
constexpr int BISP_PITCH = BISP_CHUNK + 1;  // doubles between the rows of the staged chunk (odd); 33 KB at 32 bins, four workgroups per CU
constexpr int BISP_RT = 4;                  // triangles per lane
constexpr int BISP_TILE = BISP_THREADS * BISP_RT;

struct SplitArgs {
    const float2 *spec;      // [B][nx][ny][nzh], or NULL: the unit spectrum
    long long stride;        // batch stride in complex elements (0: the same spectrum for every row)
    const double *kx, *ky, *kz;
    const double *dc, *dz;   // per-axis deconvolution factors [nx | ny | nzh] and their kz part, or NULL
    KBinTable kb;
    int n_bins, nx, ny, nzh;
    long long mh;
    float2 *out;             // [B][n_bins][nx][ny][nzh]
};

__global__ __launch_bounds__(256) void bispectrum_split_kernel(SplitArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.mh) return;
    const int b = blockIdx.y;
    const long long row = idx / a.nzh;
    const int z = (int)(idx - row * a.nzh), x = (int)(row / a.ny), y = (int)(row - (long long)x * a.ny);
    const double k = kbin_kabs(kbin_kp2(a.kx[x], a.ky[y]), a.kz[z]);
    int key = digitize(a.kb, k) - 1;      // bin index; -1 and n_bins: outside the edges
    float2 v = make_float2(1.f, 0.f);
    if (a.spec) {
        v = a.spec[(size_t)b * a.stride + idx];
        if (a.dc) {
            const double d = (a.dc[x] * a.dc[a.nx + y]) * a.dz[z];
            v = make_float2((float)((double)v.x * d), (float)((double)v.y * d));
        }
    }
    float2 *o = a.out + (size_t)b * a.n_bins * a.mh + idx;
    for (int bin = 0; bin < a.n_bins; ++bin) o[(size_t)bin * a.mh] = bin == key ? v : make_float2(0.f, 0.f);
}

struct SumsArgs {
    const float *fields;     // [B][n_bins][n_cells]
    long long n_cells, n_chunks, chunks_per_blk;
    const int *tri;          // [n_tri][3]
    int n_bins, n_tri;
    int tp_log2;             // lanes per group = 1 << tp_log2 (8: one group)
    unsigned nblk;
    double *P;               // [B][nblk][n_tri]
};

// The chunk's cells g, g + G, ... for NR triangles per lane; row offsets oi / oj / ol in doubles.
template <int NR>
__device__ __forceinline__ void bisp_walk(const double *lds, int g, int G, int cn, const int (&oi)[BISP_RT], const int (&oj)[BISP_RT],
                                          const int (&ol)[BISP_RT], double (&acc)[BISP_RT]) {
#pragma unroll 4
    for (int c = g; c < cn; c += G) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            acc[r] += (lds[oi[r] + c] * lds[oj[r] + c]) * lds[ol[r] + c];
        }
    }
}

__global__ __launch_bounds__(BISP_THREADS) void bispectrum_sums_kernel(SumsArgs a) {
    extern __shared__ double lds[];      // [n_bins][BISP_PITCH]
    __shared__ double fold[BISP_THREADS];
    const int tid = threadIdx.x;
    const int tp = 1 << a.tp_log2, G = BISP_THREADS >> a.tp_log2;
    const int g = tid >> a.tp_log2, tl = tid & (tp - 1);
    const int tile0 = blockIdx.y * BISP_TILE, nt = min(a.n_tri - tile0, BISP_TILE);
    const int nr = G == 1 ? (nt + BISP_THREADS - 1) / BISP_THREADS : 1;
    const int b = blockIdx.z;

    int oi[BISP_RT], oj[BISP_RT], ol[BISP_RT];
    double acc[BISP_RT];
#pragma unroll
    for (int r = 0; r < BISP_RT; ++r) {
        const int t = tl + BISP_THREADS * r;
        int i = 0, j = 0, l = 0;
        if (t < nt) {
            const int *p = a.tri + 3 * (size_t)(tile0 + t);
            i = min(max(p[0], 0), a.n_bins - 1);      // (the caller checks the range; the clamp keeps a bad list inside the chunk)
            j = min(max(p[1], 0), a.n_bins - 1);
            l = min(max(p[2], 0), a.n_bins - 1);
        }
        oi[r] = i * BISP_PITCH, oj[r] = j * BISP_PITCH, ol[r] = l * BISP_PITCH;
        acc[r] = 0.;
    }

    const float *F = a.fields + (size_t)b * a.n_bins * a.n_cells;
    const long long ch0 = (long long)blockIdx.x * a.chunks_per_blk, ch1 = min(ch0 + a.chunks_per_blk, a.n_chunks);
    for (long long ch = ch0; ch < ch1; ++ch) {
        const long long c0 = ch * BISP_CHUNK;
        const int cn = (int)min((long long)BISP_CHUNK, a.n_cells - c0);
        __syncthreads();      // the walk of the previous chunk is over
#pragma unroll 4
        for (int e = tid; e < a.n_bins * BISP_CHUNK; e += BISP_THREADS) {
            const int bin = e / BISP_CHUNK, c = e - bin * BISP_CHUNK;
            lds[bin * BISP_PITCH + c] = c < cn ? (double)F[(size_t)bin * a.n_cells + c0 + c] : 0.;
        }
        __syncthreads();
        switch (nr) {
            case 1: bisp_walk<1>(lds, g, G, cn, oi, oj, ol, acc); break;
            case 2: bisp_walk<2>(lds, g, G, cn, oi, oj, ol, acc); break;
            case 3: bisp_walk<3>(lds, g, G, cn, oi, oj, ol, acc); break;
            default: bisp_walk<4>(lds, g, G, cn, oi, oj, ol, acc); break;
        }
    }

    double *Pb = a.P + ((size_t)b * a.nblk + blockIdx.x) * a.n_tri + tile0;
    if (G == 1) {
#pragma unroll
        for (int r = 0; r < BISP_RT; ++r)
            if (tl + BISP_THREADS * r < nt) Pb[tl + BISP_THREADS * r] = acc[r];
    } else {      // the groups' sums, added in group order
        fold[tid] = acc[0];
        __syncthreads();
        if (tid < nt) {
            double s = 0.;
            for (int gg = 0; gg < G; ++gg) s += fold[gg * tp + tid];
            Pb[tid] = s;
        }
    }
}

struct BispLayout {
    int tp_log2, tiles;
    long long n_chunks, chunks_per_blk;
    unsigned nblk;
    size_t off_P, off_Q, bytes;
};

// The decomposition of the sums pass: a function of n_cells, n_bins and n_tri only.
int bisp_layout(int64_t n_cells, int n_bins, int n_tri, int batch, BispLayout *L) {
    if (n_cells < 1) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum: no cells");
    if (n_bins < 1 || n_bins > MCPM_BISPECTRUM_MAX_BINS) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum: 1 .. MCPM_BISPECTRUM_MAX_BINS bins");
    if (n_tri < 1 || n_tri > MCPM_BISPECTRUM_MAX_TRIANGLES)
        return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum: 1 .. MCPM_BISPECTRUM_MAX_TRIANGLES triangles");
    MCPM_TRY(mcpm_check_batch("mcpm_bispectrum", batch));
    L->tp_log2 = 8;
    if (n_tri <= BISP_THREADS / 2) {
        L->tp_log2 = 0;
        while ((1 << L->tp_log2) < n_tri) ++L->tp_log2;
        if (L->tp_log2 < 1) L->tp_log2 = 1;      // at most BISP_CHUNK groups: every group has a cell of a full chunk
    }
    L->tiles = (n_tri + BISP_TILE - 1) / BISP_TILE;
    L->n_chunks = (n_cells + BISP_CHUNK - 1) / BISP_CHUNK;
    // workgroups per tile: fewer when the partials would pass 16 MB per batch row
    const int64_t nblk = mcpm_fold_nblk((int64_t)1 << 21, n_tri, L->n_chunks);
    L->chunks_per_blk = (L->n_chunks + nblk - 1) / nblk;
    L->nblk = (unsigned)((L->n_chunks + L->chunks_per_blk - 1) / L->chunks_per_blk);
    Carve c;
    mcpm_fold_carve(c, batch, L->nblk, (size_t)n_tri, &L->off_P, &L->off_Q);
    L->bytes = c.bytes;
    return MCPM_OK;
}

int bisp_shape(int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 2 || (nz & 1)) return mcpm_fail(nullptr, MCPM_E_SHAPE, "mcpm_bispectrum: bad mesh shape (nz must be even)");
    return MCPM_OK;
}

}  // namespace

extern "C" {

int mcpm_bispectrum_workspace(int nx, int ny, int nz, int n_bins, int n_tri, int batch, int64_t *bytes) {
    if (!bytes) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum_workspace: null output");
    MCPM_TRY(bisp_shape(nx, ny, nz));
    BispLayout L;
    MCPM_TRY(bisp_layout((int64_t)nx * ny * nz, n_bins, n_tri, batch, &L));
    *bytes = (int64_t)L.bytes;
    return MCPM_OK;
}

int mcpm_bispectrum_split_c64(void *stream, int nx, int ny, int nz, const float *spec, int64_t stride, int batch, const double *ktab,
                              const double *deconv, const double *edges, int n_edges, float *out) {
    MCPM_TRY(bisp_shape(nx, ny, nz));
    if (n_edges < 2 || n_edges > MCPM_BISPECTRUM_MAX_BINS + 1)
        return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum_split_c64: need 2 .. MCPM_BISPECTRUM_MAX_BINS + 1 edges");
    MCPM_TRY(mcpm_check_batch("mcpm_bispectrum_split_c64", batch));
    if (!ktab || !edges || !out) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum_split_c64: null pointer");
    if (stride < 0) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum_split_c64: negative stride");
    MCPM_TRY(mcpm_check_edges("mcpm_bispectrum_split_c64", edges, n_edges, true));
    hipStream_t s = (hipStream_t)stream;
    const int nzh = nz / 2 + 1, nk = nx + ny + nzh;
    // tables: k [nk], deconv [nk], edges [n_edges], then the lookup table; the call owns them and waits for the pass before it frees them
    std::vector<double> host((size_t)2 * nk + n_edges, 1.);
    std::copy(ktab, ktab + nk, host.begin());
    if (deconv) std::copy(deconv, deconv + nk, host.begin() + nk);
    std::copy(edges, edges + n_edges, host.begin() + 2 * nk);
    const size_t off_lut = align256(host.size() * 8);
    char *dev = nullptr;
    MCPM_HIP(nullptr, hipMalloc((void **)&dev, off_lut + (size_t)kbin_nlut(n_edges) * 4));
    double *tab = (double *)dev;
    int rc = MCPM_OK;
    hipError_t e = hipMemcpyAsync(tab, host.data(), host.size() * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        SplitArgs a{};
        a.spec = (const float2 *)spec;
        a.stride = stride;
        a.kx = tab;
        a.ky = tab + nx;
        a.kz = tab + nx + ny;
        a.dc = deconv && spec ? tab + nk : nullptr;
        a.dz = a.dc ? a.dc + nx + ny : nullptr;
        a.n_bins = n_edges - 1;
        a.nx = nx;
        a.ny = ny;
        a.nzh = nzh;
        a.mh = (long long)nx * ny * nzh;
        a.out = (float2 *)out;
        a.kb = kbin_table(edges, n_edges, tab + 2 * nk, (int *)(dev + off_lut), s);
        bispectrum_split_kernel<<<dim3((unsigned)((a.mh + 255) / 256), batch), 256, 0, s>>>(a);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);      // `host` and the tables die on return
    }
    if (e != hipSuccess) rc = mcpm_fail(nullptr, MCPM_E_HIP, std::string("mcpm_bispectrum_split_c64: ") + hipGetErrorString(e));
    (void)hipFree(dev);
    return rc;
}

int mcpm_bispectrum_sums_f32(void *stream, const float *fields, int64_t n_cells, int n_bins, int batch, const int *tri, int n_tri,
                             void *work, int64_t work_bytes, double *out) {
    BispLayout L;
    MCPM_TRY(bisp_layout(n_cells, n_bins, n_tri, batch, &L));
    if (!fields || !tri || !work || !out) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum_sums_f32: null pointer");
    if (work_bytes < (int64_t)L.bytes) return mcpm_fail(nullptr, MCPM_E_ARG, "mcpm_bispectrum_sums_f32: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)work;
    SumsArgs a{};
    a.fields = fields;
    a.n_cells = n_cells;
    a.n_chunks = L.n_chunks;
    a.chunks_per_blk = L.chunks_per_blk;
    a.tri = tri;
    a.n_bins = n_bins;
    a.n_tri = n_tri;
    a.tp_log2 = L.tp_log2;
    a.nblk = L.nblk;
    a.P = (double *)(ws + L.off_P);
    const size_t lds = (size_t)n_bins * BISP_PITCH * 8;
    bispectrum_sums_kernel<<<dim3(L.nblk, L.tiles, batch), BISP_THREADS, lds, s>>>(a);
    MCPM_LAUNCH_CHECK(nullptr, "bispectrum_sums_kernel");
    return mcpm_fold_partials(s, a.P, batch, L.nblk, n_tri, (double *)(ws + L.off_Q), fold_dense(out));
}

}  // extern "C"
