// Bin of a wavenumber: np.digitize(|k|, edges) (right=False) restated exactly, shared by the binned spectra (spectrum.hip) and the
// shell split of the bispectrum (bispectrum.hip), so that a mode lands in the same bin in both.  The bin comes from a lookup table over
// a uniform grid of [e_0, e_last) (a lower bound of the count of edges <= |k|) and a short forward walk over the edges.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct KBinTable {
    const double *edges;                // [n_edges], strictly increasing
    const int *lut;                     // [nlut]: count of edges <= e_0 + c * lut_w
    double lut_inv, lut_w;
    int nlut, n_edges;
};

__device__ __forceinline__ int digitize(const KBinTable &a, double k) {
    // count of edges <= k (np.digitize, right=False); 0 and n_edges are dropped by the caller
    if (!(k >= a.edges[0])) return 0;
    if (k >= a.edges[a.n_edges - 1]) return a.n_edges;
    int c = (int)((k - a.edges[0]) * a.lut_inv) - 1;     // one cell below: e_0 + c * w <= k despite the rounding of c
    c = min(max(c, 0), a.nlut - 1);
    int b = a.lut[c];
    while (b < a.n_edges && a.edges[b] <= k) ++b;
    return b;
}

// |k| of a mode from kx^2 + ky^2 (formed by kbin_kp2) and kz: contraction OFF (hipcc would fuse the sums into v_fmac_f64 and move
// modes that sit on an edge) and a correctly rounded sqrt.
__device__ __forceinline__ double kbin_kp2(double kx, double ky) {
#pragma clang fp contract(off)
    return kx * kx + ky * ky;
}
__device__ __forceinline__ double kbin_kabs(double kp2, double kz) {
    double k2;
    {
#pragma clang fp contract(off)
        k2 = kp2 + kz * kz;
    }
    return __dsqrt_rn(k2);
}

// count of edges <= e_0 + c * w, by bisection
__global__ __launch_bounds__(256) void kbin_lut_kernel(const double *__restrict__ edges, int n_edges, double w, int nlut, int *lut) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nlut) return;
    const double x = edges[0] + c * w;
    int lo = 0, hi = n_edges;      // answer in [lo, hi]
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (edges[m] <= x) lo = m + 1;
        else hi = m;
    }
    lut[c] = lo;
}

inline int kbin_nlut(int n_edges) { return n_edges * 4 < 16384 ? n_edges * 4 : 16384; }

// Host side: the table of the edges `edges` (host, checked by the caller; their device copy `dev_edges` is already enqueued on `s`) with its
// lookup table in lut [kbin_nlut(n_edges)] (device), which kbin_lut_kernel fills on `s`.  The caller checks the launch.
inline KBinTable kbin_table(const double *edges, int n_edges, const double *dev_edges, int *lut, hipStream_t s) {
    KBinTable t;
    t.edges = dev_edges;
    t.lut = lut;
    t.nlut = kbin_nlut(n_edges);
    t.lut_w = (edges[n_edges - 1] - edges[0]) / t.nlut;
    t.lut_inv = 1. / t.lut_w;
    t.n_edges = n_edges;
    kbin_lut_kernel<<<(t.nlut + 255) / 256, 256, 0, s>>>(dev_edges, n_edges, t.lut_w, t.nlut, lut);
    return t;
}

}  // namespace
