// Block / grid reductions in f64 shared by the adjoint kernels (composite.hip, bias.hip, observe.hip): every workgroup writes its
// partial sums, det_fold_kernel (reduce.hip) adds them up in a fixed order (see DETERMINISTIC GRID SUMS below).  What device code includes;
// the host side of a sum is mcpm_det_begin / mcpm_det_fold (mcpm_internal.h).
#pragma once
#include <hip/hip_runtime.h>

constexpr int DET_MAXK = 10;      // most values one fold adds up

// Where the fold leaves its K values.
struct DetOuts {
    double *p[DET_MAXK];      // destination of value k (NULL: dropped)
    int accumulate;           // 1: *p[k] += scale sum, 0: *p[k] = scale sum
};
enum DetMode { DET_STORE = 0, DET_ACCUMULATE = 1 };
inline DetOuts det_outs_row(DetMode mode, double *base, int k) {      // values 0 .. k-1 to base[0 .. k)
    DetOuts o{};
    for (int i = 0; i < k; ++i) o.p[i] = base + i;
    o.accumulate = mode;
    return o;
}
inline DetOuts det_outs_ptrs(DetMode mode, double *o0, double *o1 = nullptr, double *o2 = nullptr) {      // up to three values, each to its own place
    DetOuts o{};
    o.p[0] = o0, o.p[1] = o1, o.p[2] = o2;
    o.accumulate = mode;
    return o;
}

namespace {

// Sum over the 64 lanes, valid in LANE 63, by DPP (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31 on the two halves of the double:
// 18 VALU instructions) instead of __shfl_down, which is two ds_bpermute_b32 per step through the LDS crossbar (DESIGN finding
// 27).  Every lane of the wave must be active.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_shift_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWMASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWMASK, 0xf, true);
    return __hiloint2double(hi, lo);       // lanes without a source read +0.0
}
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_shift_d<0x111, 0xf>(v);
    v += dpp_shift_d<0x112, 0xf>(v);
    v += dpp_shift_d<0x114, 0xf>(v);
    v += dpp_shift_d<0x118, 0xf>(v);
    v += dpp_shift_d<0x142, 0xa>(v);
    v += dpp_shift_d<0x143, 0xc>(v);
    return v;
}

// Epilogue of a histogram kernel of four waves (spectrum.hip, binned.hip), after its __syncthreads: the waves' LDS histograms
// hist[4][n_acc][bt] (hsz = n_acc * bt), added in a fixed tree, become the workgroup's partials P[group][blk][acc][tile0 + j], j < nbt, for
// mcpm_fold_partials (reduce.hip).
__device__ __forceinline__ void hist4_partials(const double *hist, int hsz, int n_acc, int bt, int tile0, int nbt, double *P, int group,
                                               unsigned nblk, unsigned blk, int n_bins) {
    double *Pb = P + ((size_t)group * nblk + blk) * (size_t)n_acc * n_bins;
    for (int i = threadIdx.x; i < n_acc * nbt; i += blockDim.x) {
        const int acc = i / nbt, j = i - acc * nbt;
        const int o = acc * bt + j;
        Pb[(size_t)acc * n_bins + tile0 + j] = (hist[o] + hist[hsz + o]) + (hist[2 * hsz + o] + hist[3 * hsz + o]);
    }
}

// DETERMINISTIC GRID SUMS (round 4).  Round 3 added every workgroup's float64 partial to one of NSLOT spread slots with atomicAdd: several
// workgroups per slot, in arrival order, so the last bit of a scalar cotangent moved from call to call (4e-16 .. 7e-16 relative; invisible at
// the float32 the samplers carry, visible to a float64 equality).  Now every workgroup WRITES its partials (fixed tree inside the
// workgroup) to P[k * nblk + block], and det_fold_kernel (reduce.hip) adds them up in a fixed order: a few workgroups each sum a contiguous range of P,
// the last of them to finish sums those sums with the same fixed tree.  No floating-point atomic is left on the gradient path.
template <int K>
__device__ __forceinline__ void block_partial(const double (&v)[K], double *__restrict__ P, unsigned nblk, unsigned blk) {
    __shared__ double sh[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 63) sh[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int nw = (blockDim.x + 63) >> 6;
        double t = 0.;
        for (int w = 0; w < nw; ++w) t += sh[threadIdx.x][w];
        P[(size_t)threadIdx.x * nblk + blk] = t;
    }
}

}  // namespace
