// Table look-ups shared by the kernels that read the growth / distance tables per particle or per cell (observe.hip, kaiser.hip):
// clamped linear interpolation in float64 with its bracket and slope, the zero-outside look-up of the k-space kernels (bias.hip, png.hip,
// kaiser_post.hip) with the Table argument they take, and the device side of the order-independent integer sums that
// contract per-element cotangents into the small cotangents of the tables (those two and png.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "mcpm_internal.h"

namespace {

// np.interp (clamped) and its slope
__device__ __forceinline__ double interp1(double x, const double *xp, const double *fp, int n, double &slope) {
    if (x <= xp[0]) { slope = 0.; return fp[0]; }
    if (x >= xp[n - 1]) { slope = 0.; return fp[n - 1]; }
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    slope = (fp[hi] - fp[lo]) / (xp[hi] - xp[lo]);
    return fp[lo] + slope * (x - xp[lo]);
}

// One table of the k-space kernels as they take it by value: n nodes x ascending and values f, device float64
struct Table {
    const double *x, *f;
    int n;
};
// the entry points' side of it, with the check they all make
__host__ inline int table_arg(mcpm_plan *p, const char *who, const double *x, const double *f, int n, Table *t) {
    MCPM_REQUIRE(p, x && f && n >= 2, MCPM_E_ARG, std::string(who) + ": bad argument");
    *t = Table{x, f, n};
    return MCPM_OK;
}
// jnp.interp(x, xp, fp, left=0, right=0) with its bracket: lo < 0 outside the table (t = 0, no node receives a cotangent)
struct TNode {
    int lo;
    double w, t;      // t = (1 - w) fp[lo] + w fp[lo + 1]
};
__device__ __forceinline__ TNode interp_zero(double x, const Table &tb) {
    const double *__restrict__ xp = tb.x, *__restrict__ fp = tb.f;
    const int n = tb.n;
    TNode r;
    r.lo = -1, r.w = 0., r.t = 0.;
    if (x < xp[0] || x > xp[n - 1]) return r;
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    r.lo = lo;
    r.w = (x - xp[lo]) / (xp[hi] - xp[lo]);
    r.t = fp[lo] + (fp[hi] - fp[lo]) / (xp[hi] - xp[lo]) * (x - xp[lo]);
    return r;
}

// The light-cone tables as the entry points receive them (device float64): chi[nchi] ascending, a(chi)[nchi], a[ngrow], g[ngrow], f[ngrow]
struct LcTables {
    const double *chi, *a_of_chi, *a, *g, *f;
    int nchi, ngrow;
};
__host__ inline LcTables lc_tables(const double *t, int nchi, int ngrow) {
    if (!t) return LcTables{nullptr, nullptr, nullptr, nullptr, nullptr, nchi, ngrow};
    return LcTables{t, t + nchi, t + 2 * nchi, t + 2 * nchi + ngrow, t + 2 * nchi + 2 * ngrow, nchi, ngrow};
}

// ---- cotangents of the look-up TABLES (light cone: how the cosmology enters; model.py:740, :781, bricks.py:750-768) -----------
// y = np.interp(x, xp, fp) = fp[lo] + (fp[lo+1] - fp[lo]) t,  t = (x - xp[lo]) / (xp[lo+1] - xp[lo]):
//   dy/dfp[lo] = 1 - t, dy/dfp[lo+1] = t;   dy/dxp[lo] = -slope (1 - t), dy/dxp[lo+1] = -slope t;   dy/dx = slope
// (clamped ends: y = fp[0] or fp[n-1], slope 0).  The kernels below contract those with per-particle cotangents into small
// table cotangents (integer accumulators, see ORDER-INDEPENDENT SUMS below); the host then contracts them with the tables'
// finite-difference Jacobian w.r.t. the cosmological parameters (model.py cosmo_vjp).
struct Interp {
    int lo;
    bool clamped;
    double t, slope, y;
};
__device__ __forceinline__ Interp interp_idx(double x, const double *xp, const double *fp, int n) {
    Interp r;
    r.clamped = true;
    if (x <= xp[0]) { r.lo = 0, r.t = 0., r.slope = 0., r.y = fp[0]; return r; }
    if (x >= xp[n - 1]) { r.lo = n - 2, r.t = 1., r.slope = 0., r.y = fp[n - 1]; return r; }
    r.clamped = false;
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    const double dx = xp[hi] - xp[lo];
    r.lo = lo;
    r.t = (x - xp[lo]) / dx;
    r.slope = (fp[hi] - fp[lo]) / dx;
    r.y = fp[lo] + r.slope * (x - xp[lo]);
    return r;
}
// same bracket, another value table on the same nodes
__device__ __forceinline__ void interp_at(const Interp &b, const double *xp, const double *fp, double &y, double &slope) {
    const double dx = xp[b.lo + 1] - xp[b.lo];
    const double d = fp[b.lo + 1] - fp[b.lo];
    y = fp[b.lo] + d * b.t;
    slope = b.clamped ? 0. : d / dx;
}
// ORDER-INDEPENDENT SUMS.  The table cotangents end up in d logp / d Omega_m, and every gradient of this build is bitwise the same
// call after call; float64 atomics are not (the first version of these kernels changed the last bits of Omega_m's gradient between
// two calls).  So the contributions are summed as INTEGERS: pass 0 takes the maximum |contribution| of every table (order-independent
// by nature), pass 1 rounds each contribution to 2^(e - 30) units (2^e >= that maximum, so a contribution is below 2^30 and a table
// entry holds 2^32 of them) and adds it with 64-bit integer LDS / global atomics, and a last kernel scales the integers back.
// Resolution: 10^-9 of the largest contribution per term.  A non-finite maximum makes the whole table NaN.
// The host side of a sum is mcpm_tab_begin / mcpm_tab_finish (mcpm_internal.h; reduce.hip keeps the scale kernel).  NK: the number of
// kinds (tables with a maximum of their own) the producer kernel has, at most MCPM_TAB_KINDS.
template <int NK>
struct Acc {      // PASS 0: per-thread maxima;  PASS 1: integer accumulators in LDS
    double mx[NK];
    unsigned long long *sh;
    double scale[NK];
};
template <int PASS, int NK>
__device__ __forceinline__ void acc_add(Acc<NK> &A, int kind, int off, int idx, double v) {
    if (PASS == 0) A.mx[kind] = fmax(A.mx[kind], fabs(v));      // (fmax drops a NaN operand: the callers' `bad` flag catches it)
    else if (v != 0.) atomicAdd(A.sh + off + idx, (unsigned long long)__double2ll_rn(v * A.scale[kind]));
}
template <int PASS, int NK>
__device__ __forceinline__ void scatter_fp(Acc<NK> &A, int kind, int off, const Interp &b, double ybar) {
    acc_add<PASS>(A, kind, off, b.lo, ybar * (1. - b.t));
    acc_add<PASS>(A, kind, off, b.lo + 1, ybar * b.t);
}
// ... and, for a look-up whose NODES move with the cosmology (chi -> a), into the node table's accumulator
template <int PASS, int NK>
__device__ __forceinline__ void scatter_xp(Acc<NK> &A, int kind, int off, const Interp &b, double ybar) {
    acc_add<PASS>(A, kind, off, b.lo, -ybar * b.slope * (1. - b.t));
    acc_add<PASS>(A, kind, off, b.lo + 1, -ybar * b.slope * b.t);
}
// mxbits: float bits (rounded up) of the maxima, one per kind; a NaN / inf contribution sets 0x7f800000 or above
template <int NK>
__device__ __forceinline__ void acc_begin(Acc<NK> &A, unsigned long long *sh, int ntot, const unsigned *mxbits, int pass) {
    static_assert(NK >= 1 && NK <= MCPM_TAB_KINDS, "kinds of a table sum");
    A.sh = sh;
    for (int k = 0; k < NK; ++k) {
        A.mx[k] = 0.;
        const int be = pass ? (int)(mxbits[k] >> 23) : 0;                 // biased exponent of the maximum: max < 2^(be - 126)
        A.scale[k] = (be == 0 || be >= 255) ? 0. : __longlong_as_double((long long)(1023 + 30 - (be - 126)) << 52);      // 2^(30 - e)
    }
    if (pass) {
        for (int i = threadIdx.x; i < ntot; i += blockDim.x) sh[i] = 0ull;
        __syncthreads();
    }
}
template <int PASS, int NK>
__device__ __forceinline__ void acc_end(Acc<NK> &A, int ntot, unsigned *mxbits, unsigned long long *out, bool bad) {
    if (PASS == 0) {
        for (int k = 0; k < NK; ++k) {
            unsigned b = bad ? 0x7fc00000u : __float_as_uint(__double2float_ru(A.mx[k]));
            if (!(A.mx[k] < 3.0e38)) b = 0x7fc00000u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, o));
            if ((threadIdx.x & 63) == 0 && b) atomicMax(mxbits + k, b);
        }
    } else {
        __syncthreads();
        for (int i = threadIdx.x; i < ntot; i += blockDim.x)
            if (A.sh[i] != 0ull) atomicAdd(out + i, A.sh[i]);
    }
}

}  // namespace
