// Catalogue -> register (montecosmo/model.py:1287-1362, register_catalog; bricks.py:882-1103): the per-object passes that turn a galaxy
// catalogue (RA, DEC, Z) or a simulation box (pos, vel) into positions in cell units, the exact footprint of a set of objects on a
// mesh, and the reductions the host needs around them (bounding box, weighted sizes, mean over the footprint).  The paints themselves
// are mcpm_paint_f32 / nufft; nothing here is differentiated.
//
// All five are streaming passes: coalesced loads, 256-thread workgroups, at most CAT_MAX_BLOCKS of them with a grid stride, no
// floating-point atomic.  Every sum goes through block_partial + det_fold_kernel (reduce_dev.h), minima and maxima through
// per-workgroup partials and one folding workgroup: bitwise the same call after call.
//
// Coordinates are formed in float64 and rounded ONCE to the float32 the paints take: a survey box is thousands of Mpc/h across with
// its corner thousands of Mpc/h from the observer, and float32 steps of the chain (chi ~ 2000, minus box_center, rotated) would each
// cost ~1e-4 Mpc/h.
#include "mcpm_internal.h"
#include "particles_dev.h"
#include "reduce_dev.h"
#include "tables_dev.h"

#define CAT_MAX_BLOCKS 2048
#define CAT_DEG2RAD 0.017453292519943295      // numpy.deg2rad: x * (pi / 180)
#define CAT_LDS_TABLE 1024                    // distance tables up to this length are staged in LDS (2 x 8 KB)

namespace {

struct CellGeom {      // phys2cell_pos (bricks.py:638-646): ((x - center) @ rot + half) * scale
    double center[3], rot[9], half[3], scale[3];
};
struct BoxGeom {
    CellGeom c;
    double los[3], vscale;
};

__device__ __forceinline__ void phys2cell(const CellGeom &q, const double (&x)[3], double (&y)[3]) {
    const double d0 = x[0] - q.center[0], d1 = x[1] - q.center[1], d2 = x[2] - q.center[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) y[j] = ((d0 * q.rot[j] + d1 * q.rot[3 + j] + d2 * q.rot[6 + j]) + q.half[j]) * q.scale[j];
}

// the distance table, in LDS when it fits (the search is eight dependent loads per object)
__device__ __forceinline__ void stage_table(const double *__restrict__ atab, const double *__restrict__ chitab, int nt, double *sh,
                                            const double *&xa, const double *&xc) {
    if (nt <= CAT_LDS_TABLE) {
        for (int i = threadIdx.x; i < nt; i += blockDim.x) sh[i] = atab[i], sh[CAT_LDS_TABLE + i] = chitab[i];
        __syncthreads();
        xa = sh, xc = sh + CAT_LDS_TABLE;
    } else {
        xa = atab, xc = chitab;
    }
}

// radecz2cart (bricks.py:882-890, utils.py:1186-1196): a = 1 / (1 + z), chi = max(interp(a), 0) (nbody.a2chi), x = chi (cos dec cos ra, ...)
__device__ __forceinline__ void sky2cart(double ra, double dec, double z, const double *xa, const double *xc, int nt, double (&x)[3]) {
    double slope;
    const double chi = fmax(interp1(1. / (1. + z), xa, xc, nt, slope), 0.);
    double sr, cr, sd, cd;
    sincos(ra * CAT_DEG2RAD, &sr, &cr);
    sincos(dec * CAT_DEG2RAD, &sd, &cd);
    x[0] = chi * (cd * cr), x[1] = chi * (cd * sr), x[2] = chi * sd;
}

template <bool MAX>
__device__ __forceinline__ double wave_minmax(double v) {      // over the 64 lanes, valid in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = MAX ? fmax(v, u) : fmin(v, u);
    }
    return v;
}

// P: [weight sum: nblk] [min x, y, z: 3 nblk] [max x, y, z: 3 nblk]
__global__ __launch_bounds__(256) void sky2cart_minmax_kernel(const double *__restrict__ ra, const double *__restrict__ dec,
                                                              const double *__restrict__ z, int64_t n, const double *__restrict__ atab,
                                                              const double *__restrict__ chitab, int nt, const double *__restrict__ w,
                                                              double *__restrict__ P) {
    __shared__ double tab[2 * CAT_LDS_TABLE];
    __shared__ double mm[6][4];
    const double *xa, *xc;
    stage_table(atab, chitab, nt, tab, xa, xc);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, ws[1] = {0.};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double x[3];
        sky2cart(ra[i], dec[i], z[i], xa, xc, nt, x);
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], x[a]), hi[a] = fmax(hi[a], x[a]);
        if (w) ws[0] += w[i];
    }
    block_partial<1>(ws, P, gridDim.x, blockIdx.x);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double l = wave_minmax<false>(lo[a]), h = wave_minmax<true>(hi[a]);
        if ((threadIdx.x & 63) == 0) mm[a][threadIdx.x >> 6] = l, mm[3 + a][threadIdx.x >> 6] = h;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        double t = mm[k][0];
        for (int wv = 1; wv < 4; ++wv) t = k < 3 ? fmin(t, mm[k][wv]) : fmax(t, mm[k][wv]);
        P[(size_t)(1 + k) * gridDim.x + blockIdx.x] = t;
    }
}

// one workgroup: out[k] = min (k < 3) / max (k >= 3) over the nblk partials of row k; nblk = 0 leaves +inf / -inf
__global__ __launch_bounds__(256) void minmax_fold_kernel(const double *__restrict__ P, unsigned nblk, double *__restrict__ out) {
    __shared__ double mm[6][4];
    P += nblk;      // rows 1..6 of sky2cart_minmax_kernel's partials
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double t = k < 3 ? INFINITY : -INFINITY;
        for (unsigned i = threadIdx.x; i < nblk; i += 256) t = k < 3 ? fmin(t, P[(size_t)k * nblk + i]) : fmax(t, P[(size_t)k * nblk + i]);
        t = k < 3 ? wave_minmax<false>(t) : wave_minmax<true>(t);
        if ((threadIdx.x & 63) == 0) mm[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        double t = mm[k][0];
        for (int wv = 1; wv < 4; ++wv) t = k < 3 ? fmin(t, mm[k][wv]) : fmax(t, mm[k][wv]);
        out[k] = t;
    }
}

__global__ __launch_bounds__(256) void sky2cell_kernel(const double *__restrict__ ra, const double *__restrict__ dec,
                                                       const double *__restrict__ z, int64_t n, const double *__restrict__ atab,
                                                       const double *__restrict__ chitab, int nt, CellGeom q, float r0, float r1, float r2,
                                                       float *__restrict__ out, float *__restrict__ out2) {
    __shared__ double tab[2 * CAT_LDS_TABLE];
    const double *xa, *xc;
    stage_table(atab, chitab, nt, tab, xa, xc);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double x[3], y[3];
        sky2cart(ra[i], dec[i], z[i], xa, xc, nt, x);
        phys2cell(q, x, y);
        const P3 c = {(float)y[0], (float)y[1], (float)y[2]};
        store3(out, i, c);
        if (out2) store3(out2, i, P3{c.x * r0, c.y * r1, c.z * r2});      // float32 product of the float32 result: `pos *= ratio`
    }
}

// one (x, y, z) record as doubles: float32 records through the 12-byte load3, float64 ones as three loads
__device__ __forceinline__ void read3(const float *__restrict__ p, int64_t i, double (&x)[3]) {
    const P3 d = load3(p, i);
    x[0] = (double)d.x, x[1] = (double)d.y, x[2] = (double)d.z;
}
__device__ __forceinline__ void read3(const double *__restrict__ p, int64_t i, double (&x)[3]) {
    x[0] = p[3 * i], x[1] = p[3 * i + 1], x[2] = p[3 * i + 2];
}

template <typename T>
__global__ __launch_bounds__(256) void box2cell_kernel(const T *__restrict__ pos, const T *__restrict__ vel, int64_t n, BoxGeom q,
                                                       float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double x[3], y[3];
        read3(pos, i, x);
        if (vel) {      // redshift-space distortion along los (bricks.py:1091-1094): pos + vscale (vel . los) los
            double v[3];
            read3(vel, i, v);
            const double vl = (v[0] * q.vscale * q.los[0] + v[1] * q.vscale * q.los[1]) + v[2] * q.vscale * q.los[2];
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] += vl * q.los[a];
        }
        phys2cell(q.c, x, y);
        store3(out, i, P3{(float)y[0], (float)y[1], (float)y[2]});
    }
}

// mask[c] = 1 where an object of positive weight has a non-zero assignment weight on every axis at cell c: locate / Stencil are
// the paint's own (paint_atomic_kernel), and so are the per-axis float32 weights.  Every writer stores the same byte, so the
// result does not depend on the order of the objects or of the stores.  Objects outside the paints' documented range
// (|pos| < 32767, where wrapi is exact) or with a non-finite coordinate mark nothing.
template <int ORDER>
__global__ __launch_bounds__(256) void footprint_kernel(Geom g, const float *__restrict__ pos, int64_t n, const float *__restrict__ w,
                                                        unsigned char *__restrict__ mask, int64_t M) {
    PIdx pi{};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (w && !(w[i] > 0.f)) continue;
        const P3 d = load3(pos, i);
        if (!(fabsf(d.x) < 32767.f && fabsf(d.y) < 32767.f && fabsf(d.z) < 32767.f)) continue;
        int c[3];
        float f[3];
        locate<MCPM_POS_ABSOLUTE, ORDER>(g, pi, d, c, f);
        const Stencil<ORDER> s(g, c);
        if (ORDER == 1) {
            const int64_t cell = s.xo[0] + s.yo[0] + s.zo[0];
            if (cell >= 0 && cell < M) mask[cell] = 1;
            continue;
        }
        constexpr int NP = ORDER < 2 ? 2 : ORDER;
        float k[3][NP];
        if (ORDER == 2) {
#pragma unroll
            for (int a = 0; a < 3; ++a) k[a][0] = 1.f - f[a], k[a][1] = f[a];
        } else {
            constexpr int NPG = ORDER < 3 ? 3 : ORDER;
            float wa[NPG], dd[NPG];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                axis_weights<NPG, false>(f[a], wa, dd);
#pragma unroll
                for (int j = 0; j < NP; ++j) k[a][j] = wa[j];
            }
        }
#pragma unroll
        for (int a = 0; a < NP; ++a)
#pragma unroll
            for (int b = 0; b < NP; ++b)
#pragma unroll
                for (int e = 0; e < NP; ++e) {
                    const int64_t cell = s.xo[a] + s.yo[b] + s.zo[e];
                    if (k[0][a] != 0.f && k[1][b] != 0.f && k[2][e] != 0.f && cell >= 0 && cell < M) mask[cell] = 1;
                }
    }
}

// P: [sum over mask != 0: nblk] [number of such cells: nblk]
__global__ __launch_bounds__(256) void masked_sum_kernel(const float *__restrict__ mesh, const unsigned char *__restrict__ mask, int64_t n,
                                                         double *__restrict__ P) {
    double v[2] = {0., 0.};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (mask[i]) v[0] += (double)mesh[i], v[1] += 1.;
    block_partial<2>(v, P, gridDim.x, blockIdx.x);
}

inline unsigned cat_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, CAT_MAX_BLOCKS); }

inline CellGeom cell_geom(const double *g) {      // host: center[3], rot[9], box_size[3], mesh_shape[3]
    CellGeom q;
    for (int a = 0; a < 3; ++a) q.center[a] = g[a], q.half[a] = g[12 + a] / 2, q.scale[a] = g[15 + a] / g[12 + a];
    for (int a = 0; a < 9; ++a) q.rot[a] = g[3 + a];
    return q;
}
inline bool cell_geom_ok(const double *g) {
    for (int a = 0; a < 18; ++a)
        if (!std::isfinite(g[a])) return false;
    return g[12] > 0. && g[13] > 0. && g[14] > 0. && g[15] > 0. && g[16] > 0. && g[17] > 0.;
}

}  // namespace

extern "C" {

int mcpm_sky2cart_minmax_f64(mcpm_plan *p, const double *ra, const double *dec, const double *z, int64_t n, const double *atab,
                             const double *chitab, int ntab, const double *weights, double *minmax6, double *wsum) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n >= 0 && minmax6 && atab && chitab && ntab >= 2, MCPM_E_ARG, "mcpm_sky2cart_minmax_f64: bad argument");
    MCPM_REQUIRE(p, (ra && dec && z) || n == 0, MCPM_E_ARG, "mcpm_sky2cart_minmax_f64: null coordinate array");
    MCPM_REQUIRE(p, !weights || wsum, MCPM_E_ARG, "mcpm_sky2cart_minmax_f64: weights without an output for their sum");
    const unsigned nb = cat_blocks(n);
    DetSum s;
    StageTimer st_(p, ST_AXPY, (weights ? 32.0 : 24.0) * n);
    // 7 rows of nb partials: row 0 (the weights) is folded, rows 1..6 (minima, maxima) are read by minmax_fold_kernel
    MCPM_TRY(mcpm_det_begin(p, 7, nb, &s));
    if (wsum && (!weights || n == 0)) MCPM_HIP(p, hipMemsetAsync(wsum, 0, sizeof(double), p->stream));
    if (n > 0) {
        sky2cart_minmax_kernel<<<nb, 256, 0, p->stream>>>(ra, dec, z, n, atab, chitab, ntab, weights, s.P);
        MCPM_LAUNCH_CHECK(p, "sky2cart_minmax_kernel");
        if (weights) MCPM_TRY(mcpm_det_fold(p, s, 1, 1.0, det_outs_ptrs(DET_STORE, wsum)));
    }
    minmax_fold_kernel<<<1, 256, 0, p->stream>>>(s.P, s.nblk, minmax6);
    MCPM_LAUNCH_CHECK(p, "minmax_fold_kernel");
    return MCPM_OK;
}

int mcpm_sky2cell_f32(mcpm_plan *p, const double *ra, const double *dec, const double *z, int64_t n, const double *atab,
                      const double *chitab, int ntab, const double *geom18, const double *ratio3, float *out, float *out2) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n >= 0 && atab && chitab && ntab >= 2 && geom18, MCPM_E_ARG, "mcpm_sky2cell_f32: bad argument");
    MCPM_REQUIRE(p, (ra && dec && z && out) || n == 0, MCPM_E_ARG, "mcpm_sky2cell_f32: null array");
    MCPM_REQUIRE(p, cell_geom_ok(geom18), MCPM_E_ARG, "mcpm_sky2cell_f32: geometry must be finite with positive box_size and mesh_shape");
    MCPM_REQUIRE(p, !out2 || ratio3, MCPM_E_ARG, "mcpm_sky2cell_f32: a second output needs its ratio");
    if (n == 0) return MCPM_OK;
    StageTimer st_(p, ST_AXPY, (out2 ? 48.0 : 36.0) * n);
    const float r0 = out2 ? (float)ratio3[0] : 1.f, r1 = out2 ? (float)ratio3[1] : 1.f, r2 = out2 ? (float)ratio3[2] : 1.f;
    sky2cell_kernel<<<cat_blocks(n), 256, 0, p->stream>>>(ra, dec, z, n, atab, chitab, ntab, cell_geom(geom18), r0, r1, r2, out, out2);
    MCPM_LAUNCH_CHECK(p, "sky2cell_kernel");
    return MCPM_OK;
}

int mcpm_box2cell_f32(mcpm_plan *p, const void *pos, const void *vel, int is_f64, int64_t n, const double *geom18, const double *los3,
                      double vscale, float *out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n >= 0 && geom18 && (is_f64 == 0 || is_f64 == 1), MCPM_E_ARG, "mcpm_box2cell_f32: bad argument");
    MCPM_REQUIRE(p, (pos && out) || n == 0, MCPM_E_ARG, "mcpm_box2cell_f32: null array");
    MCPM_REQUIRE(p, cell_geom_ok(geom18), MCPM_E_ARG, "mcpm_box2cell_f32: geometry must be finite with positive box_size and mesh_shape");
    MCPM_REQUIRE(p, !vel || (los3 && std::isfinite(vscale) && std::isfinite(los3[0]) && std::isfinite(los3[1]) && std::isfinite(los3[2])),
                 MCPM_E_ARG, "mcpm_box2cell_f32: velocities need a finite los and vscale");
    if (n == 0) return MCPM_OK;
    BoxGeom q{cell_geom(geom18), {0., 0., 0.}, 0.};
    if (vel) q.los[0] = los3[0], q.los[1] = los3[1], q.los[2] = los3[2], q.vscale = vscale;
    StageTimer st_(p, ST_AXPY, ((is_f64 ? 24.0 : 12.0) * (vel ? 2 : 1) + 12.0) * n);
    if (is_f64) box2cell_kernel<double><<<cat_blocks(n), 256, 0, p->stream>>>((const double *)pos, (const double *)vel, n, q, out);
    else box2cell_kernel<float><<<cat_blocks(n), 256, 0, p->stream>>>((const float *)pos, (const float *)vel, n, q, out);
    MCPM_LAUNCH_CHECK(p, "box2cell_kernel");
    return MCPM_OK;
}

int mcpm_footprint_u8(mcpm_plan *p, const float *pos, int64_t n, const float *weights, int order, unsigned char *mask, int accumulate) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, mask && (pos || n == 0) && n >= 0 && n < ((int64_t)1 << 31), MCPM_E_ARG, "mcpm_footprint_u8: bad argument");
    MCPM_REQUIRE(p, order >= 1 && order <= 4, MCPM_E_ORDER, "mcpm_footprint_u8: assignment order must be 1 (NGP), 2 (CIC), 3 (TSC) or 4 (PCS)");
    MCPM_REQUIRE(p, !p->g.xslab, MCPM_E_UNSUPPORTED, "mcpm_footprint_u8: not slab-decomposed");
    StageTimer st_(p, ST_PAINT, (weights ? 16.0 : 12.0) * n + 1.0 * p->M);
    if (!accumulate) MCPM_HIP(p, hipMemsetAsync(mask, 0, (size_t)p->M, p->stream));
    if (n == 0) return MCPM_OK;
    const unsigned nb = cat_blocks(n);
    if (order == 1) footprint_kernel<1><<<nb, 256, 0, p->stream>>>(p->g, pos, n, weights, mask, p->M);
    else if (order == 2) footprint_kernel<2><<<nb, 256, 0, p->stream>>>(p->g, pos, n, weights, mask, p->M);
    else if (order == 3) footprint_kernel<3><<<nb, 256, 0, p->stream>>>(p->g, pos, n, weights, mask, p->M);
    else footprint_kernel<4><<<nb, 256, 0, p->stream>>>(p->g, pos, n, weights, mask, p->M);
    MCPM_LAUNCH_CHECK(p, "footprint_kernel");
    return MCPM_OK;
}

int mcpm_masked_sum_f64(mcpm_plan *p, const float *mesh, const unsigned char *mask, int64_t n, double *out2) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n >= 0 && out2 && ((mesh && mask) || n == 0), MCPM_E_ARG, "mcpm_masked_sum_f64: bad argument");
    if (n == 0) {
        MCPM_HIP(p, hipMemsetAsync(out2, 0, 2 * sizeof(double), p->stream));
        return MCPM_OK;
    }
    const unsigned nb = cat_blocks(n);
    DetSum s;
    StageTimer st_(p, ST_AXPY, 5.0 * n);
    MCPM_TRY(mcpm_det_begin(p, 2, nb, &s));
    masked_sum_kernel<<<nb, 256, 0, p->stream>>>(mesh, mask, n, s.P);
    MCPM_LAUNCH_CHECK(p, "masked_sum_kernel");
    return mcpm_det_fold(p, s, 2, 1.0, det_outs_row(DET_STORE, out2, 2));
}

}  // extern "C"
