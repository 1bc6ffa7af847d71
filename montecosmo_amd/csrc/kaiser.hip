// Kaiser model on the curved sky and on the light cone (montecosmo/bricks.py:200-231, kaiser_model) and its VJP: the real-space pass
// that the flat-sky, fixed-a branch (diagonal in k, model.py) does not need.  Per cell of the evolution mesh, at
//   x = (i, j, k) box / shape - box / 2 + R^T centre      (cell axes: |R y + c| = |y + R^T c|, bricks.py:675-685)
// curved sky (C):  r = |x|, l = safe_div(x, r);   out = 1 + g(a) [ b1E tr T + f(a) sum_ij l_i l_j T_ij ] + fNL_bp phi,
//                  T_ij = irfftn(k_i k_j / k^2 lin) in the order 00 01 02 11 12 22; tr T = irfftn(lin) for a field without k = 0 mode;
// flat sky (F):    r = |x . l_flat|;              out = 1 + g(a) [ b1E delta + f(a) m2 ] + fNL_bp phi,   m2 = irfftn(mu^2 lin);
// a = a_obs (g, f host scalars) or chi2a(r) per cell (light cone: the clamped float64 look-ups of tables_dev.h, as observe.hip makes them).
// Branch and light cone are template arguments: the fixed-a instantiations carry no table code.  Streaming kernels, four cells along z per
// thread (float4 when nz % 4 == 0, element by element otherwise); scalar cotangents are per-workgroup partials folded in a fixed order
// (reduce_dev.h), table cotangents order-independent integer sums (tables_dev.h): every output is bitwise the same call after call.
#include "mcpm_internal.h"
#include "reduce_dev.h"
#include "tables_dev.h"

namespace {

struct KGeom {
    double cell[3], org[3];     // x_a = i_a cell[a] + org[a], org = -box / 2 + R^T centre
    float lf[3];                // flat-sky line of sight (cell axes)
    int nx, ny, nz, nq;         // nq = ceil(nz / 4) slots of four cells per z row
};
struct KPar {
    float g, f, b1E, fnl;       // g(a_obs), f(a_obs) (unused on the light cone), 1 + b1, fNL_bp
};
struct KCell {
    float l[3], g, f;
    double r;
};

template <int CURVED, int LC>
__device__ __forceinline__ void kaiser_cell(const KGeom &G, const LcTables &tb, const KPar &P, float x0, float x1, int iz, KCell &c) {
    const float x2 = (float)((double)iz * G.cell[2] + G.org[2]);
    float r;
    if (CURVED) {
        r = sqrtf(x0 * x0 + x1 * x1 + x2 * x2);
        const float ir = r == 0.f ? 0.f : 1.f / r;      // safe_div
        c.l[0] = x0 * ir, c.l[1] = x1 * ir, c.l[2] = x2 * ir;
    } else {
        r = fabsf(x0 * G.lf[0] + x1 * G.lf[1] + x2 * G.lf[2]);
        c.l[0] = c.l[1] = c.l[2] = 0.f;
    }
    c.r = (double)r;
    c.g = P.g, c.f = P.f;
    if (LC) {
        double s;
        const double a = interp1(c.r, tb.chi, tb.a_of_chi, tb.nchi, s);
        const Interp bg = interp_idx(a, tb.a, tb.g, tb.ngrow);
        double f, sf;
        interp_at(bg, tb.a, tb.f, f, sf);
        c.g = (float)bg.y, c.f = (float)f;
    }
}

// curved sky: (tr T, l . T l) of the six meshes; flat sky: (delta, m2) as they are
template <int CURVED>
__device__ __forceinline__ void kaiser_pair(const KCell &c, const float *t, float &d, float &q) {
    if (CURVED) {
        d = t[0] + t[3] + t[5];
        q = c.l[0] * c.l[0] * t[0] + c.l[1] * c.l[1] * t[3] + c.l[2] * c.l[2] * t[5] +
            2.f * (c.l[0] * c.l[1] * t[1] + c.l[0] * c.l[2] * t[2] + c.l[1] * c.l[2] * t[4]);
    } else {
        d = t[0], q = t[1];
    }
}

// slot -> (x0, x1) of its row, first z index, number of cells (< 4 only in a row's last slot), offset of the first cell
struct KSlot {
    float x0, x1;
    int z0, cnt;
    int64_t off;
};
__device__ __forceinline__ KSlot kaiser_slot(const KGeom &G, int64_t t) {
    KSlot s;
    const int q = (int)(t % G.nq);
    const int64_t row = t / G.nq;
    const int iy = (int)(row % G.ny), ix = (int)(row / G.ny);
    s.x0 = (float)((double)ix * G.cell[0] + G.org[0]);
    s.x1 = (float)((double)iy * G.cell[1] + G.org[1]);
    s.z0 = 4 * q;
    s.cnt = min(4, G.nz - s.z0);
    s.off = row * G.nz + s.z0;
    return s;
}
template <int VEC>
__device__ __forceinline__ void load4(const float *__restrict__ p, int cnt, float (&v)[4]) {
    if (VEC) {
        const float4 w = *reinterpret_cast<const float4 *>(p);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[j] : 0.f;
    }
}
template <int VEC>
__device__ __forceinline__ void store4(float *__restrict__ p, int cnt, const float (&v)[4]) {
    if (VEC) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) p[j] = v[j];
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int CURVED, int LC, int VEC>
__global__ __launch_bounds__(256) void kaiser_sky_kernel(KGeom G, LcTables tb, KPar P, const float *__restrict__ meshes, const float *__restrict__ phi,
                                                         int64_t M, int64_t nslot, float *__restrict__ out) {
    constexpr int NM = CURVED ? 6 : 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nslot) return;
    const KSlot s = kaiser_slot(G, t);
    float T[NM][4], ph[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
#pragma unroll
    for (int k = 0; k < NM; ++k) load4<VEC>(meshes + (size_t)k * M + s.off, s.cnt, T[k]);
    if (phi) load4<VEC>(phi + s.off, s.cnt, ph);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = 0.f;
        if (j >= s.cnt) continue;
        KCell c;
        kaiser_cell<CURVED, LC>(G, tb, P, s.x0, s.x1, s.z0 + j, c);
        float tj[NM], d, q;
#pragma unroll
        for (int k = 0; k < NM; ++k) tj[k] = T[k][j];
        kaiser_pair<CURVED>(c, tj, d, q);
        o[j] = 1.f + c.g * (P.b1E * d + c.f * q) + P.fnl * ph[j];
    }
    store4<VEC>(out + s.off, s.cnt, o);
}

// ---- adjoint ---------------------------------------------------------------------------------------------------------------
// mesh cotangents written, and per-workgroup partials of (b1E_bar, fNL_bp_bar, g_bar, f_bar); the last two are 0 on the light cone,
// where g and f are per-cell look-ups whose cotangents go to the tables (kaiser_tables_vjp_kernel)
template <int CURVED, int LC, int VEC>
__global__ __launch_bounds__(256) void kaiser_sky_vjp_kernel(KGeom G, LcTables tb, KPar P, const float *__restrict__ meshes,
                                                             const float *__restrict__ phi, const float *__restrict__ ob, int64_t M,
                                                             int64_t nslot, float *__restrict__ mb, float *__restrict__ phb,
                                                             double *__restrict__ part) {
    constexpr int NM = CURVED ? 6 : 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double red[4] = {0., 0., 0., 0.};
    if (t < nslot) {
        const KSlot s = kaiser_slot(G, t);
        float T[NM][4], Tb[NM][4], ph[4] = {0.f, 0.f, 0.f, 0.f}, b[4], pb[4];
#pragma unroll
        for (int k = 0; k < NM; ++k) load4<VEC>(meshes + (size_t)k * M + s.off, s.cnt, T[k]);
        if (phi) load4<VEC>(phi + s.off, s.cnt, ph);
        load4<VEC>(ob + s.off, s.cnt, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pb[j] = 0.f;
#pragma unroll
            for (int k = 0; k < NM; ++k) Tb[k][j] = 0.f;
            if (j >= s.cnt) continue;
            KCell c;
            kaiser_cell<CURVED, LC>(G, tb, P, s.x0, s.x1, s.z0 + j, c);
            float tj[NM], d, q;
#pragma unroll
            for (int k = 0; k < NM; ++k) tj[k] = T[k][j];
            kaiser_pair<CURVED>(c, tj, d, q);
            const float w = b[j], db = w * c.g * P.b1E, qb = w * c.g * c.f;
            if (CURVED) {
                Tb[0][j] = db + qb * c.l[0] * c.l[0];
                Tb[1][j] = 2.f * qb * c.l[0] * c.l[1];
                Tb[2][j] = 2.f * qb * c.l[0] * c.l[2];
                Tb[3][j] = db + qb * c.l[1] * c.l[1];
                Tb[4][j] = 2.f * qb * c.l[1] * c.l[2];
                Tb[5][j] = db + qb * c.l[2] * c.l[2];
            } else {
                Tb[0][j] = db;
                Tb[1][j] = qb;
            }
            pb[j] = P.fnl * w;
            red[0] += (double)w * (double)c.g * (double)d;
            red[1] += (double)w * (double)ph[j];
            if (!LC) {
                red[2] += (double)w * ((double)P.b1E * (double)d + (double)c.f * (double)q);
                red[3] += (double)w * (double)c.g * (double)q;
            }
        }
#pragma unroll
        for (int k = 0; k < NM; ++k) store4<VEC>(mb + (size_t)k * M + s.off, s.cnt, Tb[k]);
        if (phb) store4<VEC>(phb + s.off, s.cnt, pb);
    }
    block_partial<4>(red, part, gridDim.x, blockIdx.x);
}

// light cone: per cell g_bar = out_bar (b1E d + f q), f_bar = out_bar g q, and through a = chi2a(r) the cotangent of the chi nodes;
// accumulators chi_bar[nchi], g_bar[ngrow], f_bar[ngrow] (kinds 0, 1, 2), the layout of observe_tables_vjp_kernel
template <int CURVED, int PASS>
__global__ __launch_bounds__(256) void kaiser_tables_vjp_kernel(KGeom G, LcTables tb, KPar P, const float *__restrict__ meshes,
                                                                const float *__restrict__ ob, int64_t M, unsigned *__restrict__ mxbits,
                                                                unsigned long long *__restrict__ out) {
    extern __shared__ unsigned long long shl[];
    constexpr int NM = CURVED ? 6 : 2;
    const int ntot = tb.nchi + 2 * tb.ngrow;
    Acc<3> A;
    acc_begin(A, shl, ntot, mxbits, PASS);
    const int o_chi = 0, o_g = tb.nchi, o_f = tb.nchi + tb.ngrow;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int iz = (int)(i % G.nz);
        const int64_t row = i / G.nz;
        const int iy = (int)(row % G.ny), ix = (int)(row / G.ny);
        KCell c;
        kaiser_cell<CURVED, 0>(G, tb, P, (float)((double)ix * G.cell[0] + G.org[0]), (float)((double)iy * G.cell[1] + G.org[1]), iz, c);
        float tj[NM], d, q;
#pragma unroll
        for (int k = 0; k < NM; ++k) tj[k] = meshes[(size_t)k * M + i];
        kaiser_pair<CURVED>(c, tj, d, q);
        const Interp ba = interp_idx(c.r, tb.chi, tb.a_of_chi, tb.nchi);
        const Interp bg = interp_idx(ba.y, tb.a, tb.g, tb.ngrow);
        double f, sf;
        interp_at(bg, tb.a, tb.f, f, sf);
        const double w = (double)ob[i];
        const double gb = w * ((double)P.b1E * (double)d + (double)(float)f * (double)q), fb = w * (double)(float)bg.y * (double)q;
        const double ab = gb * bg.slope + fb * sf;
        bad = bad || !(gb == gb && fb == fb && ab == ab);
        scatter_fp<PASS>(A, 1, o_g, bg, gb);
        scatter_fp<PASS>(A, 2, o_f, bg, fb);
        scatter_xp<PASS>(A, 0, o_chi, ba, ab);
    }
    acc_end<PASS>(A, ntot, mxbits, out, bad);
}

struct KArgs {
    KGeom G;
    LcTables tb;
    KPar P;
    int curved, lc, vec;
    int64_t nslot;
};

int kaiser_args(mcpm_plan *p, const char *who, const double *geom, int flags, const double *tables, int nchi, int ngrow, double g_obs, double f_obs,
                double b1E, double fNL_bp, KArgs *out) {
    const std::string w(who);
    MCPM_REQUIRE(p, geom != nullptr, MCPM_E_ARG, w + ": bad argument");
    MCPM_REQUIRE(p, !p->g.xslab, MCPM_E_UNSUPPORTED, w + ": not slab-decomposed");
    MCPM_REQUIRE(p, !(flags & 2) || (tables && nchi >= 2 && ngrow >= 2), MCPM_E_ARG, w + ": light cone needs the tables");
    KArgs a{};
    const int n[3] = {p->g.nx, p->g.ny, p->g.nz};
    for (int i = 0; i < 3; ++i) {
        a.G.cell[i] = geom[i] / (double)n[i];
        a.G.org[i] = -0.5 * geom[i] + geom[3 + i];
        a.G.lf[i] = (float)geom[6 + i];
    }
    a.G.nx = n[0], a.G.ny = n[1], a.G.nz = n[2], a.G.nq = (n[2] + 3) / 4;
    a.curved = flags & 1, a.lc = (flags >> 1) & 1, a.vec = n[2] % 4 == 0;
    if (a.lc) a.tb = lc_tables(tables, nchi, ngrow);
    a.P = KPar{(float)g_obs, (float)f_obs, (float)b1E, (float)fNL_bp};
    a.nslot = (int64_t)n[0] * n[1] * a.G.nq;
    *out = a;
    return MCPM_OK;
}

#define KAISER_DISPATCH(K, A)                                                       \
    do {                                                                            \
        if ((A).curved) {                                                           \
            if ((A).lc) { if ((A).vec) { K(1, 1, 1); } else { K(1, 1, 0); } }       \
            else        { if ((A).vec) { K(1, 0, 1); } else { K(1, 0, 0); } }       \
        } else {                                                                    \
            if ((A).lc) { if ((A).vec) { K(0, 1, 1); } else { K(0, 1, 0); } }       \
            else        { if ((A).vec) { K(0, 0, 1); } else { K(0, 0, 0); } }       \
        }                                                                           \
    } while (0)

}  // namespace

extern "C" {

int mcpm_kaiser_sky_f32(mcpm_plan *p, const float *meshes, const float *phi, const double *geom, int flags, const double *tables, int nchi,
                        int ngrow, double g_obs, double f_obs, double b1E, double fNL_bp, float *out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, meshes && out, MCPM_E_ARG, "mcpm_kaiser_sky_f32: bad argument");
    KArgs a;
    MCPM_TRY(kaiser_args(p, "mcpm_kaiser_sky_f32", geom, flags, tables, nchi, ngrow, g_obs, f_obs, b1E, fNL_bp, &a));
    a.vec = a.vec && mcpm_aligned(meshes) && mcpm_aligned(phi) && mcpm_aligned(out);
    const unsigned nb = (unsigned)((a.nslot + 255) / 256);
    StageTimer st_(p, ST_LPT, (4.0 * (a.curved ? 6 : 2) + 4.0 + (phi ? 4.0 : 0.0)) * p->M);
#define K(C, L, V) kaiser_sky_kernel<C, L, V><<<nb, 256, 0, p->stream>>>(a.G, a.tb, a.P, meshes, phi, p->M, a.nslot, out)
    KAISER_DISPATCH(K, a);
#undef K
    MCPM_LAUNCH_CHECK(p, "kaiser_sky_kernel");
    return MCPM_OK;
}

int mcpm_kaiser_sky_vjp_f32(mcpm_plan *p, const float *meshes, const float *phi, const double *geom, int flags, const double *tables, int nchi,
                            int ngrow, double g_obs, double f_obs, double b1E, double fNL_bp, const float *out_bar, float *meshes_bar,
                            float *phi_bar, double *scalars_out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, meshes && out_bar && meshes_bar && scalars_out, MCPM_E_ARG, "mcpm_kaiser_sky_vjp_f32: bad argument");
    MCPM_REQUIRE(p, (phi == nullptr) == (phi_bar == nullptr), MCPM_E_ARG, "mcpm_kaiser_sky_vjp_f32: phi and phi_bar go together");
    KArgs a;
    MCPM_TRY(kaiser_args(p, "mcpm_kaiser_sky_vjp_f32", geom, flags, tables, nchi, ngrow, g_obs, f_obs, b1E, fNL_bp, &a));
    a.vec = a.vec && mcpm_aligned(meshes) && mcpm_aligned(phi) && mcpm_aligned(out_bar) && mcpm_aligned(meshes_bar) && mcpm_aligned(phi_bar);
    const unsigned nb = (unsigned)((a.nslot + 255) / 256);
    DetSum s;
    MCPM_TRY(mcpm_det_begin(p, 4, nb, &s));
    StageTimer st_(p, ST_LPT, (8.0 * (a.curved ? 6 : 2) + 4.0 + (phi ? 8.0 : 0.0)) * p->M);
#define K(C, L, V) \
    kaiser_sky_vjp_kernel<C, L, V><<<nb, 256, 0, p->stream>>>(a.G, a.tb, a.P, meshes, phi, out_bar, p->M, a.nslot, meshes_bar, phi_bar, s.P)
    KAISER_DISPATCH(K, a);
#undef K
    MCPM_LAUNCH_CHECK(p, "kaiser_sky_vjp_kernel");
    return mcpm_det_fold(p, s, 4, 1.0, det_outs_row(DET_STORE, scalars_out, 4));
}

int mcpm_kaiser_sky_tables_vjp_f32(mcpm_plan *p, const float *meshes, const double *geom, int flags, const double *tables, int nchi, int ngrow,
                                   double b1E, const float *out_bar, double *table_bar) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, meshes && out_bar && table_bar, MCPM_E_ARG, "mcpm_kaiser_sky_tables_vjp_f32: bad argument");
    MCPM_REQUIRE(p, (flags & 2) != 0, MCPM_E_ARG, "mcpm_kaiser_sky_tables_vjp_f32: light cone only (flags bit 1, tables)");
    KArgs a;
    MCPM_TRY(kaiser_args(p, "mcpm_kaiser_sky_tables_vjp_f32", geom, flags, tables, nchi, ngrow, 0., 0., b1E, 0., &a));
    TabSum t;
    MCPM_TRY(mcpm_tab_begin(p, "mcpm_kaiser_sky_tables_vjp_f32", MCPM_RED_TABLES, (size_t)nchi + 2 * (size_t)ngrow, p->M, &t));
    StageTimer st_(p, ST_LPT, 2.0 * (4.0 * (a.curved ? 6 : 2) + 4.0) * p->M);
#define K(C)                                                                                                                   \
    kaiser_tables_vjp_kernel<C, 0><<<t.nb, 256, 0, p->stream>>>(a.G, a.tb, a.P, meshes, out_bar, p->M, t.mx, t.acc);          \
    MCPM_LAUNCH_CHECK(p, "kaiser_tables_vjp_kernel");                                                                          \
    kaiser_tables_vjp_kernel<C, 1><<<t.nb, 256, t.lds, p->stream>>>(a.G, a.tb, a.P, meshes, out_bar, p->M, t.mx, t.acc);      \
    MCPM_LAUNCH_CHECK(p, "kaiser_tables_vjp_kernel")
    if (a.curved) { K(1); } else { K(0); }
#undef K
    const int kind_end[3] = {nchi, nchi + ngrow, t.ntot};      // chi, g, f
    return mcpm_tab_finish(p, t, kind_end, 3, table_bar);
}

}  // extern "C"
