// Evolved particles -> redshift-space positions on the paint mesh (montecosmo/model.py:780-797):
//   los, a   = los_scalefactor_pos(pos)                      bricks.py:750-768
//   pos_phys = cell2phys_pos(pos)                            bricks.py:628-636
//   pos_phys += rsd(vel, los, a, dvel)                       bricks.py:791-803
//   pos_phys = ap_auto(pos_phys) | ap_param(pos_phys)        bricks.py:795-814, :848-857 (Alcock-Paczynski; the *_ap_* entry points)
//   pos_out  = phys2cell_pos(pos_phys, paint_shape)          bricks.py:638-646
// fused into one pass with its VJP.  cell2phys then phys2cell with the same box cancel exactly, so the kernel evaluates
//   out = x * (cell_e / cell_p) + R^T [ (V . l) l ] / cell_p,   V = R (vel * cell_e) g(a) f(a) + dvel,
// P = R (x * cell_e - box/2) + centre, l = P/|P| (curved sky) or centre/|centre| (flat), a = chi2a(|P|) or |P . l|,
// which keeps the displacement-from-lattice encoding of the positions (no box-sized float32 round trip).
// Light cone: a and g(a) f(a) come from the same two linear-interpolation tables as the host (chi -> a, a -> g, f).
// Alcock-Paczynski: with P' = P + (V . l) l the remapped position is alpha P' (auto: alpha = a2chi(cosmo_fid, chi2a(cosmo, r')) / r',
// r' = |P'| or |P' . l_flat|; param: alpha_iso, or alpha_par / alpha_perp along / across l_flat).  It is evaluated as
//   out += R^T [ c1 P' + c2 (P' . l_flat) l_flat ] / cell_p,   c1 = alpha - 1 (alpha_perp - 1 on the flat sky), c2 = alpha_par - alpha_perp,
// with the auto c1 = (rho - r') / r' formed in float64 from the tables: the small difference of two distances of thousands of Mpc/h
// never passes through float32.
#include "mcpm_internal.h"
#include "reduce_dev.h"
#include "tables_dev.h"

namespace {

struct Obs {
    float R[9];                 // box_rot matrix, row major: apply(x) = R x
    float ce[3], cp[3];         // cell lengths (Mpc/h) of the evolution and paint meshes
    float hb[3], ctr[3];        // box_size / 2, box_center
    float lf[3];                // flat-sky line of sight
    int curved, lightcone;
    float gf;                   // g(a_obs) f(a_obs) when not on the light cone
};

// Alcock-Paczynski stage.  mode: MCPM_AP_NONE / MCPM_AP_AUTO / MCPM_AP_PARAM (a template argument of the kernels).
struct Ap {
    float c1, c2;                               // param: alpha - 1 (curved) or alpha_perp - 1, alpha_par - alpha_perp (flat)
    double dc[4];                               // param: d c1 / d alpha_iso, d c2 / d alpha_iso, d c1 / d alpha_ap, d c2 / d alpha_ap
    const double *chi, *a_of_chi, *afid, *chifid;   // auto (device float64): chi ascending -> a of the sampled cosmology; a ascending -> chi_fid
    int nap, nfid;
};

__device__ __forceinline__ void rot(const float (&R)[9], const float (&v)[3], float (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}
__device__ __forceinline__ void rot_t(const float (&R)[9], const float (&v)[3], float (&o)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = R[j] * v[0] + R[3 + j] * v[1] + R[6 + j] * v[2];
}

struct Fwd {
    float x[3], P[3], l[3], r, sgn, gf, dgf_dr, Vr[3], V[3], s;
};

// common forward evaluation of one particle; x = absolute cell coordinates on the evolution mesh
__device__ __forceinline__ void forward(const Obs &og, const LcTables &tb, const float (&x)[3], const float (&vel)[3],
                                        const float (&dv)[3], Fwd &w) {
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = x[a] * og.ce[a] - og.hb[a];
    rot(og.R, t, w.P);
#pragma unroll
    for (int a = 0; a < 3; ++a) w.P[a] += og.ctr[a];
    w.sgn = 1.f;
    if (og.curved) {
        w.r = sqrtf(w.P[0] * w.P[0] + w.P[1] * w.P[1] + w.P[2] * w.P[2]);
        const float ir = w.r == 0.f ? 0.f : 1.f / w.r;   // safe_div
#pragma unroll
        for (int a = 0; a < 3; ++a) w.l[a] = w.P[a] * ir;
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) w.l[a] = og.lf[a];
        const float d = w.P[0] * w.l[0] + w.P[1] * w.l[1] + w.P[2] * w.l[2];
        w.sgn = d < 0.f ? -1.f : 1.f;
        w.r = fabsf(d);
    }
    w.gf = og.gf;
    w.dgf_dr = 0.f;
    if (og.lightcone) {
        double da_dr, dg_da, df_da;
        const double a = interp1((double)w.r, tb.chi, tb.a_of_chi, tb.nchi, da_dr);
        const double g = interp1(a, tb.a, tb.g, tb.ngrow, dg_da), f = interp1(a, tb.a, tb.f, tb.ngrow, df_da);
        w.gf = (float)(g * f);
        w.dgf_dr = (float)((dg_da * f + g * df_da) * da_dr);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = vel[a] * og.ce[a];
    rot(og.R, t, w.Vr);
#pragma unroll
    for (int a = 0; a < 3; ++a) w.V[a] = w.Vr[a] * w.gf + dv[a];
    w.s = w.V[0] * w.l[0] + w.V[1] * w.l[1] + w.V[2] * w.l[2];
}

struct ApW {
    float Pp[3], c1, dl, dc1_dr, sgn, rp, ir;   // P', c1, P' . l_flat, d c1 / d r', sign(P' . l_flat), r', 1 / r' (0 at r' = 0)
};

// Alcock-Paczynski displacement D = alpha(P') P' - P' of one particle (Mpc/h), to be added to the RSD displacement
template <int AP>
__device__ __forceinline__ void ap_forward(const Obs &og, const Ap &ap, const Fwd &w, ApW &q, float (&D)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q.Pp[a] = w.P[a] + w.s * w.l[a];
    float rp;
    q.sgn = 1.f;
    q.dl = 0.f;
    if (og.curved) {
        rp = sqrtf(q.Pp[0] * q.Pp[0] + q.Pp[1] * q.Pp[1] + q.Pp[2] * q.Pp[2]);
    } else {
        q.dl = q.Pp[0] * og.lf[0] + q.Pp[1] * og.lf[1] + q.Pp[2] * og.lf[2];
        q.sgn = q.dl < 0.f ? -1.f : 1.f;
        rp = fabsf(q.dl);
    }
    q.rp = rp;
    q.ir = rp == 0.f ? 0.f : 1.f / rp;
    q.c1 = ap.c1;
    q.dc1_dr = 0.f;
    if (AP == MCPM_AP_AUTO) {
        q.c1 = -1.f;                                 // safe_div(rho, 0) = 0
        if (rp != 0.f) {
            const double r = (double)rp;
            double sc, sf;
            const double a = interp1(r, ap.chi, ap.a_of_chi, ap.nap, sc);
            const double rho = interp1(a, ap.afid, ap.chifid, ap.nfid, sf);
            q.c1 = (float)((rho - r) / r);
            q.dc1_dr = (float)((sc * sf - rho / r) / r);
        }
    }
    const float c2d = (AP == MCPM_AP_PARAM && !og.curved) ? ap.c2 * q.dl : 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) D[a] = q.c1 * q.Pp[a] + c2d * og.lf[a];
}

// Db: cotangent of the displacement D (and of the RSD displacement: the same R (out_bar / cell_p)).  Returns the cotangent of P'
// and the cotangents of c1 and c2.
template <int AP>
__device__ __forceinline__ void ap_backward(const Obs &og, const Ap &ap, const ApW &q, const float (&Db)[3], float (&Ppb)[3], float &c1b,
                                            float &c2b) {
    c1b = Db[0] * q.Pp[0] + Db[1] * q.Pp[1] + Db[2] * q.Pp[2];
    const float dbl = Db[0] * og.lf[0] + Db[1] * og.lf[1] + Db[2] * og.lf[2];
    const bool par = AP == MCPM_AP_PARAM && !og.curved;
    c2b = par ? dbl * q.dl : 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) Ppb[a] = q.c1 * Db[a] + (par ? ap.c2 * dbl * og.lf[a] : 0.f);
    if (AP == MCPM_AP_AUTO) {
        const float rb = c1b * q.dc1_dr;             // through r'
#pragma unroll
        for (int a = 0; a < 3; ++a) Ppb[a] += og.curved ? rb * q.Pp[a] * q.ir : rb * q.sgn * og.lf[a];
    }
}

__device__ __forceinline__ void lattice_point(const Geom &g, int64_t i, float (&q)[3]) {
    const int ipz = (int)(i % g.pz);
    const int64_t t = i / g.pz;
    const int ipy = (int)(t % g.py), ipx = (int)(t / g.py);
    q[0] = (float)((double)ipx * g.nx / g.px);
    q[1] = (float)((double)ipy * g.ny / g.py);
    q[2] = (float)((double)ipz * g.nz / g.pz);
}

template <int MODE, int AP>
__global__ __launch_bounds__(256) void observe_kernel(Geom g, Obs og, LcTables tb, Ap ap, const float *__restrict__ pos,
                                                      const float *__restrict__ vel, const float *__restrict__ dvel, int64_t n,
                                                      float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float q[3] = {0.f, 0.f, 0.f}, d[3], x[3], v[3], dv[3] = {0.f, 0.f, 0.f};
    if (MODE == MCPM_POS_LATTICE) lattice_point(g, i, q);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = pos[3 * i + a];
        x[a] = q[a] + d[a];
        v[a] = vel[3 * i + a];
        if (dvel) dv[a] = dvel[3 * i + a];
    }
    Fwd w;
    forward(og, tb, x, v, dv, w);
    float D[3] = {w.s * w.l[0], w.s * w.l[1], w.s * w.l[2]}, Dr[3];
    rot_t(og.R, D, Dr);
    if (AP == MCPM_AP_NONE) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 * i + a] = d[a] * (og.ce[a] / og.cp[a]) + Dr[a] / og.cp[a];  // lattice mode: displacement from q * ce/cp
    } else {
        ApW aw;
        float A[3], Ar[3];
        ap_forward<AP>(og, ap, w, aw, A);
        rot_t(og.R, A, Ar);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 * i + a] = d[a] * (og.ce[a] / og.cp[a]) + Dr[a] / og.cp[a] + Ar[a] / og.cp[a];
    }
}

template <int MODE, int AP>
__global__ __launch_bounds__(256) void observe_vjp_kernel(Geom g, Obs og, LcTables tb, Ap ap, const float *__restrict__ pos,
                                                          const float *__restrict__ vel, const float *__restrict__ dvel, int64_t n,
                                                          const float *__restrict__ ob, float *__restrict__ pos_bar,
                                                          float *__restrict__ vel_bar, float *__restrict__ dvel_bar, double *part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    constexpr int NR = AP == MCPM_AP_NONE ? 1 : 3;      // gf_bar [, alpha_iso_bar, alpha_ap_bar]
    double red[NR] = {};
    if (i < n) {
        float q[3] = {0.f, 0.f, 0.f}, x[3], v[3], dv[3] = {0.f, 0.f, 0.f}, o[3];
        if (MODE == MCPM_POS_LATTICE) lattice_point(g, i, q);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            x[a] = q[a] + pos[3 * i + a];
            v[a] = vel[3 * i + a];
            if (dvel) dv[a] = dvel[3 * i + a];
            o[a] = ob[3 * i + a];
        }
        Fwd w;
        forward(og, tb, x, v, dv, w);
        float t[3], Db[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a] = o[a] / og.cp[a];
        rot(og.R, t, Db);                                                   // D_bar = R (out_bar / cell_p)
        float Ppb[3] = {0.f, 0.f, 0.f};
        if constexpr (AP != MCPM_AP_NONE) {      // P' = P + s l: its cotangent joins D_bar on the way to s and l, and goes to P directly
            ApW aw;
            float A[3], c1b, c2b;
            ap_forward<AP>(og, ap, w, aw, A);
            ap_backward<AP>(og, ap, aw, Db, Ppb, c1b, c2b);
            if constexpr (AP == MCPM_AP_PARAM) {
                red[NR - 2] = (double)c1b * ap.dc[0] + (double)c2b * ap.dc[1];
                red[NR - 1] = (double)c1b * ap.dc[2] + (double)c2b * ap.dc[3];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) Db[a] += Ppb[a];
        }
        const float sb = Db[0] * w.l[0] + Db[1] * w.l[1] + Db[2] * w.l[2];  // s_bar
        float lb[3], Vb[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lb[a] = w.s * Db[a] + sb * w.V[a];
            Vb[a] = sb * w.l[a];
        }
        const float gfb = Vb[0] * w.Vr[0] + Vb[1] * w.Vr[1] + Vb[2] * w.Vr[2];
        float vt[3];
        rot_t(og.R, Vb, vt);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            vel_bar[3 * i + a] = vt[a] * og.ce[a] * w.gf;
            if (dvel_bar) dvel_bar[3 * i + a] = Vb[a];
        }
        float Pb[3];
        const float rb = gfb * w.dgf_dr;
        if (og.curved) {
            const float ir = w.r == 0.f ? 0.f : 1.f / w.r;
            const float ll = lb[0] * w.l[0] + lb[1] * w.l[1] + lb[2] * w.l[2];
#pragma unroll
            for (int a = 0; a < 3; ++a) Pb[a] = (lb[a] - ll * w.l[a]) * ir + rb * w.l[a];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) Pb[a] = rb * w.sgn * w.l[a];
        }
        if constexpr (AP != MCPM_AP_NONE) {
#pragma unroll
            for (int a = 0; a < 3; ++a) Pb[a] += Ppb[a];
        }
        float xt[3];
        rot_t(og.R, Pb, xt);
#pragma unroll
        for (int a = 0; a < 3; ++a) pos_bar[3 * i + a] = o[a] * (og.ce[a] / og.cp[a]) + xt[a] * og.ce[a];
        red[0] = og.lightcone ? 0. : (double)gfb;
    }
    block_partial<NR>(red, part, gridDim.x, blockIdx.x);
}


// Lagrangian side (model.py:740-764): a_q = chi2a(r0_q) kept in float32, then a2g(a_q) (bias weights and lpt), a2g2(a_q),
// a2dg2dg(a_q) = safe_div(g2 f2, g f) (lpt).  Cotangents per particle: gB (of a2g), g2B (of a2g2 = -3/7 g2raw), dB (of a2dg2dg).
// tables: chi[nchi] ascending, a(chi)[nchi], a[ng], g[ng], g2raw[ng], f[ng], f2[ng];  accumulators: chi_bar[nchi], g_bar, g2raw_bar, f_bar, f2_bar.
template <int PASS>
__global__ __launch_bounds__(256) void lightcone_tables_vjp_kernel(const float *__restrict__ r0, int64_t n, const double *__restrict__ tb,
                                                                   int nchi, int ng, const float *__restrict__ gB,
                                                                   const float *__restrict__ g2B, const float *__restrict__ dB,
                                                                   unsigned *__restrict__ mxbits, unsigned long long *__restrict__ out) {
    extern __shared__ unsigned long long shl[];
    const int ntot = nchi + 4 * ng;
    Acc<5> A;
    acc_begin(A, shl, ntot, mxbits, PASS);
    const double *chi = tb, *aoc = tb + nchi, *ag = tb + 2 * nchi, *tg = ag + ng, *tg2 = tg + ng, *tf = tg2 + ng, *tf2 = tf + ng;
    const int o_chi = 0, o_g = nchi, o_g2 = nchi + ng, o_f = nchi + 2 * ng, o_f2 = nchi + 3 * ng;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const Interp ba = interp_idx((double)r0[i], chi, aoc, nchi);
        const double a = (double)(float)ba.y;                 // the forward pass hands a on as float32 (mcpm_interp_f32)
        const Interp bg = interp_idx(a, ag, tg, ng);
        double g = bg.y, sg = bg.slope, g2r, sg2, f, sf, f2, sf2;
        interp_at(bg, ag, tg2, g2r, sg2);
        interp_at(bg, ag, tf, f, sf);
        interp_at(bg, ag, tf2, f2, sf2);
        double gb = (double)gB[i], g2rb = 0., fb = 0., f2b = 0.;
        if (g2B) g2rb += (-3. / 7.) * (double)g2B[i];
        if (dB) {
            const double den = g * f, db = (double)dB[i];
            if (den != 0.) {                                   // a2dg2dg = (-3/7 g2r f2) / (g f), safe_div
                const double q = (-3. / 7.) * g2r * f2 / den;
                gb += -db * q / g;
                fb += -db * q / f;
                g2rb += db * (-3. / 7.) * f2 / den;
                f2b += db * (-3. / 7.) * g2r / den;
            }
        }
        const double ab = gb * sg + g2rb * sg2 + fb * sf + f2b * sf2;
        bad = bad || !(gb == gb && g2rb == g2rb && fb == fb && f2b == f2b && ab == ab);
        scatter_fp<PASS>(A, 1, o_g, bg, gb);
        scatter_fp<PASS>(A, 2, o_g2, bg, g2rb);
        scatter_fp<PASS>(A, 3, o_f, bg, fb);
        scatter_fp<PASS>(A, 4, o_f2, bg, f2b);
        scatter_xp<PASS>(A, 0, o_chi, ba, ab);
    }
    acc_end<PASS>(A, ntot, mxbits, out, bad);
}

// Eulerian side (model.py:781-784): gf_p = a2g(a_p) a2f(a_p), a_p = chi2a(r_p) at the evolved particle's distance.
// tables as in observe_kernel (chi, a(chi), a, g, f);  accumulators: chi_bar[nchi], g_bar[ngrow], f_bar[ngrow] (kinds 0, 1, 2).
// Automatic Alcock-Paczynski (bricks.py:799-801): rho = a2chi(cosmo_fid, chi2a(cosmo, r')) moves with the NODES of the chi -> a
// look-up at r' (the fiducial table is constant): a_bar = rho_bar d chi_fid / d a goes into the same chi_bar accumulator.  Off the
// light cone (og.lightcone = 0, ngrow = 0) that is the only contribution.
template <int MODE, int AP, int PASS>
__global__ __launch_bounds__(256) void observe_tables_vjp_kernel(Geom g, Obs og, LcTables tb, Ap ap, const float *__restrict__ pos,
                                                                 const float *__restrict__ vel, const float *__restrict__ dvel, int64_t n,
                                                                 const float *__restrict__ ob, unsigned *__restrict__ mxbits,
                                                                 unsigned long long *__restrict__ out) {
    extern __shared__ unsigned long long shl[];
    const int ntot = tb.nchi + 2 * tb.ngrow;
    Acc<3> A;
    acc_begin(A, shl, ntot, mxbits, PASS);
    const int o_chi = 0, o_g = tb.nchi, o_f = tb.nchi + tb.ngrow;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float q[3] = {0.f, 0.f, 0.f}, x[3], v[3], dv[3] = {0.f, 0.f, 0.f}, o[3];
        if (MODE == MCPM_POS_LATTICE) lattice_point(g, i, q);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            x[a] = q[a] + pos[3 * i + a];
            v[a] = vel[3 * i + a];
            if (dvel) dv[a] = dvel[3 * i + a];
            o[a] = ob[3 * i + a];
        }
        Fwd w;
        forward(og, tb, x, v, dv, w);
        float t[3], Db[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a] = o[a] / og.cp[a];
        rot(og.R, t, Db);
        if constexpr (AP != MCPM_AP_NONE) {
            ApW aw;
            float D[3], Ppb[3], c1b, c2b;
            ap_forward<AP>(og, ap, w, aw, D);
            ap_backward<AP>(og, ap, aw, Db, Ppb, c1b, c2b);
            if (AP == MCPM_AP_AUTO && aw.rp != 0.f) {
                const Interp bp = interp_idx((double)aw.rp, ap.chi, ap.a_of_chi, ap.nap);
                double sfid;
                interp1(bp.y, ap.afid, ap.chifid, ap.nfid, sfid);
                const double apb = (double)c1b / (double)aw.rp * sfid;      // rho_bar = c1_bar / r';  a_bar = rho_bar d chi_fid / d a
                bad = bad || !(apb == apb);
                scatter_xp<PASS>(A, 0, o_chi, bp, apb);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) Db[a] += Ppb[a];      // the growth product moves P' = P + s l as well
        }
        if (og.lightcone) {
            const float sb = Db[0] * w.l[0] + Db[1] * w.l[1] + Db[2] * w.l[2];
            const double gfb = (double)sb * ((double)w.l[0] * w.Vr[0] + (double)w.l[1] * w.Vr[1] + (double)w.l[2] * w.Vr[2]);
            const Interp ba = interp_idx((double)w.r, tb.chi, tb.a_of_chi, tb.nchi);
            const Interp bg = interp_idx(ba.y, tb.a, tb.g, tb.ngrow);
            double f, sf;
            interp_at(bg, tb.a, tb.f, f, sf);
            const double gb = gfb * f, fb = gfb * bg.y, ab = gb * bg.slope + fb * sf;
            bad = bad || !(gb == gb && fb == fb && ab == ab);
            scatter_fp<PASS>(A, 1, o_g, bg, gb);
            scatter_fp<PASS>(A, 2, o_f, bg, fb);
            scatter_xp<PASS>(A, 0, o_chi, ba, ab);
        }
    }
    acc_end<PASS>(A, ntot, mxbits, out, bad);
}

Obs make_obs(const mcpm_plan *p, const float *geom, int flags) {
    Obs og;
    for (int i = 0; i < 9; ++i) og.R[i] = geom[i];
    const int ms[3] = {p->g.nx, p->g.ny, p->g.nz};
    float cn = 0.f;
    for (int a = 0; a < 3; ++a) {
        og.ce[a] = geom[9 + a] / (float)ms[a];
        og.cp[a] = geom[9 + a] / geom[15 + a];
        og.hb[a] = 0.5f * geom[9 + a];
        og.ctr[a] = geom[12 + a];
        cn += geom[12 + a] * geom[12 + a];
    }
    cn = sqrtf(cn);
    for (int a = 0; a < 3; ++a) og.lf[a] = cn == 0.f ? 0.f : geom[12 + a] / cn;
    og.curved = flags & 1;
    og.lightcone = (flags >> 1) & 1;
    og.gf = geom[18];
    return og;
}

// Alcock-Paczynski arguments of the *_ap_* entry points -> the kernels' struct.  ap_tables (device float64) = chi ascending [nap],
// a(chi) [nap] of the sampled cosmology, a ascending [nfid], chi_fid(a) [nfid] of the fiducial one.
int make_ap(mcpm_plan *p, const char *who, int curved, int lightcone, int nchi, int ap_mode, double alpha_iso, double alpha_ap,
            const double *t, int nap, int nfid, Ap *out) {
    Ap ap{};
    MCPM_REQUIRE(p, ap_mode == MCPM_AP_NONE || ap_mode == MCPM_AP_AUTO || ap_mode == MCPM_AP_PARAM, MCPM_E_ARG, std::string(who) + ": bad ap_mode");
    if (ap_mode == MCPM_AP_AUTO) {
        MCPM_REQUIRE(p, t && nap >= 2 && nfid >= 2, MCPM_E_ARG, std::string(who) + ": automatic Alcock-Paczynski needs ap_tables");
        MCPM_REQUIRE(p, !lightcone || nap == nchi, MCPM_E_ARG, std::string(who) + ": on the light cone ap_tables' chi nodes are those of tables (nap = nchi)");
        ap.chi = t, ap.a_of_chi = t + nap, ap.afid = t + 2 * nap, ap.chifid = t + 2 * nap + nfid;
        ap.nap = nap, ap.nfid = nfid;
    } else if (ap_mode == MCPM_AP_PARAM) {
        MCPM_REQUIRE(p, std::isfinite(alpha_iso), MCPM_E_ARG, std::string(who) + ": alpha_iso must be finite");
        MCPM_REQUIRE(p, curved || (alpha_ap > 0. && std::isfinite(alpha_ap)), MCPM_E_ARG, std::string(who) + ": alpha_ap must be positive and finite");
        if (curved) {                                   // bricks.py:852-853
            ap.c1 = (float)(alpha_iso - 1.), ap.c2 = 0.f;
            ap.dc[0] = 1.;
        } else {                                        // bricks.py:726-732, :855-856
            const double m = std::pow(alpha_ap, -1. / 3.), q = std::pow(alpha_ap, 2. / 3.);      // alpha_perp, alpha_par over alpha_iso
            ap.c1 = (float)(alpha_iso * m - 1.), ap.c2 = (float)(alpha_iso * (q - m));
            ap.dc[0] = m, ap.dc[1] = q - m;
            ap.dc[2] = -alpha_iso * m / (3. * alpha_ap), ap.dc[3] = alpha_iso * (2. * q + m) / (3. * alpha_ap);
        }
    }
    *out = ap;
    return MCPM_OK;
}

// What the three *_ap_* entry points share: the argument checks (ptrs_ok: the entry point's own required pointers) and the kernels' structs
struct ObsArgs {
    Obs og;
    LcTables tb;
    Ap ap;
};
int obs_args(mcpm_plan *p, const char *who, bool ptrs_ok, const float *pos, const float *vel, int64_t n, int mode, const float *geom, int flags,
             const double *tables, int nchi, int ngrow, int ap_mode, double alpha_iso, double alpha_ap, const double *ap_tables, int nap, int nfid,
             ObsArgs *a) {
    const std::string w(who);
    MCPM_REQUIRE(p, pos && vel && geom && ptrs_ok && n > 0, MCPM_E_ARG, w + ": bad argument");
    MCPM_REQUIRE(p, mode == MCPM_POS_ABSOLUTE || (mode == MCPM_POS_LATTICE && n == p->Np), MCPM_E_ARG, w + ": bad pos_mode / count");
    MCPM_REQUIRE(p, !(flags & 2) || (tables && nchi >= 2 && ngrow >= 2), MCPM_E_ARG, w + ": light cone needs the tables");
    a->og = make_obs(p, geom, flags);
    a->tb = lc_tables(tables, nchi, ngrow);
    return make_ap(p, who, a->og.curved, a->og.lightcone, nchi, ap_mode, alpha_iso, alpha_ap, ap_tables, nap, nfid, &a->ap);
}

#define OBS_DISPATCH(K, MO, AP, ...)                                                                    \
    do {                                                                                                \
        if ((MO) == MCPM_POS_LATTICE) {                                                                 \
            if ((AP) == MCPM_AP_NONE) { K(MCPM_POS_LATTICE, MCPM_AP_NONE); }                            \
            else if ((AP) == MCPM_AP_AUTO) { K(MCPM_POS_LATTICE, MCPM_AP_AUTO); }                       \
            else { K(MCPM_POS_LATTICE, MCPM_AP_PARAM); }                                                \
        } else {                                                                                        \
            if ((AP) == MCPM_AP_NONE) { K(MCPM_POS_ABSOLUTE, MCPM_AP_NONE); }                           \
            else if ((AP) == MCPM_AP_AUTO) { K(MCPM_POS_ABSOLUTE, MCPM_AP_AUTO); }                      \
            else { K(MCPM_POS_ABSOLUTE, MCPM_AP_PARAM); }                                               \
        }                                                                                               \
    } while (0)

}  // namespace

extern "C" {

// geom (host, 19 floats) = R[9] row major, box_size[3], box_center[3], paint_shape[3] (as floats), g(a_obs) f(a_obs).
// flags: bit 0 = curved sky, bit 1 = light cone (then the four tables, float64 on the DEVICE: chi ascending [nchi],
// a(chi) [nchi], a [ngrow], g [ngrow], f [ngrow] -- the host's growth / distance tables).  pos / out follow pos_mode:
// MCPM_POS_LATTICE: displacements from the plan's particle lattice on the evolution mesh in, displacements from the same
// lattice scaled to the paint mesh out; MCPM_POS_ABSOLUTE: absolute cell coordinates in and out.
int mcpm_observe_pos_ap_f32(mcpm_plan *p, const float *pos, const float *vel, const float *dvel, int64_t n, int mode,
                            const float *geom, int flags, const double *tables, int nchi, int ngrow, int ap_mode, double alpha_iso,
                            double alpha_ap, const double *ap_tables, int nap, int nfid, float *out) {
    if (!p) return MCPM_E_ARG;
    ObsArgs a;
    MCPM_TRY(obs_args(p, "mcpm_observe_pos_ap_f32", out != nullptr, pos, vel, n, mode, geom, flags, tables, nchi, ngrow, ap_mode, alpha_iso, alpha_ap,
                      ap_tables, nap, nfid, &a));
    const unsigned nb = (unsigned)((n + 255) / 256);
    StageTimer st_(p, ST_LPT, (dvel ? 48.0 : 36.0) * n);
#define K(MO, AP) observe_kernel<MO, AP><<<nb, 256, 0, p->stream>>>(p->g, a.og, a.tb, a.ap, pos, vel, dvel, n, out)
    OBS_DISPATCH(K, mode, ap_mode);
#undef K
    MCPM_LAUNCH_CHECK(p, "observe_kernel");
    return MCPM_OK;
}

int mcpm_observe_pos_f32(mcpm_plan *p, const float *pos, const float *vel, const float *dvel, int64_t n, int mode,
                         const float *geom, int flags, const double *tables, int nchi, int ngrow, float *out) {
    return mcpm_observe_pos_ap_f32(p, pos, vel, dvel, n, mode, geom, flags, tables, nchi, ngrow, MCPM_AP_NONE, 1., 1., nullptr, 0, 0, out);
}

// VJP: out_bar (n,3) -> pos_bar, vel_bar, dvel_bar (NULL if dvel was NULL) and gf_bar (device double; the cotangent of the
// scalar g(a_obs) f(a_obs); 0 on the light cone, where the growth dependence on the particle distance is already in pos_bar
// and the dependence of the tables on the cosmology is left to mcpm_observe_pos_ap_tables_vjp_f32).  alpha_bar (device double[2],
// NULL allowed with MCPM_AP_NONE): cotangents of alpha_iso and alpha_ap (0 unless MCPM_AP_PARAM; alpha_ap_bar = 0 on a curved sky).
int mcpm_observe_pos_ap_vjp_f32(mcpm_plan *p, const float *pos, const float *vel, const float *dvel, int64_t n, int mode,
                                const float *geom, int flags, const double *tables, int nchi, int ngrow, int ap_mode, double alpha_iso,
                                double alpha_ap, const double *ap_tables, int nap, int nfid, const float *out_bar, float *pos_bar,
                                float *vel_bar, float *dvel_bar, double *gf_bar, double *alpha_bar) {
    if (!p) return MCPM_E_ARG;
    ObsArgs a;
    MCPM_TRY(obs_args(p, "mcpm_observe_pos_ap_vjp_f32", out_bar && pos_bar && vel_bar && gf_bar, pos, vel, n, mode, geom, flags, tables, nchi, ngrow,
                      ap_mode, alpha_iso, alpha_ap, ap_tables, nap, nfid, &a));
    MCPM_REQUIRE(p, (dvel == nullptr) == (dvel_bar == nullptr), MCPM_E_ARG, "mcpm_observe_pos_ap_vjp_f32: dvel and dvel_bar go together");
    MCPM_REQUIRE(p, ap_mode == MCPM_AP_NONE || alpha_bar, MCPM_E_ARG, "mcpm_observe_pos_ap_vjp_f32: alpha_bar is required with Alcock-Paczynski");
    DetSum s;
    const unsigned nb = (unsigned)((n + 255) / 256);
    const int nred = ap_mode == MCPM_AP_NONE ? 1 : 3;
    StageTimer st_(p, ST_LPT, (dvel ? 84.0 : 60.0) * n);
    MCPM_TRY(mcpm_det_begin(p, nred, nb, &s));
#define K(MO, AP) observe_vjp_kernel<MO, AP><<<nb, 256, 0, p->stream>>>(p->g, a.og, a.tb, a.ap, pos, vel, dvel, n, out_bar, pos_bar, vel_bar, dvel_bar, s.P)
    OBS_DISPATCH(K, mode, ap_mode);
#undef K
    MCPM_LAUNCH_CHECK(p, "observe_vjp_kernel");
    return mcpm_det_fold(p, s, nred, 1.0, nred == 3 ? det_outs_ptrs(DET_STORE, gf_bar, alpha_bar, alpha_bar + 1) : det_outs_ptrs(DET_STORE, gf_bar));
}

int mcpm_observe_pos_vjp_f32(mcpm_plan *p, const float *pos, const float *vel, const float *dvel, int64_t n, int mode,
                             const float *geom, int flags, const double *tables, int nchi, int ngrow, const float *out_bar,
                             float *pos_bar, float *vel_bar, float *dvel_bar, double *gf_bar) {
    return mcpm_observe_pos_ap_vjp_f32(p, pos, vel, dvel, n, mode, geom, flags, tables, nchi, ngrow, MCPM_AP_NONE, 1., 1., nullptr, 0, 0,
                                       out_bar, pos_bar, vel_bar, dvel_bar, gf_bar, nullptr);
}

// Light cone, Lagrangian side: table cotangents of the look-ups a_q = chi2a(r0_q), a2g / a2g2 / a2dg2dg (a_q) (see
// lightcone_tables_vjp_kernel).  tables (device float64): chi[nchi] ascending, a(chi)[nchi], a[ngrow], g, g2 (raw table, without
// the -3/7), f, f2 [ngrow each]; g_bar (n) is required, g2_bar / dg2dg_bar may be NULL.  table_bar (device float64, OVERWRITTEN):
// chi_bar[nchi], g_bar[ngrow], g2_bar[ngrow], f_bar[ngrow], f2_bar[ngrow].
int mcpm_lightcone_tables_vjp_f32(mcpm_plan *p, const float *r0, int64_t n, const double *tables, int nchi, int ngrow,
                                  const float *g_bar, const float *g2_bar, const float *dg2dg_bar, double *table_bar) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, r0 && tables && g_bar && table_bar && n > 0 && nchi >= 2 && ngrow >= 2, MCPM_E_ARG, "mcpm_lightcone_tables_vjp_f32: bad argument");
    TabSum t;
    MCPM_TRY(mcpm_tab_begin(p, "mcpm_lightcone_tables_vjp_f32", MCPM_RED_TABLES, (size_t)nchi + 4 * (size_t)ngrow, n, &t));
    lightcone_tables_vjp_kernel<0><<<t.nb, 256, 0, p->stream>>>(r0, n, tables, nchi, ngrow, g_bar, g2_bar, dg2dg_bar, t.mx, t.acc);
    MCPM_LAUNCH_CHECK(p, "lightcone_tables_vjp_kernel");
    lightcone_tables_vjp_kernel<1><<<t.nb, 256, t.lds, p->stream>>>(r0, n, tables, nchi, ngrow, g_bar, g2_bar, dg2dg_bar, t.mx, t.acc);
    MCPM_LAUNCH_CHECK(p, "lightcone_tables_vjp_kernel");
    const int kind_end[5] = {nchi, nchi + ngrow, nchi + 2 * ngrow, nchi + 3 * ngrow, t.ntot};      // chi, g, g2, f, f2
    return mcpm_tab_finish(p, t, kind_end, 5, table_bar);
}

// Observation side: table cotangents of gf_p = a2g(a_p) a2f(a_p), a_p = chi2a(|P_p|) inside mcpm_observe_pos_f32 (light-cone bit) and
// of the automatic Alcock-Paczynski look-up chi2a(r') (MCPM_AP_AUTO, with or without the light-cone bit).  table_bar (device float64,
// OVERWRITTEN): chi_bar[nchi], g_bar[ngrow], f_bar[ngrow] on the light cone; chi_bar[nap] alone off it.
int mcpm_observe_pos_ap_tables_vjp_f32(mcpm_plan *p, const float *pos, const float *vel, const float *dvel, int64_t n, int mode,
                                       const float *geom, int flags, const double *tables, int nchi, int ngrow, int ap_mode,
                                       double alpha_iso, double alpha_ap, const double *ap_tables, int nap, int nfid, const float *out_bar,
                                       double *table_bar) {
    if (!p) return MCPM_E_ARG;
    const bool lc = (flags & 2) != 0;
    MCPM_REQUIRE(p, lc || ap_mode == MCPM_AP_AUTO, MCPM_E_ARG, "mcpm_observe_pos_ap_tables_vjp_f32: light cone only (flags bit 1, tables), or automatic Alcock-Paczynski");
    if (!lc) nchi = nap, ngrow = 0;      // the accumulator's layout: the Alcock-Paczynski look-up's chi nodes alone
    ObsArgs a;
    MCPM_TRY(obs_args(p, "mcpm_observe_pos_ap_tables_vjp_f32", out_bar && table_bar, pos, vel, n, mode, geom, flags, tables, nchi, ngrow, ap_mode,
                      alpha_iso, alpha_ap, ap_tables, nap, nfid, &a));
    TabSum t;
    MCPM_TRY(mcpm_tab_begin(p, "mcpm_observe_pos_ap_tables_vjp_f32", MCPM_RED_TABLES, (size_t)nchi + 2 * (size_t)ngrow, n, &t));
    StageTimer st_(ap_mode == MCPM_AP_NONE ? nullptr : p, ST_LPT, 60.0 * n);      // the mode-none light-cone call stays unbooked, as before
#define K(MO, AP)                                                                                                                             \
    observe_tables_vjp_kernel<MO, AP, 0><<<t.nb, 256, 0, p->stream>>>(p->g, a.og, a.tb, a.ap, pos, vel, dvel, n, out_bar, t.mx, t.acc);       \
    MCPM_LAUNCH_CHECK(p, "observe_tables_vjp_kernel");                                                                                        \
    observe_tables_vjp_kernel<MO, AP, 1><<<t.nb, 256, t.lds, p->stream>>>(p->g, a.og, a.tb, a.ap, pos, vel, dvel, n, out_bar, t.mx, t.acc); \
    MCPM_LAUNCH_CHECK(p, "observe_tables_vjp_kernel")
    OBS_DISPATCH(K, mode, ap_mode);
#undef K
    const int kind_end[3] = {nchi, nchi + ngrow, t.ntot};      // chi, g, f
    return mcpm_tab_finish(p, t, kind_end, 3, table_bar);
}

int mcpm_observe_pos_tables_vjp_f32(mcpm_plan *p, const float *pos, const float *vel, const float *dvel, int64_t n, int mode,
                                    const float *geom, int flags, const double *tables, int nchi, int ngrow, const float *out_bar,
                                    double *table_bar) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, (flags & 2) && tables && nchi >= 2 && ngrow >= 2, MCPM_E_ARG, "mcpm_observe_pos_tables_vjp_f32: light cone only (flags bit 1, tables)");
    return mcpm_observe_pos_ap_tables_vjp_f32(p, pos, vel, dvel, n, mode, geom, flags, tables, nchi, ngrow, MCPM_AP_NONE, 1., 1., nullptr, 0, 0,
                                              out_bar, table_bar);
}

}  // extern "C"
