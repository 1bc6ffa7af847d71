// The likelihoods of the field-level model besides 'quad_gauss' (montecosmo/model.py:872-886, :903-932) with their hand-derived
// gradients: one pass over the final mesh ('shash', 'poisson', 'two_quad_gauss') or over its half-spectrum ('fourier_gauss'); the
// primordial term s_ep phi of scale1 and the temperature of the tempered likelihood in lik_real_phi_kernel.  Elementwise, no LDS
// tiling.  Every scalar is a float64 grid sum with the fixed-order fold of reduce_dev.h: bitwise the same call after call.
#include "mcpm_internal.h"
#include "reduce_dev.h"
#include "cgh_dev.h"
#include "kmode_dev.h"      // 2 pi and sfreq: this file's wavevector is (2 pi s) / box, not the decoder's

#define LIK_HALF_LOG2PI_D 0.91893853320467274

namespace {

// numpy.polynomial.hermite_e.hermegauss(20): the rule is symmetric, so the ten positive nodes are kept -- weight / sqrt(2 pi)
// (E_{N(0,1)}[f] = sum_i w_i f(x_i), utils.py:386-390) and asinh(node).
__constant__ double SHASH_W[10] = {0.2607930634495548,     0.16173933398400003,    0.06150637206397696,   0.013997837447100996,
                                   0.0018301031310804924,  0.00012882627996192942, 4.4021210902308646e-06, 6.127490259982928e-08,
                                   2.4820623623151797e-10, 1.2578006724379264e-13};
__constant__ float SHASH_A[10] = {0.3403547958434303f, 0.911416873700513f,  1.3235373611712888f, 1.6317688191357802f, 1.8765818449800613f,
                                  2.081032277956348f,  2.259011023742613f, 2.4200476323018796f, 2.5724237074224416f, 2.7280777613108147f};

// Standardiser of SinhArcsinh (utils.py:416-429): m = E[Z], s = sqrt(E[Z^2] - m^2), Z = sinh((asinh(eps) + skew) tail), and their
// derivatives w.r.t. skew and tail from the same nodes: dZ/dskew = tail cosh(u), dZ/dtail = (asinh(eps) + skew) cosh(u).
// PRECISION of the rule: float32 exponentials (exp(u) and exp(-u) separately, so that skew = 0 gives an exactly antisymmetric Z and
// m = 0), float64 sums.  v = E[Z^2] - m^2 and dv = dE[Z^2] - 2 m dm are differences of sums of twenty terms spanning thirteen decades
// of weight, which float32 sums would carry to ~1e-6 of their size; six float64 FMAs per node cost less than the two quarter-rate
// exponentials beside them.  Float64 exponentials were tried and changed nothing: the log density of the 840-cell test mesh moved from
// 5.26e-5 to 5.29e-5 off its float64 value -- that error sat in the value's own transcendentals (see shash_term).
struct Standardiser {
    float m, s, m_sk, m_tl, s_sk, s_tl;
    double log_s;
};
__device__ __forceinline__ Standardiser shash_standardiser(float skew, float tail) {
    double sz = 0., szz = 0., sc = 0., sca = 0., szc = 0., szca = 0.;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
#pragma unroll
        for (int sgn = 0; sgn < 2; ++sgn) {
            const float a = (sgn ? -SHASH_A[i] : SHASH_A[i]) + skew, u = a * tail;
            const float ep = expf(u), en = expf(-u);
            const double Z = 0.5 * ((double)ep - (double)en), Cw = SHASH_W[i] * (0.5 * ((double)ep + (double)en));
            sz += SHASH_W[i] * Z;
            szz += SHASH_W[i] * Z * Z;
            sc += Cw;
            sca += Cw * (double)a;
            szc += Cw * Z;
            szca += Cw * Z * (double)a;
        }
    }
    const double v = szz - sz * sz, s = sqrt(v), t = (double)tail;
    Standardiser r;
    r.m = (float)sz, r.s = (float)s, r.log_s = 0.5 * log(v);
    r.m_sk = (float)(t * sc), r.m_tl = (float)sca;
    r.s_sk = (float)((t * szc - sz * t * sc) / s);      // ds = (dE[Z^2] - 2 m dm) / (2 s), dE[Z^2] = 2 E[Z dZ]
    r.s_tl = (float)((szca - sz * sca) / s);
    return r;
}

// Per-cell term: lp and its derivatives w.r.t. the location, scale1 (b) and scale2 (a) -- the triple the host chain of the
// 'quad_gauss' path works with (logdensity.py).
struct Term {
    double lp;
    float g_loc, g_b, g_a;
};

// SinhArcsinh(mean = loc, std = sqrt(b^2 + 2 a^2), skewness = 3.540 a / b, tailweight = 1 + 5.884 (a / b)^2).log_prob(obs)
// (model.py:928-932, utils.py:437-450).
__device__ __forceinline__ Term shash_term(float obs, float loc, float b, float a) {
    const float rho = a / b, skew = 3.540f * rho, tail = 1.f + 5.884f * rho * rho;
    const float sig = sqrtf(b * b + 2.f * a * a);
    const Standardiser S = shash_standardiser(skew, tail);
    const float d = (obs - loc) / sig;
    const float Z = S.m + S.s * d;
    // THE VALUE IS FLOAT64 from Z on (as the Poisson value is).  With float32 asinh, sinh, log1p and log the log density of an 840-cell
    // mesh was 4.3e-5 to 5.3e-5 off its float64 value, always to the same side, where the float32 numpy restatement loses 0.5e-5 to
    // 2.4e-5: an error of about 6e-8 per cell that does not change sign from cell to cell (eps = sinh(asinh(Z) / tail - skew) is nearly
    // the identity, and -log(2 pi) / 2 rounded to float32 alone is the same 2e-8 off everywhere) adds up N times over, not sqrt(N).
    // In float64 the same meshes are 0.2e-5 to 1.4e-5 off (what is left is the float32 Z).  Seven float64 transcendentals per cell
    // beside the forty float32 exponentials of the rule; every gradient below stays float32.
    const double Zd = (double)Z, Ad = asinh(Zd), td = Ad / (double)tail - (double)skew, epsd = sinh(td);
    const float A = (float)Ad, eps = (float)epsd;
    const float e2 = eps * eps, Z2 = Z * Z;
    Term r;
    r.lp = -LIK_HALF_LOG2PI_D - 0.5 * epsd * epsd + 0.5 * log1p(epsd * epsd) - log((double)tail) - 0.5 * log1p(Zd * Zd) + S.log_s -
           log((double)sig);
    // d lp / dt = (-eps + eps / (1 + eps^2)) cosh(t) = -eps^3 / sqrt(1 + eps^2)
    const float gt = -eps * e2 * rsqrtf(1.f + e2);
    const float gZ = gt / (tail * sqrtf(1.f + Z2)) - Z / (1.f + Z2);
    const float gs = 1.f / S.s + gZ * d;
    const float g_skew = -gt + gZ * S.m_sk + gs * S.s_sk;
    const float g_tail = -gt * A / (tail * tail) - 1.f / tail + gZ * S.m_tl + gs * S.s_tl;
    const float g_sig = -(1.f + gZ * S.s * d) / sig;
    const float g_rho = 3.540f * g_skew + 2.f * 5.884f * rho * g_tail;
    r.g_loc = -gZ * S.s / sig;
    r.g_b = g_sig * b / sig - g_rho * rho / b;
    r.g_a = g_sig * 2.f * a / sig + g_rho / b;
    return r;
}

// family 0 'shash', 1 'poisson'.  Sums (per-workgroup partials, 5 rows): lp, d/d s_e, d/d s_ed, d/d s_e2 and the sum of sqsel_bar.
// count_bar = d lp / d count at fixed selec (through the location and through delta = count / selec - 1); sqsel_bar (may be NULL) =
// d lp / d sqrt(selec) at fixed count: `wsel` of the 'quad_gauss' host chain plus the path through delta.
// Unobserved cells get safe inputs (obs 0, count 0, selec 1) BEFORE any arithmetic and are removed by selection at the end.
template <int FAMILY>
__global__ __launch_bounds__(256) void lik_real_kernel(int64_t n, const float *__restrict__ obs, const float *__restrict__ count,
                                                       const float *__restrict__ selec, float selec_scalar,
                                                       const unsigned char *__restrict__ mask, float s_e, float s_ed, float s_e2,
                                                       float *__restrict__ count_bar, float *__restrict__ sqsel_bar, double *__restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[5] = {0., 0., 0., 0., 0.};
    if (i < n) {
        const bool on = mask ? mask[i] != 0 : true;
        const float o = on ? obs[i] : 0.f, c = on ? count[i] : 0.f;
        float S = selec ? selec[i] : selec_scalar;
        S = on ? S : 1.f;
        double lp;
        float cb, qb = 0.f, ge = 0.f, ged = 0.f, ge2 = 0.f;
        if (FAMILY == 0) {
            const float q = sqrtf(S), delta = c / S - 1.f, lin = s_e + s_ed * delta, al = fabsf(lin) + 1e-9f;
            const Term T = shash_term(o, c, al * q, s_e2 * q);
            const float sg = (lin > 0.f ? 1.f : (lin < 0.f ? -1.f : 0.f)) * q, gl = T.g_b * sg;      // d lp / d lin
            lp = T.lp;
            cb = T.g_loc + gl * s_ed / S;
            ge = gl, ged = gl * delta, ge2 = T.g_a * q;
            qb = T.g_b * al + T.g_a * s_e2 - 2.f * gl * s_ed * c / (S * q);      // d delta / d q = -2 count / q^3
        } else {
            // Poisson(|count|) at temp = 1 (model.py:873): xlogy(obs, lambda) - lambda - lgamma(obs + 1).  The value is formed in float64:
            // its three terms are of size obs log(obs) (hundreds at the usual counts) and cancel to O(1), which float32 would carry
            // to two digits fewer than every other term of the log density; the gradient has no such cancellation and stays float32.
            const float lam = fabsf(c);
            if (lam > 0.f) {
                lp = (o == 0.f ? 0. : (double)o * log((double)lam)) - (double)lam - lgamma((double)o + 1.);
                cb = (c > 0.f ? 1.f : -1.f) * (o / lam - 1.f);
            } else {
                lp = o > 0.f ? -(double)INFINITY : (o == 0.f ? 0. : (double)NAN);
                cb = 0.f;
            }
        }
        count_bar[i] = on ? cb : 0.f;
        if (sqsel_bar) sqsel_bar[i] = on ? qb : 0.f;
        if (on) v[0] = lp, v[1] = (double)ge, v[2] = (double)ged, v[3] = (double)ge2, v[4] = (double)qb;
    }
    block_partial<5>(v, part, gridDim.x, blockIdx.x);
}

// TwoQuadGaussian(loc, scale1 = b, scale2 = a).log_prob(obs) (utils.py:541-616): obs = loc + b eps1 + a (eps2^2 - 1) with eps2 integrated
// out by the Gauss-Hermite rule the caller hands over,
//     lp = logsumexp_i [log wn_i - 0.5 r_i^2] - log b - log(2 pi) / 2,   r_i = (obs - loc - a (z_i^2 - 1)) / b.
// The rule is symmetric and r_i reads z_i^2 alone, so the upper half of the nodes is visited (gz, glw point at it; nh nodes) and the
// doubled weight is one log 2 at the end.  The exponents are float64 throughout: log wn_i spans 1e-1 .. 1e-46 and r_i^2 reaches
// hundreds, so the difference of the two would keep four digits in float32.  Two sweeps -- the largest exponent, then the weights
// p_i = exp(e_i - max) with their three moments -- recompute e_i (three float64 FMAs) instead of holding nh doubles per lane: the node
// index is the same in every lane, the table comes through scalar loads, and nothing is indexed at run time (no scratch).
// Gradients with the softmax weights: d/d loc = sum p_i r_i / b,  d/d b = sum p_i (r_i^2 - 1) / b,  d/d a = sum p_i r_i (z_i^2 - 1) / b.
__device__ __forceinline__ Term two_quad_term(float obs, float loc, float b, float a, const double *__restrict__ gz,
                                              const double *__restrict__ glw, int nh) {
    const double bd = (double)b, u = ((double)obs - (double)loc) / bd, k = (double)a / bd;
    double m = -(double)INFINITY;
    for (int i = 0; i < nh; ++i) {
        const double r = u - k * (gz[i] * gz[i] - 1.);
        m = fmax(m, glw[i] - 0.5 * r * r);
    }
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
    for (int i = 0; i < nh; ++i) {
        const double q = gz[i] * gz[i] - 1., r = u - k * q, p = exp(glw[i] - 0.5 * r * r - m);
        s0 += p;
        s1 += p * r;
        s2 += p * r * r;
        s3 += p * r * q;
    }
    Term T;
    T.lp = m + log(s0) + 0.69314718055994531 - log(bd) - LIK_HALF_LOG2PI_D;
    T.g_loc = (float)(s1 / s0 / bd);
    T.g_b = (float)((s2 / s0 - 1.) / bd);
    T.g_a = (float)(s3 / s0 / bd);
    return T;
}

// The real-space families with the primordial term and a temperature (model.py:873, :894-895, :905-906, :917-918):
//     scale1 = (|s_e + s_ed delta + s_ep phi| + 1e-9) sqrt(selec) sqrt(temp),   scale2 = s_e2 sqrt(selec),   Poisson rate |count|^(1 / temp).
// family 0 'shash', 1 'poisson', 2 'two_quad_gauss'.  Sums (6 rows): those of lik_real_kernel and d/d s_ep.  phi NULL: phi = 0 and no
// phi_bar.  'shash' repeats lik_real_kernel's arithmetic expression by expression, with the factors of the temperature multiplied on
// (st = 1 leaves every float as it is) and the phi term added under `if (phi)`: at phi NULL, temp 1 it returns lik_real_kernel's bits.
template <int FAMILY>
__global__ __launch_bounds__(256) void lik_real_phi_kernel(int64_t n, const float *__restrict__ obs, const float *__restrict__ count,
                                                           const float *__restrict__ selec, float selec_scalar,
                                                           const unsigned char *__restrict__ mask, const float *__restrict__ phi, float s_e,
                                                           float s_ed, float s_e2, float s_ep, float temp, const double *__restrict__ gz,
                                                           const double *__restrict__ glw, int nh, float *__restrict__ count_bar,
                                                           float *__restrict__ phi_bar, float *__restrict__ sqsel_bar,
                                                           double *__restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[6] = {0., 0., 0., 0., 0., 0.};
    if (i < n) {
        const bool on = mask ? mask[i] != 0 : true;
        const float o = on ? obs[i] : 0.f, c = on ? count[i] : 0.f;
        float S = selec ? selec[i] : selec_scalar;
        S = on ? S : 1.f;
        double lp;
        float cb, pb = 0.f, qb = 0.f, ge = 0.f, ged = 0.f, ge2 = 0.f, gep = 0.f;
        if (FAMILY != 1) {
            const float st = sqrtf(temp), ph = (phi && on) ? phi[i] : 0.f;
            const float q = sqrtf(S), delta = c / S - 1.f;
            float lin = s_e + s_ed * delta;
            if (phi) lin += s_ep * ph;
            const float al = fabsf(lin) + 1e-9f;
            const Term T = FAMILY == 0 ? shash_term(o, c, al * q * st, s_e2 * q) : two_quad_term(o, c, al * q * st, s_e2 * q, gz, glw, nh);
            const float sg = (lin > 0.f ? 1.f : (lin < 0.f ? -1.f : 0.f)) * q * st, gl = T.g_b * sg;      // d lp / d lin
            lp = T.lp;
            cb = T.g_loc + gl * s_ed / S;
            ge = gl, ged = gl * delta, ge2 = T.g_a * q, gep = gl * ph;
            pb = gl * s_ep;
            const float alt = al * st;      // d scale1 / d q
            qb = T.g_b * alt + T.g_a * s_e2 - 2.f * gl * s_ed * c / (S * q);      // d delta / d q = -2 count / q^3
        } else {
            // Poisson(|count|^(1 / temp)).  temp = 1 keeps lik_real_kernel's expressions (and bits); else log(rate) = log|count| / temp
            // in float64 and d rate / d |count| = rate / (temp |count|).
            const float ac = fabsf(c);
            if (ac > 0.f) {
                const bool unit = temp == 1.f;
                const double ll = unit ? log((double)ac) : log((double)ac) / (double)temp, lamd = unit ? (double)ac : exp(ll);
                lp = (o == 0.f ? 0. : (double)o * ll) - lamd - lgamma((double)o + 1.);
                cb = (c > 0.f ? 1.f : -1.f) * (unit ? o / ac - 1.f : (o - (float)lamd) / (temp * ac));
            } else {
                lp = o > 0.f ? -(double)INFINITY : (o == 0.f ? 0. : (double)NAN);
                cb = 0.f;
            }
        }
        count_bar[i] = on ? cb : 0.f;
        if (phi_bar) phi_bar[i] = on ? pb : 0.f;
        if (sqsel_bar) sqsel_bar[i] = on ? qb : 0.f;
        if (on) v[0] = lp, v[1] = (double)ge, v[2] = (double)ged, v[3] = (double)ge2, v[4] = (double)qb, v[5] = (double)gep;
    }
    block_partial<6>(v, part, gridDim.x, blockIdx.x);
}

// 'fourier_gauss' (model.py:875-886): obs_rg[r] ~ Normal(cgh2rg(Y)[r], sigma), sigma = |s_e + s_k2e k^2 + s_kmu2e (k mu)^2| sqrt(selec)
// laid out by cgh2rg(norm = "amp"): both real elements of a mode take that mode's sigma.  k mu = k . los (mu = k . los / |k| with
// mu = 0 at k = 0, where k mu = 0 either way), so no division is formed.  One thread per STORED mode: rg2cgh's rule (cgh_source) names
// the two real elements the mode pairs with, cgh2rg's rule (cgh2rg_read) says whether that element really reads this mode and with which
// weight.  A mode that no element reads -- the redundant mirror half of the kz = 0 and kz = nz/2 faces -- writes zero.  So every
// element of Y_bar is written exactly once, by its own thread: no atomic, no zero fill.
// Sums (5 rows): lp, d/d s_e, d/d s_k2e, d/d s_kmu2e, d/d sqrt(selec).  A temperature (model.py:883) multiplies sigma by sqrt(temp): the
// caller folds that factor into `sqsel` and passes it again as `q4`, the factor the last sum still lacks (1 at temp = 1: the same bits).
__global__ __launch_bounds__(256) void lik_fourier_kernel(int nx, int ny, int nz, float bx, float by, float bz, float lx, float ly, float lz,
                                                          const float2 *__restrict__ Y, const float *__restrict__ obs_rg, float sqsel,
                                                          float s_e, float s_k2e, float s_kmu2e, float q4, float2 *__restrict__ Y_bar,
                                                          double *__restrict__ part) {
    const int nzc = nz / 2 + 1;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, Mh = (int64_t)nx * ny * nzc;
    double v[5] = {0., 0., 0., 0., 0.};
    if (idx < Mh) {
        const int k = (int)(idx % nzc);
        const int64_t t = idx / nzc;
        const int j = (int)(t % ny), i = (int)(t / ny);
        const float k0 = TWO_PI * (float)sfreq(i, nx) / bx, k1 = TWO_PI * (float)sfreq(j, ny) / by, k2 = TWO_PI * (float)k / bz;      // h/Mpc
        const float kk = k0 * k0 + k1 * k1 + k2 * k2, kl = k0 * lx + k1 * ly + k2 * lz, kl2 = kl * kl;
        const float lin = s_e + s_k2e * kk + s_kmu2e * kl2, al = fabsf(lin), sigma = al * sqsel;
        const float sg = (lin > 0.f ? 1.f : (lin < 0.f ? -1.f : 0.f)) * sqsel;
        const double scd = sqrt(2. / ((double)nx * (double)ny * (double)nz));      // cgh2rg, norm = "backward"
        const float sc = (float)scd;
        const CghSrc src = cgh_source(nx, ny, nz, i, j, k);
        const float2 y = Y[idx];
        float yb[2] = {0.f, 0.f};
#pragma unroll
        for (int part_ = 0; part_ < 2; ++part_) {
            const int64_t r = part_ ? src.im : src.re;
            if (r < 0) continue;
            const int z_ = (int)(r % nz);
            const int64_t t_ = r / nz;
            const CghRead rd = cgh2rg_read(nx, ny, nz, (int)(t_ / ny), (int)(t_ % ny), z_);
            if (rd.mode != idx || rd.part != part_) continue;      // this element reads the Hermitian mirror, not this mode
            // the residual and the value in float64 (the weights sqrt(2 / M) and 1 / sqrt2 enter every element alike, and obs - loc cancels
            // numbers of the size of the mean count times sqrt(M)); the cotangents are float32
            const double wd = (rd.w == 1.f || rd.w == -1.f) ? (double)rd.w : 0.70710678118654752;
            const double zd = ((double)obs_rg[r] - scd * wd * (double)(part_ ? y.y : y.x)) / (double)sigma;
            const float zz = (float)zd;
            const float gs = (zz * zz - 1.f) / sigma;
            yb[part_] = zz / sigma * sc * rd.w;
            v[0] += -LIK_HALF_LOG2PI_D - log((double)sigma) - 0.5 * zd * zd;
            v[1] += (double)(gs * sg);
            v[2] += (double)(gs * sg * kk);
            v[3] += (double)(gs * sg * kl2);
            v[4] += (double)(gs * al * q4);
        }
        Y_bar[idx] = make_float2(yb[0], yb[1]);
    }
    block_partial<5>(v, part, gridDim.x, blockIdx.x);
}

}  // namespace

extern "C" {

int mcpm_lik_real_f32(mcpm_plan *p, int family, int64_t n, const float *obs, const float *count, const float *selec, float selec_scalar,
                      const unsigned char *mask, float s_e, float s_ed, float s_e2, float *count_bar, float *sqsel_bar, double *sums_out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n > 0 && n < ((int64_t)1 << 39) && obs && count && count_bar && sums_out, MCPM_E_ARG, "mcpm_lik_real_f32: bad argument");
    MCPM_REQUIRE(p, family == MCPM_LIK_SHASH || family == MCPM_LIK_POISSON, MCPM_E_ARG, "mcpm_lik_real_f32: unknown family");
    DetSum s;
    const unsigned nb = (unsigned)((n + 255) / 256);
    StageTimer st_(p, ST_LPT, (family == MCPM_LIK_SHASH ? 400.0 : 40.0) * n);
    MCPM_TRY(mcpm_det_begin(p, 5, nb, &s));
    if (family == MCPM_LIK_SHASH)
        lik_real_kernel<0><<<nb, 256, 0, p->stream>>>(n, obs, count, selec, selec_scalar, mask, s_e, s_ed, s_e2, count_bar, sqsel_bar, s.P);
    else
        lik_real_kernel<1><<<nb, 256, 0, p->stream>>>(n, obs, count, selec, selec_scalar, mask, s_e, s_ed, s_e2, count_bar, sqsel_bar, s.P);
    MCPM_LAUNCH_CHECK(p, "lik_real_kernel");
    return mcpm_det_fold(p, s, 5, 1.0, det_outs_row(DET_STORE, sums_out, 5));
}

int mcpm_lik_real_phi_f32(mcpm_plan *p, int family, int64_t n, const float *obs, const float *count, const float *selec, float selec_scalar,
                          const unsigned char *mask, const float *phi, float s_e, float s_ed, float s_e2, float s_ep, float temp,
                          const double *quad_z, const double *quad_logw, int n_quad, float *count_bar, float *phi_bar, float *sqsel_bar,
                          double *sums_out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, n > 0 && n < ((int64_t)1 << 39) && obs && count && count_bar && sums_out && temp > 0.f, MCPM_E_ARG,
                 "mcpm_lik_real_phi_f32: bad argument");
    MCPM_REQUIRE(p, family == MCPM_LIK_SHASH || family == MCPM_LIK_POISSON || family == MCPM_LIK_TWO_QUAD, MCPM_E_ARG,
                 "mcpm_lik_real_phi_f32: unknown family");
    MCPM_REQUIRE(p, !phi == !phi_bar, MCPM_E_ARG, "mcpm_lik_real_phi_f32: phi and phi_bar go together");
    MCPM_REQUIRE(p, family != MCPM_LIK_TWO_QUAD || (quad_z && quad_logw && n_quad >= 2 && n_quad <= 512 && !(n_quad & 1)), MCPM_E_ARG,
                 "mcpm_lik_real_phi_f32: two_quad_gauss needs a symmetric rule with an even number of nodes");
    DetSum s;
    const unsigned nb = (unsigned)((n + 255) / 256);
    const int nh = n_quad / 2;
    StageTimer st_(p, ST_LPT, (family == MCPM_LIK_SHASH ? 400.0 : family == MCPM_LIK_POISSON ? 40.0 : 60.0 * nh) * n);
    MCPM_TRY(mcpm_det_begin(p, 6, nb, &s));
#define LIK_PHI_LAUNCH(F)                                                                                                                  \
    lik_real_phi_kernel<F><<<nb, 256, 0, p->stream>>>(n, obs, count, selec, selec_scalar, mask, phi, s_e, s_ed, s_e2, s_ep, temp,         \
                                                      quad_z ? quad_z + nh : nullptr, quad_logw ? quad_logw + nh : nullptr, nh, count_bar, \
                                                      phi_bar, sqsel_bar, s.P)
    if (family == MCPM_LIK_SHASH)
        LIK_PHI_LAUNCH(0);
    else if (family == MCPM_LIK_POISSON)
        LIK_PHI_LAUNCH(1);
    else
        LIK_PHI_LAUNCH(2);
#undef LIK_PHI_LAUNCH
    MCPM_LAUNCH_CHECK(p, "lik_real_phi_kernel");
    return mcpm_det_fold(p, s, 6, 1.0, det_outs_row(DET_STORE, sums_out, 6));
}

int mcpm_lik_fourier_temp_f32(mcpm_plan *p, const float *Y, const float *obs_rg, float box_x, float box_y, float box_z, float los_x,
                              float los_y, float los_z, float selec, float s_e, float s_k2e, float s_kmu2e, float temp, float *Y_bar,
                              double *sums_out) {
    if (!p) return MCPM_E_ARG;
    MCPM_REQUIRE(p, Y && obs_rg && Y_bar && sums_out && box_x > 0.f && box_y > 0.f && box_z > 0.f && selec > 0.f && temp > 0.f, MCPM_E_ARG,
                 "mcpm_lik_fourier_f32: bad argument");
    MCPM_REQUIRE(p, !p->g.xslab, MCPM_E_UNSUPPORTED, "mcpm_lik_fourier_f32: not slab-decomposed");
    const int nx = p->g.nx, ny = p->g.ny, nz = p->g.nz;
    MCPM_REQUIRE(p, !(nx & 1) && !(ny & 1) && !(nz & 1), MCPM_E_SHAPE, "mcpm_lik_fourier_f32: rg2cgh / cgh2rg need even sides");
    DetSum s;
    const unsigned nb = (unsigned)((p->Mh + 255) / 256);
    StageTimer st_(p, ST_KSPACE, 24.0 * p->Mh);
    MCPM_TRY(mcpm_det_begin(p, 5, nb, &s));
    // sqrt(selec temp) rounded once (it enters every mode alike, so its rounding is a coherent error of the sums); temp = 1: sqrtf(selec)
    const float sq = (float)sqrt((double)selec * (double)temp);
    lik_fourier_kernel<<<nb, 256, 0, p->stream>>>(nx, ny, nz, box_x, box_y, box_z, los_x, los_y, los_z, (const float2 *)Y, obs_rg, sq, s_e,
                                                  s_k2e, s_kmu2e, sqrtf(temp), (float2 *)Y_bar, s.P);
    MCPM_LAUNCH_CHECK(p, "lik_fourier_kernel");
    return mcpm_det_fold(p, s, 5, 1.0, det_outs_row(DET_STORE, sums_out, 5));
}

int mcpm_lik_fourier_f32(mcpm_plan *p, const float *Y, const float *obs_rg, float box_x, float box_y, float box_z, float los_x, float los_y,
                         float los_z, float selec, float s_e, float s_k2e, float s_kmu2e, float *Y_bar, double *sums_out) {
    return mcpm_lik_fourier_temp_f32(p, Y, obs_rg, box_x, box_y, box_z, los_x, los_y, los_z, selec, s_e, s_k2e, s_kmu2e, 1.f, Y_bar, sums_out);
}

}  // extern "C"
