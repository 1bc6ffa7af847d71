// Posterior of the initial field under the fiducial flat-sky Kaiser model, given the observed contrast (montecosmo/bricks.py:234-247,
// kaiser_posterior; :159-164, lin2white; model.py:1444-1477, kaiser_post): where the reference's drivers start their chains.  Per stored
// mode of the plan's half-spectrum, k in h/Mpc from the decoder of kmode_dev.h:
//   mu     = safe_div(k . los, |k|)
//   P      = amp * interp(|k|; ks, pows)            (0 outside the table)
//   p      = P * cell_power                         (power in cell units)
//   boost  = g (b1E + f mu^2)
//   stds^2 = p / (1 + boost^2 / var_noise * p)
//   means  = stds^2 boost / var_noise * delta_obs
//   white[b] = scale_field * safe_div(sqrt(temp) stds noise[b] + means, sqrt(P))       (0 where P = 0, k = 0 included)
// One thread per stored mode: the per-mode factors (the table search among them) are formed once in float64 and the chains are a loop
// inside the thread.  A streaming pass: no LDS, no atomics, no reductions, so every output is bitwise the same call after call.
#include "tables_dev.h"
#include "kmode_dev.h"

namespace {

struct KPost {
    double amp, los[3], g, f, b1E, var_noise, temp, scale_field, cell_power;
};

__global__ __launch_bounds__(256) void kaiser_post_kernel(KGeom kg, KPost q, Table pw, const float2 *__restrict__ dobs,
                                                          const float2 *__restrict__ noise, int n_chains, float2 *__restrict__ white,
                                                          float2 *__restrict__ means, float *__restrict__ stds, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    const double k0 = (double)m.k[0], k1 = (double)m.k[1], k2 = (double)m.k[2], k = m.kn;
    const double mu = k == 0. ? 0. : (k0 * q.los[0] + k1 * q.los[1] + k2 * q.los[2]) / k;
    const double P = q.amp * interp_zero(k, pw).t;
    const double p = P * q.cell_power;
    const double boost = q.g * (q.b1E + q.f * mu * mu);
    const double s2 = p / (1. + boost * boost / q.var_noise * p);
    const double sd = sqrt(s2), mfac = s2 * boost / q.var_noise;
    const float2 d = dobs[idx];
    if (means) means[idx] = make_float2((float)mfac * d.x, (float)mfac * d.y);
    if (stds) stds[idx] = (float)sd;
    if (!white) return;
    if (!(P > 0.)) {      // safe_div by sqrt(P): exactly 0, whatever the noise holds
        for (int b = 0; b < n_chains; ++b) white[(int64_t)b * Mh + idx] = make_float2(0.f, 0.f);
        return;
    }
    const double wfac = q.scale_field / sqrt(P);
    const float cm = (float)(wfac * mfac), cn = (float)(wfac * sqrt(q.temp) * sd);
    const float mx = cm * d.x, my = cm * d.y;
    for (int b = 0; b < n_chains; ++b) {
        const int64_t o = (int64_t)b * Mh + idx;
        float2 w = make_float2(mx, my);
        if (noise) {
            const float2 n = noise[o];
            w.x += cn * n.x, w.y += cn * n.y;
        }
        white[o] = w;
    }
}

}  // namespace

extern "C" {

int mcpm_kaiser_post_c64(mcpm_plan *p, const float *delta_obs, const float *noise, int n_chains, float kpx, float kpy, float kpz, double amp,
                         const double *ks, const double *pows, int ntab, double los_x, double los_y, double los_z, double g, double f,
                         double b1E, double var_noise, double temp, double scale_field, double cell_power, float *white, float *means,
                         float *stds) {
    if (!p) return MCPM_E_ARG;
    KGeom kg;
    Table pw;
    MCPM_TRY(table_arg(p, "mcpm_kaiser_post_c64", ks, pows, ntab, &pw));
    MCPM_REQUIRE(p, delta_obs && n_chains >= 1, MCPM_E_ARG, "mcpm_kaiser_post_c64: bad argument");
    MCPM_REQUIRE(p, white || means || stds, MCPM_E_ARG, "mcpm_kaiser_post_c64: no output requested");
    MCPM_REQUIRE(p, var_noise > 0. && temp >= 0. && cell_power > 0. && amp >= 0., MCPM_E_ARG,
                 "mcpm_kaiser_post_c64: var_noise and cell_power must be positive, temp and amp non-negative");
    MCPM_REQUIRE(p, noise || temp == 0., MCPM_E_ARG, "mcpm_kaiser_post_c64: noise may be NULL only with temp = 0");
    MCPM_TRY(kgeom_arg(p, "mcpm_kaiser_post_c64", kpx, kpy, kpz, &kg));
    const KPost q{amp, {los_x, los_y, los_z}, g, f, b1E, var_noise, temp, scale_field, cell_power};
    StageTimer st_(p, ST_KSPACE, (8.0 + 16.0 * n_chains) * p->Mh);
    kaiser_post_kernel<<<(unsigned)((p->Mh + 255) / 256), 256, 0, p->stream>>>(kg, q, pw, (const float2 *)delta_obs,
                                                                              temp == 0. ? nullptr : (const float2 *)noise, n_chains,
                                                                              (float2 *)white, (float2 *)means, stds, p->Mh);
    MCPM_LAUNCH_CHECK(p, "kaiser_post_kernel");
    return MCPM_OK;
}

}  // extern "C"
