// Internal declarations shared by the HIP translation units of libmcpm.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/mcpm.h"

// The store-data hazard of wide vector-memory stores.  The rule (LLVM AMDGPU GCNHazardRecognizer::checkVALUHazardsHelper /
// createsVALUHazard, "VMEM instructions that store more than 8 bytes can have their store data overwritten by the next
// instruction"): a FLAT / global / buffer store whose data operand is wider than 64 bits reads its data VGPRs after issue, and a
// VALU instruction that WRITES one of them must be at least VALUWaitStates behind the store -- 1 wait state up to gfx90a, **2 on
// parts with the gfx940 instruction set (ST.hasGFX940Insts(), which gfx950 has)**.  The compiler pads its own stores; it does
// not look inside inline asm, so every hand-written global_store_dwordx3 below carries the padding itself: `s_nop 2` = 3 wait
// states (s_nop N idles N + 1), one more than the rule asks.  Without it a few cells in ten thousand received whatever the
// next instructions had put into the data registers (round 3, gpurun_out/r03l).  mcpm_selftest_store3_nt (particles.hip) runs
// this exact sequence with the data registers overwritten by the very next instructions; tests/test_gpu_parity.py holds it to
// a plain-store twin over 2^26 records.
#define MCPM_STORE_DATA_HAZARD_NOP "s_nop 2"


// MAP OF plan->reduce: MCPM_NREDUCE device doubles for the scalar results of the model-side and adjoint entry points (offsets and extents
// in doubles).  The table cotangents and the reverse sweep start at 0 and overlay the scalars, the PNG accumulators and each other.  That
// is safe: every user is one entry point on the plan's one stream, it clears what it accumulates into, and its values are read only by
// work the same call enqueues behind them (its next kernel, the copy to the caller's buffer), so nothing here is live between two calls.
enum McpmReduceMap {
    MCPM_NREDUCE = 6144,
    // doubles [0, 8).  bias.hip: <d^2> [0]; png.hip: <d^2>, <phi d> [0, 1], S0, S1 [0, 1], the mean of mcpm_png_add_f32 [0]; eulerian.hip: the
    // two moment cotangents [0, 1]; composite.hip: the three LPT scalar cotangents of mcpm_lpt_vjp*_f32 [0, 3)
    MCPM_RED_SCALARS = 0,
    MCPM_RED_NSCALARS = 8,
    // The two regions of the integer table sums (mcpm_tab_begin): ntot 64-bit integer accumulators, then MCPM_RED_TAB_TAIL doubles whose
    // head holds the bits of the maxima, one unsigned per kind (MCPM_TAB_KINDS at most).
    MCPM_TAB_KINDS = 5,
    MCPM_RED_TAB_TAIL = 8,
    // mcpm_png_add_vjp_f32: ntab <= MCPM_RED_PNG_NTAB accumulators of one kind; BEHIND the scalars, because the same call holds S0, S1 there
    MCPM_RED_PNG_ACC = MCPM_RED_SCALARS + MCPM_RED_NSCALARS,
    MCPM_RED_PNG_NTAB = 2048,
    // mcpm_*_tables_vjp_f32 (observe.hip, kaiser.hip): ntot + MCPM_RED_TAB_TAIL <= MCPM_RED_TABLES_END - MCPM_RED_TABLES
    MCPM_RED_TABLES = 0,
    MCPM_RED_TABLES_END = 3072,
    // mcpm_nbody_bf_vjp_f32, doubles: alpha_bar[n_steps], beta_bar[n_steps], then the tail (3 LPT scalar cotangents, dg_bar), up to MCPM_NREDUCE
    MCPM_RED_SWEEP = 0,
    MCPM_RED_SWEEP_TAIL = 4,
};
static_assert(MCPM_RED_PNG_ACC + MCPM_RED_PNG_NTAB + MCPM_RED_TAB_TAIL <= MCPM_NREDUCE && MCPM_RED_TABLES_END <= MCPM_NREDUCE &&
                  MCPM_TAB_KINDS * sizeof(unsigned) <= MCPM_RED_TAB_TAIL * sizeof(double), "plan->reduce map");
// pass 1 of a table sum keeps one 64-bit LDS accumulator per entry: the larger region fits the default dynamic-LDS limit of a launch
static_assert(MCPM_RED_PNG_NTAB <= MCPM_RED_TABLES_END - MCPM_RED_TABLES && (MCPM_RED_TABLES_END - MCPM_RED_TABLES) * sizeof(double) <= 64 * 1024, "table sums: LDS");
#ifndef MCPM_NZPAD
#define MCPM_NZPAD 16  // complex elements added to the nz/2 pitch of the internal spectra
#endif

// Stages of the path, for the optional per-stage HIP-event profile (mcpm_plan_profile*).
enum McpmStage {
    ST_PAINT = 0,   // paint_tile_kernel + paint_outlier_kernel, or paint_atomic_kernel
    ST_R2C,         // rocFFT real forward
    ST_C2R,         // rocFFT real inverse
    ST_KSPACE,      // k-space force / hessian kernels and their adjoints
    ST_READ,        // read / read_vjp / paint_vjp gathers
    ST_KICKDRIFT,   // fused read + kick + drift
    ST_STEPADJ,     // fused adjoint particle kernel
    ST_AXPY,        // drift / kick / cotangent axpy
    ST_LPT,         // lattice kernels of lpt and its adjoint, hessian combine
    ST_PAINT3,      // three-component tiled paint (adjoint of the three-component read)
    ST_NSTAGES
};

struct StageRec {
    hipEvent_t e0, e1;
    int stage;
    double bytes;
};

// Mesh + particle-lattice geometry handed to kernels by value.
struct Geom {
    int nx, ny, nz;   // mesh
    int px, py, pz;   // particle lattice (regular_pos(mesh, ptcl))
    int nzh;          // nz/2 + 1
    int same_lattice; // px==nx && py==ny && pz==nz (unit lattice spacing)
    int xoff;         // slab mode: mesh plane of lattice plane 0 (= ghost width); 0 otherwise
    int xslab;        // slab mode: x is NOT periodic on this (ghost-extended) mesh
    int patch;        // lattice-mode particle kernels: a 256-thread workgroup is four waves on a 2 x 2 (x, y) patch of lattice rows
                      // (64 consecutive z each) instead of 256 consecutive z of one row (particles_dev.h::particle_index)
};

#define MCPM_FX_SLOTS 64
#define MCPM_FX_STRIDE 32   // unsigned per slot: one 128-byte line each

struct mcpm_plan {
    Geom g;
    hipStream_t stream;
    int64_t M;   // nx*ny*nz
    int64_t Mh;  // nx*ny*nzh
    int64_t Np;  // px*py*pz
    int halo;    // tiled paints: > 0 = fixed halo H (a tile's window is (16 + 2H + 1)^3 lattice points around its bulk offset); 0 = boxes chosen on the device
    int centre;  // tiled paints: windows centred on the local bulk displacement (paint_tiled.hip); 0 = on the tile itself
    int *halo_sel;    // 3 x ntiles packed words: per 16^3 Lagrangian block the sampled range of floor(d) per axis ([ntiles] minima, [ntiles] maxima), from which
                      // box_tile_kernel sizes every tile's window, then [ntiles] upper corners of the windows
    int *tile_off;    // packed lower corners of the windows' floor(d) boxes per 16^3 tile (device; NULL if the mesh cannot be tiled)
    int *bucket_cnt;  // per-tile bucket fill counts
    int *bucket;      // [tile][bucket_cap] particles a tile's window misses
    int bucket_cap;
    int *bucket_tiles; // list of tiles with a non-empty bucket (built by the duty, walked by the bucket kernels)
    int paint_variant;  // threads/unroll variant of the tiled paint (tuning)
    int paint3_variant; // three-component tiled paint variant (tuning); < 0 disables it; 4 = fixed-point tile
    unsigned *fx_wmax;  // fixed-point paint: bits of max|w|, maximum over MCPM_FX_SLOTS slots (device)
    int *fx_redo;       // fixed-point paint: [0] = number of flagged tiles, then their indices (device)
    int fx_tiles;       // capacity of fx_redo
    const float *fx_src; // weights whose max|fx_scale w| a producer kernel already left in fx_wmax (else NULL): a three-component paint of
                         // this array with wscale == fx_scale skips its absmax pass
    float fx_scale;      // 1 for a materialised F_bar (axpby, the adjoint kernel's fb_next); beta_next for the carried u' array
    int fx_clean;        // fx_wmax is all zero (the last three-component paint's epilogue cleared it): producers skip their memset
    long long *gx_acc;  // generic (order-independent) paint: int64 fixed-point accumulator mesh, all-zero between calls; allocated on first use
    unsigned *gx_wmax;  // generic paint: bits of max|w| (MCPM_FX_SLOTS slots)
    // chaining of adjoint steps (mcpm_plan_hint_next_adjoint): hint_* = (beta, tau) of step i-1, pending until the adjoint particle
    // kernel of step i consumes them.  Two forms (composite.hip, step_adjoint_particles):
    //   carry_* (the composite drivers, mcpm_bullfrog_step_vjp*_f32): the kernel left u' = v_bar + tau' x_bar in the caller's
    //     vel_bar array (carry_vb; carry_xb = its pos_bar) -- no F_bar array exists; the next call's paint scales u' by beta'.
    //     Pending until that call matches it (same pointers, same scalars as float) or any other adjoint-step call turns it back.
    //   fb_* (mcpm_step_adjoint_particles*_f32 + mcpm_plan_chained_fb: callers that compose the step, slabs): the kernel also
    //     wrote F_bar' = beta' u' to plan scratch and vel_bar is the true v_bar.
    // Who resets hint_set: the adjoint particle kernel's launcher that consumes it; mcpm_fail (any failing call on the plan, so an
    // adjoint step that fails its argument checks takes its hint with it); mcpm_nbody_bf_vjp_f32 and mcpm_lpt_vjp*_f32 at entry (not
    // adjoint steps); the pitch probe.  fx_src (above) goes with it in mcpm_fail.
    int hint_set, fb_valid, carry_valid;
    float hint_beta, hint_tau, fb_beta, fb_tau, carry_beta, carry_tau;
    const void *fb_xb, *fb_vb, *carry_xb, *carry_vb;
    // x-slab decomposition (mcpm_plan_create_slab): this rank owns global planes [rank*nxl, (rank+1)*nxl)
    int nranks, rank, ghost, nx_global, nxl;
    unsigned *dmax; // caller's MCPM_FX_SLOTS x MCPM_FX_STRIDE slots: kick_drift leaves max |d_x| (as float bits) there; NULL = off
    int xw0, xwn;  // window of local planes the slab z / y passes work on (mcpm_slab_set_window; default all nxl)
    int chunks;    // chunks of the all-to-all layouts (mcpm_slab_set_chunks; 1 = one all-to-all per spectrum)
    void *slab_state;  // transport + workspace of the native slab steps (slab.hip); NULL until mcpm_slab_comm_init_*

    // rocFFT plans keyed by batch
    std::map<int, rocfft_plan> r2c, c2r;
    std::map<int, rocfft_execution_info> r2c_info, c2r_info;
    std::map<int, void *> r2c_work, c2r_work;

    // scratch owned by the plan
    float *rho;      // M floats: painted density / real scratch
    float *spec;     // 6 half-spectra (complex64) scratch
    float *fmesh;    // 9 real meshes scratch (force meshes / hessians)
    float *spec1;    // 1 half-spectrum scratch
    float *fft_pad;  // 1 padded spectrum: scratch of the generic hand-written R2C / C2R (allocated on first use)
    int *outliers;   // lists of the tiled paint: suspects (Np ints), then wild particles (Np ints)
    int *outlier_count;  // device counters (8 ints, see paint_tiled.hip: wild, last, slab oob, overflow pairs, dropped, bucketed)
    double *reduce;  // device accumulators for scalar cotangents (MCPM_NREDUCE doubles)
    float *pscratch; // 3 (N, 3) arrays mcpm_pitch_max() apart, allocated on first VJP (adjoint state x_bar, v_bar + force cotangent F_bar)
    // Pitch (floats) between consecutive (N, 3) particle arrays of the composite entry points' checkpoint (mcpm_nbody_bf_f32: x'_0, v_0,
    // x'_1, ...) and of pscratch; 0 = contiguous (3 N).  The step kernels stream four to seven such arrays at the same particle index:
    // back to back they are IN PHASE in every low address bit and may meet in one memory channel, depending on where the process's
    // memory was placed (DESIGN finding 29); a pitch of 3 N + a few KB takes them out of phase.  mcpm_plan_probe_particle_pitch
    // measures the candidates on the caller's buffer; mcpm_plan_set_particle_pitch fixes one.
    int64_t ppitch;
    float *vscratch;  // variable-size particle scratch (pm_forces_vjp)
    double *part;     // scratch of the deterministic grid sums (reduce.hip lays it out), allocated on first use
    int64_t part_n;
    int det_stale;    // a HIP error may have kept a fold from resetting its counter: mcpm_det_begin clears it before the next sum
    int64_t vscratch_n;
    float *tw[3];    // twiddle tables exp(-2 pi i j / n) of the hand-written FFT, per axis (x, y, z)

    // optional profile: HIP events recorded on the plan's stream around every leaf stage
    int profiling;
    std::vector<StageRec> recs;
    std::vector<hipEvent_t> event_pool;

    std::string err;
};

// RAII stage bracket: records two events on the plan's stream when profiling is on.
struct StageTimer {
    mcpm_plan *p;
    StageRec r;
    bool on;
    StageTimer(mcpm_plan *plan, int stage, double bytes) : p(plan), on(plan && plan->profiling) {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!p->event_pool.empty()) {
                e = p->event_pool.back();
                p->event_pool.pop_back();
            } else {
                (void)hipEventCreate(&e);
            }
            return e;
        };
        r.e0 = get();
        r.e1 = get();
        r.stage = stage;
        r.bytes = bytes;
        (void)hipEventRecord(r.e0, p->stream);
    }
    ~StageTimer() {
        if (!on) return;
        (void)hipEventRecord(r.e1, p->stream);
        p->recs.push_back(r);
    }
};

extern thread_local std::string g_mcpm_create_error;

int mcpm_fail(mcpm_plan *plan, int code, const std::string &msg);
// One deterministic f64 grid sum (reduce.hip).  mcpm_det_begin: room for K rows of partials from nblk workgroups; the producer kernel leaves
// row k at P[k * nblk + block] (reduce_dev.h::block_partial).  mcpm_det_fold: adds up rows 0 .. K-1 (K at most the begin's) in a fixed order
// and leaves scale * sum where `outs` says (det_outs_row / det_outs_ptrs).  A begin invalidates the plan's earlier sum.
struct DetOuts;
struct DetSum {
    double *P;
    unsigned nblk;
};
int mcpm_det_begin(mcpm_plan *p, int K, unsigned nblk, DetSum *s);
int mcpm_det_fold(mcpm_plan *p, const DetSum &s, int K, double scale, const DetOuts &outs);
// One order-independent integer table sum (reduce.hip; the rule and the device side: tables_dev.h).  mcpm_tab_begin: checks that ntot entries
// fit `region` of plan->reduce (MCPM_RED_TABLES or MCPM_RED_PNG_ACC), clears its accumulators and maxima and sizes the grid for nelem elements.
// The caller launches its producer kernel twice on (t.mx, t.acc): pass 0 <<<t.nb, 256, 0>>>, pass 1 <<<t.nb, 256, t.lds>>>.  mcpm_tab_finish
// scales the integers back into out[ntot] (device); kind_end[k] = one past the last entry of kind k, kind_end[nkinds - 1] = ntot.
struct TabSum {
    unsigned long long *acc;
    unsigned *mx;
    int ntot;
    unsigned nb;
    size_t lds;
};
int mcpm_tab_begin(mcpm_plan *p, const char *who, int region, size_t ntot, int64_t nelem, TabSum *t);
int mcpm_tab_finish(mcpm_plan *p, const TabSum &t, const int *kind_end, int nkinds, double *out);

// One fold of workgroup partials (reduce.hip), for the binned statistics (spectrum.hip, binned.hip, bispectrum.hip): the producer kernel
// leaves P[group][nblk][nout] in the caller's workspace, mcpm_fold_partials adds the workgroups up in a fixed order through Q[group]
// [MCPM_FOLD_R][nout] (two launches on `s`) and leaves the sums where `o` says.  No plan, no ticket, any nout; the det fold above has a plan
// and at most DET_MAXK values.
constexpr int MCPM_FOLD_R = 32;      // first-level chunks of the fold
struct FoldOut {
    double *out;
    int n_bins, rb, batch;      // n_bins 0: dense, out[g * nout + o].  Else nout = (2 + rb) * n_bins and out is [2 + batch][n_bins]: accumulators
                                // 0, 1 of group 0 to rows 0, 1; accumulator 2 + r of group g to row 2 + g * rb + r where g * rb + r < batch
};
inline FoldOut fold_dense(double *out) { return FoldOut{out, 0, 0, 0}; }
inline FoldOut fold_binned(double *out, int n_bins, int rb, int batch) { return FoldOut{out, n_bins, rb, batch}; }
int mcpm_fold_partials(hipStream_t s, const double *P, int groups, unsigned nblk, int nout, double *Q, const FoldOut &o);

// The layout of such a workspace: regions carved one after the other, each starting on a 256-byte boundary.
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Carve {
    size_t bytes = 0;      // the running offset: the size of the workspace once every region is taken
    size_t take(size_t n) {
        const size_t off = bytes;
        bytes += align256(n);
        return off;
    }
};
inline void mcpm_fold_carve(Carve &c, int groups, unsigned nblk, size_t nout, size_t *off_P, size_t *off_Q) {
    *off_P = c.take((size_t)groups * nblk * nout * 8);
    *off_Q = c.take((size_t)groups * MCPM_FOLD_R * nout * 8);
}
// Workgroups of a producer: enough to fill the chip, fewer when a group's partials (per_block doubles per workgroup) would pass `budget`
// doubles, and never more than there are units of work.
inline int64_t mcpm_fold_nblk(int64_t budget, int64_t per_block, int64_t units) {
    return std::min(std::min<int64_t>(2048, std::max<int64_t>(64, budget / per_block)), units);
}
// Bins per tile (gridDim.z tiles) of a kernel that keeps one LDS histogram [n_acc][bt] per wave in lds_doubles doubles.
inline void mcpm_hist_tiles(int n_bins, int lds_doubles, int waves, int n_acc, int *bt, int *tiles) {
    *bt = std::min(n_bins, lds_doubles / (waves * n_acc));
    *tiles = (n_bins + *bt - 1) / *bt;
}

// The small host checks of those entry points.
inline int mcpm_check_edges(const char *who, const double *edges, int n_edges, bool strict) {
    for (int i = 0; i < n_edges; ++i)
        if (!std::isfinite(edges[i]) || (i > 0 && !(strict ? edges[i] > edges[i - 1] : edges[i] >= edges[i - 1])))
            return mcpm_fail(nullptr, MCPM_E_ARG, std::string(who) + (strict ? ": edges must be finite and strictly increasing" : ": edges must be finite and non-decreasing"));
    return MCPM_OK;
}
inline int mcpm_check_batch(const char *who, int batch) {      // gridDim.y / .z carry the batch
    if (batch < 1 || batch > 65535) return mcpm_fail(nullptr, MCPM_E_ARG, std::string(who) + ": batch out of range");
    return MCPM_OK;
}
inline bool mcpm_aligned(const void *p, uintptr_t a = 16) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }      // (NULL counts as aligned)

void mcpm_slab_state_free(mcpm_plan *p);   // slab.hip
#define MCPM_PITCH_MAX_SHIFT 17472      // floats: 64 KB + 4 KB + 256 B, the largest candidate shift between particle arrays
static inline int64_t mcpm_pitch_max(const mcpm_plan *p) { return 3 * p->Np + MCPM_PITCH_MAX_SHIFT; }
static inline int64_t mcpm_pitch(const mcpm_plan *p) { return p->ppitch > 0 ? p->ppitch : 3 * p->Np; }
static inline int mcpm_default_halo(int64_t M) { return M <= ((int64_t)1 << 24) ? 4 : 3; }   // the static rule (plan.hip: where it comes from)

// hand-written FFT Poisson solve (fftpm.hip); power-of-two axes only
bool mcpm_fftpm_supported(const mcpm_plan *p);
int mcpm_fftpm_force_meshes(mcpm_plan *p, const float *rho, float *fm3, int interleaved = 0, int nt_out = 0);
int mcpm_kick_drift_layout(mcpm_plan *p, const float *pos_in, const float *vel_in, int64_t n, int mode, const float *meshes3,
                                      int layout, int order, float alpha, float beta, float dt, float *pos_out, float *vel_out);
int mcpm_read3_il(mcpm_plan *p, const float *pos, int64_t n, int mode, const float *fm_il, int order, float *out);
int mcpm_fftpm_force_meshes_vjp(mcpm_plan *p, const float *fbar3, float *rho_bar);
int mcpm_fftpm_r2c(mcpm_plan *p, const float *real, float *spec, int batch);
int mcpm_fftpm_c2r(mcpm_plan *p, const float *spec, float *real, int batch);
// plain half-spectrum -> nc = 3 force meshes or nc = 6 Hessian meshes (00 01 02 11 12 22), and the adjoints
// (spec_bar overwritten for nc = 3, accumulated into for nc = 6)
int mcpm_fftpm_spec_meshes(mcpm_plan *p, const float *spec, float *meshes, int nc);
int mcpm_fftpm_spec_meshes_vjp(mcpm_plan *p, const float *meshes_bar, float *spec_bar, int nc);

// tiled CIC paints (paint_tiled.hip); false: geometry not tileable, the caller takes the generic path
bool mcpm_paint_tiled(mcpm_plan *p, const float *pos, const float *w, int64_t wstride, float wscalar, float *mesh, int accumulate);
// every consumer of the weights sees wscale * weights3 (one f32 product, as if the scaled array had been formed in memory)
bool mcpm_paint3_tiled(mcpm_plan *p, const float *pos, const float *weights3, float wscale, float *meshes3, int accumulate);
int mcpm_paint3_scaled(mcpm_plan *p, const float *pos, int64_t n, int mode, const float *weights3, float wscale, int order, float *meshes3,
                       int accumulate);

// light-cone selection of the N-body state (lightcone.hip), the two passes its reverse sweep (composite.hip) is built from.
// mcpm_lc_gbar: g_bar_p (N floats) from the loss cotangents (Xb, Vb); *g_bar -= sum g_bar_p and *dg_bar -= sum g_bar_p (g_p - g0) / dg
// + sum_{j < K} w_j Xb . v_j / 2 (DEVICE doubles, deterministic grid sums).  mcpm_lc_inject: state j's share of (Xb, Vb) into the running
// cotangents, pos_bar += w Xb, vel_bar += w (Vb + cu Xb); init: pos_bar = w Xb, vel_bar = w Vb instead (state K).
int mcpm_lc_gbar(mcpm_plan *p, const float *ckpt, int n_steps, double dg, double g0, const float *pos_out, const float *vel_out,
                 const float *g_p, const float *Xb, const float *Vb, float *g_bar_p, double *g_bar, double *dg_bar);
int mcpm_lc_inject(mcpm_plan *p, int j, int n_steps, double dg, double g0, const float *g_p, const float *Xb, const float *Vb, float cu,
                   int init, float *xb, float *vb);

// adjoint of the NGP lattice read on a lattice != mesh: order-independent fixed-point sums (particles.hip)
int mcpm_lattice_scatter_fx(mcpm_plan *p, const float *xb, const float *vb, float a, float b, float *meshes3);

#define MCPM_HIP(plan, expr)                                                                         \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return mcpm_fail(plan, MCPM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

#define MCPM_LAUNCH_CHECK(plan, name)                                                                \
    do {                                                                                             \
        hipError_t _e = hipGetLastError();                                                           \
        if (_e != hipSuccess)                                                                        \
            return mcpm_fail(plan, MCPM_E_HIP, std::string("launch ") + name + ": " + hipGetErrorString(_e)); \
    } while (0)

#define MCPM_REQUIRE(plan, cond, code, msg)                  \
    do {                                                     \
        if (!(cond)) return mcpm_fail(plan, code, msg);      \
    } while (0)

#define MCPM_TRY(expr)               \
    do {                             \
        int _rc = (expr);            \
        if (_rc != MCPM_OK) return _rc; \
    } while (0)
