// Order statistics of MCMC draws: the device half of montecosmo/bdec.py (quantile, qbci, sci_noweights; bdec.py holds the formulas).
// Per dimension d the M = n_chain n_draw pooled draws x[c, t, d] are sorted on chip, and only what was asked for leaves it: the values at a
// few ranks, the smallest window of L + 1 consecutive order statistics, the counts of draws below and equal to a truth, and, on request,
// the sorted block itself.
//
// Addressing is chains.hip's: element (c, t, d) is x[offset0 + c stride_chain + t stride_draw + d], d contiguous, every index 64-bit; the
// pooled index is m = c n_draw + t.
//
// Keys.  A float becomes an unsigned key whose integer order is the IEEE total order of the values: negative values have all their bits
// flipped, the others only the sign bit, so -inf < .. < -0 < +0 < .. < +inf.  Every NaN, whatever its sign and payload, becomes the key of
// the canonical quiet NaN (BD_NAN_KEY), above +inf; rows are padded to a power of two P with BD_PAD_KEY, above that.  A key maps back to
// the bits of its value, so every output is an exact copy of an input value (a NaN comes back as the canonical one).
//
// Layout.  One workgroup of BD_THREADS lanes sorts a TILE of TD = min(BD_MAX_TD, BD_TILE_KEYS / P) consecutive dimensions, all in LDS: row r of
// the tile holds the P keys of dimension d0 + r.  The loads walk the draws with TD consecutive lanes on TD consecutive d (one contiguous run
// of 4 TD bytes per draw; the neighbouring tiles read the rest of the line).  A ragged last tile and the tail of a row are filled with
// BD_PAD_KEY, and every store is masked by d < n_dim: no lane leaves before the last barrier.
//   position p of a row lives at word p + 4 (p >> 5) of the row (four words of padding after every 32 keys), rows are P + P / 8 + 4 words
//   apart.  So a lane that holds 32 consecutive keys reads them as eight 16-byte words at a lane stride of 36 words (sixteen lanes: sixteen
//   distinct groups of four banks), and lanes that walk consecutive positions at any stride >= 32 between their own keys hit consecutive words.
//
// The sort is a bitonic network.  A pass takes NL <= 5 consecutive stages (compare distances s 2^(NL-1) .. s) at once: a lane loads the 2^NL
// keys base + e s of a chunk into registers (static indices under full unrolling), runs the stages there and stores them back; one barrier
// per pass.  The first pass sorts every aligned run of 32 keys completely (the merges k = 2 .. 32, fifteen stages, in registers), then each
// merge k = 64 .. P takes ceil(log2 k / 5) passes, the last of them on 32 consecutive keys with 16-byte accesses: 17 passes at P = 4096.
// P < 32 is one pass.
//
// Epilogue, from the sorted rows (G = BD_THREADS / TD lanes per dimension, partial results joined through LDS in a fixed order by one lane):
//   out[r][d] = value at rank ranks[r];
//   sci: the first i in 0 .. M - L - 1 that minimises (double) x_(i+L) - (double) x_(i), a NaN length (both ends the same infinity) counting
//     as +inf; a row that holds a NaN gives (NaN, NaN) and index -1;
//   below[d], equal[d] = the number of draws with x < truth[d] and x == truth[d] as IEEE compares them (-0 == +0, a NaN is neither);
//   sorted[m][d], m < M.
// No atomics; integer counts and a lexicographic (length, index) minimum do not depend on how the lanes share the work.  So every output
// is bitwise reproducible and independent of n_dim, of the tile a dimension falls in, of its neighbours and of the alignment of x.
#include "mcpm_internal.h"

namespace {

constexpr int BD_THREADS = 1024;
constexpr int BD_MAX_TD = 32;
constexpr int BD_TILE_KEYS = MCPM_BDEC_MAX_M;                       // keys of a tile (without padding): one row of the largest P
constexpr int BD_TILE_WORDS = BD_TILE_KEYS + BD_TILE_KEYS / 8 + 128;      // TD rows of P + P / 8 + 4 words, TD <= 32
constexpr unsigned BD_NAN_KEY = 0xFFC00000u, BD_PAD_KEY = 0xFFFFFFFFu;
static_assert(BD_TILE_KEYS == 32768 && BD_TILE_WORDS * 4 + BD_THREADS * 12 <= 160 * 1024, "bdec tile: LDS");

struct BdecArgs {
    const float *x;
    long long offset0, n_dim, stride_chain, stride_draw;
    int n_chain, n_draw, M, p_log, td_log, n_rank, L;
    float *out, *sci, *sorted;
    int *sci_idx, *below, *equal;
    const float *truth;
    int ranks[MCPM_BDEC_MAX_RANKS];
};

__device__ __forceinline__ unsigned bd_key(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return BD_NAN_KEY;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float bd_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ int bd_word(int pos) { return pos + ((pos >> 5) << 2); }

__device__ __forceinline__ void bd_cmpx(unsigned &a, unsigned &b, bool up) {
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    a = up ? lo : hi;
    b = up ? hi : lo;
}

// One pass over the tile: every chunk of 2^NL keys base + e 2^s_log takes the stages of distance 2^(s_log + NL - 1) .. 2^s_log of the merge k.
// presort (s_log = 0 only): first the whole merges 2 .. 2^(NL-1) inside the chunk.
template <int NL>
__device__ __forceinline__ void bd_pass(unsigned *keys, int n_rows, int p_log, int pitch, unsigned k, int s_log, bool presort) {
    constexpr int E = 1 << NL;
    const int cpr_log = p_log - NL;
    const int total = n_rows << cpr_log;
    for (int w = threadIdx.x; w < total; w += BD_THREADS) {
        const int row = w >> cpr_log, c = w & ((1 << cpr_log) - 1);
        const int low = c & ((1 << s_log) - 1), high = c >> s_log;
        const int base = (high << (s_log + NL)) | low;
        unsigned *rowp = keys + row * pitch;
        unsigned v[E];
        if (NL == 5 && s_log == 0) {      // 32 consecutive keys: one padding block, 16-byte aligned
            const uint4 *q = reinterpret_cast<const uint4 *>(rowp + bd_word(base));
#pragma unroll
            for (int i = 0; i < E / 4; ++i) {
                const uint4 t = q[i];
                v[4 * i] = t.x;
                v[4 * i + 1] = t.y;
                v[4 * i + 2] = t.z;
                v[4 * i + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = rowp[bd_word(base + (e << s_log))];
        }
        if (presort) {
#pragma unroll
            for (int kk = 2; kk < E; kk <<= 1) {
#pragma unroll
                for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (!(e & j)) bd_cmpx(v[e], v[e | j], !(e & kk));
                }
            }
        }
        const bool up = (base & k) == 0;      // k >= 2^(s_log + NL): one direction for the chunk
#pragma unroll
        for (int j = E >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (!(e & j)) bd_cmpx(v[e], v[e | j], up);
        }
        if (NL == 5 && s_log == 0) {
            uint4 *q = reinterpret_cast<uint4 *>(rowp + bd_word(base));
#pragma unroll
            for (int i = 0; i < E / 4; ++i) q[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) rowp[bd_word(base + (e << s_log))] = v[e];
        }
    }
}

__device__ __forceinline__ void bd_pass_nl(int nl, unsigned *keys, int n_rows, int p_log, int pitch, unsigned k, int s_log, bool presort) {
    switch (nl) {      // (uniform over the workgroup)
        case 1: bd_pass<1>(keys, n_rows, p_log, pitch, k, s_log, presort); break;
        case 2: bd_pass<2>(keys, n_rows, p_log, pitch, k, s_log, presort); break;
        case 3: bd_pass<3>(keys, n_rows, p_log, pitch, k, s_log, presort); break;
        case 4: bd_pass<4>(keys, n_rows, p_log, pitch, k, s_log, presort); break;
        default: bd_pass<5>(keys, n_rows, p_log, pitch, k, s_log, presort); break;
    }
}

__global__ __launch_bounds__(BD_THREADS) void bdec_sort_kernel(BdecArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned keys[BD_TILE_WORDS];
    __shared__ double part_len[BD_THREADS];
    __shared__ int part_idx[BD_THREADS];

    const int tid = threadIdx.x;
    const int P = 1 << a.p_log, TD = 1 << a.td_log, M = a.M;
    const int pitch = P + ((P >> 5) << 2) + 4;
    const long long d0 = (long long)blockIdx.x * TD;

    // load: lane (m_lane, r) takes the draws m_lane, m_lane + BD_THREADS / TD, .. of dimension d0 + r; TD consecutive lanes, TD consecutive d
    {
        const int r = tid & (TD - 1), m_lane = tid >> a.td_log, m_step = BD_THREADS >> a.td_log;
        const bool live = d0 + r < a.n_dim;
        const float *col = a.x + a.offset0 + (live ? d0 + r : 0);
        unsigned *rowp = keys + r * pitch;
        for (int m = m_lane; m < P; m += m_step) {
            unsigned key = BD_PAD_KEY;
            if (live && m < M) {
                const int c = m / a.n_draw, t = m - c * a.n_draw;
                key = bd_key(col[c * a.stride_chain + t * a.stride_draw]);
            }
            rowp[bd_word(m)] = key;
        }
    }
    __syncthreads();

    // sort
    if (a.p_log > 0) {
        const int nl0 = a.p_log < 5 ? a.p_log : 5;
        bd_pass_nl(nl0, keys, TD, a.p_log, pitch, 1u << nl0, 0, true);
        __syncthreads();
        for (int lk = 6; lk <= a.p_log; ++lk) {
            int rem = lk;
            while (rem > 0) {
                const int nl = rem % 5 ? rem % 5 : 5;
                bd_pass_nl(nl, keys, TD, a.p_log, pitch, 1u << lk, rem - nl, false);
                __syncthreads();
                rem -= nl;
            }
        }
    }

    // the values at the ranks
    for (int q = 0; q < a.n_rank; ++q) {      // (q is uniform: the rank comes from the kernel arguments by a scalar load)
        const int word = bd_word(a.ranks[q]);
        if (tid < TD && d0 + tid < a.n_dim) a.out[(long long)q * a.n_dim + d0 + tid] = bd_val(keys[tid * pitch + word]);
    }
    if (a.sorted) {
        for (int i = tid; i < (M << a.td_log); i += BD_THREADS) {
            const int r = i & (TD - 1), m = i >> a.td_log;
            if (d0 + r < a.n_dim) a.sorted[(long long)m * a.n_dim + d0 + r] = bd_val(keys[r * pitch + bd_word(m)]);
        }
    }

    const int g_log = 10 - a.td_log, G = 1 << g_log;      // BD_THREADS = 2^10 lanes: G per row, lane g of row r is r G + g
    const int r = tid >> g_log, g = tid & (G - 1);
    const unsigned *rowp = keys + r * pitch;
    const bool live = d0 + r < a.n_dim;

    if (a.sci) {
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        double best = inf;
        int best_i = 0x7fffffff;
        for (int i = g; i < M - a.L; i += G) {
            double len = (double)bd_val(rowp[bd_word(i + a.L)]) - (double)bd_val(rowp[bd_word(i)]);
            if (len != len) len = inf;
            if (len < best || best_i == 0x7fffffff) {
                best = len;
                best_i = i;
            }
        }
        part_len[tid] = best;
        part_idx[tid] = best_i;
        __syncthreads();
        if (g == 0 && live) {
            for (int j = 1; j < G; ++j) {
                const double len = part_len[tid + j];
                const int i = part_idx[tid + j];
                if (len < best || (len == best && i < best_i)) {
                    best = len;
                    best_i = i;
                }
            }
            float lo = bd_val(rowp[bd_word(best_i)]), hi = bd_val(rowp[bd_word(best_i + a.L)]);
            if (rowp[bd_word(M - 1)] == BD_NAN_KEY) {
                lo = hi = bd_val(BD_NAN_KEY);
                best_i = -1;
            }
            a.sci[d0 + r] = lo;
            a.sci[a.n_dim + d0 + r] = hi;
            a.sci_idx[d0 + r] = best_i;
        }
        __syncthreads();
    }

    if (a.truth) {
        const float t = live ? a.truth[d0 + r] : 0.f;
        int lt = 0, eq = 0;
        for (int m = g; m < M; m += G) {
            const float v = bd_val(rowp[bd_word(m)]);
            lt += v < t;
            eq += v == t;
        }
        int *part_lt = part_idx, *part_eq = reinterpret_cast<int *>(part_len);
        part_lt[tid] = lt;
        part_eq[tid] = eq;
        __syncthreads();
        if (g == 0 && live) {
            for (int j = 1; j < G; ++j) {
                lt += part_lt[tid + j];
                eq += part_eq[tid + j];
            }
            a.below[d0 + r] = lt;
            a.equal[d0 + r] = eq;
        }
    }
}

}  // namespace

extern "C" {

int mcpm_bdec_sort_f32(void *stream, const float *x, int64_t offset0, int64_t n_dim, int n_chain, int64_t stride_chain, int64_t n_draw,
                       int64_t stride_draw, const int *ranks, int n_rank, float *out, int64_t sci_len, float *sci, int *sci_idx,
                       const float *truth, int *below, int *equal, float *sorted) {
    const std::string w("mcpm_bdec_sort_f32");
    if (!x || !ranks || !out) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": null pointer");
    if (n_dim < 1 || n_chain < 1 || n_draw < 1) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": need n_dim, n_chain, n_draw >= 1");
    if (offset0 < 0 || stride_chain < 0 || stride_draw < 0) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": negative offset or stride");
    if (n_rank < 1 || n_rank > MCPM_BDEC_MAX_RANKS) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": need 1 <= n_rank <= MCPM_BDEC_MAX_RANKS");
    if (n_draw > 0x7fffffff || (int64_t)n_chain * n_draw > 0x7fffffff) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": n_chain n_draw out of range");
    const int64_t M = (int64_t)n_chain * n_draw;
    for (int r = 0; r < n_rank; ++r)
        if (ranks[r] < 0 || ranks[r] >= M) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": rank outside [0, n_chain n_draw)");
    if (sci && (!sci_idx || sci_len < 0 || sci_len > M - 1)) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": sci needs sci_idx and 0 <= L <= M - 1");
    if (truth && (!below || !equal)) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": truth needs below and equal");
    if (M > MCPM_BDEC_MAX_M) return mcpm_fail(nullptr, MCPM_E_UNSUPPORTED, w + ": n_chain n_draw above MCPM_BDEC_MAX_M does not fit the LDS tile");
    BdecArgs a;
    a.x = x;
    a.offset0 = offset0;
    a.n_dim = n_dim;
    a.stride_chain = stride_chain;
    a.stride_draw = stride_draw;
    a.n_chain = n_chain;
    a.n_draw = (int)n_draw;
    a.M = (int)M;
    a.p_log = 0;
    while ((1ll << a.p_log) < M) ++a.p_log;
    int td = BD_TILE_KEYS >> a.p_log;
    if (td > BD_MAX_TD) td = BD_MAX_TD;
    a.td_log = 0;
    while ((1 << (a.td_log + 1)) <= td) ++a.td_log;
    a.n_rank = n_rank;
    a.L = sci ? (int)sci_len : 0;
    a.out = out;
    a.sci = sci;
    a.sorted = sorted;
    a.sci_idx = sci_idx;
    a.below = below;
    a.equal = equal;
    a.truth = truth;
    for (int r = 0; r < MCPM_BDEC_MAX_RANKS; ++r) a.ranks[r] = r < n_rank ? ranks[r] : 0;
    const int64_t tiles = (n_dim + (1 << a.td_log) - 1) >> a.td_log;
    if (tiles > 0x7fffffff) return mcpm_fail(nullptr, MCPM_E_ARG, w + ": n_dim out of range");
    bdec_sort_kernel<<<(unsigned)tiles, BD_THREADS, 0, (hipStream_t)stream>>>(a);
    MCPM_LAUNCH_CHECK(nullptr, "bdec_sort_kernel");
    return MCPM_OK;
}

}  // extern "C"
