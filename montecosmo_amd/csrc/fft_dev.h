// Device-side FFT building blocks of the hand-written Poisson solve (fftpm.hip) -- and of the micro-benchmarks under
// tools/ that take its passes apart (tools/xpass_bench.hip).  See fftpm.hip for the design notes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A complex number is a native two-float vector: the compiler then keeps (re, im) in one aligned register pair and
// maps complex adds to v_pk_add_f32 and complex multiplies to v_pk_mul_f32 + v_pk_fma_f32 (swaps and sign flips ride
// the op_sel / neg modifiers) instead of pairing unrelated scalars and shuffling them with v_mov.
typedef float cf __attribute__((ext_vector_type(2)));
// Streaming stores for pass outputs that the next kernel reads only after everything else has gone by (a 0.5-1.6 GB
// spectrum never survives in the 4 MB L2s): they keep the L2 for the twiddles and the read stream.  Measured at 512^3:
// z / y passes 7 % faster; outputs the fused x pass reads next stay plain stores (with streaming stores there it loses 2 %).
#define NTSTORE(v, p) __builtin_nontemporal_store((v), (p))

__device__ __forceinline__ cf mkc(float x, float y) {
    cf r = {x, y};
    return r;
}
__device__ __forceinline__ cf cadd(cf a, cf b) { return a + b; }
__device__ __forceinline__ cf csub(cf a, cf b) { return a - b; }
__device__ __forceinline__ cf cmul(cf a, cf b) {
    const cf bs = {-b.y, b.x};
    return __builtin_elementwise_fma(a.yy, bs, a.xx * b);
}
// multiply by exp(SIGN * i * pi/2): SIGN = -1 (forward) -> -i, +1 (inverse) -> +i
template <int SIGN>
__device__ __forceinline__ cf mul_i(cf a) {
    return SIGN < 0 ? mkc(a.y, -a.x) : mkc(-a.y, a.x);
}

template <int SIGN>
__device__ __forceinline__ void fft4(cf &a0, cf &a1, cf &a2, cf &a3) {
    cf t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_i<SIGN>(csub(a1, a3));
    a0 = cadd(t0, t2);
    a2 = csub(t0, t2);
    a1 = cadd(t1, t3);
    a3 = csub(t1, t3);
}

// in-place radix-8 DFT: v[k] <- sum_n v[n] exp(SIGN 2 pi i n k / 8)
// This form leaves e + w8^j o to -ffp-contract: the compiler fuses the multiply into the add wherever both land in one basic
// block.  The one-line passes (z, spectrum-side x) keep it -- their code and their bits stay what they were.
template <int SIGN>
__device__ __forceinline__ void fft8(cf (&v)[8]) {
    cf e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    cf o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    fft4<SIGN>(e0, e1, e2, e3);
    fft4<SIGN>(o0, o1, o2, o3);
    const float h = 0.70710678118654752f;
    // w8^1 = (1 + SIGN i)/sqrt2, w8^2 = SIGN i, w8^3 = (-1 + SIGN i)/sqrt2
    cf w1 = SIGN < 0 ? mkc(h * (o1.x + o1.y), h * (o1.y - o1.x)) : mkc(h * (o1.x - o1.y), h * (o1.y + o1.x));
    cf w2 = mul_i<SIGN>(o2);
    cf w3 = SIGN < 0 ? mkc(h * (o3.y - o3.x), -h * (o3.x + o3.y)) : mkc(-h * (o3.x + o3.y), h * (o3.x - o3.y));
    v[0] = cadd(e0, o0);
    v[4] = csub(e0, o0);
    v[1] = cadd(e1, w1);
    v[5] = csub(e1, w1);
    v[2] = cadd(e2, w2);
    v[6] = csub(e2, w2);
    v[3] = cadd(e3, w3);
    v[7] = csub(e3, w3);
}

// The same DFT with the fused multiply-adds of the odd outputs WRITTEN OUT (what the form above compiles to in straight-line
// code), for the passes that hold two lines per thread: there the compiler's choice would depend on the code around the
// transform (a branch in a pass's epilogue, the number of lines a thread holds), and with it the rounding of a line.
// (s[m], d[m] = v[m] + v[m + 4], v[m] - v[m + 4], m = 0..3: the first butterflies, formed by the caller)
template <int SIGN>
__device__ __forceinline__ void fft8_tail(cf (&v)[8], const cf (&s)[4], const cf (&d)[4]) {
#pragma clang fp contract(off)
    // even points 0 2 4 6 and odd points 1 3 5 7: a radix-4 each, first butterflies done
    const cf te = mul_i<SIGN>(d[2]), to = mul_i<SIGN>(d[3]);
    const cf e0 = cadd(s[0], s[2]), e2 = csub(s[0], s[2]), e1 = cadd(d[0], te), e3 = csub(d[0], te);
    const cf o0 = cadd(s[1], s[3]), o2 = csub(s[1], s[3]), o1 = cadd(d[1], to), o3 = csub(d[1], to);
    const cf h = {0.70710678118654752f, 0.70710678118654752f};
    // w8^1 = (1 + SIGN i)/sqrt2, w8^2 = SIGN i, w8^3 = (-1 + SIGN i)/sqrt2; s1 = w8^1 o1 sqrt2, s3 = w8^3 o3 sqrt2
    const cf s1 = SIGN < 0 ? mkc(o1.x + o1.y, o1.y - o1.x) : mkc(o1.x - o1.y, o1.y + o1.x);
    const cf w2 = mul_i<SIGN>(o2);
    const cf s3 = SIGN < 0 ? mkc(o3.y - o3.x, -(o3.x + o3.y)) : mkc(-(o3.x + o3.y), o3.x - o3.y);
    v[0] = cadd(e0, o0);
    v[4] = csub(e0, o0);
    v[1] = __builtin_elementwise_fma(h, s1, e1);
    v[5] = __builtin_elementwise_fma(-h, s1, e1);
    v[2] = cadd(e2, w2);
    v[6] = csub(e2, w2);
    v[3] = __builtin_elementwise_fma(h, s3, e3);
    v[7] = __builtin_elementwise_fma(-h, s3, e3);
}
template <int SIGN>
__device__ __forceinline__ void fft8x(cf (&v)[8]) {
    cf s[4], d[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        s[m] = cadd(v[m], v[m + 4]);
        d[m] = csub(v[m], v[m + 4]);
    }
    fft8_tail<SIGN>(v, s, d);
}
// radix-8 DFT of the points f[m] v[m] (f real): the scaling rides the first butterflies, f[m] v[m] +- (f[m+4] v[m+4]) with the
// second product rounded and the first fused
template <int SIGN>
__device__ __forceinline__ void fft8_scaled(cf (&v)[8], const float (&f)[8]) {
#pragma clang fp contract(off)
    cf s[4], d[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const cf fm = {f[m], f[m]}, fp = {f[m + 4], f[m + 4]};
        const cf p = fp * v[m + 4];
        s[m] = __builtin_elementwise_fma(fm, v[m], p);
        d[m] = __builtin_elementwise_fma(fm, v[m], -p);
    }
    fft8_tail<SIGN>(v, s, d);
}

// LDS addressing of a tile of LINES lines of N points.  `e` is the point index; each exchange skews it by
// (e / S) * S2 (S = size of the sub-transform that READS the exchange) to spread the strided reads over banks.
template <int N, int LINES, bool LINE_FASTEST>
struct Tile {
    static constexpr int NP = N + N / 8 + 8;  // padded points per line
    static constexpr int FLOATS2 = NP * LINES;
    int l;
    __device__ __forceinline__ int operator()(int e_padded) const {
        return LINE_FASTEST ? e_padded * LINES + l : l * NP + e_padded;
    }
};

template <int N>
struct FftShape {
    static constexpr int T = N / 8;
    static constexpr int NST8 = (N == 64 || N == 128 || N == 256) ? 2 : 3;
    static constexpr int P8 = NST8 == 2 ? 64 : 512;
    static constexpr int RL = N / P8;  // last radix: 1 (none), 2 or 4
    static_assert(N == 64 || N == 128 || N == 256 || N == 512 || N == 1024, "unsupported FFT length");
};

// NL complex numbers that sit next to each other in memory (the kz = 2j, 2j+1 columns of a column pass): one 16-byte access
typedef float cf2 __attribute__((ext_vector_type(4)));
template <int NL>
__device__ __forceinline__ void lds_put(cf *p, const cf (&v)[NL][8], int k) {
    if (NL == 1) *p = v[0][k];
    else *reinterpret_cast<cf2 *>(p) = __builtin_shufflevector(v[0][k], v[NL - 1][k], 0, 1, 2, 3);
}
template <int NL>
__device__ __forceinline__ void lds_get(const cf *p, cf (&v)[NL][8], int k) {
    if (NL == 1) v[0][k] = *p;
    else {
        const cf2 t = *reinterpret_cast<const cf2 *>(p);
        v[0][k] = t.xy;
        v[NL - 1][k] = t.zw;
    }
}

// Length-N FFT of NL lines (NL = 1, or 2: the thread's two ADJACENT lines of a line-fastest tile, tile.l even and the tile
// 16-byte aligned, so that every exchange moves the pair as one 16-byte LDS access; the two chains are independent and run
// the one-line arithmetic each, sharing the stage twiddles).
// In: v[i][m] = x_i[u + T m].  Out: v[i][m] = X_i[u + T m].  W[j] = exp(-2 pi i j / N).
// Every thread of the workgroup must call it (it synchronises the workgroup).
// DBG (micro-benchmarks only; 0 in the library): bit 0 drops the workgroup barriers (wrong results, right instruction
// stream: what the barriers cost), bit 1 replaces the twiddle-table loads by a constant (what their latency costs).
// PRE (micro-benchmark only; the library passes false): the stage twiddles come from registers (`tw`, filled by fft_twiddles
// before the pass's global loads were issued) instead of a table load behind every exchange barrier.  Measured SLOWER
// (tools/xpass_bench.hip: fused x pass 0.545 vs 0.505 ms): the six extra registers cost more than the hidden latency gains.
// SCALED: the transform of f[i][m] v[i][m] (fft8_scaled).
template <int N, int SIGN, class TILE, int DBG, bool PRE, int NL, bool SCALED = false>
__device__ __forceinline__ void fft_line_core(cf (&v)[NL][8], cf *lds, const cf *__restrict__ W, const cf (&tw)[3], int u, const TILE &tile,
                                              const float (*f)[8] = nullptr) {
    static_assert(NL == 1 || NL == 2, "one line or one pair of lines per thread");
    constexpr int T = FftShape<N>::T, NST8 = FftShape<N>::NST8, RL = FftShape<N>::RL;
    int P = 1, S = N;
#pragma unroll
    for (int s = 0; s < NST8; ++s) {
        const int S2 = S / 8;
        const int K = u / S2, n2 = u - K * S2;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            if (SCALED && s == 0) fft8_scaled<SIGN>(v[i], f[i]);
            else if (NL == 1) fft8<SIGN>(v[i]);
            else fft8x<SIGN>(v[i]);
        }
        if (S2 > 1) {
            cf w1 = (DBG & 2) ? mkc(0.6f, 0.8f) : (PRE ? tw[s] : W[n2 * P]);
            // the powers of a register-held twiddle are recomputed by every transform of a kernel: left to common-subexpression
            // elimination they stay live across all of them (28 registers per stage; the fused x pass went from 108 to 152)
            if (PRE) asm volatile("" : "+v"(w1));
            if (SIGN > 0) w1.y = -w1.y;
            const cf w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                v[i][1] = cmul(v[i][1], w1);
                v[i][2] = cmul(v[i][2], w2);
                v[i][3] = cmul(v[i][3], w3);
                v[i][4] = cmul(v[i][4], w4);
                v[i][5] = cmul(v[i][5], cmul(w4, w1));
                v[i][6] = cmul(v[i][6], cmul(w4, w2));
                v[i][7] = cmul(v[i][7], cmul(w4, w3));
            }
        }
        const bool final_stage = (s == NST8 - 1) && (RL == 1);
        if (!final_stage) {
            // exchange: outputs at e = (K + P k) S2 + n2; next stage (sub-size S2) reads e = K' S2 + n1 (S2/R') + n2'
            const int Snext = S2;
            const int S2next = (s == NST8 - 1) ? 1 : S2 / 8;
            if (!(DBG & 1)) __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = (K + P * k) * S2 + n2;
                // the small last radix reads with stride RL: skew by one point per 32 instead
                lds_put<NL>(&lds[tile((s == NST8 - 1) ? e + (e >> 5) : e + (e / Snext) * S2next)], v, k);
            }
            if (!(DBG & 1)) __syncthreads();
            if (s < NST8 - 1) {
                const int Kn = u / S2next, n2n = u - Kn * S2next;
#pragma unroll
                for (int n1 = 0; n1 < 8; ++n1) {
                    const int e = Kn * Snext + n1 * S2next + n2n;
                    lds_get<NL>(&lds[tile(e + (e / Snext) * S2next)], v, n1);
                }
            }
        }
        P *= 8;
        S = S2;
    }
    if (RL > 1) {
        // last stage, radix RL: thread u owns butterflies K = u + T j; inputs e = K RL + n1; outputs X[K + P k]
        constexpr int NB = 8 / (RL > 1 ? RL : 8);
        cf x[NL][8];
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int n1 = 0; n1 < RL; ++n1) {
                const int e = (u + T * j) * RL + n1;
                lds_get<NL>(&lds[tile(e + (e >> 5))], x, j * RL + n1);
            }
#pragma unroll
        for (int i = 0; i < NL; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (RL == 2) {
                    cf a = x[i][2 * j], b = x[i][2 * j + 1];
                    v[i][j] = cadd(a, b);
                    v[i][j + NB] = csub(a, b);
                } else {
                    cf a0 = x[i][4 * j], a1 = x[i][4 * j + 1], a2 = x[i][4 * j + 2], a3 = x[i][4 * j + 3];
                    fft4<SIGN>(a0, a1, a2, a3);
                    v[i][j] = a0;
                    v[i][j + NB] = a1;
                    v[i][j + 2 * NB] = a2;
                    v[i][j + 3 * NB] = a3;
                }
            }
    }
}


// first twiddle of every radix-8 stage of thread u: tw[s] = W[(u mod S2_s) P_s], S2_s = N / 8^(s+1), P_s = 8^s
template <int N>
__device__ __forceinline__ void fft_twiddles(const cf *__restrict__ W, int u, cf (&tw)[3]) {
    constexpr int NST8 = FftShape<N>::NST8;
    int P = 1, S = N;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int S2 = S / 8;
        tw[s] = (s < NST8 && S2 > 1) ? W[(u % S2) * P] : mkc(1.f, 0.f);
        P *= 8;
        S = S2 > 0 ? S2 : 1;
    }
}

// The one-line core (z passes, plain y pass, spectrum-side x passes; a line held as cf[8]): kept as it always was,
// word for word, so that those kernels keep their code objects and their bits; DBG / PRE as above.
template <int N, int SIGN, class TILE, int DBG, bool PRE>
__device__ __forceinline__ void fft_line_core(cf (&v)[8], cf *lds, const cf *__restrict__ W, const cf (&tw)[3], int u, const TILE &tile) {
    constexpr int T = FftShape<N>::T, NST8 = FftShape<N>::NST8, RL = FftShape<N>::RL;
    int P = 1, S = N;
#pragma unroll
    for (int s = 0; s < NST8; ++s) {
        const int S2 = S / 8;
        const int K = u / S2, n2 = u - K * S2;
        fft8<SIGN>(v);
        if (S2 > 1) {
            cf w1 = (DBG & 2) ? mkc(0.6f, 0.8f) : (PRE ? tw[s] : W[n2 * P]);
            // the powers of a register-held twiddle are recomputed by every transform of a kernel: left to common-subexpression
            // elimination they stay live across all of them (28 registers per stage; the fused x pass went from 108 to 152)
            if (PRE) asm volatile("" : "+v"(w1));
            if (SIGN > 0) w1.y = -w1.y;
            const cf w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
            v[1] = cmul(v[1], w1);
            v[2] = cmul(v[2], w2);
            v[3] = cmul(v[3], w3);
            v[4] = cmul(v[4], w4);
            v[5] = cmul(v[5], cmul(w4, w1));
            v[6] = cmul(v[6], cmul(w4, w2));
            v[7] = cmul(v[7], cmul(w4, w3));
        }
        const bool final_stage = (s == NST8 - 1) && (RL == 1);
        if (!final_stage) {
            // exchange: outputs at e = (K + P k) S2 + n2; next stage (sub-size S2) reads e = K' S2 + n1 (S2/R') + n2'
            const int Snext = S2;
            const int S2next = (s == NST8 - 1) ? 1 : S2 / 8;
            if (!(DBG & 1)) __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = (K + P * k) * S2 + n2;
                // the small last radix reads with stride RL: skew by one point per 32 instead
                lds[tile((s == NST8 - 1) ? e + (e >> 5) : e + (e / Snext) * S2next)] = v[k];
            }
            if (!(DBG & 1)) __syncthreads();
            if (s < NST8 - 1) {
                const int Kn = u / S2next, n2n = u - Kn * S2next;
#pragma unroll
                for (int n1 = 0; n1 < 8; ++n1) {
                    const int e = Kn * Snext + n1 * S2next + n2n;
                    v[n1] = lds[tile(e + (e / Snext) * S2next)];
                }
            }
        }
        P *= 8;
        S = S2;
    }
    if (RL > 1) {
        // last stage, radix RL: thread u owns butterflies K = u + T j; inputs e = K RL + n1; outputs X[K + P k]
        constexpr int NB = 8 / (RL > 1 ? RL : 8);
        cf x[8];
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int n1 = 0; n1 < RL; ++n1) {
                const int e = (u + T * j) * RL + n1;
                x[j * RL + n1] = lds[tile(e + (e >> 5))];
            }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (RL == 2) {
                cf a = x[2 * j], b = x[2 * j + 1];
                v[j] = cadd(a, b);
                v[j + NB] = csub(a, b);
            } else {
                cf a0 = x[4 * j], a1 = x[4 * j + 1], a2 = x[4 * j + 2], a3 = x[4 * j + 3];
                fft4<SIGN>(a0, a1, a2, a3);
                v[j] = a0;
                v[j + NB] = a1;
                v[j + 2 * NB] = a2;
                v[j + 3 * NB] = a3;
            }
        }
    }
}


template <int N, int SIGN, class TILE, int DBG = 0>
__device__ __forceinline__ void fft_line(cf (&v)[8], cf *lds, const cf *__restrict__ W, int u, const TILE &tile) {
    const cf none[3] = {mkc(1.f, 0.f), mkc(1.f, 0.f), mkc(1.f, 0.f)};
    fft_line_core<N, SIGN, TILE, DBG, false>(v, lds, W, none, u, tile);
}
template <int N, int SIGN, class TILE, int DBG = 0>
__device__ __forceinline__ void fft_line_tw(cf (&v)[8], cf *lds, const cf (&tw)[3], int u, const TILE &tile) {
    fft_line_core<N, SIGN, TILE, DBG, true>(v, lds, nullptr, tw, u, tile);
}

// NL lines per thread held as v[NL][8] (the column passes that have a pair form; their one-column forms, NL = 1, take this
// core too: it fits the 1024-thread forms into 128 VGPRs without scratch)
template <int N, int SIGN, class TILE, int DBG = 0, int NL>
__device__ __forceinline__ void fft_line(cf (&v)[NL][8], cf *lds, const cf *__restrict__ W, int u, const TILE &tile) {
    const cf none[3] = {mkc(1.f, 0.f), mkc(1.f, 0.f), mkc(1.f, 0.f)};
    fft_line_core<N, SIGN, TILE, DBG, false, NL>(v, lds, W, none, u, tile);
}
template <int N, int SIGN, class TILE, int DBG = 0, int NL>
__device__ __forceinline__ void fft_line_tw(cf (&v)[NL][8], cf *lds, const cf (&tw)[3], int u, const TILE &tile) {
    fft_line_core<N, SIGN, TILE, DBG, true, NL>(v, lds, nullptr, tw, u, tile);
}
// the transform of the lines f[i][m] v[i][m]
template <int N, int SIGN, class TILE, int NL>
__device__ __forceinline__ void fft_line_scaled(cf (&v)[NL][8], const float (&f)[NL][8], cf *lds, const cf *__restrict__ W, int u, const TILE &tile) {
    const cf none[3] = {mkc(1.f, 0.f), mkc(1.f, 0.f), mkc(1.f, 0.f)};
    fft_line_core<N, SIGN, TILE, 0, false, NL, true>(v, lds, W, none, u, tile, f);
}
