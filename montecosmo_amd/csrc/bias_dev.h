// Mesh-side spectral machinery of the bias expansions, shared by bias.hip (Lagrangian) and eulerian.hip (Eulerian): on the mode decoder
// of kmode_dev.h, the 10-multiplier table {1, k_i k_j / k^2 (5), -k^2, i k_c (3)} with numpy irfftn's Hermitian projection, and the
// spectra kernels out[s] = scale m_s in with their adjoint.
#pragma once
#include "kmode_dev.h"

namespace {

// the 10 multipliers y_s = irfftn(m_s X): real part re[s] (s = 0..6) or imaginary part im (s = 7..9)
//  0: 1   1: kx kx/k2   2: ky ky/k2   3: kx ky/k2   4: kx kz/k2   5: ky kz/k2   6: -k2   7..9: i k_c
// `herm`: apply numpy irfftn's projection on the kz = 0 / Nyquist planes (odd number of Nyquist factors -> 0)
__device__ __forceinline__ void multipliers(const KMode &m, bool herm, float (&re)[7], float (&im)[3]) {
    const float k2 = m.k[0] * m.k[0] + m.k[1] * m.k[1] + m.k[2] * m.k[2];
    const float ik2 = k2 == 0.f ? 0.f : 1.f / k2;
    const bool pr = herm && m.special;
    re[0] = 1.f;
    re[1] = m.k[0] * m.k[0] * ik2;
    re[2] = m.k[1] * m.k[1] * ik2;
    re[3] = (pr && m.nyq[0] != m.nyq[1]) ? 0.f : m.k[0] * m.k[1] * ik2;
    re[4] = (pr && m.nyq[0] != m.nyq[2]) ? 0.f : m.k[0] * m.k[2] * ik2;
    re[5] = (pr && m.nyq[1] != m.nyq[2]) ? 0.f : m.k[1] * m.k[2] * ik2;
    re[6] = -k2;
#pragma unroll
    for (int c = 0; c < 3; ++c) im[c] = (pr && m.nyq[c]) ? 0.f : m.k[c];
}

// GROUP 0: spectra 0..5 (6 outputs), GROUP 1: spectra 6..9 (4 outputs); out[s] = scale * m_s * in
template <int GROUP>
__global__ __launch_bounds__(256) void bias_spectra_kernel(KGeom kg, float scale,
                                                           const float2 *__restrict__ in, float2 *__restrict__ out, int64_t Mh) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    float re[7], im[3];
    multipliers(m, true, re, im);
    const float2 v = in[idx];
    if (GROUP == 0) {
#pragma unroll
        for (int s = 0; s < 6; ++s) out[s * Mh + idx] = make_float2(scale * re[s] * v.x, scale * re[s] * v.y);
    } else {
        out[idx] = make_float2(scale * re[6] * v.x, scale * re[6] * v.y);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(1 + c) * Mh + idx] = make_float2(-scale * im[c] * v.y, scale * im[c] * v.x);  // (a+ib)(i s)
    }
}

// out (+)= scale * zw * sum_s conj(m_s) in[s]   (adjoint of irfftn o multiply; un-projected multipliers)
template <int GROUP>
__global__ __launch_bounds__(256) void bias_spectra_vjp_kernel(KGeom kg, float scale,
                                                               const float2 *__restrict__ in, float2 *__restrict__ out,
                                                               int64_t Mh, int accumulate) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= Mh) return;
    const KMode m = kdecode(kg, idx);
    float re[7], im[3];
    multipliers(m, false, re, im);
    float ar = 0.f, ai = 0.f;
    if (GROUP == 0) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const float2 v = in[s * Mh + idx];
            ar += re[s] * v.x;
            ai += re[s] * v.y;
        }
    } else {
        const float2 v = in[idx];
        ar += re[6] * v.x;
        ai += re[6] * v.y;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float2 w = in[(1 + c) * Mh + idx];
            ar += im[c] * w.y;   // (a+ib)(-i s)
            ai += -im[c] * w.x;
        }
    }
    ar *= scale * m.zw;
    ai *= scale * m.zw;
    if (accumulate) {
        const float2 o = out[idx];
        ar += o.x;
        ai += o.y;
    }
    out[idx] = make_float2(ar, ai);
}

}  // namespace
