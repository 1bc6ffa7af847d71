// The permutation and weight rules of rg2cgh / cgh2rg (montecosmo/utils.py:785-921) as device functions, shared by the kernels of
// reshape.hip and by the Fourier-space likelihood (likelihood.hip): one statement of which real element pairs with which stored mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// rg2cgh: source of the real / imaginary part of output mode (i, j, k) (the table at the head of the rg2cgh section of reshape.hip)
struct CghSrc {
    int64_t re, im;   // flat indices into the real tensor (im < 0: none)
    float wre, wim;
};
__device__ __forceinline__ CghSrc cgh_source(int nx, int ny, int nz, int i, int j, int k) {
    const int hx = nx / 2, hy = ny / 2, hz = nz / 2;
    auto at = [&](int a, int b, int c) { return ((int64_t)a * ny + b) * nz + c; };
    CghSrc r;
    r.wre = 1.f;
    r.wim = 1.f;
    if (k > 0 && k < hz) {
        r.re = at(i, j, k);
        r.im = at(i, j, hz + k);
    } else if (j != 0 && j != hy) {
        if (j < hy) {
            r.re = at(i, j, k);
            r.im = at(i, hy + j, k);
        } else {
            const int mi = i ? nx - i : 0;
            r.re = at(mi, ny - j, k);
            r.im = at(mi, hy + ny - j, k);
            r.wim = -1.f;
        }
    } else if (i != 0 && i != hx) {
        if (i < hx) {
            r.re = at(i, j, k);
            r.im = at(hx + i, j, k);
        } else {
            r.re = at(nx - i, j, k);
            r.im = at(hx + nx - i, j, k);
            r.wim = -1.f;
        }
    } else {
        r.re = at(i, j, k);
        r.im = -1;
        r.wre = 1.41421356237309505f;
        r.wim = 0.f;
    }
    return r;
}

// cgh2rg (utils.py:839-889): every real element (x, y, z) takes the value of ONE stored mode -- the mirrored one on the faces and
// edges, as the reference's last assignment does: flat complex index `mode` into the (nx, ny, nz/2+1) half-spectrum, part 0 = real /
// 1 = imaginary, and the weight w (a sign, or 1 / sqrt2 on the eight self-conjugate corners).  norm = "amp" reads Re in[mode] for both
// parts, unsigned and unweighted.
struct CghRead {
    int64_t mode;
    int part;
    float w;
};
__device__ __forceinline__ CghRead cgh2rg_read(int nx, int ny, int nz, int x, int y, int z) {
    const int hx = nx / 2, hy = ny / 2, hz = nz / 2, nzc = hz + 1;
    auto at = [&](int a, int b, int c) { return ((int64_t)a * ny + b) * nzc + c; };
    CghRead r;
    r.part = 0;
    r.w = 1.f;
    if (z != 0 && z != hz) {
        if (z < hz) r.mode = at(x, y, z);
        else r.mode = at(x, y, z - hz), r.part = 1;
    } else if (y != 0 && y != hy) {
        const int mx_ = x ? nx - x : 0;
        if (y < hy) r.mode = at(mx_, ny - y, z);
        else r.mode = at(mx_, ny + hy - y, z), r.part = 1, r.w = -1.f;
    } else if (x != 0 && x != hx) {
        if (x < hx) r.mode = at(nx - x, y, z);
        else r.mode = at(nx + hx - x, y, z), r.part = 1, r.w = -1.f;
    } else {
        r.mode = at(x, y, z);
        r.w = 0.70710678118654752f;
    }
    return r;
}

}  // namespace
