// The mode side of every kernel that runs one thread per stored mode of the plan's half-spectrum: 2 pi fftfreq, the index split, and the
// decoder of the physical wavevector k_cell * kphys[axis] in h/Mpc (float components, float64 norm) with the Nyquist flags and irfftn's
// multiplicity weight.  One copy, so that the transfer table, the linear power and the Kaiser posterior see the same |k| to the bit.
#pragma once
#include "mcpm_internal.h"

namespace {

constexpr float TWO_PI = 6.283185307179586f;

__device__ __forceinline__ int sfreq(int i, int n) { return (i < (n + 1) / 2) ? i : i - n; }  // n * fftfreq(n)[i]
__device__ __forceinline__ float kfreq(int i, int n) {  // 2*pi*fftfreq(n)[i]
    return TWO_PI * (float)sfreq(i, n) / (float)n;
}

struct Idx3 {
    int ix, iy, iz;
};
__device__ __forceinline__ Idx3 ksplit(Geom g, uint32_t idx) {
    Idx3 i;
    i.iz = idx % (uint32_t)g.nzh;
    const uint32_t r = idx / (uint32_t)g.nzh;
    i.iy = r % (uint32_t)g.ny;
    i.ix = r / (uint32_t)g.ny;
    return i;
}

struct KMode {
    float k[3];     // physical wavevector
    double kn;      // its norm
    bool nyq[3], special;
    float zw;       // irfftn multiplicity of the mode: 1 on the kz = 0 / Nyquist planes, 2 elsewhere
};
// what the kernels take by value: the plan's geometry and kphys = mesh_shape / box_size per axis
struct KGeom {
    Geom g;
    float kphys[3];
};
// the entry points' side of it; every one of them that checks for a slab-decomposed plan does it here
__host__ inline int kgeom_arg(mcpm_plan *p, const char *who, float kpx, float kpy, float kpz, KGeom *kg) {
    MCPM_REQUIRE(p, !p->g.xslab, MCPM_E_UNSUPPORTED, std::string(who) + ": not slab-decomposed");
    *kg = KGeom{p->g, {kpx, kpy, kpz}};
    return MCPM_OK;
}
__device__ __forceinline__ KMode kdecode(const KGeom &kg, uint32_t idx) {
    KMode m;
    const Geom &g = kg.g;
    const Idx3 i = ksplit(g, idx);
    m.k[0] = kfreq(i.ix, g.nx) * kg.kphys[0];
    m.k[1] = kfreq(i.iy, g.ny) * kg.kphys[1];
    m.k[2] = TWO_PI * (float)i.iz / (float)g.nz * kg.kphys[2];
    m.kn = sqrt((double)m.k[0] * m.k[0] + (double)m.k[1] * m.k[1] + (double)m.k[2] * m.k[2]);
    m.nyq[0] = !(g.nx & 1) && i.ix == g.nx / 2;
    m.nyq[1] = !(g.ny & 1) && i.iy == g.ny / 2;
    m.nyq[2] = i.iz == g.nz / 2;
    m.special = i.iz == 0 || m.nyq[2];
    m.zw = m.special ? 1.f : 2.f;
    return m;
}

}  // namespace
