// grid.h - the query lattice of mesh extraction (SSR/geometry/occupancy.py:5-48: grid_within_bound / make_3D_grid), one point at a
// time: grid_point() is the ONE place the lattice is evaluated - by k_grid_points and the host entry point (grid.hip) and by the
// occupancy-grid mode of the 128-point tile body (mlp_f16_t128.hip, kGridTrunk), so all three give the same bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INERF_GRID_HD __host__ __device__ __forceinline__
#else
#define INERF_GRID_HD inline
#endif

namespace inerf {

struct GridSpec {
    const float* t;         // [dim] the axis table (torch.linspace(occ_range[0], occ_range[1], dim), evaluated by the caller)
    int dim;
    float scale[3];         // extents / (0.9 (occ_range[1] - occ_range[0])), rounded to fp32 once (occupancy.py:10-11)
    float m[12];            // rows 0..2 of the box-to-scene transform, row-major 3 x 4
};

// World position of lattice index g = (i * dim + j) * dim + k (torch.meshgrid 'ij', last axis fastest).  make_3D_grid scales the axis
// values (occupancy.py:34), multiplies by a row of the rotation and sums the three products left to right (:40-42), then adds the
// translation (:46): every product and every sum rounded to fp32 on its own.  Device: explicit round-to-nearest intrinsics; host: the
// tree is built with -ffp-contract=off.
INERF_GRID_HD void grid_point(const GridSpec& s, int g, float (&x)[3]) {
    const int k = g % s.dim, ij = g / s.dim;
    const int j = ij % s.dim, i = ij / s.dim;
#if defined(__HIP_DEVICE_COMPILE__)
    const float gx = __fmul_rn(s.t[i], s.scale[0]), gy = __fmul_rn(s.t[j], s.scale[1]), gz = __fmul_rn(s.t[k], s.scale[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
        x[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(s.m[4 * r], gx), __fmul_rn(s.m[4 * r + 1], gy)), __fmul_rn(s.m[4 * r + 2], gz)), s.m[4 * r + 3]);
#else
    const float gx = s.t[i] * s.scale[0], gy = s.t[j] * s.scale[1], gz = s.t[k] * s.scale[2];
    for (int r = 0; r < 3; ++r) {
        const float a = s.m[4 * r] * gx, b = s.m[4 * r + 1] * gy, c = s.m[4 * r + 2] * gz;
        const float ab = a + b;
        const float abc = ab + c;
        x[r] = abc + s.m[4 * r + 3];
    }
#endif
}

}  // namespace inerf
