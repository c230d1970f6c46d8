// grid.hip - the query lattice of mesh extraction and its occupancy grid (include/inerf.h, "Mesh extraction"): the lattice points as
// a tensor (k_grid_points: the test boundary of grid_point() and what the exact-fp32 and layer-by-layer paths are fed with), the same
// on host pointers, and the launch of the 128-point tile body's occupancy-grid mode (mlp_f16_t128.hip, kGridTrunk).
#include "mlp_common.h"

namespace inerf {

__global__ __launch_bounds__(256) void k_grid_points(const GridSpec g, int first, int64_t count, float* __restrict__ out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= count) return;
    float x[3];
    grid_point(g, first + (int)n, x);
    out[3 * n] = x[0];
    out[3 * n + 1] = x[1];
    out[3 * n + 2] = x[2];
}

// INERF_OK when the lattice and the index range are ones the kernels take
static int grid_args(const float* t, int dim, const float* scale, const float* transform, int64_t first, int64_t count, GridSpec* g) {
    if (!t || !scale || !transform || dim < 2 || dim > INERF_MAX_GRID_DIM || first < 0 || count < 0) return INERF_E_INVALID;
    const int64_t total = (int64_t)dim * dim * dim;
    if (first > total || count > total - first) return INERF_E_INVALID;
    g->t = t;
    g->dim = dim;
    for (int c = 0; c < 3; ++c) g->scale[c] = scale[c];
    for (int c = 0; c < 12; ++c) g->m[c] = transform[c];
    return INERF_OK;
}

}  // namespace inerf

extern "C" int inerf_grid_points(const float* t, int dim, const float* scale, const float* transform, int64_t first, int64_t count,
                                 float* out, void* stream) {
    using namespace inerf;
    GridSpec g;
    const int rc = grid_args(t, dim, scale, transform, first, count, &g);
    if (rc != INERF_OK) return rc;
    if (count == 0) return INERF_OK;
    if (!out) return INERF_E_INVALID;
    hipLaunchKernelGGL(k_grid_points, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, (int)first, count, out);
    return record(hipGetLastError());
}

extern "C" int inerf_grid_points_host(const float* t, int dim, const float* scale, const float* transform, int64_t first, int64_t count,
                                      float* out) {
    using namespace inerf;
    GridSpec g;
    const int rc = grid_args(t, dim, scale, transform, first, count, &g);
    if (rc != INERF_OK) return rc;
    if (count == 0) return INERF_OK;
    if (!out) return INERF_E_INVALID;
    for (int64_t n = 0; n < count; ++n) {
        float x[3];
        grid_point(g, (int)(first + n), x);
        out[3 * n] = x[0];
        out[3 * n + 1] = x[1];
        out[3 * n + 2] = x[2];
    }
    return INERF_OK;
}

extern "C" int inerf_occupancy_grid(const inerf_net_desc* net, const float* packed_weights, const float* t, int dim, const float* scale,
                                    const float* transform, float dist, int64_t first_point, int64_t n_points, float* occ_out,
                                    float* sigma_out, int32_t* status, int64_t status_points, void* stream) {
    using namespace inerf;
    if (!net || !packed_weights || status_points < 0) return INERF_E_INVALID;
    MlpParams p{};
    const int rc = grid_args(t, dim, scale, transform, first_point, n_points, &p.grid);
    if (rc != INERF_OK) return rc;
    if (!net_supported(*net) || net->precision != INERF_PREC_F16X3) return INERF_E_UNSUPPORTED;
    if (n_points == 0) return INERF_OK;
    if (!occ_out) return INERF_E_INVALID;
    const bool ssr = net->variant == INERF_VARIANT_SSR;
    p.wts = packed_weights;
    p.status = status;
    // one range word per status_points LATTICE points: word (first_point + i) / status_points for point i of the launch
    p.status_rays = (status && status_points > 0) ? (int)(status_points < ((int64_t)1 << 30) ? status_points : (int64_t)1 << 30) : 0;
    p.ray0 = (int)first_point;           // ... and lattice index first_point + i
    p.L = make_layout(*net);
    p.n_points = (int)n_points;          // (<= dim^3 <= 2^30)
    p.n_samples = 1;
    p.n_classes = ssr ? net->n_classes : 0;
    p.channels = INERF_BASE_CHANNELS + p.n_classes;
    p.l_xyz = net->l_xyz; p.l_dir = net->l_dir; p.xyz_div = net->xyz_div;
    p.grid_dist = dist;
    p.occ = occ_out;
    p.sigma_out = sigma_out;
    return launch_grid_trunk_f16x3(p, n_points, ssr, (hipStream_t)stream);
}
