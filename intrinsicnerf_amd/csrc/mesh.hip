// mesh.hip - the last step of mesh extraction (SSR/extract_colour_mesh.py:248-257): the 8-bit colour of every mesh vertex from what
// render_rays returned for the vertex's ray, written on the device so that three bytes per vertex are all that travels to the host:
//   colour mode   : to8b(rgb) (:253-255) - to_u8.h's conversion, byte-equal to inerf_frame_to_u8 (NaN -> 0)
//   semantic mode : colour_map[label] (:249-251) with the label of sem_label.h's sem_tile, the device function inerf_sem_maps uses
//                   (the lowest index of the row's maximum logit; a NaN in the row or a non-finite maximum: label 0)
// A few bytes per vertex either way: one thread per vertex in colour mode, one wave per 64 rows of logits in semantic mode (sem_tile's
// own row-to-lane mapping, which reads the rows coalesced and hands row r of the tile to lane r).  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/inerf.h"
#include "sem_label.h"
#include "to_u8.h"

namespace inerf {

int record(hipError_t e);

constexpr int kMeshThreads = 256;

__global__ __launch_bounds__(kMeshThreads) void k_vertex_rgb(const float* __restrict__ rgb, long long stride, long long n,
                                                             unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
    if (i >= n) return;
    const float* __restrict__ src = rgb + i * stride;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = (unsigned char)to_u8(src[k]);
}

template <int G>
__global__ __launch_bounds__(kMeshThreads) void k_vertex_labels(const SemIO io, long long n, const unsigned char* __restrict__ cmap,
                                                                unsigned char* __restrict__ out, int* __restrict__ labels) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row0 = ((long long)blockIdx.x * (kMeshThreads / 64) + wave) * 64;
    if (row0 >= n) return;                              // the whole wave leaves together: sem_tile shuffles across it
    float label, entropy;
    sem_tile<G>(io, row0, n, lane, label, entropy);
    const long long i = row0 + lane;
    if (i >= n) return;
    const int l = (int)label;                           // 0 <= l < n_classes: an index sem_tile saw, or 0
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = cmap[3 * l + k];
    if (labels) labels[i] = l;
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace inerf

extern "C" int inerf_vertex_colours(const float* rgb, int64_t rgb_stride, const float* logits, int64_t logits_stride, int64_t n,
                                    int n_classes, const unsigned char* colour_map, unsigned char* colours_out, int32_t* labels_out,
                                    void* stream) {
    using namespace inerf;
    if ((rgb != nullptr) == (logits != nullptr) || n < 0) return INERF_E_INVALID;
    if (logits && (n_classes < 1 || n_classes > INERF_MAX_CLASSES)) return INERF_E_UNSUPPORTED;
    if (rgb ? rgb_stride < 3 : logits_stride < n_classes) return INERF_E_INVALID;
    if (n == 0) return INERF_OK;
    if (!colours_out || (logits && !colour_map) || misaligned(rgb, 4) || misaligned(logits, 4) || misaligned(labels_out, 4)) return INERF_E_INVALID;
    const long long blocks = (n + kMeshThreads - 1) / kMeshThreads;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    const dim3 grid((unsigned)blocks), block(kMeshThreads);
    hipStream_t s = (hipStream_t)stream;
    if (rgb) {
        hipLaunchKernelGGL(k_vertex_rgb, grid, block, 0, s, rgb, (long long)rgb_stride, (long long)n, colours_out);
        return record(hipGetLastError());
    }
    const SemIO io{logits, (long long)logits_stride, n_classes, nullptr, 1, nullptr, 1};
#define INERF_MESH_CASE(G) case G: hipLaunchKernelGGL((k_vertex_labels<G>), grid, block, 0, s, io, (long long)n, colour_map, colours_out, labels_out); break;
    switch (lanes_per_row(n_classes)) {
        INERF_MESH_CASE(1) INERF_MESH_CASE(2) INERF_MESH_CASE(4) INERF_MESH_CASE(8) INERF_MESH_CASE(16) INERF_MESH_CASE(32) INERF_MESH_CASE(64)
    }
#undef INERF_MESH_CASE
    return record(hipGetLastError());
}
