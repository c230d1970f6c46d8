// cluster.hip - nearest-anchor lookup of the albedo clustering:
//   Cluster_Manager.dest_color / dest_class  SSR/training/cluster.py:73-98
//   Cluster.dest_color / dest_class          cluster.py:275-297   (batches of 10 240 pixels)
//   compute_dist + nearest_anchor            cluster.py:299-310   ([anchors, batch] distance matrix + argmin)
//   mapping_color                            cluster.py:324-330
// The reference loops over the semantic classes on the host (a boolean-mask gather, a distance matrix of
// anchors x 10 240 floats, an argmin and a scatter per class: ~10 launches and one host sync each).  Here ONE launch
// covers every class: the anchors of all classes sit in one table ({a0, a1, a2, |a|^2} per anchor, class c owning
// rows anchor_begin[c] .. anchor_begin[c+1]) and nothing but the 12-byte pixel and its label is read from HBM -
// the distance matrix never exists.
//
// Mapping: a wave owns a tile of 8 consecutive pixels, its 64 lanes stride over the anchors of the tile's class
// (16-byte coalesced loads out of L2; every anchor is used for all 8 pixels), each lane keeps its best
// (distance, index) per pixel and a 6-step butterfly picks the winner.  Tiles whose pixels belong to several
// classes (class boundaries in a frame) take one pass per distinct class.  Batches of up to 16 384 pixels (a
// training step: 1 024 random pixels) get one wave per pixel instead, so that the chip is filled and no tile mixes classes.
//
// Arithmetic: d_rgb = (sum/3*f, g/sum, b/sum) and dist = (|a|^2 + |b|^2) - 2 a.b exactly as written in the
// reference (fp32, true divisions, no contraction); a.b, which the reference takes from a library GEMM with an
// unspecified accumulation order, is the FMA chain fma(a2,b2, fma(a1,b1, a0*b0)).  argmin follows torch's rule:
// the first minimal index wins, a NaN distance counts as smaller than everything.
#include <hip/hip_runtime.h>

#include "cluster_search.h"        // ClusterTables, loses, scan_anchors, map_color, nearest_anchor: shared with refresh.hip
#include "layout.h"

namespace inerf {

int record(hipError_t e);

template <int kPixTile>
__global__ __launch_bounds__(256) void k_cluster_lookup(const float* __restrict__ rgb, const long long* __restrict__ label,
                                                        long long n, ClusterTables t, int ignore_label,
                                                        float* __restrict__ out_color, long long* __restrict__ out_class) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long p = tile * kPixTile + lane;
    if (tile * kPixTile >= n) return;                       // whole wave
    const bool pixel_lane = lane < kPixTile && p < n;

    float r = 0.f, g = 0.f, b = 0.f;
    int cls = -1;
    if (pixel_lane) {
        r = rgb[p * 3 + 0]; g = rgb[p * 3 + 1]; b = rgb[p * 3 + 2];
        const long long lab = ignore_label ? 0 : label[p];
        cls = cluster_class(t, lab);
    }
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, sb = 0.f;
    if (cls >= 0) map_color(r, g, b, t.factor[cls], d0, d1, d2, sb);
    const int winner = nearest_anchor<kPixTile>(t, cls, lane, d0, d1, d2, sb);

    if (!pixel_lane) return;
    if (cls >= 0) {
        const int link = t.links[t.anchor_begin[cls] + winner];
        if (out_color) {
            const float* ctr = t.centers + 3ll * (t.center_begin[cls] + link);
            out_color[p * 3 + 0] = ctr[0]; out_color[p * 3 + 1] = ctr[1]; out_color[p * 3 + 2] = ctr[2];
        }
        if (out_class) out_class[p] = link;
    } else {                                                // no cluster for this label: colour unchanged, class 0
        if (out_color) { out_color[p * 3 + 0] = r; out_color[p * 3 + 1] = g; out_color[p * 3 + 2] = b; }
        if (out_class) out_class[p] = 0;
    }
}

}  // namespace inerf

extern "C" int inerf_cluster_lookup(const float* rgb, const int64_t* label, int64_t n_pixels, const float* anchors,
                                    const int32_t* links, const int32_t* anchor_begin, const float* factor,
                                    const float* centers, const int32_t* center_begin, int n_classes, uint32_t flags,
                                    float* out_color, int64_t* out_class, void* stream) {
    using namespace inerf;
    if (n_pixels == 0) return INERF_OK;
    const bool ignore_label = (flags & INERF_CLUSTER_IGNORE_LABEL) != 0;
    if (n_pixels < 0 || !rgb || (!label && !ignore_label) || !anchors || !links || !anchor_begin || !factor || !centers ||
        !center_begin || n_classes < 1 || (!out_color && !out_class))
        return INERF_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(anchors) & 15) != 0) return INERF_E_INVALID;      // float4 loads
    const bool small = n_pixels <= kSmallBatch;
    const int tile = small ? kBatchTile : kFrameTile;
    const long long tiles = (n_pixels + tile - 1) / tile;
    const long long blocks = (tiles + 3) / 4;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    ClusterTables t{reinterpret_cast<const float4*>(anchors), links, anchor_begin, factor, centers, center_begin, n_classes};
    auto kernel = small ? k_cluster_lookup<kBatchTile> : k_cluster_lookup<kFrameTile>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rgb,
                       reinterpret_cast<const long long*>(label), (long long)n_pixels, t, ignore_label ? 1 : 0, out_color,
                       reinterpret_cast<long long*>(out_class));
    return record(hipGetLastError());
}
