// cluster_search.h - the per-tile nearest-anchor search of the albedo clustering, shared by the kernels that snap a
// pixel to its cluster centre: k_cluster_lookup (cluster.hip) and k_cluster_snap_compose (refresh.hip).  One
// instruction sequence, one argmin rule, one NaN rule for both - see cluster.hip's header comment for the mapping
// of pixels and anchors onto a wave and for the rounding order.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace inerf {

constexpr int kFrameTile = 8;      // pixels per wave when there are enough pixels to fill the chip that way
constexpr int kBatchTile = 1;      // ... and for small batches (a training step): one pixel per wave

struct ClusterTables {
    const float4* anchors;        // [A] {a0, a1, a2, a0^2+a1^2+a2^2}
    const int* links;             // [A] centre of each anchor, relative to its class
    const int* anchor_begin;      // [K+1]
    const float* factor;          // [K] intensity_factor of each class's cluster
    const float* centers;         // [Ctot,3]
    const int* center_begin;      // [K+1]
    int n_classes;
};

constexpr long long kSmallBatch = 16384;

// true when (d1, i1) loses against (d2, i2) under torch.argmin's ordering
__device__ __forceinline__ bool loses(float d1, int i1, float d2, int i2) {
    if (i2 == INT_MAX) return false;
    if (i1 == INT_MAX) return true;
    const bool n1 = d1 != d1, n2 = d2 != d2;
    if (n1 || n2) return n1 && n2 ? i2 < i1 : n2;
    return d2 < d1 || (d2 == d1 && i2 < i1);
}

// every lane strides over the class's anchors and keeps, per pixel of the tile, the best (distance, index) it has seen
template <int kPixTile, bool kMasked>
__device__ __forceinline__ void scan_anchors(const float4* __restrict__ rows, int count, int lane, unsigned long long members,
                                             const float (&q0)[kPixTile], const float (&q1)[kPixTile], const float (&q2)[kPixTile],
                                             const float (&qs)[kPixTile], float (&best)[kPixTile], int (&idx)[kPixTile]) {
    constexpr int kAhead = kPixTile == 1 ? 8 : 4;                               // independent 16-byte loads in flight per lane (L2 latency)
    for (int a0 = lane; a0 < count; a0 += 64 * kAhead) {
        float4 an[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) an[u] = a0 + 64 * u < count ? rows[a0 + 64 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int a = a0 + 64 * u;
            if (a >= count) break;
#pragma unroll
            for (int j = 0; j < kPixTile; ++j) {
                if (kMasked && !((members >> j) & 1ull)) continue;      // wave-uniform
                const float dot = __fmaf_rn(an[u].z, q2[j], __fmaf_rn(an[u].y, q1[j], __fmul_rn(an[u].x, q0[j])));
                const float dist = __fsub_rn(__fadd_rn(an[u].w, qs[j]), __fmul_rn(2.0f, dot));
                // ascending a inside the lane: strict < keeps the first minimum, a NaN sticks once taken
                const bool take = idx[j] == INT_MAX || dist < best[j] || (dist != dist && best[j] == best[j]);
                best[j] = take ? dist : best[j];
                idx[j] = take ? a : idx[j];
            }
        }
    }
}

// the class a label selects: -1 where it lies outside [0, K) or its class has no cluster (an empty anchor range)
__device__ __forceinline__ int cluster_class(const ClusterTables& t, long long lab) {
    return lab >= 0 && lab < t.n_classes && t.anchor_begin[lab + 1] > t.anchor_begin[lab] ? (int)lab : -1;
}

// mapping_color (cluster.py:324-330): intensity = r+g+b; (intensity/3.0*factor, g/intensity, b/intensity), and its |.|^2
__device__ __forceinline__ void map_color(float r, float g, float b, float factor, float& d0, float& d1, float& d2, float& sb) {
    const float intensity = __fadd_rn(__fadd_rn(r, g), b);
    d0 = __fmul_rn(__fdiv_rn(intensity, 3.0f), factor);
    d1 = __fdiv_rn(g, intensity);
    d2 = __fdiv_rn(b, intensity);
    sb = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
}

// Whole wave.  Lane j < kPixTile holds pixel j of the tile: its class `cls` (-1: none) and mapped colour (d0, d1, d2,
// sb = |d|^2).  Returns, in the pixel lanes with a class, the index of the nearest anchor inside that class (-1 elsewhere).
template <int kPixTile>
__device__ __forceinline__ int nearest_anchor(const ClusterTables& t, int cls, int lane, float d0, float d1, float d2, float sb) {
    float q0[kPixTile], q1[kPixTile], q2[kPixTile], qs[kPixTile];
#pragma unroll
    for (int j = 0; j < kPixTile; ++j) {
        q0[j] = __shfl(d0, j); q1[j] = __shfl(d1, j); q2[j] = __shfl(d2, j); qs[j] = __shfl(sb, j);
    }

    int winner = -1;                                        // pixel lanes: index of the nearest anchor inside the class
    unsigned long long todo = __ballot(cls >= 0);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int c = __shfl(cls, first);
        const unsigned long long members = __ballot(cls == c) & todo;
        todo &= ~members;
        const int begin = t.anchor_begin[c], count = t.anchor_begin[c + 1] - begin;
        float best[kPixTile];
        int idx[kPixTile];
#pragma unroll
        for (int j = 0; j < kPixTile; ++j) { best[j] = 0.f; idx[j] = INT_MAX; }
        const float4* __restrict__ rows = t.anchors + begin;
        if (__popcll(members) == kPixTile)                  // the usual tile of a frame: one class, no tests inside the loop
            scan_anchors<kPixTile, false>(rows, count, lane, members, q0, q1, q2, qs, best, idx);
        else                                                // mixed tile (training batch): only this class's pixels
            scan_anchors<kPixTile, true>(rows, count, lane, members, q0, q1, q2, qs, best, idx);
#pragma unroll
        for (int j = 0; j < kPixTile; ++j) {
            if (!((members >> j) & 1ull)) continue;         // wave-uniform
            float bd = best[j];
            int bi = idx[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float od = __shfl_xor(bd, o);
                const int oi = __shfl_xor(bi, o);
                if (loses(bd, bi, od, oi)) { bd = od; bi = oi; }
            }
            if (lane == j) winner = bi;
        }
    }
    return winner;
}

}  // namespace inerf
