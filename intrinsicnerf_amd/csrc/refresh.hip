// refresh.hip - the cluster-refresh pass of render_path(update_cluster=True) (run_nerf.py:142-272 | trainer.py:1221-1443)
// on the device, either side of the mean-shift fit (cluster_fit.hip):
//   k_frame_subsample       : every step-th pixel of a rendered frame's albedo (and label) columns into the fit's sample
//                             table, plus the per-class pixel counts the fit's host side needs
//                             (albedos[-1][::2, ::2, :].reshape(-1, 3), label[::2, ::2].reshape(-1, 1);
//                             run_nerf.py:176-178 | trainer.py:1287-1289)
//   k_cluster_snap_compose  : dest_color of every pixel of a frame and the two 8-bit images written from it -
//                             c = to8b(clustered), edit = to8b(clustered * shading + residual)
//                             (run_nerf.py:226-241 | trainer.py:1425-1440); the float colour and the float edit image
//                             never reach HBM
// The nearest-anchor search is cluster.hip's (cluster_search.h): the same instruction sequence, argmin and NaN rules.
// edit rounds as numpy does: one fp32 product, one fp32 sum (no contraction); to8b is k_frame_to_u8's rule
// (frame_ops.hip): clip to [0, 1], the fp32 product 255 * c, truncation, NaN -> 0.
#include <hip/hip_runtime.h>

#include "cluster_search.h"
#include "layout.h"
#include "to_u8.h"

namespace inerf {

int record(hipError_t e);

constexpr int kMaxLdsClasses = 256;       // class counts are summed per block in LDS up to here, by global atomics beyond

// One thread per output row o = (r / step) * ceil(W / step) + c / step.  Loads are `step * row_stride` floats apart (a
// gather by nature); the stores of a wave are 768 / 512 contiguous bytes.
__global__ __launch_bounds__(256) void k_frame_subsample(const float* __restrict__ frame, long long row_stride, int albedo_col,
                                                         int label_col, int width, int step, int out_w, long long rows,
                                                         float* __restrict__ out_pixels, long long* __restrict__ out_labels,
                                                         int* __restrict__ class_counts, int n_classes) {
    __shared__ int hist[kMaxLdsClasses];
    const bool count = label_col >= 0 && class_counts != nullptr;
    const bool in_lds = count && n_classes <= kMaxLdsClasses;            // block-uniform
    if (in_lds) {
        for (int c = threadIdx.x; c < n_classes; c += 256) hist[c] = 0;
        __syncthreads();
    }
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o < rows) {
        const long long r = o / out_w, c = o - r * out_w;
        const float* __restrict__ src = frame + (r * step * width + c * step) * row_stride;
        out_pixels[o * 3 + 0] = src[albedo_col + 0];
        out_pixels[o * 3 + 1] = src[albedo_col + 1];
        out_pixels[o * 3 + 2] = src[albedo_col + 2];
        if (label_col >= 0) {
            const long long lab = (long long)src[label_col];             // a float column of exact small integers: truncation
            out_labels[o] = lab;
            if (count && lab >= 0 && lab < n_classes) {
                if (in_lds) atomicAdd(&hist[lab], 1);
                else atomicAdd(&class_counts[lab], 1);
            }
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int c = threadIdx.x; c < n_classes; c += 256)
            if (hist[c]) atomicAdd(&class_counts[c], hist[c]);
    }
}

struct SnapInputs {               // columns of one [n, row_stride] fp32 tensor (a frame's pack)
    const float* albedo;          // 3 floats per pixel
    const float* label;           // 1 float per pixel (exact small integers); unused with ignore_label
    const float* shading;         // 1 float
    const float* residual;        // 3 floats
    long long row_stride;         // floats between consecutive pixels
};

template <int kPixTile>
__global__ __launch_bounds__(256) void k_cluster_snap_compose(SnapInputs in, long long n, ClusterTables t, int ignore_label,
                                                              unsigned char* __restrict__ out_c, unsigned char* __restrict__ out_edit,
                                                              float* __restrict__ out_color) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long p = tile * kPixTile + lane;
    if (tile * kPixTile >= n) return;                       // whole wave
    const bool pixel_lane = lane < kPixTile && p < n;

    float r = 0.f, g = 0.f, b = 0.f;
    int cls = -1;
    if (pixel_lane) {
        const float* __restrict__ a = in.albedo + p * in.row_stride;
        r = a[0]; g = a[1]; b = a[2];
        const long long lab = ignore_label ? 0 : (long long)in.label[p * in.row_stride];
        cls = cluster_class(t, lab);
    }
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, sb = 0.f;
    if (cls >= 0) map_color(r, g, b, t.factor[cls], d0, d1, d2, sb);
    const int winner = nearest_anchor<kPixTile>(t, cls, lane, d0, d1, d2, sb);

    // pixel lanes: the clustered colour, then its two 8-bit pixels packed as 0x00c2c1c0
    unsigned pc = 0u, pe = 0u;
    if (pixel_lane) {
        float s[3] = {r, g, b};                             // no cluster for this label: colour unchanged
        if (cls >= 0) {
            const int link = t.links[t.anchor_begin[cls] + winner];
            const float* ctr = t.centers + 3ll * (t.center_begin[cls] + link);
            s[0] = ctr[0]; s[1] = ctr[1]; s[2] = ctr[2];
        }
        if (out_color) { out_color[p * 3 + 0] = s[0]; out_color[p * 3 + 1] = s[1]; out_color[p * 3 + 2] = s[2]; }
        const float sh = in.shading[p * in.row_stride];
        const float* __restrict__ res = in.residual + p * in.row_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pc |= to_u8(s[k]) << (8 * k);
            pe |= to_u8(__fadd_rn(__fmul_rn(s[k], sh), res[k])) << (8 * k);
        }
    }

    if (kPixTile == 8 && (tile + 1) * 8 <= n) {
        // A whole tile is 24 consecutive bytes of each image, 8-byte aligned: six dwords.  Lanes 0-5 assemble out_c's,
        // lanes 8-13 out_edit's: dword d holds bytes 4d .. 4d+3 of the tile, i.e. the tail of pixel 4d/3 and the head of
        // the next - ONE store instruction for both images instead of six byte stores per pixel lane.
        const int d = lane & 7;
        const int p0 = (4 * d) / 3;
        const unsigned c_lo = __shfl(pc, p0 & 7), c_hi = __shfl(pc, (p0 + 1) & 7);
        const unsigned e_lo = __shfl(pe, p0 & 7), e_hi = __shfl(pe, (p0 + 1) & 7);
        const bool edit = lane >= 8;
        const unsigned long long both = (unsigned long long)(edit ? e_lo : c_lo) | ((unsigned long long)(edit ? e_hi : c_hi) << 24);
        const unsigned word = (unsigned)(both >> (8 * (4 * d - 3 * p0)));
        if (lane < 16 && d < 6) reinterpret_cast<unsigned*>(edit ? out_edit : out_c)[tile * 6 + d] = word;
    } else {
        // the one-pixel tile (3 bytes per image) and the last, partial tile of a frame: byte stores, one instruction -
        // lane 3j + k writes channel k of pixel j, lanes 0-23 to out_c and lanes 32-55 to out_edit
        const int q = lane & 31, j = q / 3, k = q - 3 * j;
        const unsigned c_px = __shfl(pc, j & 7), e_px = __shfl(pe, j & 7);
        const bool edit = lane >= 32;
        if (j < kPixTile && tile * kPixTile + j < n)
            (edit ? out_edit : out_c)[(tile * kPixTile + j) * 3 + k] = (unsigned char)(((edit ? e_px : c_px) >> (8 * k)) & 0xffu);
    }
}

}  // namespace inerf

extern "C" int inerf_frame_subsample(const float* frame, int64_t row_stride, int albedo_col, int label_col, int height, int width,
                                     int step, float* out_pixels, int64_t* out_labels, int32_t* class_counts, int n_classes,
                                     void* stream) {
    using namespace inerf;
    if (height < 0 || width < 0 || step < 1) return INERF_E_INVALID;
    if (height == 0 || width == 0) return INERF_OK;
    const bool labelled = label_col >= 0;
    if (!frame || !out_pixels || albedo_col < 0 || row_stride < (int64_t)albedo_col + 3 || (labelled && row_stride <= label_col) ||
        (labelled && !out_labels) || (labelled && class_counts && n_classes < 1))
        return INERF_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(frame) & 3) != 0 || (reinterpret_cast<uintptr_t>(out_pixels) & 3) != 0 ||
        (labelled && (reinterpret_cast<uintptr_t>(out_labels) & 7) != 0) || (labelled && (reinterpret_cast<uintptr_t>(class_counts) & 3) != 0))
        return INERF_E_INVALID;
    const long long out_h = ((long long)height + step - 1) / step, out_w = ((long long)width + step - 1) / step;
    const long long rows = out_h * out_w;
    const long long blocks = (rows + 255) / 256;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_frame_subsample, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frame, (long long)row_stride,
                       albedo_col, label_col, width, step, (int)out_w, rows, out_pixels, reinterpret_cast<long long*>(out_labels),
                       labelled ? class_counts : nullptr, n_classes);
    return record(hipGetLastError());
}

extern "C" int inerf_cluster_snap_compose(const float* albedo, const float* label, const float* shading, const float* residual,
                                          int64_t row_stride, int64_t n_pixels, const float* anchors, const int32_t* links,
                                          const int32_t* anchor_begin, const float* factor, const float* centers,
                                          const int32_t* center_begin, int n_classes, uint32_t flags, unsigned char* out_c,
                                          unsigned char* out_edit, float* out_color, void* stream) {
    using namespace inerf;
    if (n_pixels == 0) return INERF_OK;
    const bool ignore_label = (flags & INERF_CLUSTER_IGNORE_LABEL) != 0;
    if (n_pixels < 0 || row_stride < 3 || !albedo || (!label && !ignore_label) || !shading || !residual || !anchors || !links ||
        !anchor_begin || !factor || !centers || !center_begin || n_classes < 1 || !out_c || !out_edit)
        return INERF_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(anchors) & 15) != 0) return INERF_E_INVALID;      // float4 loads
    const uintptr_t floats = reinterpret_cast<uintptr_t>(albedo) | reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(shading) |
                             reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(out_color);
    if ((floats & 3) != 0) return INERF_E_INVALID;
    if (((reinterpret_cast<uintptr_t>(out_c) | reinterpret_cast<uintptr_t>(out_edit)) & 3) != 0) return INERF_E_INVALID;   // dword stores of whole tiles
    const bool small = n_pixels <= kSmallBatch;
    const int tile = small ? kBatchTile : kFrameTile;
    const long long tiles = (n_pixels + tile - 1) / tile;
    const long long blocks = (tiles + 3) / 4;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    ClusterTables t{reinterpret_cast<const float4*>(anchors), links, anchor_begin, factor, centers, center_begin, n_classes};
    SnapInputs in{albedo, label, shading, residual, (long long)row_stride};
    auto kernel = small ? k_cluster_snap_compose<kBatchTile> : k_cluster_snap_compose<kFrameTile>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, (long long)n_pixels, t,
                       ignore_label ? 1 : 0, out_c, out_edit, out_color);
    return record(hipGetLastError());
}
