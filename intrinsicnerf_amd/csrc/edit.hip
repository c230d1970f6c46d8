// edit.hip - the edit engine of the reference's GUI (gui.py | gui_obj.py) on the device: a frame's albedo snapped to its
// cluster centres, the centres recoloured, shading and residual reshaped and rescaled, the frame composed again.
//   k_edit_frame      : search form, for a frame seen for the first time.  k_cluster_snap_compose (refresh.hip) with the
//                       colour read from the EDITED centre table, update_img's compose line (gui.py:163) and the slot of
//                       every pixel - the global row of its centre - as an output (cluster_img, gui.py:268-281)
//   k_edit_recompose  : cached form, for every later tick (update_img, gui.py:155-163).  No search: the slot selects the
//                       centre.  A pure stream - 8 pixels per lane, no LDS - over fp32 pack columns or over the three
//                       8-bit planes the reference loads (gui.py:216-228: u8 / 255)
// Rounding (gui.py:163, torch fp32, left to right): ((c * ts) * gs) + (tr * gr), every product and the sum rounded on its
// own; ts = s or s * s, tr = r or (sin(r * pi - pi / 2) + 1) / 2 with pi and pi / 2 rounded to fp32 first and the accurate
// sinf (r * pi is not confined to [-pi, pi]).  to8b is to_u8.h's.
#include <hip/hip_runtime.h>

#include "cluster_search.h"
#include "layout.h"
#include "to_u8.h"

namespace inerf {

int record(hipError_t e);

struct EditState {                // inerf_edit_params by value
    const float* centers;         // [Ctot,3] the edited centres
    int shading_mode, residual_mode;
    float shading_scale, residual_scale;
};

constexpr float kPi = 3.14159265358979323846f;          // (float)math.pi, (float)(math.pi / 2): torch's scalar casts
constexpr float kHalfPi = 1.57079632679489661923f;

__device__ __forceinline__ float t_shading(float s, int mode) { return mode ? __fmul_rn(s, s) : s; }

__device__ __forceinline__ float t_residual(float r, int mode) {
    return mode ? __fdiv_rn(__fadd_rn(sinf(__fsub_rn(__fmul_rn(r, kPi), kHalfPi)), 1.0f), 2.0f) : r;
}

// one pixel: colour c[3], shading s, residual r[3] -> the float result and the packed 8-bit pixels 0x00c2c1c0
__device__ __forceinline__ void compose(const EditState& e, const float (&c)[3], float s, const float (&r)[3], float (&out)[3],
                                        unsigned& px_c, unsigned& px_result) {
    const float ts = t_shading(s, e.shading_mode);
    px_c = px_result = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = __fadd_rn(__fmul_rn(__fmul_rn(c[k], ts), e.shading_scale), __fmul_rn(t_residual(r[k], e.residual_mode), e.residual_scale));
        px_c |= to_u8(c[k]) << (8 * k);
        px_result |= to_u8(out[k]) << (8 * k);
    }
}

struct EditInputs {               // columns of one [n, row_stride] fp32 tensor (a frame's pack), as refresh.hip's SnapInputs
    const float* albedo;
    const float* label;
    const float* shading;
    const float* residual;
    long long row_stride;
};

template <int kPixTile>
__global__ __launch_bounds__(256) void k_edit_frame(EditInputs in, long long n, ClusterTables t, int ignore_label, EditState e,
                                                    unsigned char* __restrict__ out_result, unsigned char* __restrict__ out_c,
                                                    float* __restrict__ out_f32, int* __restrict__ out_slot) {
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

    unsigned pc = 0u, pe = 0u;
    if (pixel_lane) {
        float c[3] = {r, g, b};                             // no cluster for this label: colour unchanged, slot -1
        int slot = -1;
        if (cls >= 0) {
            slot = t.center_begin[cls] + t.links[t.anchor_begin[cls] + winner];
            const float* ctr = e.centers + 3ll * slot;
            c[0] = ctr[0]; c[1] = ctr[1]; c[2] = ctr[2];
        }
        if (out_slot) out_slot[p] = slot;
        const float sh = in.shading[p * in.row_stride];
        const float* __restrict__ res = in.residual + p * in.row_stride;
        const float rr[3] = {res[0], res[1], res[2]};
        float o[3];
        compose(e, c, sh, rr, o, pc, pe);
        if (out_f32) { out_f32[p * 3 + 0] = o[0]; out_f32[p * 3 + 1] = o[1]; out_f32[p * 3 + 2] = o[2]; }
    }

    // the image stores are k_cluster_snap_compose's: whole tiles as six dwords per image, anything else as bytes
    if (kPixTile == 8 && (tile + 1) * 8 <= n) {
        const int d = lane & 7;
        const int p0 = (4 * d) / 3;
        const unsigned c_lo = __shfl(pc, p0 & 7), c_hi = __shfl(pc, (p0 + 1) & 7);
        const unsigned e_lo = __shfl(pe, p0 & 7), e_hi = __shfl(pe, (p0 + 1) & 7);
        const bool edit = lane >= 8;
        const unsigned long long both = (unsigned long long)(edit ? e_lo : c_lo) | ((unsigned long long)(edit ? e_hi : c_hi) << 24);
        const unsigned word = (unsigned)(both >> (8 * (4 * d - 3 * p0)));
        unsigned char* dst = edit ? out_result : out_c;
        if (lane < 16 && d < 6 && dst) reinterpret_cast<unsigned*>(dst)[tile * 6 + d] = word;
    } else {
        const int q = lane & 31, j = q / 3, k = q - 3 * j;
        const unsigned c_px = __shfl(pc, j & 7), e_px = __shfl(pe, j & 7);
        const bool edit = lane >= 32;
        unsigned char* dst = edit ? out_result : out_c;
        if (j < kPixTile && tile * kPixTile + j < n && dst)
            dst[(tile * kPixTile + j) * 3 + k] = (unsigned char)(((edit ? e_px : c_px) >> (8 * k)) & 0xffu);
    }
}

// ---- cached form ------------------------------------------------------------------------------------------------------------------
constexpr int kGroup = 8;         // pixels per lane of the vector path: 24 bytes of each 8-bit image = six dwords
constexpr int kEdgeMax = 14;      // byte-path pixels of a launch: a head of up to 7 in front of the groups, a tail of up to 7 behind

struct RecomposeInputs {
    const void* albedo;           // fp32: 3 floats per pixel, row_stride apart | u8: [n,3]
    const void* shading;          // fp32: 1 float                              | u8: [n]
    const void* residual;         // fp32: 3 floats                             | u8: [n,3]
    long long row_stride;         // fp32 only
    const int* slot;              // [n] global centre row, -1: the pixel keeps its albedo
};

__device__ __forceinline__ float from_u8(unsigned v) { return __fdiv_rn((float)v, 255.0f); }      // (v / 255.).astype(float32), all 256 values

// kWords dwords starting `shift` bytes into the aligned dword at `base`: one more aligned dword is read only when
// shift != 0, so no load touches a dword that holds none of the wanted bytes
template <int kWords>
__device__ __forceinline__ void load_bytes(const unsigned char* ptr, unsigned (&w)[kWords]) {
    const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(ptr) & 3);
    const unsigned* __restrict__ base = reinterpret_cast<const unsigned*>(ptr - shift);
    unsigned raw[kWords + 1];
#pragma unroll
    for (int i = 0; i < kWords; ++i) raw[i] = base[i];
    raw[kWords] = shift ? base[kWords] : 0u;                // the same for every group of a launch: 4 | 8 and 4 | 24
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], shift);
}

__device__ __forceinline__ unsigned byte_of(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

template <bool kU8>
__device__ __forceinline__ void load_pixel(const RecomposeInputs& in, long long p, float (&a)[3], float& s, float (&r)[3]) {
    if (kU8) {
        const unsigned char* pa = static_cast<const unsigned char*>(in.albedo) + 3 * p;
        const unsigned char* pr = static_cast<const unsigned char*>(in.residual) + 3 * p;
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = from_u8(pa[k]); r[k] = from_u8(pr[k]); }
        s = from_u8(static_cast<const unsigned char*>(in.shading)[p]);
    } else {
        const float* pa = static_cast<const float*>(in.albedo) + p * in.row_stride;
        const float* pr = static_cast<const float*>(in.residual) + p * in.row_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = pa[k]; r[k] = pr[k]; }
        s = static_cast<const float*>(in.shading)[p * in.row_stride];
    }
}

// Thread i < groups owns pixels head + 8 i .. head + 8 i + 7: the vector path.  `head` (host side) makes out_result + 3 * head
// 4-byte aligned, so the 24 result bytes of a group are six aligned dwords; out_c goes the same way when it is aligned there too
// (c_words) and as bytes otherwise; 8-bit sources are read as aligned dwords and shifted into place.  The threads behind take
// one byte-path pixel each: the head, then the tail.
template <bool kU8>
__global__ __launch_bounds__(256) void k_edit_recompose(RecomposeInputs in, long long n, long long head, long long groups, EditState e,
                                                        unsigned char* __restrict__ out_result, unsigned char* __restrict__ out_c,
                                                        int c_words, float* __restrict__ out_f32) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= groups) {
        const long long j = i - groups;                     // byte path
        const long long p = j < head ? j : head + 8 * groups + (j - head);
        if (p >= n) return;
        float c[3], r[3], o[3], s;
        load_pixel<kU8>(in, p, c, s, r);
        const int slot = in.slot[p];
        if (slot >= 0) { c[0] = e.centers[3ll * slot]; c[1] = e.centers[3ll * slot + 1]; c[2] = e.centers[3ll * slot + 2]; }
        unsigned pc, pe;
        compose(e, c, s, r, o, pc, pe);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_result[3 * p + k] = (unsigned char)((pe >> (8 * k)) & 0xffu);
            if (out_c) out_c[3 * p + k] = (unsigned char)((pc >> (8 * k)) & 0xffu);
            if (out_f32) out_f32[3 * p + k] = o[k];
        }
        return;
    }
    const long long p0 = head + kGroup * i;
    float a[kGroup][3], r[kGroup][3], s[kGroup];
    if (kU8) {
        unsigned wa[6], wr[6], ws[2];
        load_bytes<6>(static_cast<const unsigned char*>(in.albedo) + 3 * p0, wa);
        load_bytes<6>(static_cast<const unsigned char*>(in.residual) + 3 * p0, wr);
        load_bytes<2>(static_cast<const unsigned char*>(in.shading) + p0, ws);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            s[j] = from_u8(byte_of(ws, j));
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[j][k] = from_u8(byte_of(wa, 3 * j + k)); r[j][k] = from_u8(byte_of(wr, 3 * j + k)); }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kGroup; ++j) load_pixel<false>(in, p0 + j, a[j], s[j], r[j]);
    }
    int slot[kGroup];
    if ((reinterpret_cast<uintptr_t>(in.slot + p0) & 15) == 0) {            // the same for every group: two dwordx4
        const int4 lo = *reinterpret_cast<const int4*>(in.slot + p0), hi = *reinterpret_cast<const int4*>(in.slot + p0 + 4);
        slot[0] = lo.x; slot[1] = lo.y; slot[2] = lo.z; slot[3] = lo.w; slot[4] = hi.x; slot[5] = hi.y; slot[6] = hi.z; slot[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < kGroup; ++j) slot[j] = in.slot[p0 + j];
    }
    unsigned pc[kGroup], pe[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
        if (slot[j] >= 0) {
            const float* ctr = e.centers + 3ll * slot[j];
            a[j][0] = ctr[0]; a[j][1] = ctr[1]; a[j][2] = ctr[2];
        }
        float o[3];
        compose(e, a[j], s[j], r[j], o, pc[j], pe[j]);
        if (out_f32) { out_f32[3 * (p0 + j) + 0] = o[0]; out_f32[3 * (p0 + j) + 1] = o[1]; out_f32[3 * (p0 + j) + 2] = o[2]; }
    }
    // 8 pixels of 0x00c2c1c0 -> six dwords: dword d holds bytes 4d .. 4d+3 of the group, the tail of pixel 4d/3 and the head of the next
    unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(out_result + 3 * p0);
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const int q = (4 * d) / 3, sh = 8 * (4 * d - 3 * q);
        dst[d] = (unsigned)(((unsigned long long)pe[q] | ((unsigned long long)pe[(q + 1) & 7] << 24)) >> sh);
    }
    if (out_c && c_words) {
        unsigned* __restrict__ dc = reinterpret_cast<unsigned*>(out_c + 3 * p0);
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const int q = (4 * d) / 3, sh = 8 * (4 * d - 3 * q);
            dc[d] = (unsigned)(((unsigned long long)pc[q] | ((unsigned long long)pc[(q + 1) & 7] << 24)) >> sh);
        }
    } else if (out_c) {
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) out_c[3 * (p0 + j) + k] = (unsigned char)((pc[j] >> (8 * k)) & 0xffu);
    }
}

static bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

static bool bad_params(const inerf_edit_params* params) {
    return !params || !params->edit_centers || misaligned4(params->edit_centers) || (params->shading_mode != 0 && params->shading_mode != 1) ||
           (params->residual_mode != 0 && params->residual_mode != 1);
}

template <bool kU8>
static int launch_recompose(const void* albedo, const void* shading, const void* residual, int64_t row_stride, const int32_t* slot,
                            int64_t n_pixels, const inerf_edit_params* params, unsigned char* out_result, unsigned char* out_c,
                            float* out_result_f32, void* stream) {
    if (n_pixels == 0) return INERF_OK;
    if (n_pixels < 0 || !albedo || !shading || !residual || !slot || !out_result || bad_params(params) || (!kU8 && row_stride < 3))
        return INERF_E_INVALID;
    if (misaligned4(slot) || misaligned4(out_result_f32) || (!kU8 && (misaligned4(albedo) || misaligned4(shading) || misaligned4(residual))))
        return INERF_E_INVALID;
    // 3 h = -out_result (mod 4)  <=>  h = out_result (mod 4)
    long long head = (long long)(reinterpret_cast<uintptr_t>(out_result) & 3);
    if (head > n_pixels) head = n_pixels;
    const long long groups = (n_pixels - head) / kGroup;
    const long long threads = groups + kEdgeMax;
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    RecomposeInputs in{albedo, shading, residual, (long long)row_stride, slot};
    EditState e{params->edit_centers, params->shading_mode, params->residual_mode, params->shading_scale, params->residual_scale};
    const int c_words = out_c && ((reinterpret_cast<uintptr_t>(out_c) + 3 * (uintptr_t)head) & 3) == 0;
    hipLaunchKernelGGL(k_edit_recompose<kU8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, (long long)n_pixels, head, groups, e,
                       out_result, out_c, c_words, out_result_f32);
    return record(hipGetLastError());
}

}  // namespace inerf

extern "C" int inerf_edit_frame(const float* albedo, const float* label, const float* shading, const float* residual, int64_t row_stride,
                                int64_t n_pixels, const float* anchors, const int32_t* links, const int32_t* anchor_begin,
                                const float* factor, const int32_t* center_begin, int n_classes, uint32_t flags,
                                const inerf_edit_params* params, unsigned char* out_result, unsigned char* out_c, float* out_result_f32,
                                int32_t* out_slot, void* stream) {
    using namespace inerf;
    if (n_pixels == 0) return INERF_OK;
    const bool ignore_label = (flags & INERF_CLUSTER_IGNORE_LABEL) != 0;
    if (n_pixels < 0 || row_stride < 3 || !albedo || (!label && !ignore_label) || !shading || !residual || !anchors || !links ||
        !anchor_begin || !factor || !center_begin || n_classes < 1 || !out_result || bad_params(params))
        return INERF_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(anchors) & 15) != 0) return INERF_E_INVALID;      // float4 loads
    if (misaligned4(albedo) || misaligned4(label) || misaligned4(shading) || misaligned4(residual) || misaligned4(out_result_f32) ||
        misaligned4(out_slot) || misaligned4(out_result) || misaligned4(out_c))         // the images: dword stores of whole tiles
        return INERF_E_INVALID;
    const bool small = n_pixels <= kSmallBatch;
    const int tile = small ? kBatchTile : kFrameTile;
    const long long tiles = (n_pixels + tile - 1) / tile;
    const long long blocks = (tiles + 3) / 4;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    ClusterTables t{reinterpret_cast<const float4*>(anchors), links, anchor_begin, factor, params->edit_centers, center_begin, n_classes};
    EditInputs in{albedo, label, shading, residual, (long long)row_stride};
    EditState e{params->edit_centers, params->shading_mode, params->residual_mode, params->shading_scale, params->residual_scale};
    auto kernel = small ? k_edit_frame<kBatchTile> : k_edit_frame<kFrameTile>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, (long long)n_pixels, t, ignore_label ? 1 : 0, e,
                       out_result, out_c, out_result_f32, out_slot);
    return record(hipGetLastError());
}

extern "C" int inerf_edit_recompose(const float* albedo, const float* shading, const float* residual, int64_t row_stride, const int32_t* slot,
                                    int64_t n_pixels, const inerf_edit_params* params, unsigned char* out_result, unsigned char* out_c,
                                    float* out_result_f32, void* stream) {
    return inerf::launch_recompose<false>(albedo, shading, residual, row_stride, slot, n_pixels, params, out_result, out_c, out_result_f32, stream);
}

extern "C" int inerf_edit_recompose_u8(const unsigned char* albedo, const unsigned char* shading, const unsigned char* residual,
                                       const int32_t* slot, int64_t n_pixels, const inerf_edit_params* params, unsigned char* out_result,
                                       unsigned char* out_c, float* out_result_f32, void* stream) {
    return inerf::launch_recompose<true>(albedo, shading, residual, 0, slot, n_pixels, params, out_result, out_c, out_result_f32, stream);
}
