// frame_vis.hip - every 8- and 16-bit image a render_path loop writes or returns, made on the device from the packed frame
// (frames.pack_maps: [n, stride] fp32, array-of-structures):
//   inerf_frame_products : up to 16 image planes of one frame in ONE launch - to8b (run_nerf_helpers.py:13 | trainer.py:1242), the
//                          16-bit casts of disparity and depth in mm (trainer.py:1344-1345), the label map's uint8 cast, the
//                          (acc > 10) mask (run_nerf.py:173), the palette gather valid_colour_map[label] (trainer.py:1269, 1294)
//                          and the jet colour map of depth and entropy (imgviz.depth2rgb, trainer.py:1314, 1321)
//   inerf_frame_range    : nanmin / nanmax of one column into a device float[2] - the range of a jet product that colours a map
//                          by its own extent; read by the product kernel, so a frame needs no host synchronisation
// Rules (include/inerf.h has the table).  All fp32, every operation rounded on its own (__fsub_rn, __fmul_rn, __fdiv_rn):
//   (int32)x      truncation toward zero; NaN or |x| >= 2^31 -> 0 (what numpy's float32 -> uint16 / uint8 casts give on x86-64)
//   JET           t = (x - lo) / (hi - lo); NaN -> black; i = min((int)(clamp(t, 0, 1) * 256), 255).  No special case for hi == lo,
//                 +-inf or values outside [lo, hi]: IEEE arithmetic decides (0 / 0 = NaN -> black, +-x / 0 = +-inf -> entry 255 / 0)
// Layout of the work.  A workgroup owns 512 consecutive pixels = 512 * stride consecutive floats of the frame: it copies the
// used columns [0, span) into LDS with consecutive lanes on consecutive floats (16-byte loads when the frame allows it) - every
// column is read from memory once, however many products use it - transposed to [column][pixel] so that a lane's four
// consecutive pixels of a column are one aligned 16-byte LDS read.  Each lane then takes 4 consecutive pixels through all products
// and writes whole dwords: 4 bytes of a grey plane, 8 of a 16-bit plane, 12 of an RGB plane.  The n mod 4 tail pixels are
// written byte by byte.  The jet table sits in LDS as 256 packed words, loaded once per workgroup.  No atomics, no hand-off
// between workgroups; the grid is a function of n alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/inerf.h"
#include "jet_table.h"
#include "to_u8.h"

namespace inerf {

int record(hipError_t e);

constexpr int kVisThreads = 128;                    // two waves; 4 pixels per lane
constexpr int kVisTile = kVisThreads * 4;           // pixels per workgroup
constexpr int kVisLd = kVisTile + 4;                // floats between two columns in LDS: quads stay 16-byte aligned, the staging
                                                    // writes of one wave (a few rows x all columns) spread over the banks
constexpr int kVisMaxSpan = 31;                     // 1 KB of jet words + 31 columns x 516 floats <= 64 KB of LDS
constexpr int kJetBytes = 256 * 4;

__device__ const unsigned d_jet[256] = {INERF_JET256_WORDS};
static const unsigned h_jet[256] = {INERF_JET256_WORDS};

struct VisProduct {
    int kind, column, width;
    float a, b;
    const float* range;
    long long offset;
};

struct VisParams {
    const float* frame;
    long long stride, n;
    int span, n_products, n_colours, vec4;
    const unsigned char* palette;
    unsigned char* out;
    VisProduct p[INERF_FRAME_MAX_PRODUCTS];
};

// (int32)x: truncation toward zero; NaN (fails the comparison) and |x| >= 2^31 give 0
__device__ __forceinline__ int to_i32(float v) { return fabsf(v) < 2147483648.0f ? (int)v : 0; }

// r | g << 8 | b << 16 of one jet pixel
__device__ __forceinline__ unsigned jet_word(const unsigned* __restrict__ s_jet, float x, float lo, float den) {
    const float t = __fdiv_rn(__fsub_rn(x, lo), den);
    if (t != t) return 0u;
    const float c = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    const int i = (int)__fmul_rn(c, 256.0f);
    return s_jet[i > 255 ? 255 : i];
}

__device__ __forceinline__ unsigned palette_word(const unsigned char* __restrict__ palette, int n_colours, float x) {
    if (!(n_colours > 0 && x > -1.0f && x < (float)n_colours)) return 0u;      // NaN, labels < 0 or >= n_colours, an empty palette: black
    const unsigned char* __restrict__ c = palette + 3 * (int)x;      // (int)x in [0, n_colours)
    return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
}

// four grey bytes of pixels p0 .. p0 + 3 (w: pixel j in byte j)
__device__ __forceinline__ void store_grey(unsigned char* __restrict__ plane, long long p0, int cnt, unsigned w) {
    if (cnt == 4) {
        *reinterpret_cast<unsigned*>(plane + p0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < cnt) plane[p0 + j] = (unsigned char)(w >> (8 * j));
    }
}

// four little-endian 16-bit values (lo: pixels 0, 1; hi: pixels 2, 3)
__device__ __forceinline__ void store_u16(unsigned char* __restrict__ plane, long long p0, int cnt, unsigned lo, unsigned hi) {
    if (cnt == 4) {
        *reinterpret_cast<uint2*>(plane + 2 * p0) = make_uint2(lo, hi);
    } else {
        unsigned short* __restrict__ o = reinterpret_cast<unsigned short*>(plane + 2 * p0);
        if (cnt > 0) o[0] = (unsigned short)lo;
        if (cnt > 1) o[1] = (unsigned short)(lo >> 16);
        if (cnt > 2) o[2] = (unsigned short)hi;
    }
}

// four RGB pixels, each w = r | g << 8 | b << 16, as the 12 bytes r0 g0 b0 r1 ... b3
__device__ __forceinline__ void store_rgb(unsigned char* __restrict__ plane, long long p0, int cnt, unsigned w0, unsigned w1, unsigned w2,
                                          unsigned w3) {
    if (cnt == 4) {
        unsigned* __restrict__ o = reinterpret_cast<unsigned*>(plane + 3 * p0);
        o[0] = w0 | w1 << 24;
        o[1] = w1 >> 8 | w2 << 16;
        o[2] = w2 >> 16 | w3 << 8;
    } else {
        unsigned char* __restrict__ o = plane + 3 * p0;
        if (cnt > 0) { o[0] = (unsigned char)w0; o[1] = (unsigned char)(w0 >> 8); o[2] = (unsigned char)(w0 >> 16); }
        if (cnt > 1) { o[3] = (unsigned char)w1; o[4] = (unsigned char)(w1 >> 8); o[5] = (unsigned char)(w1 >> 16); }
        if (cnt > 2) { o[6] = (unsigned char)w2; o[7] = (unsigned char)(w2 >> 8); o[8] = (unsigned char)(w2 >> 16); }
    }
}

__global__ __launch_bounds__(kVisThreads) void k_frame_products(const VisParams a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    unsigned* __restrict__ s_jet = reinterpret_cast<unsigned*>(s_raw);                   // [256]
    float* __restrict__ s_tile = reinterpret_cast<float*>(s_raw + kJetBytes);            // [span][kVisLd]
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kVisTile;
    const long long left = a.n - base;
    const int npix = left < kVisTile ? (int)left : kVisTile;
    const int span = a.span;

    for (int i = tid; i < 256; i += kVisThreads) s_jet[i] = d_jet[i];

    // the tile's rows, columns [0, span): with stride == span they are npix * span consecutive floats
    const float* __restrict__ src = a.frame + base * a.stride;
    int e0 = 0;
    if (a.vec4) {                          // stride == span and a 16-byte aligned frame: a full tile starts on a 16-byte boundary
        const int quads = npix * span / 4;
        for (int q = tid; q < quads; q += kVisThreads) {
            const float4 v = reinterpret_cast<const float4*>(src)[q];
            int r = 4 * q / span, c = 4 * q - r * span;
            const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s_tile[c * kVisLd + r] = x[j];
                if (++c == span) { c = 0; ++r; }
            }
        }
        e0 = quads * 4;
    }
    for (int e = e0 + tid; e < npix * span; e += kVisThreads) {
        const int r = e / span, c = e - r * span;
        s_tile[c * kVisLd + r] = src[(long long)r * a.stride + c];
    }
    __syncthreads();

    const long long p0 = base + 4 * tid;
    if (p0 >= a.n) return;
    const long long rest = a.n - p0;
    const int cnt = rest < 4 ? (int)rest : 4;

    for (int k = 0; k < a.n_products; ++k) {
        const VisProduct& pr = a.p[k];
        unsigned char* __restrict__ plane = a.out + pr.offset;
        const float* __restrict__ col = s_tile + pr.column * kVisLd + 4 * tid;
        const float4 x = *reinterpret_cast<const float4*>(col);
        switch (pr.kind) {
        case INERF_FRAME_TO8B:
            if (pr.width == 1) {
                store_grey(plane, p0, cnt, to_u8(x.x) | to_u8(x.y) << 8 | to_u8(x.z) << 16 | to_u8(x.w) << 24);
            } else {
                const float4 y = *reinterpret_cast<const float4*>(col + kVisLd);
                const float4 z = *reinterpret_cast<const float4*>(col + 2 * kVisLd);
                store_rgb(plane, p0, cnt, to_u8(x.x) | to_u8(y.x) << 8 | to_u8(z.x) << 16, to_u8(x.y) | to_u8(y.y) << 8 | to_u8(z.y) << 16,
                          to_u8(x.z) | to_u8(y.z) << 8 | to_u8(z.z) << 16, to_u8(x.w) | to_u8(y.w) << 8 | to_u8(z.w) << 16);
            }
            break;
        case INERF_FRAME_U16: {
            const unsigned v0 = (unsigned)to_i32(__fmul_rn(x.x, pr.a)) & 0xffffu, v1 = (unsigned)to_i32(__fmul_rn(x.y, pr.a)) & 0xffffu;
            const unsigned v2 = (unsigned)to_i32(__fmul_rn(x.z, pr.a)) & 0xffffu, v3 = (unsigned)to_i32(__fmul_rn(x.w, pr.a)) & 0xffffu;
            store_u16(plane, p0, cnt, v0 | v1 << 16, v2 | v3 << 16);
            break;
        }
        case INERF_FRAME_U8_CAST:
            store_grey(plane, p0, cnt, ((unsigned)to_i32(x.x) & 0xffu) | ((unsigned)to_i32(x.y) & 0xffu) << 8 |
                                           ((unsigned)to_i32(x.z) & 0xffu) << 16 | ((unsigned)to_i32(x.w) & 0xffu) << 24);
            break;
        case INERF_FRAME_THRESH:
            store_grey(plane, p0, cnt, (x.x > pr.a ? 0xffu : 0u) | (x.y > pr.a ? 0xff00u : 0u) | (x.z > pr.a ? 0xff0000u : 0u) |
                                           (x.w > pr.a ? 0xff000000u : 0u));
            break;
        case INERF_FRAME_PALETTE:
            store_rgb(plane, p0, cnt, palette_word(a.palette, a.n_colours, x.x), palette_word(a.palette, a.n_colours, x.y),
                      palette_word(a.palette, a.n_colours, x.z), palette_word(a.palette, a.n_colours, x.w));
            break;
        default: {                          // INERF_FRAME_JET
            float lo = pr.a, hi = pr.b;
            if (pr.range) { lo = pr.range[0]; hi = pr.range[1]; }
            const float den = __fsub_rn(hi, lo);
            store_rgb(plane, p0, cnt, jet_word(s_jet, x.x, lo, den), jet_word(s_jet, x.y, lo, den), jet_word(s_jet, x.z, lo, den),
                      jet_word(s_jet, x.w, lo, den));
        }
        }
    }
}

// ---- nanmin / nanmax of one column -----------------------------------------------------------------------------------------
constexpr int kRangeThreads = 256;
constexpr int kRangeMaxBlocks = 256;     // a 320x240 frame is 300 blocks' worth: anything beyond 65 536 values loops

__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? b : (b != b ? a : (b < a ? b : a)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? b : (b != b ? a : (b > a ? b : a)); }

// (lo, hi) of the workgroup's lanes into lane 0 of wave 0: xor trees inside a wave, then the waves' pairs through LDS
__device__ __forceinline__ void range_reduce(float& lo, float& hi) {
    __shared__ float s_lo[kRangeThreads / 64], s_hi[kRangeThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, off));
        hi = nan_max(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kRangeThreads / 64; ++w) { lo = nan_min(lo, s_lo[w]); hi = nan_max(hi, s_hi[w]); }
    }
}

__global__ __launch_bounds__(kRangeThreads) void k_frame_range(const float* __restrict__ values, long long stride, long long n,
                                                               float* __restrict__ partial) {
    float lo = __builtin_nanf(""), hi = __builtin_nanf("");
    for (long long i = (long long)blockIdx.x * kRangeThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kRangeThreads) {
        const float x = values[i * stride];
        lo = nan_min(lo, x);
        hi = nan_max(hi, x);
    }
    range_reduce(lo, hi);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo; partial[2 * blockIdx.x + 1] = hi; }
}

// the second launch: the workgroups' pairs (and, accumulating, the range so far) into minmax
__global__ __launch_bounds__(kRangeThreads) void k_frame_range_finish(const float* __restrict__ partial, int rows, float* __restrict__ minmax,
                                                                      int accumulate) {
    float lo = __builtin_nanf(""), hi = __builtin_nanf("");
    for (int r = threadIdx.x; r < rows; r += kRangeThreads) {
        lo = nan_min(lo, partial[2 * r]);
        hi = nan_max(hi, partial[2 * r + 1]);
    }
    if (threadIdx.x == 0 && accumulate) { lo = nan_min(lo, minmax[0]); hi = nan_max(hi, minmax[1]); }
    range_reduce(lo, hi);
    if (threadIdx.x == 0) { minmax[0] = lo; minmax[1] = hi; }
}

static long long range_blocks(long long n) {
    const long long b = (n + kRangeThreads - 1) / kRangeThreads;
    return b < kRangeMaxBlocks ? b : kRangeMaxBlocks;
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

static bool overlaps(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

// bytes per pixel of a product's plane; 0: not a product (bad kind or width)
static int plane_bytes_per_pixel(const inerf_frame_product& p) {
    switch (p.kind) {
    case INERF_FRAME_TO8B: return p.width == 1 || p.width == 3 ? p.width : 0;
    case INERF_FRAME_U16: return p.width == 1 ? 2 : 0;
    case INERF_FRAME_U8_CAST:
    case INERF_FRAME_THRESH: return p.width == 1 ? 1 : 0;
    case INERF_FRAME_PALETTE:
    case INERF_FRAME_JET: return p.width == 1 ? 3 : 0;
    default: return 0;
    }
}

// the planes' offsets (each a multiple of 16) into `offsets`, the total byte count returned; negative: an error code
static long long plan_planes(const inerf_frame_products_args* args, long long* offsets) {
    if (!args || args->n < 0 || args->n_products < 0 || args->n_products > INERF_FRAME_MAX_PRODUCTS) return INERF_E_INVALID;
    long long at = 0;
    for (int k = 0; k < args->n_products; ++k) {
        const int bpp = plane_bytes_per_pixel(args->products[k]);
        if (bpp == 0) return INERF_E_INVALID;
        if (args->n > (0x7fffffffffffffffLL - at) / bpp - 16) return INERF_E_UNSUPPORTED;
        offsets[k] = at;
        at += (args->n * bpp + 15) / 16 * 16;
    }
    return at;
}

}  // namespace inerf

extern "C" const unsigned char* inerf_jet_table(void) {
    struct Bytes { unsigned char b[256 * 3]; };
    static const Bytes table = [] {                  // a function-local static: initialised once, also under concurrent first calls
        Bytes t;
        for (int i = 0; i < 256; ++i) {
            t.b[3 * i] = (unsigned char)inerf::h_jet[i];
            t.b[3 * i + 1] = (unsigned char)(inerf::h_jet[i] >> 8);
            t.b[3 * i + 2] = (unsigned char)(inerf::h_jet[i] >> 16);
        }
        return t;
    }();
    return table.b;
}

extern "C" int64_t inerf_frame_products_layout(inerf_frame_products_args* args) {
    long long offsets[INERF_FRAME_MAX_PRODUCTS];
    const long long total = inerf::plan_planes(args, offsets);
    if (total < 0) return total;
    for (int k = 0; k < args->n_products; ++k) args->products[k].offset = offsets[k];
    return total;
}

extern "C" int inerf_frame_products(const inerf_frame_products_args* args, void* stream) {
    using namespace inerf;
    long long offsets[INERF_FRAME_MAX_PRODUCTS];
    const long long total = plan_planes(args, offsets);
    if (total < 0) return (int)total;
    if (args->stride < 1 || args->n_colours < 0) return INERF_E_INVALID;
    int span = 0;
    bool palette = false;
    for (int k = 0; k < args->n_products; ++k) {
        const inerf_frame_product& p = args->products[k];
        if (p.column < 0 || (long long)p.column + p.width > args->stride) return INERF_E_INVALID;
        if (p.offset != offsets[k]) return INERF_E_INVALID;            // inerf_frame_products_layout was not called on these args
        if (p.kind != INERF_FRAME_JET && p.range) return INERF_E_INVALID;
        span = p.column + p.width > span ? p.column + p.width : span;
        palette = palette || p.kind == INERF_FRAME_PALETTE;
    }
    if (args->n == 0 || args->n_products == 0) return INERF_OK;
    if (!args->frame || !args->out || (palette && args->n_colours > 0 && !args->palette) || args->out_bytes < total) return INERF_E_INVALID;
    if (misaligned(args->frame, 4) || misaligned(args->out, 16)) return INERF_E_INVALID;
    if (span > kVisMaxSpan) return INERF_E_UNSUPPORTED;
    const long long blocks = (args->n + kVisTile - 1) / kVisTile;
    if (blocks > 0x7fffffffLL || args->n > 0x7fffffffffffffffLL / 4 / args->stride) return INERF_E_UNSUPPORTED;
    if (overlaps(args->out, total, args->frame, ((args->n - 1) * args->stride + span) * 4)) return INERF_E_INVALID;
    if (palette && args->n_colours > 0 && overlaps(args->out, total, args->palette, 3LL * args->n_colours)) return INERF_E_INVALID;
    for (int k = 0; k < args->n_products; ++k) {
        const float* r = args->products[k].range;
        if (r && (misaligned(r, 4) || overlaps(args->out, total, r, 8))) return INERF_E_INVALID;
    }

    VisParams a{};
    a.frame = args->frame; a.stride = args->stride; a.n = args->n;
    a.span = span; a.n_products = args->n_products; a.n_colours = args->n_colours;
    a.vec4 = args->stride == span && !misaligned(args->frame, 16);
    a.palette = args->palette; a.out = args->out;
    for (int k = 0; k < args->n_products; ++k) {
        const inerf_frame_product& p = args->products[k];
        a.p[k] = VisProduct{p.kind, p.column, p.width, p.a, p.b, p.range, offsets[k]};
    }
    const size_t lds = kJetBytes + sizeof(float) * (size_t)span * kVisLd;
    hipLaunchKernelGGL(k_frame_products, dim3((unsigned)blocks), dim3(kVisThreads), lds, (hipStream_t)stream, a);
    return record(hipGetLastError());
}

extern "C" int64_t inerf_frame_range_workspace_bytes(int64_t n) {
    return n <= 0 ? 0 : (int64_t)(inerf::range_blocks(n) * 2 * sizeof(float));
}

extern "C" int inerf_frame_range(const float* values, int64_t stride, int64_t n, float* minmax, void* workspace, int64_t workspace_bytes,
                                 int accumulate, void* stream) {
    using namespace inerf;
    if (n < 0 || stride < 1) return INERF_E_INVALID;
    if (n == 0) return INERF_OK;
    if (!values || !minmax || misaligned(values, 4) || misaligned(minmax, 4)) return INERF_E_INVALID;
    if (n > 0x7fffffffffffffffLL / 4 / stride) return INERF_E_UNSUPPORTED;
    if (!workspace || misaligned(workspace, 4) || workspace_bytes < inerf_frame_range_workspace_bytes(n)) return INERF_E_WORKSPACE;
    if (overlaps(minmax, 8, values, ((n - 1) * stride + 1) * 4) || overlaps(workspace, inerf_frame_range_workspace_bytes(n), minmax, 8) ||
        overlaps(workspace, inerf_frame_range_workspace_bytes(n), values, ((n - 1) * stride + 1) * 4))
        return INERF_E_INVALID;
    const unsigned blocks = (unsigned)range_blocks(n);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(k_frame_range, dim3(blocks), dim3(kRangeThreads), 0, (hipStream_t)stream, values, (long long)stride, (long long)n, partial);
    const int rc = record(hipGetLastError());
    if (rc != INERF_OK) return rc;
    hipLaunchKernelGGL(k_frame_range_finish, dim3(1), dim3(kRangeThreads), 0, (hipStream_t)stream, partial, (int)blocks, minmax, accumulate ? 1 : 0);
    return record(hipGetLastError());
}
