// batch.hip - the first part of a training iteration: from a pixel draw to the finished batch, one thread per selected pixel.
//   k_batch_object : object_level/run_nerf.py:886-938 (img_i, get_rays, coords, select_inds, select_neighbor, the gathers)
//                    -> batch_rays [2, 2N, 3], target_s [2N, 3], target_m [2N, 1]
//   k_batch_ssr    : SSR/training/trainer.py:627-691 with no_batching=True + sampling_index (SSR/models/rays.py:153-172)
//                    -> sampled_rays [2n, 11], gt_rgb [2n, 3], gt_depth [2n], gt_semantic [2n] int64, mask_ids[image]
// The 2N rows are the N selected pixels followed by their N neighbours.  Contract: include/inerf.h (inerf_batch_assemble).
//
// Indices come from the caller (device arrays, the reference's draw order) or are drawn here from (seed, step, ray) with 32-bit
// integer hashing only - tests/_batch_draw.py restates every function of the "draw" section below in NumPy, bit for bit:
//   mix32        the 32-bit finaliser  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
//   step_key     seed (64 bit) and step (64 bit) absorbed 32 bits at a time, one mix32 each
//   stream_key   one key per use: 0 image, 1 / 2 the two offsets in the reference's draw order, 3 the SSR pixels, 4.. the rounds
//   draw         mix32(stream key ^ mix32(ray + golden ratio)): one word per (stream, ray)
//   perm         kRounds alternating Feistel rounds on b = a + c bits (a = b / 2 left, c = b - a right; unbalanced for odd b):
//                  even round  L ^= (mix32(R ^ key) >> 16) & (2^a - 1)        odd round  R ^= (mix32(L ^ key) >> 16) & (2^c - 1)
//                each round is an involution of the b-bit domain, so perm is a bijection of [0, 2^b); with 2^(b-1) < M <= 2^b more than
//                half of the domain is in range, and walking x -> perm(x) from an in-range start until it is in range again is a
//                bijection of [0, M).  The walk stops after INERF_BATCH_MAX_WALK applications whatever the data ("Training batches").
//
// Rays are computed from the pose with k_gen_rays' operations in k_gen_rays' order (frame_ops.hip; restated here because that file
// is the frozen producer of the golden ray tables): one subtraction, one true division, three products and two additions left to
// right without fma, |d| with the two fmas torch.norm's vectorised kernel contracts.  Built with -ffp-contract=off.
//
// Stores: every output is a run of consecutive rows per half (selected | neighbours) and workgroup, so rows of 3 and 11 floats are
// staged in LDS and written one element per lane, consecutive lanes to consecutive addresses; one-element rows go out directly.
// Only 4- and 8-byte per-lane stores (no 12- or 16-byte ones).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout.h"

namespace inerf {

int record(hipError_t e);

namespace {

constexpr int kThreads = 256;
constexpr int kRounds = 8;
constexpr int kMaxWalk = INERF_BATCH_MAX_WALK;

static_assert(sizeof(inerf_batch_args) == 288, "_capi.BatchArgs mirrors this layout");

struct BatchParams {
    inerf_batch_args a;
    unsigned m;            // pixels of the window (OBJECT) / of the frame (SSR)
    int bits_l, bits_r;    // Feistel halves: bits_l + bits_r = smallest b with 2^b >= m
};

// ---------------------------------------------------------------- draw (restated in tests/_batch_draw.py)
__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ unsigned step_key(unsigned long long seed, long long step) {
    unsigned h = mix32((unsigned)seed + 0x9e3779b9U);
    h = mix32(h ^ (unsigned)(seed >> 32));
    h = mix32(h ^ (unsigned)(unsigned long long)step);
    h = mix32(h ^ (unsigned)((unsigned long long)step >> 32));
    return h;
}

__device__ __forceinline__ unsigned stream_key(unsigned k0, unsigned stream) { return mix32(k0 + 0x85ebca6bU * (stream + 1u)); }

__device__ __forceinline__ unsigned draw(unsigned key, unsigned ray) { return mix32(key ^ mix32(ray + 0x9e3779b9U)); }

// uniform on {0 .. n-1} up to n / 2^32: the high word of the 64-bit product
__device__ __forceinline__ unsigned below(unsigned word, unsigned n) { return (unsigned)(((unsigned long long)word * n) >> 32); }

__device__ __forceinline__ unsigned perm_once(unsigned x, int bits_l, int bits_r, const unsigned (&key)[kRounds]) {
    const unsigned mask_l = (1u << bits_l) - 1u, mask_r = (1u << bits_r) - 1u;       // halves hold at most 16 bits
    unsigned l = x >> bits_r, r = x & mask_r;
#pragma unroll
    for (int i = 0; i < kRounds; ++i) {
        if ((i & 1) == 0) l ^= (mix32(r ^ key[i]) >> 16) & mask_l;
        else              r ^= (mix32(l ^ key[i]) >> 16) & mask_r;
    }
    return (l << bits_r) | r;
}

// perm(k) on [0, m): cycle walk with a compile-time bound; `walked` is set when the bound was reached
__device__ __forceinline__ unsigned perm(unsigned k, unsigned m, int bits_l, int bits_r, unsigned k0, bool& walked) {
    unsigned key[kRounds];
#pragma unroll
    for (int i = 0; i < kRounds; ++i) key[i] = stream_key(k0, 4u + i);
    unsigned x = k;
    for (int it = 0; it < kMaxWalk; ++it) {
        x = perm_once(x, bits_l, bits_r, key);
        if (x < m) return x;
    }
    walked = true;
    return x % m;
}

// ---------------------------------------------------------------- selection shared by both forms
struct Pick {
    int img, row, col, nrow, ncol;
    long long q, off_row, off_col;
    int status;
};

template <bool kSsr>
__device__ __forceinline__ Pick pick(const BatchParams& p, long long t) {
    const inerf_batch_args& a = p.a;
    Pick s;
    s.status = 0;
    long long img;
    if (a.flags & INERF_BATCH_DRAW) {
        const long long step = a.step_dev ? *a.step_dev : a.step;
        const unsigned k0 = step_key(a.seed, step);
        const unsigned j = below(draw(stream_key(k0, 0u), 0u), (unsigned)(a.image_ids ? a.n_image_ids : a.n_images));
        img = a.image_ids ? a.image_ids[j] : (long long)j;
        const int first = (int)below(draw(stream_key(k0, 1u), (unsigned)t), 3u) - 1;       // the offset the reference draws first
        const int second = (int)below(draw(stream_key(k0, 2u), (unsigned)t), 3u) - 1;
        if (kSsr) {                                   // rays.py:161-162: bias_w, then bias_h; pixels with replacement
            s.off_col = first; s.off_row = second;
            s.q = draw(stream_key(k0, 3u), (unsigned)t) % p.m;
        } else {                                      // run_nerf.py:920-921: bias_x (row), then bias_y (column); distinct pixels
            s.off_row = first; s.off_col = second;
            bool walked = false;
            s.q = perm((unsigned)t, p.m, p.bits_l, p.bits_r, k0, walked);
            if (walked) s.status |= INERF_BATCH_STATUS_WALK;
        }
    } else {
        img = a.image_index ? *a.image_index : (long long)a.image_host;
        s.q = a.pixels[t];
        s.off_row = a.off_row[t];
        s.off_col = a.off_col[t];
        if (s.q < 0 || s.q >= (long long)p.m) { s.q = s.q < 0 ? 0 : (long long)p.m - 1; s.status |= INERF_BATCH_STATUS_INDEX; }
        if (s.off_row < -1 || s.off_row > 1) { s.off_row = s.off_row < 0 ? -1 : 1; s.status |= INERF_BATCH_STATUS_INDEX; }
        if (s.off_col < -1 || s.off_col > 1) { s.off_col = s.off_col < 0 ? -1 : 1; s.status |= INERF_BATCH_STATUS_INDEX; }
    }
    if (img < 0 || img >= a.n_images) { img = img < 0 ? 0 : a.n_images - 1; s.status |= INERF_BATCH_STATUS_INDEX; }
    s.img = (int)img;
    const int q = (int)s.q;
    if (kSsr) { s.row = q / a.width; s.col = q - s.row * a.width; }
    else      { const int r = q / a.win_w; s.row = a.row0 + r; s.col = a.col0 + (q - r * a.win_w); }
    int nr = s.row + (int)s.off_row, nc = s.col + (int)s.off_col;
    s.nrow = nr < 0 ? 0 : (nr > a.height - 1 ? a.height - 1 : nr);                         // clamped to the image, not the window
    s.ncol = nc < 0 ? 0 : (nc > a.width - 1 ? a.width - 1 : nc);
    return s;
}

// ---------------------------------------------------------------- rays (k_gen_rays' arithmetic, frame_ops.hip)
__device__ __forceinline__ void rotate(const float* __restrict__ p, float x, float y, float z, float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
        d[k] = __fadd_rn(__fadd_rn(__fmul_rn(x, p[4 * k + 0]), __fmul_rn(y, p[4 * k + 1])), __fmul_rn(z, p[4 * k + 2]));
}

__device__ __forceinline__ void pixel_dir(const inerf_batch_args& a, const float* __restrict__ cam, int row, int col, float (&d)[3]) {
    const float x = __fdiv_rn(__fsub_rn((float)col, a.cx), a.fx);
    float y = __fdiv_rn(__fsub_rn((float)row, a.cy), a.fy);
    float z = 1.0f;
    if (a.flags & INERF_BATCH_OPENGL) { y = -y; z = -1.0f; }
    rotate(cam, x, y, z, d);
}

// one element of `bytes` bytes (4 or 8) moved as raw bits
__device__ __forceinline__ unsigned long long load_bits(const void* base, size_t index, int bytes) {
    return bytes == 8 ? reinterpret_cast<const unsigned long long*>(base)[index] : (unsigned long long)reinterpret_cast<const unsigned*>(base)[index];
}

__device__ __forceinline__ void store_bits(void* base, size_t index, int bytes, unsigned long long v) {
    if (bytes == 8) reinterpret_cast<unsigned long long*>(base)[index] = v;
    else reinterpret_cast<unsigned*>(base)[index] = (unsigned)v;
}

__device__ __forceinline__ void store_indices(const inerf_batch_args& a, long long t, const Pick& s) {
    if (a.out_pixels) a.out_pixels[t] = s.q;
    if (a.out_off_row) a.out_off_row[t] = s.off_row;
    if (a.out_off_col) a.out_off_col[t] = s.off_col;
    if (t == 0 && a.out_image) a.out_image[0] = s.img;
    if (s.status && a.status) atomicOr(a.status, s.status);
}

// ---------------------------------------------------------------- object level
__global__ __launch_bounds__(kThreads) void k_batch_object(const BatchParams p) {
    // per half (0 selected, 1 neighbours): origins, directions, colours (3 floats per row) and masks (1)
    __shared__ float st_o[2][kThreads * 3], st_d[2][kThreads * 3], st_s[2][kThreads * 3];
    const inerf_batch_args& a = p.a;
    const long long base = (long long)blockIdx.x * kThreads;
    const long long t = base + threadIdx.x;
    const long long left = a.n - base;
    const int rows = (int)(left < kThreads ? left : kThreads);
    const float* images = reinterpret_cast<const float*>(a.images);
    const float* masks = reinterpret_cast<const float*>(a.aux);
    float* out_s = reinterpret_cast<float*>(a.out_rgb);
    float* out_m = reinterpret_cast<float*>(a.out_aux);
    if (t < a.n) {
        const Pick s = pick<false>(p, t);
        store_indices(a, t, s);
        const float* __restrict__ cam = a.poses + (size_t)s.img * a.pose_stride;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h ? s.nrow : s.row, col = h ? s.ncol : s.col;
            float d[3];
            pixel_dir(a, cam, row, col, d);
            const size_t pix = ((size_t)s.img * a.height + row) * a.width + col;
            float* o = st_o[h] + threadIdx.x * 3;
            float* dd = st_d[h] + threadIdx.x * 3;
            float* c = st_s[h] + threadIdx.x * 3;
            o[0] = cam[3]; o[1] = cam[7]; o[2] = cam[11];
            dd[0] = d[0]; dd[1] = d[1]; dd[2] = d[2];
            c[0] = images[pix * 3 + 0]; c[1] = images[pix * 3 + 1]; c[2] = images[pix * 3 + 2];
            if (masks) out_m[(size_t)h * a.n + t] = masks[pix];                            // one float per row: already coalesced
        }
    }
    __syncthreads();
    const int n_floats = rows * 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const size_t row0 = (size_t)h * a.n + base;
        float* __restrict__ oo = a.out_rays + row0 * 3;                                    // batch_rays[0]
        float* __restrict__ od = a.out_rays + ((size_t)2 * a.n + row0) * 3;                // batch_rays[1]
        float* __restrict__ os = out_s + row0 * 3;
        for (int i = threadIdx.x; i < n_floats; i += kThreads) {
            oo[i] = st_o[h][i];
            od[i] = st_d[h][i];
            os[i] = st_s[h][i];
        }
    }
}

// ---------------------------------------------------------------- SSR
__global__ __launch_bounds__(kThreads) void k_batch_ssr(const BatchParams p) {
    __shared__ float st_r[2][kThreads * INERF_RAY_FLOATS];
    __shared__ unsigned long long st_c[2][kThreads * 3];
    const inerf_batch_args& a = p.a;
    const long long base = (long long)blockIdx.x * kThreads;
    const long long t = base + threadIdx.x;
    const long long left = a.n - base;
    const int rows = (int)(left < kThreads ? left : kThreads);
    const size_t hw = (size_t)a.height * a.width;
    if (t < a.n) {
        const Pick s = pick<true>(p, t);
        store_indices(a, t, s);
        if (t == 0 && a.avail) a.out_avail[0] = a.avail[s.img];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h ? s.nrow : s.row, col = h ? s.ncol : s.col;
            const size_t pix = (size_t)s.img * hw + (size_t)row * a.width + col;
            float* r = st_r[h] + threadIdx.x * INERF_RAY_FLOATS;
            if (a.ray_table) {
                const float* __restrict__ src = a.ray_table + pix * INERF_RAY_FLOATS;
#pragma unroll
                for (int k = 0; k < INERF_RAY_FLOATS; ++k) r[k] = src[k];
            } else {
                const float* __restrict__ cam = a.poses + (size_t)s.img * a.pose_stride;
                float v[3];
                pixel_dir(a, cam, row, col, v);
                // sqrtf, not __fsqrt_rn: ocml's sqrtf carries the correctly-rounding fix-up (frame_ops.hip)
                const float nrm = sqrtf(__fmaf_rn(v[2], v[2], __fmaf_rn(v[1], v[1], __fmul_rn(v[0], v[0]))));
                r[0] = cam[3]; r[1] = cam[7]; r[2] = cam[11];
                r[3] = v[0]; r[4] = v[1]; r[5] = v[2];
                r[6] = a.near; r[7] = a.far;
                r[8] = __fdiv_rn(v[0], nrm); r[9] = __fdiv_rn(v[1], nrm); r[10] = __fdiv_rn(v[2], nrm);
            }
            unsigned long long* c = st_c[h] + threadIdx.x * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = load_bits(a.images, pix * 3 + k, a.image_bytes);
            const size_t out_row = (size_t)h * a.n + t;                                    // one element per row: already coalesced
            if (a.aux) store_bits(a.out_aux, out_row, a.aux_bytes, load_bits(a.aux, pix, a.aux_bytes));
            if (a.semantic) {
                long long label;
                switch (a.semantic_bytes) {
                    case 1: label = reinterpret_cast<const unsigned char*>(a.semantic)[pix]; break;
                    case 2: label = reinterpret_cast<const short*>(a.semantic)[pix]; break;
                    case 4: label = reinterpret_cast<const int*>(a.semantic)[pix]; break;
                    default: label = reinterpret_cast<const long long*>(a.semantic)[pix]; break;
                }
                a.out_semantic[out_row] = label;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const size_t row0 = (size_t)h * a.n + base;
        float* __restrict__ orr = a.out_rays + row0 * INERF_RAY_FLOATS;
        for (int i = threadIdx.x; i < rows * INERF_RAY_FLOATS; i += kThreads) orr[i] = st_r[h][i];
        for (int i = threadIdx.x; i < rows * 3; i += kThreads) store_bits(a.out_rgb, row0 * 3 + i, a.image_bytes, st_c[h][i]);
    }
}

__global__ __launch_bounds__(64) void k_batch_advance(long long* step) {
    if (threadIdx.x == 0) *step = *step + 1;
}

}  // namespace
}  // namespace inerf

extern "C" int inerf_batch_assemble(const inerf_batch_args* args, void* stream) {
    using namespace inerf;
    if (!args) return INERF_E_INVALID;
    const inerf_batch_args& a = *args;
    if ((a.form != INERF_BATCH_OBJECT && a.form != INERF_BATCH_SSR) || a.n < 0) return INERF_E_INVALID;
    if (a.flags & ~(INERF_BATCH_DRAW | INERF_BATCH_ADVANCE | INERF_BATCH_OPENGL)) return INERF_E_INVALID;
    if (a.n == 0) return INERF_OK;
    const bool ssr = a.form == INERF_BATCH_SSR, drawn = (a.flags & INERF_BATCH_DRAW) != 0;
    if (a.n_images <= 0 || a.height <= 0 || a.width <= 0) return INERF_E_INVALID;
    if ((long long)a.height * a.width > 0x7fffffffLL || a.n > 0x7fffffffLL / 2) return INERF_E_UNSUPPORTED;
    if (!a.images || !a.out_rays || !a.out_rgb) return INERF_E_INVALID;
    if (a.image_bytes != 4 && !(ssr && a.image_bytes == 8)) return INERF_E_INVALID;
    if (a.aux && (!a.out_aux || (a.aux_bytes != 4 && !(ssr && a.aux_bytes == 8)))) return INERF_E_INVALID;
    if (ssr) {
        if (!a.ray_table && (!a.poses || a.pose_stride < 12)) return INERF_E_INVALID;
        if (a.semantic && (!a.out_semantic || (a.semantic_bytes != 1 && a.semantic_bytes != 2 && a.semantic_bytes != 4 && a.semantic_bytes != 8)))
            return INERF_E_INVALID;
        if (a.avail && !a.out_avail) return INERF_E_INVALID;
    } else {
        if (!a.poses || a.pose_stride < 12 || a.semantic || a.avail || a.ray_table) return INERF_E_INVALID;
        if (a.row0 < 0 || a.col0 < 0 || a.win_h <= 0 || a.win_w <= 0 || (long long)a.row0 + a.win_h > a.height || (long long)a.col0 + a.win_w > a.width)
            return INERF_E_INVALID;
    }
    BatchParams p;
    p.a = a;
    p.m = ssr ? (unsigned)((long long)a.height * a.width) : (unsigned)((long long)a.win_h * a.win_w);
    if (drawn) {
        if (!ssr && a.n > (long long)p.m) return INERF_E_INVALID;                           // distinct pixels: at most M of them
        if (a.image_ids && a.n_image_ids <= 0) return INERF_E_INVALID;
        if ((a.flags & INERF_BATCH_ADVANCE) && !a.step_dev) return INERF_E_INVALID;
        if ((uintptr_t)a.step_dev & 7u) return INERF_E_INVALID;
    } else {
        if (!a.pixels || !a.off_row || !a.off_col) return INERF_E_INVALID;
        if (!a.image_index && (a.image_host < 0 || a.image_host >= a.n_images)) return INERF_E_INVALID;
        if (a.flags & INERF_BATCH_ADVANCE) return INERF_E_INVALID;
    }
    int bits = 0;
    while ((1ull << bits) < p.m) ++bits;                                                    // smallest b with 2^b >= m (0 for m = 1)
    p.bits_l = bits / 2;
    p.bits_r = bits - p.bits_l;
    const unsigned blocks = (unsigned)((a.n + kThreads - 1) / kThreads);
    if (ssr) hipLaunchKernelGGL(k_batch_ssr, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_batch_object, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
    if (drawn && (a.flags & INERF_BATCH_ADVANCE))
        hipLaunchKernelGGL(k_batch_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<long long*>(a.step_dev));
    return record(hipGetLastError());
}
