// imq.hip - intrinsic-image quality metrics on the device (definitions: include/inerf.h, inerf_image_quality):
//   the moments behind mse / psnr / si-MSE, the windowed LMSE of Grosse et al. and the Gaussian-window SSIM of Wang et al. of a
//   stack of [H, W, C] image pairs, as seven fp64 sums and three int64 counts per image.  Four launches on one stream:
//     k_imq_moments : every pixel once.  The image is cut into s x s cells (s = window_shift, edge cells clipped); L = min(64,
//                     pow2ceil(s s)) consecutive lanes walk one cell, a wave takes 64 / L cells per step.  Each cell's (Spp, Spg,
//                     Sgg) over its valid pixels goes to `workspace` after log2 L xor-shuffles; the lanes' own running sums of the
//                     same three, of (g - p)^2 and of the valid count are the image's whole-frame moments.
//     k_imq_windows : every cell (k / s)^2 times, every pixel never.  One thread per k x k window adds its cells' moments in
//                     row-major order, takes the window's scale a_w and adds Sgg - 2 a_w Spg + a_w^2 Spp and Sgg to its sums.
//     k_imq_ssim    : every pixel once per tile that needs it.  A workgroup owns a kTileX x kTileY patch of the valid region per
//                     trip and channel: the (kTileY + 10) x (kTileX + 10) fp32 inputs with their halo go to LDS, the horizontal
//                     11-tap pass writes the five filtered rows (x, y, x^2, y^2, xy) to LDS as fp64, the vertical pass reads them
//                     back column-wise and forms the SSIM value of each position whose centre pixel is valid.
//     k_imq_finish  : one workgroup per image adds the three stages' partial rows in index order and WRITES sums and counts.
// Arithmetic.  fp64 from fp32 inputs throughout: sigma^2 = E[x^2] - mu^2 cancels to ~1e-16 of a value near 1 and is divided by
// C2 = 9e-4; in fp32 the same cancellation would leave 1e-4 of SSIM.  The taps come from the host as 11 doubles.
// LDS (k_imq_ssim).  Inputs: 2 x 26 x 42 floats = 8.5 KiB, lanes of a half-wave read 32 consecutive floats (ds_read_b32, 32
// banks: conflict-free).  Filtered rows: 5 x 26 x 32 doubles = 32.5 KiB, a half-wave writes and reads 32 consecutive doubles
// (ds_read_b64, 64 banks: conflict-free).  41 KiB per workgroup: three workgroups, twelve waves per CU.
// Determinism.  As eval.hip: no floating-point atomic, lane -> wave -> workgroup through fixed trees into one plain-stored row
// per workgroup, rows added in index order by the last launch; no kernel waits on another workgroup; every grid is a function of
// the shapes alone (capped at kImqMaxBlocks per image and stage, workgroups loop beyond); nothing is allocated or synchronised.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/inerf.h"

namespace inerf {

int record(hipError_t e);

namespace {

constexpr int kImqThreads = 256;
constexpr int kImqWaves = kImqThreads / 64;
constexpr int kImqMaxBlocks = 256;      // per image and stage: one row of partials each, all of them staged in the finish kernel's LDS
constexpr int kTileX = 32, kTileY = 16; // SSIM positions per workgroup trip
constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kInW = kTileX + kHalo, kInH = kTileY + kHalo;
constexpr int kRowA = 5, kRowB = 2, kRowC = 2;      // 8-byte slots per partial row of the three stages

struct ImqView {
    const float* p;
    long long pixel_stride, image_stride;
};

struct ImqArgs {
    int H, W;
    ImqView pred, trgt, mask;
    int k, s, r;                        // window size, shift, cells per window side
    int lanes_per_cell;
    int cells_x, cells_y;
    int win_x, win_y;
    int tiles_x, tiles_y;
    int blocks_a, blocks_b, blocks_c;
    long long image_slots;              // 8-byte slots of workspace per image
    double taps[kTaps];
    double c1, c2;
    double* workspace;
    double* sums;
    long long* counts;
};

// one image's workspace: [blocks_a, kRowA] | cells [cells_y * cells_x, 3] | [blocks_b, kRowB] | [blocks_c, kRowC]
__device__ __forceinline__ double* ws_rows_a(const ImqArgs& a, int img) { return a.workspace + (long long)img * a.image_slots; }
__device__ __forceinline__ double* ws_cells(const ImqArgs& a, int img) { return ws_rows_a(a, img) + (long long)a.blocks_a * kRowA; }
__device__ __forceinline__ double* ws_rows_b(const ImqArgs& a, int img) { return ws_cells(a, img) + (long long)a.cells_x * a.cells_y * 3; }
__device__ __forceinline__ double* ws_rows_c(const ImqArgs& a, int img) { return ws_rows_b(a, img) + (long long)a.blocks_b * kRowB; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ bool pixel_valid(const ImqView& m, int img, long long pix) {
    return !m.p || m.p[(long long)img * m.image_stride + pix * m.pixel_stride] > 0.f;      // NaN: invalid
}

template <int C>
__global__ __launch_bounds__(kImqThreads) void k_imq_moments(ImqArgs a) {
    __shared__ double s_part[kImqWaves][kRowA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, img = blockIdx.y;
    const int L = a.lanes_per_cell, per_wave = 64 / L, sub = lane / L, l = lane % L;
    const long long n_cells = (long long)a.cells_x * a.cells_y;
    const float* __restrict__ pred = a.pred.p + (long long)img * a.pred.image_stride;
    const float* __restrict__ trgt = a.trgt.p + (long long)img * a.trgt.image_stride;
    double* __restrict__ cells = ws_cells(a, img);

    double tot[4] = {0.0, 0.0, 0.0, 0.0};      // Spp, Spg, Sgg, S(g-p)^2 of this lane
    long long n_valid = 0;
    for (long long base = ((long long)blockIdx.x * kImqWaves + wave) * per_wave; base < n_cells; base += (long long)gridDim.x * kImqWaves * per_wave) {
        const long long cell = base + sub;
        const bool live = cell < n_cells;
        double m[3] = {0.0, 0.0, 0.0};
        if (live) {
            const int y0 = (int)(cell / a.cells_x) * a.s, x0 = (int)(cell % a.cells_x) * a.s;
            const int h = min(a.s, a.H - y0), w = min(a.s, a.W - x0);
            for (int i = l; i < h * w; i += L) {
                const long long pix = (long long)(y0 + i / w) * a.W + (x0 + i % w);
                if (!pixel_valid(a.mask, img, pix)) continue;
                ++n_valid;
                const float* __restrict__ pp = pred + pix * a.pred.pixel_stride;
                const float* __restrict__ gg = trgt + pix * a.trgt.pixel_stride;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double p = (double)pp[c], g = (double)gg[c], d = g - p;
                    m[0] += p * p;
                    m[1] += p * g;
                    m[2] += g * g;
                    tot[3] += d * d;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            tot[q] += m[q];
            for (int off = L >> 1; off > 0; off >>= 1) m[q] += __shfl_xor(m[q], off);      // (the loop above is left wave-uniformly)
        }
        if (live && l == 0) {
            cells[cell * 3 + 0] = m[0];
            cells[cell * 3 + 1] = m[1];
            cells[cell * 3 + 2] = m[2];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double v = wave_sum(tot[q]);
        if (lane == 0) s_part[wave][q] = v;
    }
    long long nv = n_valid;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off);
    if (lane == 0) s_part[wave][4] = __longlong_as_double(nv);
    __syncthreads();
    double* __restrict__ row = ws_rows_a(a, img) + (long long)blockIdx.x * kRowA;
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        row[q] = ((s_part[0][q] + s_part[1][q]) + s_part[2][q]) + s_part[3][q];
    } else if (threadIdx.x == 4) {
        long long t = 0;
        for (int wv = 0; wv < kImqWaves; ++wv) t += __double_as_longlong(s_part[wv][4]);
        row[4] = __longlong_as_double(t);
    }
}

__global__ __launch_bounds__(kImqThreads) void k_imq_windows(ImqArgs a) {
    __shared__ double s_part[kImqWaves][kRowB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, img = blockIdx.y;
    const long long n_win = (long long)a.win_x * a.win_y;
    const double* __restrict__ cells = ws_cells(a, img);
    double num = 0.0, den = 0.0;
    for (long long wi = (long long)blockIdx.x * kImqThreads + threadIdx.x; wi < n_win; wi += (long long)gridDim.x * kImqThreads) {
        const int wy = (int)(wi / a.win_x), wx = (int)(wi % a.win_x);      // window origin (wy s, wx s) = cell (wy, wx)
        double spp = 0.0, spg = 0.0, sgg = 0.0;
        for (int cy = 0; cy < a.r; ++cy)
            for (int cx = 0; cx < a.r; ++cx) {
                const double* __restrict__ m = cells + ((long long)(wy + cy) * a.cells_x + (wx + cx)) * 3;
                spp += m[0];
                spg += m[1];
                sgg += m[2];
            }
        const double alpha = spp > 1e-5 ? spg / spp : 0.0;
        num += (sgg - 2.0 * alpha * spg) + alpha * alpha * spp;            // alpha = 0 keeps a NaN of p: 0 * NaN
        den += sgg;
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) {
        s_part[wave][0] = num;
        s_part[wave][1] = den;
    }
    __syncthreads();
    if (threadIdx.x < kRowB) {
        const int q = threadIdx.x;
        ws_rows_b(a, img)[(long long)blockIdx.x * kRowB + q] = ((s_part[0][q] + s_part[1][q]) + s_part[2][q]) + s_part[3][q];
    }
}

template <int C>
__global__ __launch_bounds__(kImqThreads) void k_imq_ssim(ImqArgs a) {
    __shared__ float s_in[2][kInH][kInW];
    __shared__ double s_mid[5][kInH][kTileX];
    __shared__ double s_part[kImqWaves][kRowC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, img = blockIdx.y;
    const float* __restrict__ pred = a.pred.p + (long long)img * a.pred.image_stride;
    const float* __restrict__ trgt = a.trgt.p + (long long)img * a.trgt.image_stride;
    const int out_h = a.H - kHalo, out_w = a.W - kHalo;
    const int n_tiles = a.tiles_x * a.tiles_y;
    double sum = 0.0;
    long long n_pos = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int ty0 = (tile / a.tiles_x) * kTileY, tx0 = (tile % a.tiles_x) * kTileX;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            __syncthreads();                                                 // the previous trip's readers are done with s_in / s_mid
            for (int i = threadIdx.x; i < kInH * kInW; i += kImqThreads) {
                const int r = i / kInW, x = i % kInW;
                const int y = ty0 + r, xx = tx0 + x;
                float p = 0.f, g = 0.f;
                if (y < a.H && xx < a.W) {
                    const long long pix = (long long)y * a.W + xx;
                    p = pred[pix * a.pred.pixel_stride + c];
                    g = trgt[pix * a.trgt.pixel_stride + c];
                }
                s_in[0][r][x] = p;
                s_in[1][r][x] = g;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < kInH * kTileX; i += kImqThreads) {
                const int r = i / kTileX, x = i % kTileX;
                double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < kTaps; ++t) {
                    const double p = (double)s_in[0][r][x + t], g = (double)s_in[1][r][x + t], w = a.taps[t];
                    f[0] += w * p;
                    f[1] += w * g;
                    f[2] += w * (p * p);
                    f[3] += w * (g * g);
                    f[4] += w * (p * g);
                }
#pragma unroll
                for (int q = 0; q < 5; ++q) s_mid[q][r][x] = f[q];
            }
            __syncthreads();
            for (int i = threadIdx.x; i < kTileY * kTileX; i += kImqThreads) {
                const int r = i / kTileX, x = i % kTileX;
                const int oy = ty0 + r, ox = tx0 + x;
                if (oy >= out_h || ox >= out_w) continue;
                if (!pixel_valid(a.mask, img, (long long)(oy + kHalo / 2) * a.W + (ox + kHalo / 2))) continue;
                double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < kTaps; ++t) {
                    const double w = a.taps[t];
#pragma unroll
                    for (int q = 0; q < 5; ++q) f[q] += w * s_mid[q][r + t][x];
                }
                const double mx = f[0], my = f[1];
                const double vx = f[2] - mx * mx, vy = f[3] - my * my, vxy = f[4] - mx * my;
                sum += ((2.0 * mx * my + a.c1) * (2.0 * vxy + a.c2)) / ((mx * mx + my * my + a.c1) * (vx + vy + a.c2));
                n_pos += c == 0;
            }
        }
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_pos += __shfl_xor(n_pos, off);
    if (lane == 0) {
        s_part[wave][0] = sum;
        s_part[wave][1] = __longlong_as_double(n_pos);
    }
    __syncthreads();
    double* __restrict__ row = ws_rows_c(a, img) + (long long)blockIdx.x * kRowC;
    if (threadIdx.x == 0) row[0] = ((s_part[0][0] + s_part[1][0]) + s_part[2][0]) + s_part[3][0];
    if (threadIdx.x == 1) {
        long long t = 0;
        for (int wv = 0; wv < kImqWaves; ++wv) t += __double_as_longlong(s_part[wv][1]);
        row[1] = __longlong_as_double(t);
    }
}

// the last launch: one workgroup per image; the rows are staged in LDS by the whole workgroup (as k_eval_finish), then nine threads
// add one column each in index order
__global__ __launch_bounds__(kImqThreads) void k_imq_finish(ImqArgs a) {
    __shared__ double s_rows[kImqMaxBlocks * (kRowA + kRowB + kRowC)];
    const int img = blockIdx.x;
    double* s_a = s_rows;
    double* s_b = s_a + kImqMaxBlocks * kRowA;
    double* s_c = s_b + kImqMaxBlocks * kRowB;
    const double* __restrict__ ra = ws_rows_a(a, img);
    const double* __restrict__ rb = ws_rows_b(a, img);
    const double* __restrict__ rc = ws_rows_c(a, img);
    for (int i = threadIdx.x; i < a.blocks_a * kRowA; i += kImqThreads) s_a[i] = ra[i];
    for (int i = threadIdx.x; i < a.blocks_b * kRowB; i += kImqThreads) s_b[i] = rb[i];
    for (int i = threadIdx.x; i < a.blocks_c * kRowC; i += kImqThreads) s_c[i] = rc[i];
    __syncthreads();
    double* __restrict__ sums = a.sums + (long long)img * INERF_IMQ_SUMS;
    long long* __restrict__ counts = a.counts + (long long)img * INERF_IMQ_COUNTS;
    const int t = threadIdx.x;
    if (t < 4) {                                         // INERF_IMQ_SPP, SPG, SGG, SQ_DIFF
        double v = 0.0;
        for (int b = 0; b < a.blocks_a; ++b) v += s_a[b * kRowA + t];
        sums[t] = v;
    } else if (t == 4) {
        long long n = 0;
        for (int b = 0; b < a.blocks_a; ++b) n += __double_as_longlong(s_a[b * kRowA + 4]);
        counts[INERF_IMQ_N_VALID] = n;
    } else if (t < 7) {                                  // INERF_IMQ_LMSE_NUM, LMSE_DEN
        double v = 0.0;
        for (int b = 0; b < a.blocks_b; ++b) v += s_b[b * kRowB + (t - 5)];
        sums[INERF_IMQ_LMSE_NUM + (t - 5)] = v;
    } else if (t == 7) {
        double v = 0.0;
        for (int b = 0; b < a.blocks_c; ++b) v += s_c[b * kRowC];
        sums[INERF_IMQ_SSIM_SUM] = v;
    } else if (t == 8) {
        long long n = 0;
        for (int b = 0; b < a.blocks_c; ++b) n += __double_as_longlong(s_c[b * kRowC + 1]);
        counts[INERF_IMQ_N_SSIM] = n;
    } else if (t == 9) {
        counts[INERF_IMQ_N_WINDOWS] = (long long)a.win_x * a.win_y;
    }
}

bool misaligned(const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }

int capped(long long blocks) { return (int)(blocks < kImqMaxBlocks ? blocks : kImqMaxBlocks); }

// the shape-derived half of ImqArgs; INERF_OK, or the error of an unsupported window / size
int imq_plan(int64_t n_images, int64_t H, int64_t W, int64_t channels, int64_t k, int64_t s, ImqArgs& a) {
    if (n_images < 0 || H < 0 || W < 0 || (channels != 1 && channels != 3)) return INERF_E_INVALID;
    if (s < 1 || s > k || k % s != 0 || k / s > 8) return INERF_E_UNSUPPORTED;
    if (n_images > 65535 || H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL || k > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    a.H = (int)H;
    a.W = (int)W;
    a.k = (int)k;
    a.s = (int)s;
    a.r = (int)(k / s);
    int L = 1;
    while (L < 64 && (long long)L < s * s) L <<= 1;
    a.lanes_per_cell = L;
    a.cells_x = (int)((W + s - 1) / s);
    a.cells_y = (int)((H + s - 1) / s);
    a.win_x = W >= k ? (int)((W - k) / s + 1) : 0;
    a.win_y = H >= k ? (int)((H - k) / s + 1) : 0;
    if (a.win_x == 0 || a.win_y == 0) a.win_x = a.win_y = 0;
    a.tiles_x = W > kHalo ? (int)((W - kHalo + kTileX - 1) / kTileX) : 0;
    a.tiles_y = H > kHalo ? (int)((H - kHalo + kTileY - 1) / kTileY) : 0;
    if (a.tiles_x == 0 || a.tiles_y == 0) a.tiles_x = a.tiles_y = 0;
    const long long n_cells = (long long)a.cells_x * a.cells_y, per_block = (long long)kImqWaves * (64 / L);
    a.blocks_a = capped((n_cells + per_block - 1) / per_block);
    a.blocks_b = capped(((long long)a.win_x * a.win_y + kImqThreads - 1) / kImqThreads);
    a.blocks_c = capped((long long)a.tiles_x * a.tiles_y);
    a.image_slots = (long long)a.blocks_a * kRowA + n_cells * 3 + (long long)a.blocks_b * kRowB + (long long)a.blocks_c * kRowC;
    return INERF_OK;
}

}  // namespace
}  // namespace inerf

extern "C" int64_t inerf_image_quality_workspace_bytes(int64_t n_images, int64_t height, int64_t width, int channels, int window_size,
                                                       int window_shift) {
    inerf::ImqArgs a{};
    const int rc = inerf::imq_plan(n_images, height, width, channels, window_size, window_shift, a);
    if (rc != INERF_OK) return rc;
    if (n_images == 0 || height * width == 0) return 0;
    return (int64_t)(n_images * a.image_slots * (int64_t)sizeof(double));
}

extern "C" int inerf_image_quality(const inerf_imq_args* args, void* stream) {
    using namespace inerf;
    if (!args) return INERF_E_INVALID;
    ImqArgs a{};
    const int C = args->channels;
    const int rc = imq_plan(args->n_images, args->height, args->width, C, args->window_size, args->window_shift, a);
    if (rc != INERF_OK) return rc;
    if (args->pred_pixel_stride < C || args->trgt_pixel_stride < C || (args->mask && args->mask_pixel_stride < 1)) return INERF_E_INVALID;
    if (args->pred_image_stride < 0 || args->trgt_image_stride < 0 || args->mask_image_stride < 0) return INERF_E_INVALID;
    if (args->n_images == 0 || (int64_t)args->height * args->width == 0) return INERF_OK;
    if (!args->pred || !args->trgt || !args->sums || !args->counts) return INERF_E_INVALID;
    if (misaligned(args->pred, 4) || misaligned(args->trgt, 4) || misaligned(args->mask, 4) || misaligned(args->sums, 8) ||
        misaligned(args->counts, 8))
        return INERF_E_INVALID;
    const int64_t need = (int64_t)args->n_images * a.image_slots * (int64_t)sizeof(double);
    if (!args->workspace || misaligned(args->workspace, 8) || args->workspace_bytes < need) return INERF_E_WORKSPACE;

    a.pred = ImqView{args->pred, (long long)args->pred_pixel_stride, (long long)args->pred_image_stride};
    a.trgt = ImqView{args->trgt, (long long)args->trgt_pixel_stride, (long long)args->trgt_image_stride};
    a.mask = ImqView{args->mask, (long long)args->mask_pixel_stride, (long long)args->mask_image_stride};
    for (int t = 0; t < kTaps; ++t) a.taps[t] = args->taps[t];
    a.c1 = args->c1;
    a.c2 = args->c2;
    a.workspace = static_cast<double*>(args->workspace);
    a.sums = args->sums;
    a.counts = reinterpret_cast<long long*>(args->counts);
    const unsigned n = (unsigned)args->n_images;
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) hipLaunchKernelGGL(k_imq_moments<1>, dim3(a.blocks_a, n), dim3(kImqThreads), 0, st, a);
    else hipLaunchKernelGGL(k_imq_moments<3>, dim3(a.blocks_a, n), dim3(kImqThreads), 0, st, a);
    int e = record(hipGetLastError());
    if (e != INERF_OK) return e;
    if (a.blocks_b > 0) {
        hipLaunchKernelGGL(k_imq_windows, dim3(a.blocks_b, n), dim3(kImqThreads), 0, st, a);
        if ((e = record(hipGetLastError())) != INERF_OK) return e;
    }
    if (a.blocks_c > 0) {
        if (C == 1) hipLaunchKernelGGL(k_imq_ssim<1>, dim3(a.blocks_c, n), dim3(kImqThreads), 0, st, a);
        else hipLaunchKernelGGL(k_imq_ssim<3>, dim3(a.blocks_c, n), dim3(kImqThreads), 0, st, a);
        if ((e = record(hipGetLastError())) != INERF_OK) return e;
    }
    hipLaunchKernelGGL(k_imq_finish, dim3(n), dim3(kImqThreads), 0, st, a);
    return record(hipGetLastError());
}
