// jpeg.hip - the frames of a render_path loop as baseline JPEG files inside AVI chunks, encoded on the device from the planes
// inerf_frame_products wrote (include/inerf.h has the format, DESIGN.md section 3 the arithmetic).  Three launches per call, for all
// images together, ordered by the stream alone:
//   k_jpeg_segment : one workgroup per SEGMENT = one MCU row of one image (the restart interval is the MCUs of a row, so the DC
//                    predictors start from 0 and the segment ends on a byte).  The row is walked in chunks of 96 blocks (96 grey or 32
//                    colour MCUs): colour conversion and the row pass of the DCT on 8 lanes per block, the column pass, quantisation
//                    and zigzag on 8 lanes per block, then one WAVE per block - lane i holds zigzag coefficient i, a ballot gives the
//                    zero runs, a wave reduction the block's bits, a workgroup scan the blocks' bit positions, and the codes are ORed
//                    into LDS (big-endian words).  Whole bytes are stuffed (FF -> FF 00, a scan of the FF counts) into the segment's
//                    worst-case slot of the workspace; up to 7 bits, the predictors and the byte count are carried to the next chunk.
//   k_jpeg_finish  : ONE workgroup: 16 lanes per image sum the segment lengths, lane 0 walks the images in the call's order (images
//                    of one call may share an arena - a batch of one movie's frames - and must land in that order), reserves each
//                    frame's place, advances the cursor, writes the index entry or the status word; the 16 lanes then give every
//                    segment its place.
//   k_jpeg_gather  : one workgroup per segment copies the slot to its place; the first also writes the chunk header and the file
//                    header, the last EOI and the pad byte.
// Integer arithmetic only; LDS atomics are ORs, which have no order: the bytes are the same on every run.
// LDS per workgroup: 12 KiB coefficients + 12 KiB row-pass results + 19.5 KiB bits + 4 KiB tables = 48 KiB: three per CU.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/inerf.h"
#include "jpeg_tables.h"
#include "mlp_common.h"

namespace inerf {

constexpr int kJpegThreads = 256;
constexpr int kJpegChunk = 96;                                       // blocks per chunk: a multiple of 3, and of the 4 waves
constexpr int kJpegBitWords = kJpegChunk * kJpegBlockBytes / 4 + 4;  // 7 carried bits + 96 * 1660 bits, and the word after the last
constexpr int kJpegMetaBytes = 16;                                   // per segment: length (4), -, place in the arena (8)
constexpr int kJpegHeadBytes = 256;                                  // the workspace starts with {place, file size} per image

struct JpegImg {
    long long src_off, cap, index_frames, slot_base;
    const unsigned char* header;
    unsigned char* arena;
    long long* cursor;
    long long* index;
    long long* status;
    int h, w, c, nbx, nseg, seg_base, slot, header_bytes;
};

struct JpegParams {
    const unsigned char* src;
    unsigned char* ws;
    int n_images, n_segs;
    JpegImg img[INERF_JPEG_MAX_IMAGES];
};

struct JpegOrder { unsigned char nat2zz[64]; };
constexpr JpegOrder jpeg_make_order() {
    JpegOrder o{};
    for (int k = 0; k < 64; ++k) o.nat2zz[kJpegZigzag[k]] = (unsigned char)k;
    return o;
}
__device__ const JpegCodes d_jpeg_codes = jpeg_make_codes();
__device__ const JpegOrder d_jpeg_order = jpeg_make_order();

struct JpegShared {
    short coef[kJpegChunk][64];                        // quantised, zigzag order
    short tmp[kJpegChunk][64];                         // the row pass: [y][u], 4 fraction bits
    uint32_t bits[kJpegBitWords];                      // big-endian words: bit 31 of word 0 is the chunk's first bit
    uint32_t dc[2][12], ac[2][256];
    int scan[kJpegThreads];
    int blk_bits[kJpegChunk];
    unsigned short qt[2][64];                          // zigzag order
    unsigned char nat2zz[64];
    int pred[3];
};

__device__ __forceinline__ int jpeg_image_of(const JpegParams& a, int seg) {
    int k = 0;
    while (k + 1 < a.n_images && seg >= a.img[k + 1].seg_base) ++k;
    return k;
}

// n <= 32 bits of `value` (its low n bits, the first one highest) at bit position p of the big-endian words
__device__ __forceinline__ void jpeg_or_bits(uint32_t* words, int p, uint32_t value, int n) {
    const int w = p >> 5, off = p & 31;
    const unsigned long long v = (unsigned long long)value << (64 - off - n);
    atomicOr(&words[w], (uint32_t)(v >> 32));
    if ((uint32_t)v) atomicOr(&words[w + 1], (uint32_t)v);
}

__device__ __forceinline__ int jpeg_size_of(int a) { return a ? 32 - __clz(a) : 0; }      // a >= 0: the bits of its magnitude

// what lane `lane` of a wave contributes to block b: `zrl` ZRL codes, then n bits `value`.  Every lane of the wave calls it.
__device__ __forceinline__ void jpeg_symbol(const JpegShared& sh, int b, int c, int lane, int& zrl, uint32_t& value, int& n) {
    const int comp = b % c, t = comp ? 1 : 0;
    const int v = sh.coef[b][lane];
    const unsigned long long mask = __ballot(v != 0) | 1ull;            // the DC position bounds the first run
    zrl = 0; value = 0; n = 0;
    if (lane == 0) {
        const int d = v - (b >= c ? (int)sh.coef[b - c][0] : sh.pred[comp]);
        const int s = jpeg_size_of(d < 0 ? -d : d);
        const uint32_t cd = sh.dc[t][s];
        value = (cd & 0xffffu) << s | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u));
        n = (int)(cd >> 16) + s;
    } else if (v != 0) {
        const int before = 63 - __clzll((long long)(mask & ((1ull << lane) - 1ull)));
        const int run = lane - before - 1;
        const int s = jpeg_size_of(v < 0 ? -v : v);
        const uint32_t cd = sh.ac[t][(run & 15) << 4 | s];
        zrl = run >> 4;
        value = (cd & 0xffffu) << s | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u));
        n = (int)(cd >> 16) + s;
    } else if (lane == 63) {                                            // zeros up to the end: EOB
        const uint32_t cd = sh.ac[t][0];
        value = cd & 0xffffu;
        n = (int)(cd >> 16);
    }
}

__device__ __forceinline__ int jpeg_sum_scan(int v, int* s) {          // inclusive, going up the lanes
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kJpegThreads; d <<= 1) {
        const int x = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        v += x;
        s[tid] = v;
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(kJpegThreads) void k_jpeg_segment(const JpegParams a) {
    __shared__ JpegShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x;
    const JpegImg& im = a.img[jpeg_image_of(a, seg)];
    const int row = seg - im.seg_base, c = im.c;
    const unsigned char* __restrict__ plane = a.src + im.src_off;
    unsigned char* __restrict__ slot = a.ws + im.slot_base + (long long)row * im.slot;

    for (int i = tid; i < 24; i += kJpegThreads) (&sh.dc[0][0])[i] = (&d_jpeg_codes.dc[0][0])[i];
    for (int i = tid; i < 512; i += kJpegThreads) (&sh.ac[0][0])[i] = (&d_jpeg_codes.ac[0][0])[i];
    if (tid < 64) {
        const int q0 = im.header[kJpegLumaAt + tid], q1 = c == 3 ? im.header[kJpegChromaAt + tid] : 1;
        sh.qt[0][tid] = (unsigned short)(q0 ? q0 : 1);
        sh.qt[1][tid] = (unsigned short)(q1 ? q1 : 1);
        sh.nat2zz[tid] = d_jpeg_order.nat2zz[tid];
    }
    if (tid < 3) sh.pred[tid] = 0;
    __syncthreads();

    const uint32_t zrl0 = sh.ac[0][0xf0], zrl1 = sh.ac[1][0xf0];     // ZRL: code | length << 16
    const int per_chunk = kJpegChunk / c;                  // MCUs
    int carry_bits = 0, out_bytes = 0;
    uint32_t carry_byte = 0;                               // the carried bits, in the high bits of a byte

    for (int m0 = 0; m0 < im.nbx; m0 += per_chunk) {
        const int nm = im.nbx - m0 < per_chunk ? im.nbx - m0 : per_chunk, nb = nm * c;
        const bool last = m0 + nm == im.nbx;

        // ---- level shift (and colour conversion), row pass: lane (b, y) -------------------------------------------------------------
        for (int i = tid; i < nb * 8; i += kJpegThreads) {
            const int b = i >> 3, y = i & 7, mcu = m0 + b / c, comp = b % c;
            const int yy = row * 8 + y < im.h ? row * 8 + y : im.h - 1;
            const unsigned char* __restrict__ line = plane + (long long)yy * im.w * c;
            int p[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int xx = mcu * 8 + x < im.w ? mcu * 8 + x : im.w - 1;
                int s;
                if (c == 1) {
                    s = line[xx];
                } else {
                    const int r = line[3 * xx], g = line[3 * xx + 1], bl = line[3 * xx + 2];
                    if (comp == 0) s = (19595 * r + 38470 * g + 7471 * bl + 32768) >> 16;
                    else if (comp == 1) s = (-11059 * r - 21709 * g + 32768 * bl + 8388608 + 32767) >> 16;
                    else s = (32768 * r - 27439 * g - 5329 * bl + 8388608 + 32767) >> 16;
                }
                p[x] = s - 128;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int s = 0;
#pragma unroll
                for (int x = 0; x < 8; ++x) s += kJpegDct[u][x] * p[x];
                sh.tmp[b][y * 8 + u] = (short)((s + (1 << (kJpegPass1Shift - 1))) >> kJpegPass1Shift);
            }
        }
        __syncthreads();

        // ---- column pass, quantisation, zigzag: lane (b, u) ---------------------------------------------------------------------------
        for (int i = tid; i < nb * 8; i += kJpegThreads) {
            const int b = i >> 3, u = i & 7, t = (b % c) ? 1 : 0;
            int r[8];
#pragma unroll
            for (int y = 0; y < 8; ++y) r[y] = sh.tmp[b][y * 8 + u];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                int s = 0;
#pragma unroll
                for (int y = 0; y < 8; ++y) s += kJpegDct[v][y] * r[y];
                const int cf = (s + (1 << (kJpegPass2Shift - 1))) >> kJpegPass2Shift;
                const int z = sh.nat2zz[v * 8 + u], q = sh.qt[t][z];
                const int mag = ((cf < 0 ? -cf : cf) + 4 * q) / (8 * q);       // cf has 3 fraction bits: round half away from zero
                sh.coef[b][z] = (short)(cf < 0 ? -mag : mag);
            }
        }
        __syncthreads();

        // ---- the bits of every block: a wave per block --------------------------------------------------------------------------------
        for (int b = wave; b < nb; b += kJpegThreads / 64) {
            int zrl, n;
            uint32_t value;
            jpeg_symbol(sh, b, c, lane, zrl, value, n);
            int bits = n + zrl * (int)(((b % c) ? zrl1 : zrl0) >> 16);
            for (int d = 32; d >= 1; d >>= 1) bits += __shfl_xor(bits, d, 64);
            if (lane == 0) sh.blk_bits[b] = bits;
        }
        __syncthreads();
        const int mine = tid < nb ? sh.blk_bits[tid] : 0;
        const int incl = jpeg_sum_scan(mine, sh.scan);
        const int total_bits = carry_bits + sh.scan[kJpegThreads - 1];
        __syncthreads();
        if (tid < nb) sh.blk_bits[tid] = carry_bits + incl - mine;            // now: where the block's bits start
        for (int w = tid; w < (total_bits + 31) / 32 + 1; w += kJpegThreads) sh.bits[w] = w == 0 ? carry_byte << 24 : 0u;
        __syncthreads();

        for (int b = wave; b < nb; b += kJpegThreads / 64) {
            int zrl, n;
            uint32_t value;
            jpeg_symbol(sh, b, c, lane, zrl, value, n);
            const uint32_t zc = (b % c) ? zrl1 : zrl0;
            const int zl = (int)(zc >> 16);
            const int bits = n + zrl * zl;
            int upto = bits;                                                   // inclusive scan over the wave
            for (int d = 1; d < 64; d <<= 1) {
                const int x = __shfl_up(upto, d, 64);
                if (lane >= d) upto += x;
            }
            int at = sh.blk_bits[b] + upto - bits;
            for (int j = 0; j < zrl; ++j, at += zl) jpeg_or_bits(sh.bits, at, zc & 0xffffu, zl);
            if (n) jpeg_or_bits(sh.bits, at, value, n);
        }
        __syncthreads();
        if (tid < c) sh.pred[tid] = sh.coef[nb - c + tid][0];

        // ---- whole bytes, stuffed, to the slot; the last chunk fills its last byte with 1-bits ---------------------------------------
        int full = total_bits >> 3, rem = total_bits & 7;
        if (last && rem) {
            if (tid == 0) atomicOr(&sh.bits[full >> 2], ((1u << (8 - rem)) - 1u) << (24 - 8 * (full & 3)));
            ++full;
            rem = 0;
            __syncthreads();
        }
        const int strip = (full + kJpegThreads - 1) / kJpegThreads;
        const int b0 = tid * strip < full ? tid * strip : full, b1 = b0 + strip < full ? b0 + strip : full;
        int ff = 0;
        for (int i = b0; i < b1; ++i) ff += ((sh.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u ? 1 : 0;
        const int ff_incl = jpeg_sum_scan(ff, sh.scan);
        const int ff_all = sh.scan[kJpegThreads - 1];
        {
            unsigned char* __restrict__ out = slot + out_bytes + b0 + (ff_incl - ff);
            for (int i = b0; i < b1; ++i) {
                const uint32_t v = (sh.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
                *out++ = (unsigned char)v;
                if (v == 255u) *out++ = 0;
            }
        }
        carry_byte = rem ? (sh.bits[full >> 2] >> (24 - 8 * (full & 3))) & 255u : 0u;
        carry_bits = rem;
        out_bytes += full + ff_all;
        __syncthreads();
    }

    if (tid == 0) {
        if (row + 1 < im.nseg) {
            slot[out_bytes] = 0xff;
            slot[out_bytes + 1] = (unsigned char)(0xd0 + (row & 7));
            out_bytes += 2;
        }
        uint32_t* __restrict__ meta = reinterpret_cast<uint32_t*>(a.ws + kJpegHeadBytes + (long long)seg * kJpegMetaBytes);
        meta[0] = (uint32_t)out_bytes;
    }
}

__global__ __launch_bounds__(kJpegThreads) void k_jpeg_finish(const JpegParams a) {
    __shared__ long long part[INERF_JPEG_MAX_IMAGES][16];
    __shared__ long long place[INERF_JPEG_MAX_IMAGES];
    const int tid = threadIdx.x, k = tid >> 4, l = tid & 15;
    const bool act = k < a.n_images;
    const JpegImg& im = a.img[act ? k : 0];
    const int per = (im.nseg + 15) / 16;
    const int j0 = l * per < im.nseg ? l * per : im.nseg, j1 = j0 + per < im.nseg ? j0 + per : im.nseg;
    unsigned char* __restrict__ metas = a.ws + kJpegHeadBytes;
    long long sum = 0;
    if (act)
        for (int j = j0; j < j1; ++j) sum += *reinterpret_cast<const uint32_t*>(metas + (long long)(im.seg_base + j) * kJpegMetaBytes);
    part[k][l] = sum;
    __syncthreads();
    if (tid == 0) {
        long long* __restrict__ head = reinterpret_cast<long long*>(a.ws);
        for (int i = 0; i < a.n_images; ++i) {
            const JpegImg& o = a.img[i];
            long long data = 0;
            for (int j = 0; j < 16; ++j) data += part[i][j];
            const long long file = o.header_bytes + data + 2, chunk = 8 + file + (file & 1);
            volatile long long* cursor = o.cursor;
            const long long used = cursor[0], frames = cursor[1];
            if (used >= 0 && frames >= 0 && frames < o.index_frames && chunk <= o.cap - used) {
                place[i] = used;
                cursor[0] = used + chunk;
                cursor[1] = frames + 1;
                o.index[2 * frames] = used;
                o.index[2 * frames + 1] = file;
            } else {
                place[i] = -1;
                *o.status = used + chunk;
            }
            head[2 * i] = place[i];
            head[2 * i + 1] = file;
        }
    }
    __syncthreads();
    if (act) {
        long long at = place[k] < 0 ? -1 : place[k] + 8 + im.header_bytes;
        for (int j = 0; j < l; ++j) at += place[k] < 0 ? 0 : part[k][j];
        for (int j = j0; j < j1; ++j) {
            unsigned char* meta = metas + (long long)(im.seg_base + j) * kJpegMetaBytes;
            *reinterpret_cast<long long*>(meta + 8) = at;
            if (at >= 0) at += *reinterpret_cast<const uint32_t*>(meta);
        }
    }
}

__global__ __launch_bounds__(kJpegThreads) void k_jpeg_gather(const JpegParams a) {
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int k = jpeg_image_of(a, seg);
    const JpegImg& im = a.img[k];
    const unsigned char* __restrict__ meta = a.ws + kJpegHeadBytes + (long long)seg * kJpegMetaBytes;
    const int m = (int)*reinterpret_cast<const uint32_t*>(meta);
    const long long at = *reinterpret_cast<const long long*>(meta + 8);
    if (at < 0) return;                                                // the frame did not fit: nothing of it is written
    const int row = seg - im.seg_base;
    const unsigned char* __restrict__ slot = a.ws + im.slot_base + (long long)row * im.slot;
    unsigned char* __restrict__ out = im.arena + at;
    // bytes up to the arena's first dword boundary one by one, then whole dwords put together from the slot's bytes, then the tail
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(out) & 3)) & 3);
    if (head > m) head = m;
    const int body = (m - head) / 4;
    if (tid < head) out[tid] = slot[tid];
    uint32_t* __restrict__ out_words = reinterpret_cast<uint32_t*>(out + head);
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(slot);      // slots are 16-byte aligned and end on a dword
    const int shift = 8 * head;
    for (int w = tid; w < body; w += kJpegThreads) {
        const unsigned long long two = (unsigned long long)words[w] | (unsigned long long)words[w + 1] << 32;
        out_words[w] = (uint32_t)(two >> shift);
    }
    const int done = head + 4 * body;
    if (tid < m - done) out[done + tid] = slot[done + tid];

    const long long file = reinterpret_cast<const long long*>(a.ws)[2 * k + 1];
    if (row == 0) {
        unsigned char* __restrict__ chunk = im.arena + reinterpret_cast<const long long*>(a.ws)[2 * k];
        if (tid < 4) chunk[tid] = (unsigned char)("00dc"[tid]);
        else if (tid < 8) chunk[tid] = (unsigned char)((unsigned long long)file >> (8 * (tid - 4)));
        for (int i = tid; i < im.header_bytes; i += kJpegThreads) chunk[8 + i] = im.header[i];
    }
    if (row == im.nseg - 1) {
        if (tid == 0) out[m] = 0xff;
        if (tid == 1) out[m + 1] = 0xd9;
        if (tid == 2 && (file & 1)) out[m + 2] = 0;
    }
}

static bool jpeg_misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

static int jpeg_slot_bytes(int nbx, int channels) { return (nbx * channels * 2 * kJpegBlockBytes + 2 + 15) / 16 * 16; }

static bool jpeg_shape_ok(int height, int width, int channels) {
    return height >= 1 && height <= 65535 && width >= 1 && width <= 65535 && (channels == 1 || channels == 3);
}

struct JpegPlan {
    long long n_segs, workspace;
    JpegImg img[INERF_JPEG_MAX_IMAGES];
};

// shapes only: the segments and the workspace; a negative error code otherwise
static long long jpeg_plan(const inerf_jpeg_args* args, JpegPlan* plan) {
    if (!args || args->n_images < 0 || args->n_images > INERF_JPEG_MAX_IMAGES) return INERF_E_INVALID;
    long long segs = 0, slots = 0;
    for (int k = 0; k < args->n_images; ++k) {
        const inerf_jpeg_image& im = args->images[k];
        if (!jpeg_shape_ok(im.height, im.width, im.channels) || im.quality < 1 || im.quality > 100) return INERF_E_INVALID;
        JpegImg& o = plan->img[k];
        o.h = im.height; o.w = im.width; o.c = im.channels;
        o.nbx = (im.width + 7) / 8; o.nseg = (im.height + 7) / 8; o.seg_base = (int)segs;
        o.slot = jpeg_slot_bytes(o.nbx, o.c);
        o.header_bytes = jpeg_header_bytes(o.c);
        o.slot_base = slots;                               // from the first slot; the meta records come before it
        segs += o.nseg;
        slots += (long long)o.nseg * o.slot;
    }
    for (int k = 0; k < args->n_images; ++k) plan->img[k].slot_base += kJpegHeadBytes + segs * kJpegMetaBytes;
    plan->n_segs = segs;
    plan->workspace = kJpegHeadBytes + segs * kJpegMetaBytes + slots;
    return plan->workspace;
}

}  // namespace inerf

extern "C" int64_t inerf_jpeg_workspace_bytes(const inerf_jpeg_args* args) {
    inerf::JpegPlan plan;
    return inerf::jpeg_plan(args, &plan);
}

extern "C" int64_t inerf_jpeg_frame_bound(int32_t height, int32_t width, int32_t channels) {
    if (!inerf::jpeg_shape_ok(height, width, channels)) return INERF_E_INVALID;
    const int nbx = (width + 7) / 8, nseg = (height + 7) / 8;
    const long long file = inerf::jpeg_header_bytes(channels) + (long long)nseg * (nbx * channels * 2 * inerf::kJpegBlockBytes + 2) + 2;
    return 8 + file + 1;
}

extern "C" int inerf_jpeg_tables(int32_t quality, unsigned char* luma, unsigned char* chroma) {
    if (quality < 1 || quality > 100 || !luma || !chroma) return INERF_E_INVALID;
    for (int i = 0; i < 64; ++i) {
        luma[i] = (unsigned char)inerf::jpeg_quant(inerf::kJpegLumaBase[i], quality);
        chroma[i] = (unsigned char)inerf::jpeg_quant(inerf::kJpegChromaBase[i], quality);
    }
    return INERF_OK;
}

extern "C" int64_t inerf_jpeg_header(int32_t height, int32_t width, int32_t channels, int32_t quality, unsigned char* dst, int64_t capacity) {
    using namespace inerf;
    if (!jpeg_shape_ok(height, width, channels) || quality < 1 || quality > 100 || !dst) return INERF_E_INVALID;
    const int need = jpeg_header_bytes(channels);
    if (capacity < need) return INERF_E_INVALID;
    unsigned char* p = dst;
    auto put = [&](int v) { *p++ = (unsigned char)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
    put16(0xffd8);
    put16(0xffe0); put16(16);                                              // JFIF 1.01, no units, 1 : 1, no thumbnail
    for (const char ch : {'J', 'F', 'I', 'F', '\0'}) put(ch);
    put16(0x0101); put(0); put16(1); put16(1); put(0); put(0);
    for (int t = 0; t < (channels == 3 ? 2 : 1); ++t) {
        put16(0xffdb); put16(67); put(t);
        for (int k = 0; k < 64; ++k) put(jpeg_quant((t ? kJpegChromaBase : kJpegLumaBase)[kJpegZigzag[k]], quality));
    }
    put16(0xffc0); put16(8 + 3 * channels); put(8); put16(height); put16(width); put(channels);
    for (int i = 0; i < channels; ++i) { put(i + 1); put(0x11); put(i ? 1 : 0); }
    for (int t = 0; t < (channels == 3 ? 2 : 1); ++t) {
        put16(0xffc4); put16(2 + 1 + 16 + 12); put(t);
        for (int i = 0; i < 16; ++i) put(kJpegDcBits[t][i]);
        for (int i = 0; i < 12; ++i) put(kJpegDcVals[i]);
        put16(0xffc4); put16(2 + 1 + 16 + 162); put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(kJpegAcBits[t][i]);
        for (int i = 0; i < 162; ++i) put(kJpegAcVals[t][i]);
    }
    put16(0xffdd); put16(4); put16((width + 7) / 8);                       // one restart interval per MCU row
    put16(0xffda); put16(6 + 2 * channels); put(channels);
    for (int i = 0; i < channels; ++i) { put(i + 1); put(i ? 0x11 : 0x00); }
    put(0); put(63); put(0);
    return p - dst == need ? need : INERF_E_UNSUPPORTED;
}

extern "C" int inerf_jpeg_encode(const inerf_jpeg_args* args, void* stream) {
    using namespace inerf;
    JpegPlan plan;
    const long long need = jpeg_plan(args, &plan);
    if (need < 0) return (int)need;
    if (args->src_bytes < 0) return INERF_E_INVALID;
    for (int k = 0; k < args->n_images; ++k) {
        const inerf_jpeg_image& im = args->images[k];
        const long long plane = (long long)im.height * im.width * im.channels;
        if (im.src_offset < 0 || im.src_offset > args->src_bytes || plane > args->src_bytes - im.src_offset) return INERF_E_INVALID;
        if (!im.header || im.header_bytes != plan.img[k].header_bytes) return INERF_E_INVALID;
        if (!im.arena || im.arena_bytes < im.header_bytes) return INERF_E_INVALID;
        if (!im.cursor || !im.index || !im.status || im.index_frames < 1) return INERF_E_INVALID;
        if (jpeg_misaligned(im.cursor, 8) || jpeg_misaligned(im.index, 8) || jpeg_misaligned(im.status, 8)) return INERF_E_INVALID;
    }
    if (args->n_images == 0) return INERF_OK;
    if (!args->src) return INERF_E_INVALID;
    if (!args->workspace || args->workspace_bytes < need) return INERF_E_WORKSPACE;
    if (jpeg_misaligned(args->workspace, 16)) return INERF_E_INVALID;
    if (plan.n_segs > 0x7fffffffLL / kJpegThreads) return INERF_E_UNSUPPORTED;

    JpegParams a{};
    a.src = args->src; a.ws = static_cast<unsigned char*>(args->workspace);
    a.n_images = args->n_images; a.n_segs = (int)plan.n_segs;
    for (int k = 0; k < args->n_images; ++k) {
        const inerf_jpeg_image& im = args->images[k];
        JpegImg& o = a.img[k];
        o = plan.img[k];
        o.src_off = im.src_offset; o.cap = im.arena_bytes; o.index_frames = im.index_frames;
        o.header = im.header; o.arena = im.arena; o.cursor = reinterpret_cast<long long*>(im.cursor); o.index = reinterpret_cast<long long*>(im.index);
        o.status = reinterpret_cast<long long*>(im.status);
    }
    hipLaunchKernelGGL(k_jpeg_segment, dim3((unsigned)plan.n_segs), dim3(kJpegThreads), 0, (hipStream_t)stream, a);
    int rc = record(hipGetLastError());
    if (rc != INERF_OK) return rc;
    hipLaunchKernelGGL(k_jpeg_finish, dim3(1), dim3(kJpegThreads), 0, (hipStream_t)stream, a);
    rc = record(hipGetLastError());
    if (rc != INERF_OK) return rc;
    hipLaunchKernelGGL(k_jpeg_gather, dim3((unsigned)plan.n_segs), dim3(kJpegThreads), 0, (hipStream_t)stream, a);
    return record(hipGetLastError());
}
