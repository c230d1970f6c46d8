// png.hip - the frame images of a render_path loop as PNG files, encoded on the device from the planes inerf_frame_products wrote
// (include/inerf.h has the format).  Three launches per call, for all images together, ordered by the stream alone:
//   k_png_segment : one workgroup per SEGMENT (whole rows, at most 32 KiB of filtered bytes).  Filters its rows into LDS (adaptive:
//                   per row the type with the smallest sum of min(b, 256 - b)), sums Adler-32's two terms, finds the runs of equal
//                   bytes (start flags per 128-byte chunk, then a max / min scan over the chunks for the runs that cross them), counts
//                   the tokens with LDS atomics, builds the dynamic code (symbols sorted by rank on all lanes, the lengths on one lane:
//                   png_huff.h, the canonical codes and the header's bits on all lanes again), lays the tokens out by a prefix
//                   sum of their code lengths and ORs their bits into LDS; a segment the code does not shrink is stored.  The
//                   segment's bytes go to its fixed slot of the workspace with their length, their CRC-32 register from 0 and
//                   x^(8 * length) mod P.
//   k_png_finish  : one workgroup, image k on lane k: scans the segment lengths, combines Adler-32 and CRC-32, writes the signature,
//                   IHDR, the IDAT frame, the final empty block, the trailers, IEND and sizes[k].
//   k_png_gather  : one workgroup per segment copies the slot to its place in the file.
// Integer arithmetic only; LDS atomics are integer adds and ORs, which have no order: the bytes are the same on every run.
// LDS per workgroup: 33 KiB filtered bytes + 33 KiB output + 8 KiB tables = 74 KiB, so two workgroups share a CU's 160 KiB.  Both
// byte buffers skip 4 bytes after every 128: lane t works on bytes [128 t, 128 t + 128), and the skew puts the lanes of a wave on
// 32 different banks.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/inerf.h"
#include "mlp_common.h"
#include "png_huff.h"

namespace inerf {

constexpr int kPngThreads = 256;
constexpr int kPngCap = 32768;                         // filtered bytes per segment
constexpr int kPngChunk = 128;                         // bytes per lane: kPngThreads * kPngChunk == kPngCap
constexpr int kPngSlot = kPngCap + 16;                 // a segment's slot in the workspace: 5 + kPngCap bytes at most, whole dwords
constexpr int kPngCrcChunk = 136;                      // bytes per lane of the CRC pass: 256 * 136 >= kPngCap + 5
constexpr int kPngMetaWords = 8;                       // per segment: length, Adler s1, s2, CRC register, x^(8 length), -, dst position (2)
constexpr int kPngFixedBytes = 68;                     // signature 8, IHDR 25, IDAT frame 12, zlib header 2, final block 5, Adler 4, IEND 12

__host__ __device__ constexpr int png_pad(int i) { return i + ((i >> 7) << 2); }
constexpr int kPngInBytes = png_pad(kPngCap);                    // 33 792
constexpr int kPngOutBytes = png_pad(kPngSlot) + 16;             // 33 824

struct PngImg {
    long long src_off, dst_off;
    int h, w, rowraw, bpp, swap16, colour, depth, filter, rps, nseg, seg_base, group;
};

struct PngParams {
    const unsigned char* src;
    unsigned char* dst;
    long long* sizes;
    uint32_t* meta;
    unsigned char* slots;
    int n_images, n_segs;
    uint32_t xpow_tree[8];                             // x^(8 * 136 * 2^l) mod P
    PngImg img[INERF_PNG_MAX_IMAGES];
};

struct PngShared {
    uint32_t hist[kPngMaxSymbols];
    uint32_t code[kPngMaxSymbols];                     // bit-reversed code | length << 16
    uint32_t work[2 * kPngMaxSymbols + 40];
    unsigned char len[kPngMaxSymbols];
    uint32_t count[16];                                // literal/length codes per length
    int used, hlit;
    uint32_t crc_table[256];
    int scan[kPngThreads];
    uint32_t crc[kPngThreads];
    uint32_t fsum[2][32][5];
    uint32_t cl_freq[20], cl_code[20];
    unsigned char cl_len[20];
    uint32_t adler[2];
    uint32_t xpow;
    int hdr_bits;
};

__device__ const unsigned char d_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t& out_word(unsigned char* s_out, int w) { return *reinterpret_cast<uint32_t*>(s_out + png_pad(4 * w)); }

__device__ __forceinline__ void or_bits(unsigned char* s_out, int bitpos, uint32_t value) {
    const int w = bitpos >> 5, sh = bitpos & 31;
    const unsigned long long v = (unsigned long long)value << sh;
    atomicOr(&out_word(s_out, w), (uint32_t)v);
    if (v >> 32) atomicOr(&out_word(s_out, w + 1), (uint32_t)(v >> 32));
}

__device__ __forceinline__ uint32_t bit_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// inclusive scan of one int per lane over the workgroup (max going up the lanes, or min going down); every lane calls it
template <bool kMin>
__device__ __forceinline__ int block_scan(int v, int* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kPngThreads; d <<= 1) {
        const int o = kMin ? tid + d : tid - d;
        const bool in = o >= 0 && o < kPngThreads;
        const int x = in ? s[o] : 0;
        __syncthreads();
        if (in) { v = kMin ? (x < v ? x : v) : (x > v ? x : v); s[tid] = v; }
        __syncthreads();
    }
    return v;
}

// inclusive sum going up the lanes
__device__ __forceinline__ int block_sum_scan(int v, int* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kPngThreads; d <<= 1) {
        const int x = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        v += x;
        s[tid] = v;
        __syncthreads();
    }
    return v;
}

// f(position, token, byte) for every token that starts in [c0, c1): `carry` is where the run that holds byte c0 starts when c0 does
// not start one, `after` where the run that holds byte c1 - 1 ends when it goes on past c1
template <class F>
__device__ __forceinline__ void walk_tokens(const unsigned char* s_in, int c0, int c1, int len, int carry, int after, F f) {
    if (c0 >= c1) return;
    int s = (c0 == 0 || s_in[png_pad(c0)] != s_in[png_pad(c0 - 1)]) ? c0 : carry;
    int p = c0;
    while (p < c1) {
        const int v = s_in[png_pad(p)];
        int stop = p + 1;
        while (stop < c1 && s_in[png_pad(stop)] == v) ++stop;
        int e = stop;
        if (stop == c1 && c1 < len && s_in[png_pad(c1)] == v) e = after;
        const int run = e - s;
        if (run < 4) {
            for (; p < stop; ++p) f(p, 1, v);
        } else {
            for (; p < stop; ++p) {
                const int t = png_run_token(p - s, run);
                if (t) f(p, t, v);
            }
        }
        s = stop;
    }
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filtered(int type, int x, int a, int b, int c) {
    switch (type) {
    case 0: return x;
    case 1: return (x - a) & 255;
    case 2: return (x - b) & 255;
    case 3: return (x - ((a + b) >> 1)) & 255;
    default: return (x - paeth(a, b, c)) & 255;
    }
}

__device__ __forceinline__ int filter_cost(int f) { return f < 128 ? f : 256 - f; }

__global__ __launch_bounds__(kPngThreads) void k_png_segment(const PngParams a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    unsigned char* __restrict__ s_in = s_raw;
    unsigned char* __restrict__ s_out = s_raw + kPngInBytes;
    PngShared& sh = *reinterpret_cast<PngShared*>(s_raw + kPngInBytes + kPngOutBytes);
    const int tid = threadIdx.x;
    const int seg = blockIdx.x;
    int k = 0;
    while (k + 1 < a.n_images && seg >= a.img[k + 1].seg_base) ++k;
    const PngImg& im = a.img[k];
    const int r0 = (seg - im.seg_base) * im.rps;
    const int nrows = im.h - r0 < im.rps ? im.h - r0 : im.rps;
    const int rowbytes = im.rowraw + 1;
    const int len = nrows * rowbytes;

    for (int i = tid; i < kPngMaxSymbols; i += kPngThreads) sh.hist[i] = i == 256 ? 1u : 0u;      // the end of block occurs once
    if (tid < 16) sh.count[tid] = 0;
    if (tid < 20) sh.cl_freq[tid] = 0;
    if (tid == 0) { sh.used = 0; sh.hlit = 257; }
    for (int i = tid; i < kPngOutBytes / 4; i += kPngThreads) reinterpret_cast<uint32_t*>(s_out)[i] = 0;
    sh.crc_table[tid] = crc_table_entry((uint32_t)tid);
    if (tid < 2) sh.adler[tid] = 0;

    // ---- filter: a group of lanes per row, 256 / group rows per round ----------------------------------------------------------
    {
        const int group = im.group, rows_round = kPngThreads / group, g = tid / group, lane = tid % group;
        const unsigned char* __restrict__ plane = a.src + im.src_off;
        const int bpp = im.bpp, sw = im.swap16;
        int round = 0;
        for (int base = 0; base < nrows; base += rows_round, ++round) {
            const int rr = base + g;
            const bool act = rr < nrows;
            const long long r = (long long)r0 + rr;
            const unsigned char* __restrict__ cur = plane + r * im.rowraw;
            const unsigned char* __restrict__ up = cur - im.rowraw;          // read only when r > 0
            int type = im.filter;
            if (im.filter < 0) {
                uint32_t* __restrict__ sums = sh.fsum[round & 1][g];
                if (lane < 5) sums[lane] = 0;
                __syncthreads();
                if (act) {
                    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
                    for (int j = lane; j < im.rowraw; j += group) {
                        const int x = cur[j ^ sw], av = j >= bpp ? cur[(j - bpp) ^ sw] : 0;
                        const int bv = r > 0 ? up[j ^ sw] : 0, cv = (r > 0 && j >= bpp) ? up[(j - bpp) ^ sw] : 0;
                        c0 += filter_cost(x);
                        c1 += filter_cost(filtered(1, x, av, bv, cv));
                        c2 += filter_cost(filtered(2, x, av, bv, cv));
                        c3 += filter_cost(filtered(3, x, av, bv, cv));
                        c4 += filter_cost(filtered(4, x, av, bv, cv));
                    }
                    atomicAdd(&sums[0], c0); atomicAdd(&sums[1], c1); atomicAdd(&sums[2], c2); atomicAdd(&sums[3], c3); atomicAdd(&sums[4], c4);
                }
                __syncthreads();
                type = 0;
                for (int t = 1; t < 5; ++t)
                    if (sums[t] < sums[type]) type = t;                      // ties go to the lowest type
            }
            if (act) {
                const int at = rr * rowbytes;
                if (lane == 0) s_in[png_pad(at)] = (unsigned char)type;
                for (int j = lane; j < im.rowraw; j += group) {
                    const int x = cur[j ^ sw], av = j >= bpp ? cur[(j - bpp) ^ sw] : 0;
                    const int bv = r > 0 ? up[j ^ sw] : 0, cv = (r > 0 && j >= bpp) ? up[(j - bpp) ^ sw] : 0;
                    s_in[png_pad(at + 1 + j)] = (unsigned char)filtered(type, x, av, bv, cv);
                }
            }
        }
    }
    __syncthreads();

    // ---- this lane's chunk: Adler terms, run flags -------------------------------------------------------------------------------
    const int c0 = tid * kPngChunk < len ? tid * kPngChunk : len;
    const int c1 = c0 + kPngChunk < len ? c0 + kPngChunk : len;
    int first_flag = len, last_flag = -1;
    {
        uint32_t s1 = 0, s2 = 0;
        int prev = c0 > 0 ? s_in[png_pad(c0 - 1)] : -1;
        for (int i = c0; i < c1; ++i) {
            const int d = s_in[png_pad(i)];
            s1 += (uint32_t)d;
            s2 += (uint32_t)(len - i) * (uint32_t)d;
            if (d != prev) { if (first_flag == len) first_flag = i; last_flag = i; }
            prev = d;
        }
        if (c0 < c1) { atomicAdd(&sh.adler[0], s1); atomicAdd(&sh.adler[1], s2 % 65521u); }
    }
    block_scan<false>(last_flag, sh.scan);
    const int carry = tid > 0 ? sh.scan[tid - 1] : 0;
    __syncthreads();
    block_scan<true>(first_flag, sh.scan);
    const int after = tid + 1 < kPngThreads ? sh.scan[tid + 1] : len;
    __syncthreads();

    // ---- histogram ---------------------------------------------------------------------------------------------------------------
    walk_tokens(s_in, c0, c1, len, carry, after, [&](int, int t, int v) {
        if (t == 1) {
            atomicAdd(&sh.hist[v], 1u);
        } else {
            int symbol, eb, ev;
            png_length_symbol(t, &symbol, &eb, &ev);
            atomicAdd(&sh.hist[symbol], 1u);
        }
    });
    __syncthreads();

    // ---- the code.  Sorting by rank (every lane compares its symbols with all), the lengths on one lane, the canonical codes per
    // symbol, the code-length code on one lane, the header's lengths by a prefix sum ------------------------------------------------
    for (int s = tid; s < kPngMaxSymbols; s += kPngThreads) {
        const uint32_t f = s < 286 ? sh.hist[s] : 0u;
        sh.len[s] = 0;
        if (f) {
            int rank = 0;
            for (int o = 0; o < 286; ++o) {
                const uint32_t fo = sh.hist[o];
                rank += (fo != 0u && (fo < f || (fo == f && o < s))) ? 1 : 0;
            }
            sh.work[rank] = f;
            sh.work[kPngMaxSymbols + rank] = (uint32_t)s;
            atomicAdd(reinterpret_cast<uint32_t*>(&sh.used), 1u);
        }
    }
    __syncthreads();
    if (tid == 0)                                            // (two symbols at least: a literal and the end of block)
        png_code_lengths_sorted(sh.work, sh.work + kPngMaxSymbols, sh.used, 15, sh.len, reinterpret_cast<int*>(sh.work + 2 * kPngMaxSymbols));
    __syncthreads();
    for (int s = tid; s < 286; s += kPngThreads) {
        const int l = sh.len[s];
        atomicAdd(&sh.cl_freq[l], 1u);
        if (l) {
            atomicAdd(&sh.count[l], 1u);
            atomicMax(&sh.hlit, s + 1);
        }
    }
    __syncthreads();
    for (int s = tid; s < kPngMaxSymbols; s += kPngThreads) {
        const int l = s < 286 ? sh.len[s] : 0;
        uint32_t cd = 0;
        if (l) {
            uint32_t c = 0;                                  // the first code of length l, then this symbol's place among them
            for (int b = 1; b <= l; ++b) c = (c + (b > 1 ? sh.count[b - 1] : 0u)) << 1;
            for (int o = 0; o < s; ++o) c += sh.len[o] == l ? 1u : 0u;
            cd = bit_reverse(c, l) | (uint32_t)l << 16;
        }
        sh.code[s] = cd;
    }
    if (tid == 0) {
        // the code-length code over the lengths 0 .. 15 (no repeat codes), 7 bits at most, complete
        const int hlit = sh.hlit;
        sh.cl_freq[0] -= (uint32_t)(286 - hlit);             // the trimmed trailing zeros are not sent
        sh.cl_freq[1]++;                                     // the one distance code, 1 bit
        png_code_lengths(sh.cl_freq, 19, 7, sh.cl_len, sh.work);
        int used = 0, only = 0;
        for (int i = 0; i < 19; ++i)
            if (sh.cl_len[i]) { ++used; only = i; }
        if (used == 1) sh.cl_len[only == 0 ? 1 : 0] = 1;
        uint32_t* __restrict__ next = sh.work;               // [8]: the next code of each length
        for (int b = 0; b < 8; ++b) next[b] = 0;
        for (int i = 0; i < 19; ++i) next[sh.cl_len[i]]++;
        uint32_t c = 0, before = 0;
        for (int b = 1; b < 8; ++b) { c = (c + before) << 1; before = next[b]; next[b] = c; }
        for (int i = 0; i < 19; ++i) {
            const int l = sh.cl_len[i];
            sh.cl_code[i] = l ? bit_reverse(next[l]++, l) : 0u;
        }
        unsigned long long acc = 0;
        int nb = 0, w = 0;
        auto put = [&](uint32_t v, int n) {
            acc |= (unsigned long long)v << nb;
            nb += n;
            if (nb >= 32) { out_word(s_out, w++) = (uint32_t)acc; acc >>= 32; nb -= 32; }
        };
        put(0u, 1); put(2u, 2);                              // not final, dynamic
        put((uint32_t)(hlit - 257), 5); put(0u, 5); put(15u, 4);
        for (int i = 0; i < 19; ++i) put(sh.cl_len[d_cl_order[i]], 3);
        if (nb) out_word(s_out, w) = (uint32_t)acc;
        sh.hdr_bits = 32 * w + nb;
    }
    __syncthreads();
    {
        // the hlit literal/length lengths and the distance code's, two per lane
        const int hlit = sh.hlit, j = 2 * tid;
        const int x0 = j < hlit ? sh.len[j] : 1, x1 = j + 1 < hlit ? sh.len[j + 1] : 1;
        const int n0 = j <= hlit ? sh.cl_len[x0] : 0, n1 = j + 1 <= hlit ? sh.cl_len[x1] : 0;
        const int incl = block_sum_scan(n0 + n1, sh.scan);
        const int at = sh.hdr_bits + incl - n0 - n1;
        const int all = sh.scan[kPngThreads - 1];
        if (n0) or_bits(s_out, at, sh.cl_code[x0]);
        if (n1) or_bits(s_out, at + n0, sh.cl_code[x1]);
        __syncthreads();
        if (tid == 0) sh.hdr_bits += all;
        __syncthreads();
    }

    // ---- token bits: a prefix sum of code lengths ----------------------------------------------------------------------------------
    int bits = 0;
    walk_tokens(s_in, c0, c1, len, carry, after, [&](int, int t, int v) {
        if (t == 1) {
            bits += (int)(sh.code[v] >> 16);
        } else {
            int symbol, eb, ev;
            png_length_symbol(t, &symbol, &eb, &ev);
            bits += (int)(sh.code[symbol] >> 16) + eb + 1;
        }
    });
    const int incl = block_sum_scan(bits, sh.scan);
    const int token_bits = sh.scan[kPngThreads - 1];
    const int eob_at = sh.hdr_bits + token_bits;
    const int dyn_bits = eob_at + (int)(sh.code[256] >> 16);
    const int dyn_bytes = (dyn_bits & 7) ? (dyn_bits + 3 + 7) / 8 + 4 : dyn_bits / 8;      // an empty stored block brings it to a byte
    const bool stored = dyn_bytes >= 5 + len;
    const int m = stored ? 5 + len : dyn_bytes;
    __syncthreads();

    if (!stored) {
        int at = sh.hdr_bits + incl - bits;
        walk_tokens(s_in, c0, c1, len, carry, after, [&](int, int t, int v) {
            if (t == 1) {
                const uint32_t cd = sh.code[v];
                or_bits(s_out, at, cd & 0xffffu);
                at += (int)(cd >> 16);
            } else {
                int symbol, eb, ev;
                png_length_symbol(t, &symbol, &eb, &ev);
                const uint32_t cd = sh.code[symbol];
                const int l = (int)(cd >> 16);
                or_bits(s_out, at, (cd & 0xffffu) | (uint32_t)ev << l);          // code, extra bits, then the distance code: one 0 bit
                at += l + eb + 1;
            }
        });
        if (tid == 0) {
            or_bits(s_out, eob_at, sh.code[256] & 0xffffu);
            if (dyn_bits & 7) {                                                    // 000, zeros to the byte, LEN = 0, NLEN = 0xffff
                const int b = (dyn_bits + 3 + 7) / 8;
                or_bits(s_out, 8 * (b + 2), 0xffffu);
            }
        }
    } else {
        for (int i = tid; i < 5 + len; i += kPngThreads) {
            unsigned v;
            switch (i) {
            case 0: v = 0; break;
            case 1: v = (unsigned)len & 255u; break;
            case 2: v = (unsigned)len >> 8; break;
            case 3: v = ~(unsigned)len & 255u; break;
            case 4: v = (~(unsigned)len >> 8) & 255u; break;
            default: v = s_in[png_pad(i - 5)];
            }
            s_out[png_pad(i)] = (unsigned char)v;
        }
    }
    __syncthreads();

    // ---- CRC-32 register of the m bytes from 0: 136 bytes per lane of the bytes right-aligned in 256 * 136, then a tree ------------
    {
        const int lead = kPngThreads * kPngCrcChunk - m;
        uint32_t c = 0;
        for (int v = tid * kPngCrcChunk; v < (tid + 1) * kPngCrcChunk; ++v) {
            const int i = v - lead;
            if (i >= 0) c = sh.crc_table[(c ^ s_out[png_pad(i)]) & 255u] ^ (c >> 8);
        }
        sh.crc[tid] = c;
        if (tid == kPngThreads - 1) sh.xpow = crc_xpow8((uint64_t)m);
        for (int l = 0; l < 8; ++l) {
            __syncthreads();
            if ((tid & ((2 << l) - 1)) == 0) sh.crc[tid] = crc_mul(sh.crc[tid], a.xpow_tree[l]) ^ sh.crc[tid + (1 << l)];
        }
        __syncthreads();
    }

    uint32_t* __restrict__ slot = reinterpret_cast<uint32_t*>(a.slots + (long long)seg * kPngSlot);
    for (int w = tid; w < (m + 3) / 4; w += kPngThreads) slot[w] = out_word(s_out, w);
    if (tid == 0) {
        uint32_t* __restrict__ meta = a.meta + (long long)seg * kPngMetaWords;
        meta[0] = (uint32_t)m;
        meta[1] = sh.adler[0] % 65521u;
        meta[2] = sh.adler[1] % 65521u;
        meta[3] = sh.crc[0];
        meta[4] = sh.xpow;
        meta[5] = 0;
    }
}

// a few header and trailer bytes: bit by bit, no table
__device__ __forceinline__ uint32_t crc_bytes(uint32_t c, const unsigned char* p, int n) {
    for (int i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
    return c;
}

__device__ __forceinline__ void put_be32(unsigned char* p, uint32_t v) {
    p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

__global__ __launch_bounds__(kPngThreads) void k_png_finish(const PngParams a) {
    const int tid = threadIdx.x;
    if (tid >= a.n_images) return;
    const PngImg& im = a.img[tid];
    unsigned char* __restrict__ file = a.dst + im.dst_off;
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; ++i) file[i] = sig[i];
    unsigned char* p = file + 8;
    put_be32(p, 13u);
    p[4] = 'I'; p[5] = 'H'; p[6] = 'D'; p[7] = 'R';
    put_be32(p + 8, (uint32_t)im.w);
    put_be32(p + 12, (uint32_t)im.h);
    p[16] = (unsigned char)im.depth; p[17] = (unsigned char)im.colour; p[18] = 0; p[19] = 0; p[20] = 0;
    put_be32(p + 21, crc_bytes(0xffffffffu, p + 4, 17) ^ 0xffffffffu);
    p += 25;                                                         // the IDAT frame: length, tag, zlib header
    p[4] = 'I'; p[5] = 'D'; p[6] = 'A'; p[7] = 'T'; p[8] = 0x78; p[9] = 0x01;
    uint32_t c = crc_bytes(0xffffffffu, p + 4, 6);
    long long off = 0;
    uint32_t A = 1, B = 0;
    const int rowbytes = im.rowraw + 1;
    for (int j = 0; j < im.nseg; ++j) {
        uint32_t* __restrict__ meta = a.meta + (long long)(im.seg_base + j) * kPngMetaWords;
        const int rows = im.h - j * im.rps < im.rps ? im.h - j * im.rps : im.rps;
        const uint32_t n = (uint32_t)(rows * rowbytes);
        *reinterpret_cast<long long*>(meta + 6) = im.dst_off + 43 + off;
        off += meta[0];
        B = (uint32_t)((B + (unsigned long long)(n % 65521u) * A + meta[2]) % 65521u);
        A = (A + meta[1]) % 65521u;
        c = crc_mul(c, meta[4]) ^ meta[3];
    }
    put_be32(p, (uint32_t)(2 + off + 5 + 4));
    unsigned char* t = file + 43 + off;                              // the final empty stored block, Adler-32, the chunk's CRC
    t[0] = 1; t[1] = 0; t[2] = 0; t[3] = 0xff; t[4] = 0xff;
    put_be32(t + 5, B << 16 | A);
    c = crc_bytes(c, t, 9);
    put_be32(t + 9, c ^ 0xffffffffu);
    t += 13;
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) t[i] = iend[i];
    a.sizes[tid] = off + kPngFixedBytes;
}

__global__ __launch_bounds__(kPngThreads) void k_png_gather(const PngParams a) {
    const int seg = blockIdx.x, tid = threadIdx.x;
    const uint32_t* __restrict__ meta = a.meta + (long long)seg * kPngMetaWords;
    const int m = (int)meta[0];
    unsigned char* __restrict__ out = a.dst + *reinterpret_cast<const long long*>(meta + 6);
    const unsigned char* __restrict__ slot = a.slots + (long long)seg * kPngSlot;
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(slot);
    // bytes up to the file's first dword boundary one by one, then whole dwords put together from two of the slot's, then the tail
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(out) & 3)) & 3);
    if (head > m) head = m;
    const int body = (m - head) / 4;
    if (tid < head) out[tid] = slot[tid];
    uint32_t* __restrict__ out_words = reinterpret_cast<uint32_t*>(out + head);
    const int shift = 8 * head;
    for (int w = tid; w < body; w += kPngThreads) {
        const unsigned long long two = (unsigned long long)words[w] | (unsigned long long)words[w + 1] << 32;
        out_words[w] = (uint32_t)(two >> shift);
    }
    const int done = head + 4 * body;
    if (tid < m - done) out[done + tid] = slot[done + tid];
}

static bool png_misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

static bool png_overlaps(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

struct PngPlan {
    long long offset[INERF_PNG_MAX_IMAGES], capacity[INERF_PNG_MAX_IMAGES], total, n_segs;
    PngImg img[INERF_PNG_MAX_IMAGES];
};

// the images' segments, offsets (multiples of 16) and capacities; negative: an error code
static long long png_plan(const inerf_png_args* args, PngPlan* plan) {
    if (!args || args->n_images < 0 || args->n_images > INERF_PNG_MAX_IMAGES) return INERF_E_INVALID;
    long long at = 0, segs = 0;
    for (int k = 0; k < args->n_images; ++k) {
        const inerf_png_image& im = args->images[k];
        if (im.height < 1 || im.width < 1 || (im.channels != 1 && im.channels != 3) || (im.bit_depth != 8 && im.bit_depth != 16) ||
            (im.bit_depth == 16 && im.channels != 1) || im.filter < INERF_PNG_FILTER_ADAPTIVE || im.filter > 4)
            return INERF_E_INVALID;
        const long long rowraw = (long long)im.width * im.channels * (im.bit_depth / 8);
        if (rowraw + 1 > kPngCap) return INERF_E_UNSUPPORTED;
        const int rps = (int)(kPngCap / (rowraw + 1));
        const long long nseg = ((long long)im.height + rps - 1) / rps;
        const long long capacity = kPngFixedBytes + (long long)im.height * (rowraw + 1) + 5 * nseg;
        if (segs + nseg > 0x7fffffffLL / kPngThreads) return INERF_E_UNSUPPORTED;
        PngImg& o = plan->img[k];
        o.src_off = im.src_offset; o.dst_off = at;
        o.h = im.height; o.w = im.width; o.rowraw = (int)rowraw;
        o.bpp = im.channels * (im.bit_depth / 8); o.swap16 = im.bit_depth == 16 ? 1 : 0;
        o.colour = im.channels == 3 ? 2 : 0; o.depth = im.bit_depth; o.filter = im.filter;
        o.rps = rps; o.nseg = (int)nseg; o.seg_base = (int)segs;
        o.group = rowraw > 32 ? 64 : 8;
        plan->offset[k] = at; plan->capacity[k] = capacity;
        at += (capacity + 15) / 16 * 16;
        segs += nseg;
    }
    plan->total = at; plan->n_segs = segs;
    return at;
}

static long long png_workspace(long long n_segs) { return n_segs * (kPngMetaWords * 4 + kPngSlot); }

}  // namespace inerf

extern "C" int64_t inerf_png_layout(inerf_png_args* args) {
    inerf::PngPlan plan;
    const long long total = inerf::png_plan(args, &plan);
    if (total < 0) return total;
    for (int k = 0; k < args->n_images; ++k) {
        args->images[k].dst_offset = plan.offset[k];
        args->images[k].dst_capacity = plan.capacity[k];
    }
    return total;
}

extern "C" int64_t inerf_png_workspace_bytes(const inerf_png_args* args) {
    inerf::PngPlan plan;
    const long long total = inerf::png_plan(args, &plan);
    return total < 0 ? total : inerf::png_workspace(plan.n_segs);
}

extern "C" int inerf_png_code_lengths(const uint32_t* freq, int n, int limit, unsigned char* lengths) {
    if (!freq || !lengths || n < 1 || n > inerf::kPngMaxSymbols || limit < 1 || limit > 15) return INERF_E_INVALID;
    int used = 0;
    unsigned long long sum = 0;
    for (int s = 0; s < n; ++s) { used += freq[s] != 0; sum += freq[s]; }
    if (used > (1 << limit) || sum > 0xffffffffull) return INERF_E_INVALID;
    uint32_t work[2 * inerf::kPngMaxSymbols + 40];
    inerf::png_code_lengths(freq, n, limit, lengths, work);
    return INERF_OK;
}

extern "C" int inerf_png_encode(const inerf_png_args* args, void* stream) {
    using namespace inerf;
    PngPlan plan;
    const long long total = png_plan(args, &plan);
    if (total < 0) return (int)total;
    if (args->src_bytes < 0) return INERF_E_INVALID;
    for (int k = 0; k < args->n_images; ++k) {
        const inerf_png_image& im = args->images[k];
        if (im.dst_offset != plan.offset[k] || im.dst_capacity != plan.capacity[k]) return INERF_E_INVALID;      // inerf_png_layout was not called
        if (im.src_offset < 0 || im.src_offset > args->src_bytes || (long long)im.height * plan.img[k].rowraw > args->src_bytes - im.src_offset)
            return INERF_E_INVALID;
    }
    if (args->n_images == 0) return INERF_OK;
    if (!args->src || !args->dst || !args->sizes || args->dst_bytes < total) return INERF_E_INVALID;
    if (png_misaligned(args->dst, 16) || png_misaligned(args->sizes, 8)) return INERF_E_INVALID;
    const long long need = png_workspace(plan.n_segs), sizes_bytes = 8LL * args->n_images;
    if (!args->workspace || args->workspace_bytes < need) return INERF_E_WORKSPACE;
    if (png_misaligned(args->workspace, 16)) return INERF_E_INVALID;
    if (png_overlaps(args->dst, total, args->src, args->src_bytes) || png_overlaps(args->sizes, sizes_bytes, args->src, args->src_bytes) ||
        png_overlaps(args->workspace, need, args->src, args->src_bytes) || png_overlaps(args->dst, total, args->sizes, sizes_bytes) ||
        png_overlaps(args->dst, total, args->workspace, need) || png_overlaps(args->sizes, sizes_bytes, args->workspace, need))
        return INERF_E_INVALID;

    PngParams a{};
    a.src = args->src; a.dst = args->dst; a.sizes = reinterpret_cast<long long*>(args->sizes);
    a.meta = static_cast<uint32_t*>(args->workspace);
    a.slots = static_cast<unsigned char*>(args->workspace) + plan.n_segs * kPngMetaWords * 4;
    a.n_images = args->n_images; a.n_segs = (int)plan.n_segs;
    for (int l = 0; l < 8; ++l) a.xpow_tree[l] = crc_xpow8((uint64_t)kPngCrcChunk << l);
    for (int k = 0; k < args->n_images; ++k) a.img[k] = plan.img[k];
    const size_t lds = kPngInBytes + kPngOutBytes + sizeof(PngShared);
    static PerDeviceOnce attr_set;
    if (attr_set.first()) {                            // more than 64 KiB of LDS per workgroup
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_png_segment), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return record(e);
        attr_set.mark();
    }
    hipLaunchKernelGGL(k_png_segment, dim3((unsigned)plan.n_segs), dim3(kPngThreads), lds, (hipStream_t)stream, a);
    int rc = record(hipGetLastError());
    if (rc != INERF_OK) return rc;
    hipLaunchKernelGGL(k_png_finish, dim3(1), dim3(kPngThreads), 0, (hipStream_t)stream, a);
    rc = record(hipGetLastError());
    if (rc != INERF_OK) return rc;
    hipLaunchKernelGGL(k_png_gather, dim3((unsigned)plan.n_segs), dim3(kPngThreads), 0, (hipStream_t)stream, a);
    return record(hipGetLastError());
}
