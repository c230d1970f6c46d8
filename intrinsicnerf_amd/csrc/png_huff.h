// png_huff.h - the serial pieces of the PNG encoder (csrc/png.hip) that the host can run too: length-limited Huffman code lengths,
// the token rule of a run of equal bytes, DEFLATE's length symbols and CRC-32 polynomial arithmetic.  Integer only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INERF_PNG_HD __host__ __device__ inline
#else
#define INERF_PNG_HD inline
#endif

namespace inerf {

constexpr int kPngMaxSymbols = 288;      // the literal/length alphabet has 286 used symbols; 288 keeps arrays word-sized

// Code lengths of a minimum-redundancy prefix code, no length above `limit`, for m >= 2 symbols given SORTED: a[i] the count of
// sym[i], ascending by (count, symbol).  Writes lengths[sym[i]] only; `a` is overwritten; `num`: 34 ints of scratch.
// Method: the in-place two-pass length computation of Moffat and Katajainen ("In-place calculation of minimum-redundancy codes",
// 1995); where the deepest leaf exceeds the limit, the lengths' histogram is clamped and repaired - one code leaves the limit's level
// and one shorter code is split into two, which takes exactly 2^-limit off the Kraft sum, until it is 1 - and the lengths are handed
// out again, longest to the rarest symbol.  The result is complete (Kraft sum exactly 1) and the Huffman optimum whenever that fits
// the limit.  Needs 2^limit >= m, limit <= 15, and the sum of the counts in 32 bits.
INERF_PNG_HD void png_code_lengths_sorted(uint32_t* a, const uint32_t* sym, int m, int limit, unsigned char* lengths, int* num) {
    // Moffat-Katajainen: parents, then depths of the internal nodes, then depths of the leaves
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; ++next) {
        if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; } else a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; } else a[next] += a[leaf++];
    }
    a[m - 2] = 0;
    for (int next = m - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, next = m - 1;
    root = m - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)a[root] == dpth) { ++used; --root; }
        while (avbl > used) { a[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used; ++dpth; used = 0;
    }
    // a[i]: the length of sorted slot i, longest first (a[0] belongs to the rarest symbol)
    if ((int)a[0] <= limit) {
        for (int i = 0; i < m; ++i) lengths[sym[i]] = (unsigned char)a[i];
        return;
    }
    for (int i = 0; i <= 32; ++i) num[i] = 0;
    for (int i = 0; i < m; ++i) num[(int)a[i] < limit ? (int)a[i] : limit]++;
    uint32_t total = 0;
    for (int i = limit; i > 0; --i) total += (uint32_t)num[i] << (limit - i);
    while (total > (1u << limit)) {
        num[limit]--;
        for (int i = limit - 1; i > 0; --i)
            if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        --total;
    }
    int at = 0;
    for (int len = limit; len > 0; --len)
        for (int j = 0; j < num[len]; ++j) lengths[sym[at++]] = (unsigned char)len;
}

// ... over freq[0 .. n) in any order: a zero count gives length 0, one used symbol length 1 (an incomplete code: the caller decides
// what to do with it), two or more the code above, ties broken by the symbol index (a shell sort on (count, symbol) first).
// `work`: 2 * n + 34 words of scratch; n <= kPngMaxSymbols.
INERF_PNG_HD void png_code_lengths(const uint32_t* freq, int n, int limit, unsigned char* lengths, uint32_t* work) {
    uint32_t* a = work;            // counts, ascending
    uint32_t* sym = work + n;      // the symbol of each sorted slot
    int m = 0;
    for (int s = 0; s < n; ++s) {
        lengths[s] = 0;
        if (freq[s]) { a[m] = freq[s]; sym[m] = (uint32_t)s; ++m; }
    }
    if (m == 0) return;
    if (m == 1) { lengths[sym[0]] = 1; return; }
    for (int gap = m / 2; gap > 0; gap = gap == 2 ? 1 : gap * 5 / 11) {
        for (int i = gap; i < m; ++i) {
            const uint32_t ka = a[i], ks = sym[i];
            int j = i;
            for (; j >= gap && (a[j - gap] > ka || (a[j - gap] == ka && sym[j - gap] > ks)); j -= gap) { a[j] = a[j - gap]; sym[j] = sym[j - gap]; }
            a[j] = ka; sym[j] = ks;
        }
    }
    png_code_lengths_sorted(a, sym, m, limit, lengths, reinterpret_cast<int*>(work + 2 * n));
}

// The token that starts at byte `off` of a run of `len` equal bytes: 0 none (the byte lies inside a match), 1 a literal, else the
// length (3 .. 258) of a distance-1 match.  A run of 4 or more is one literal and matches over the other len - 1 bytes: 258s, then
// the remainder r; where r is 1 or 2 the last 258 gives up 3 - r bytes so that the final match is a 3.
INERF_PNG_HD int png_run_token(int off, int len) {
    if (len < 4 || off == 0) return 1;
    const int m = len - 1, q = m / 258, r = m % 258, o = off - 1, k = o / 258, rem = o % 258;
    if (r == 0) return rem == 0 ? 258 : 0;
    if (r >= 3) return rem == 0 ? (k < q ? 258 : r) : 0;
    const int last = 258 * q - (3 - r);          // q >= 1 here
    if (o == last) return 3;
    if (o > last || rem != 0) return 0;
    return k < q - 1 ? 258 : 258 - (3 - r);
}

// DEFLATE's length code of a match length 3 .. 258: the symbol (257 .. 285), the number of extra bits and their value
INERF_PNG_HD void png_length_symbol(int len, int* symbol, int* extra_bits, int* extra) {
    if (len == 258) { *symbol = 285; *extra_bits = 0; *extra = 0; return; }
    const int l = len - 3;
    if (l < 8) { *symbol = 257 + l; *extra_bits = 0; *extra = 0; return; }
    int e = 1;
    while ((l >> (e + 3)) != 0) ++e;             // e = floor(log2(l)) - 2
    *symbol = 261 + 4 * e + ((l >> e) & 3);
    *extra_bits = e;
    *extra = l & ((1 << e) - 1);
}

// CRC-32 (reflected, polynomial 0xEDB88320) as arithmetic on polynomials mod P: bit 31 of a word is x^0.
// The running register c after n more bytes is c * x^(8n) + (the register those bytes give from 0), so pieces hashed apart combine.
constexpr uint32_t kCrcPoly = 0xEDB88320u;

INERF_PNG_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

// x^(8 * bytes) mod P
INERF_PNG_HD uint32_t crc_xpow8(uint64_t bytes) {
    uint32_t r = 0x80000000u, base = 0x00800000u;      // 1, x^8
    for (; bytes; bytes >>= 1) {
        if (bytes & 1) r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}

INERF_PNG_HD uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i >> 1) ^ ((i & 1u) ? kCrcPoly : 0u);
    return i;
}

}  // namespace inerf
