// jpeg_tables.h - the constants of the baseline JPEG encoder (csrc/jpeg.hip), shared by host and device: the Annex K quantisation
// and Huffman tables of ITU-T T.81, the zigzag order, the fixed-point DCT matrix and the canonical codes derived at compile time.
// DESIGN.md section 3 ("Frame movies") has the arithmetic these constants belong to.
#ifndef INERF_JPEG_TABLES_H
#define INERF_JPEG_TABLES_H

#include <cstdint>

namespace inerf {

// T.81 Table K.1 / K.2, natural (row-major) order
constexpr unsigned char kJpegLumaBase[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kJpegChromaBase[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// the natural index of zigzag position k
constexpr unsigned char kJpegZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Tables K.3 - K.6: the number of codes of each length 1 .. 16, then the symbols in code order
constexpr unsigned char kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char kJpegDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// round(8192 * a(u) * cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u > 0) = 1 / 2: row u, column x
constexpr int kJpegDct[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},       {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},   {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},   {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},   {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
constexpr int kJpegPass1Shift = 9;       // the row pass keeps 4 fraction bits: (sum + 2^8) >> 9; |t| <= 5793 fits 16 bits
constexpr int kJpegPass2Shift = 14;      // the column pass keeps 3, as libjpeg's coefficients do: (sum + 2^13) >> 14; quantised by 8 q

// the worst case of one block's entropy-coded bits: a DC code of 11 bits with 11 value bits, 63 AC codes of 16 bits with 10 value bits
constexpr int kJpegBlockBits = 22 + 63 * 26;
constexpr int kJpegBlockBytes = (kJpegBlockBits + 7) / 8;          // 208; twice that once every byte is FF and stuffed

// the canonical codes of the tables above: code | length << 16, indexed by the symbol; [0]: luminance, [1]: chrominance
struct JpegCodes {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

constexpr JpegCodes jpeg_make_codes() {
    JpegCodes t{};
    for (int k = 0; k < 2; ++k) {
        uint32_t code = 0;
        int at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kJpegDcBits[k][len - 1]; ++i) t.dc[k][kJpegDcVals[at++]] = code++ | (uint32_t)len << 16;
            code <<= 1;
        }
        code = 0;
        at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kJpegAcBits[k][len - 1]; ++i) t.ac[k][kJpegAcVals[k][at++]] = code++ | (uint32_t)len << 16;
            code <<= 1;
        }
    }
    return t;
}

// libjpeg's quality rule: s = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((base * s + 50) / 100, 1, 255)
constexpr int jpeg_quant(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int t = (base * s + 50) / 100;
    return t < 1 ? 1 : (t > 255 ? 255 : t);
}

constexpr int jpeg_header_bytes(int channels) {
    // SOI 2, APP0 18, DQT 69 each, SOF0 10 + 3 c, DHT 33 (DC) + 183 (AC) per table pair, DRI 6, SOS 8 + 2 c
    return channels == 1 ? 2 + 18 + 69 + 13 + 216 + 6 + 10 : 2 + 18 + 138 + 19 + 432 + 6 + 14;
}
constexpr int kJpegLumaAt = 25, kJpegChromaAt = 94;                 // the tables' 64 bytes (zigzag order) inside the header

}  // namespace inerf
#endif
