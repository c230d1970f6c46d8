// sem_label.h - the label and entropy of rows of semantic logits, one 64-row tile per wave: sem_tile() is the ONE place the label rule
// is evaluated - by inerf_sem_maps and inerf_eval_accumulate (eval.hip, whose header comment states the rule and the row-to-lane
// mapping) and by the semantic mode of inerf_vertex_colours (mesh.hip), so all three give the same label.
#pragma once
#include <hip/hip_runtime.h>

namespace inerf {

struct SemIO {
    const float* logits;
    long long ld;
    int n_classes;
    float* label;
    long long label_stride;
    float* entropy;
    long long entropy_stride;
};

// rows row0 .. row0 + 63 (those below n): on return lane r holds row row0 + r's label and entropy.  The whole wave calls it.
template <int G>
__device__ __forceinline__ void sem_tile(const SemIO& io, long long row0, long long n, int lane, float& label, float& entropy) {
    constexpr int kRows = 64 / G;                   // rows per step
    constexpr int kMax = G == 64 ? 4 : 1;           // logits per lane: C <= G below 64 lanes, C <= 240 < 4 * 64 at 64
    const int sub = lane & (G - 1), grp = lane / G;
    const int C = io.n_classes;
    label = 0.f;
    entropy = 0.f;
    // no early exit: the steps are independent chains of load -> shuffles -> expf -> shuffles -> log, and a wave has little company
    // on its SIMD (a 320x240 frame is 1 200 waves), so four of them are unrolled into one block for the scheduler to interleave
#pragma unroll 4
    for (int s = 0; s < G; ++s) {
        const long long row = row0 + (long long)s * kRows + grp;
        const bool live = row < n;
        const float* __restrict__ src = io.logits + row * io.ld;
        float x[kMax];
        float m = -INFINITY;
        int mi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < kMax; ++k) {
            const int c = sub + k * G;
            const bool have = live && c < C;
            x[k] = have ? src[c] : -INFINITY;
            const float v = x[k] != x[k] ? INFINITY : x[k];     // a NaN makes the maximum non-finite: label 0, entropy NaN
            if (have && v > m) { m = v; mi = c; }               // c rises with k: the first of equals stays
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const float om = __shfl_xor(m, off);
            const int oi = __shfl_xor(mi, off);
            if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
        }
        double S = 0.0, T = 0.0;
#pragma unroll
        for (int k = 0; k < kMax; ++k) {
            if (live && sub + k * G < C) {
                const float d = __fsub_rn(x[k], m);
                const float e = expf(d);
                S += (double)e;
                T += (double)e * (double)d;
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            S += __shfl_xor(S, off);
            T += __shfl_xor(T, off);
        }
        const bool bad = !(fabsf(m) < INFINITY);
        const float h = bad ? __builtin_nanf("") : (float)(log(S) - T / S);
        const float lab = bad ? 0.f : (float)mi;
        const int from = (lane % kRows) * G;                    // lane r of the tile: step r / kRows, group r % kRows
        const float vh = __shfl(h, from), vl = __shfl(lab, from);
        if (lane / kRows == s) { entropy = vh; label = vl; }
    }
}

// G of sem_tile for C classes: min(64, pow2ceil(C))
static inline int lanes_per_row(int C) {
    int g = 1;
    while (g < C && g < 64) g <<= 1;
    return g;
}

}  // namespace inerf
