// draws.h - the training step's random variates, counter-based: a sample's draw is a pure function of
// (seed, step, stream, global ray index, sample index), so it does not depend on chunking, on the split of the rays over ranks or on
// call order, and a backward pass regenerates what its forward drew.  The layout is part of the C ABI (include/inerf.h, "Training
// draws"); tests/_draws.py restates it in NumPy.
//
//   Philox4x32-10 (Random123): key = {seed lo, seed hi}, counter = {ray, block | stream << 16, step lo, step hi}, block = sample >> 2;
//   the four output words belong to samples 4 block .. 4 block + 3.
//   uniform (streams 0 jitter, 2 u):  (word >> 8) * 2^-24                       in [0, 1), torch.rand's fp32 lattice
//   normal  (streams 1 coarse noise, 3 fine noise): Box-Muller on the word pairs (0, 1) and (2, 3):
//       u1 = ((w_even >> 9) + 1) * 2^-23 in (0, 1],  u2 = (w_odd >> 8) * 2^-24,  r = sqrtf(-2 logf(u1)),  theta = 2 pi u2
//       even sample of the pair: r cosf(theta), odd sample: r sinf(theta)       |z| <= sqrt(46 ln 2) < 5.65
// Host part: plain C++; device part: only when compiled as HIP.
#pragma once
#include <stdint.h>

#include "layout.h"

namespace inerf {

// what a drawing kernel receives by value
struct DrawParams {
    unsigned key0, key1;           // seed lo / hi
    unsigned ray_base;             // global index of the launch's first ray
    unsigned stream;               // INERF_DRAW_STREAM_*
    long long step;                // used when step_dev is null
    const long long* step_dev;     // device-resident step (wins when not null); never written by a drawing kernel
    float noise_std;
};

// Validation shared by every drawn entry point: INERF_OK, or the error to return before anything is enqueued.
// `allowed_flags`: the INERF_DRAW_* bits that mean something to the calling entry point; any other bit is an error.
inline int draw_check(const inerf_draw_args* d, int64_t n_rays, uint32_t allowed_flags) {
    if (!d || n_rays < 0) return INERF_E_INVALID;
    if (reinterpret_cast<uintptr_t>(d->step_dev) & 7u) return INERF_E_INVALID;
    if (d->flags & ~allowed_flags) return INERF_E_INVALID;
    if (!(d->noise_std >= 0.0f) || d->noise_std > 3.0e38f) return INERF_E_INVALID;        // NaN, negative, infinite
    if (d->ray_base > (1ull << 32) || d->ray_base + (uint64_t)n_rays > (1ull << 32)) return INERF_E_UNSUPPORTED;   // the counter's ray word is 32 bits
    return INERF_OK;
}

inline DrawParams draw_params(const inerf_draw_args& d, unsigned stream) {
    DrawParams p;
    p.key0 = (unsigned)(d.seed & 0xffffffffull);
    p.key1 = (unsigned)(d.seed >> 32);
    p.ray_base = (unsigned)d.ray_base;
    p.stream = stream;
    p.step = (long long)d.step;
    p.step_dev = reinterpret_cast<const long long*>(d.step_dev);
    p.noise_std = d.noise_std;
    return p;
}

#ifdef __HIP__
}  // namespace inerf
#include <hip/hip_runtime.h>
namespace inerf {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
    constexpr unsigned kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
        const unsigned hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kW0;
        k1 += kW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the launch's step: wave-uniform, read once per thread
__device__ __forceinline__ long long draw_step(const DrawParams& p) { return p.step_dev ? *p.step_dev : p.step; }

// the Philox block that holds `sample` of local ray `ray`
__device__ __forceinline__ void draw_block(const DrawParams& p, long long step, long long ray, int sample, unsigned (&w)[4]) {
    philox4x32_10(p.ray_base + (unsigned)ray, (unsigned)(sample >> 2) | (p.stream << 16), (unsigned)((unsigned long long)step & 0xffffffffull),
                  (unsigned)((unsigned long long)step >> 32), p.key0, p.key1, w);
}

__device__ __forceinline__ float draw_uniform(const DrawParams& p, long long step, long long ray, int sample) {
    unsigned w[4];
    draw_block(p, step, ray, sample, w);
    const unsigned word = (sample & 2) ? ((sample & 1) ? w[3] : w[2]) : ((sample & 1) ? w[1] : w[0]);
    return __fmul_rn((float)(word >> 8), 5.9604644775390625e-8f);                 // 24 bits * 2^-24: exact
}

// standard normal; the caller scales it (one rounding: __fmul_rn(z, noise_std), as randn * std)
__device__ __forceinline__ float draw_normal(const DrawParams& p, long long step, long long ray, int sample) {
    unsigned w[4];
    draw_block(p, step, ray, sample, w);
    const unsigned we = (sample & 2) ? w[2] : w[0], wo = (sample & 2) ? w[3] : w[1];
    const float u1 = __fmul_rn((float)((we >> 9) + 1u), 1.1920928955078125e-7f);  // (23 bits + 1) * 2^-23: exact, in (0, 1]
    const float u2 = __fmul_rn((float)(wo >> 8), 5.9604644775390625e-8f);
    const float r = sqrtf(__fmul_rn(-2.0f, logf(u1)));
    const float theta = __fmul_rn(6.2831854820251465f, u2);                        // fp32(2 pi)
    float sn, cs;
    sincosf(theta, &sn, &cs);
    return __fmul_rn(r, (sample & 1) ? sn : cs);
}

__device__ __forceinline__ float draw_noise(const DrawParams& p, long long step, long long ray, int sample) {
    return __fmul_rn(draw_normal(p, step, ray, sample), p.noise_std);
}

#endif  // __HIP__

}  // namespace inerf
