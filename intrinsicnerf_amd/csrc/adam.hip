// adam.hip - the parameter update of both trainers: optimizer.step() of torch.optim.Adam (object_level/run_nerf.py:304,1019;
// SSR/training/trainer.py:842,991) for a LIST of fp32 tensors, as one streaming launch per table of kMaxTensors tensors.
//
// Arithmetic: torch's eager single-tensor Adam (torch/optim/adam.py, _single_tensor_adam) with weight_decay = 0, amsgrad = False,
// maximize = False.  Per tensor, in fp64 and rounded to fp32 once (the eager path forms them in Python doubles on the host):
//     bc1 = 1 - beta1^t        bc2_sqrt = sqrt(1 - beta2^t)        step_size = lr / bc1
// and per element in fp32, one rounding per operation (this file is compiled with -ffp-contract=off; division and square root
// are the correctly rounded forms) - except the one place where ATen itself fuses: its lerp kernels form weight * diff + self as
// ONE fused multiply-add (vec::fmadd on the CPU, a contracted expression on the GPU), so the explicit fma below is torch's m:
//     m = fma(1 - beta1, g - m, m)                                     exp_avg.lerp_(grad, 1 - beta1)   (weight < 0.5)
//     v = v * beta2 + ((1 - beta2) * g) * g                            exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
//     p = p + (-step_size) * (m / (sqrt(v) / bc2_sqrt + eps))          param.addcdiv_(exp_avg, denom, value = -step_size)
// t is the tensor's own step count, one fp32 on the device (torch's capturable layout), after its increment.
//
// Two kernels per table.  k_adam_advance (one workgroup) adds 1 to every step count; k_adam then streams.  Every workgroup of
// a tensor reads that tensor's count, so the count may only change where no workgroup of the same launch can still be reading
// it: advancing it inside the streaming launch would need a hand-over between workgroups (an atomic ticket or a flag), which
// this library does not use.  The stream orders the two launches; a captured graph holds them as two kernel nodes.
//
// The table (pointers, counts, first workgroup of every tensor) travels BY VALUE in the kernel arguments - no host-to-device copy,
// no allocation, nothing read on the host - which bounds it to the 4 KiB a dispatch packet's arguments may take: kMaxTensors = 72
// (both SSR networks, 36 + 36) is what fits.  A longer list takes ceil(n / 72) such pairs of launches.
//
// Memory: 28 B per element (read p, g, m, v; write p, m, v), no reuse: HBM bound.  A workgroup of 256 threads takes 2048
// consecutive elements, two float4 per thread and array, all eight loads issued before the first use.  16-byte accesses need
// p, g, m and v of a tensor to sit at the same offset from a 16-byte boundary (a view into a flat buffer may start on any
// 4-byte boundary): then up to three head elements and up to three tail elements go one float at a time; a tensor whose four
// arrays are misaligned differently goes one float per access throughout (still coalesced, 4 B per lane).
//
// No atomics, no cross-workgroup communication, every element written by exactly one thread: bit-identical from run to run and
// between a launch-by-launch step and a replayed one.  Every store below is an ordinary per-lane store.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout.h"

namespace inerf {

int record(hipError_t e);

namespace {

constexpr int kMaxTensors = 72;
constexpr int kThreads = 256;
constexpr int kVecPerThread = 2;                              // float4 per thread and array
constexpr int kChunk = kThreads * 4 * kVecPerThread;          // elements per workgroup

struct AdamTable {
    float* p[kMaxTensors];
    const float* g[kMaxTensors];
    float* m[kMaxTensors];
    float* v[kMaxTensors];
    float* step[kMaxTensors];
    long long count[kMaxTensors];
    int first_block[kMaxTensors + 1];     // workgroups [first_block[i], first_block[i + 1]) belong to tensor i
    int n;
    float lr;
    const float* lr_dev;
    double beta1, beta2;
    float one_minus_beta1, beta2_f, one_minus_beta2, eps;     // fp32(1 - beta1), fp32(beta2), fp32(1 - beta2), fp32(eps): what ATen's kernels receive
};
static_assert(sizeof(AdamTable) <= 4096, "the table must fit the kernel-argument segment");

struct Scalars {
    float bc2_sqrt, neg_step_size;
};

__device__ __forceinline__ void update(float& p, float g, float& m, float& v, const AdamTable& t, Scalars s) {
    m = __fmaf_rn(t.one_minus_beta1, g - m, m);
    v = v * t.beta2_f + (t.one_minus_beta2 * g) * g;
    const float denom = __fdiv_rn(__fsqrt_rn(v), s.bc2_sqrt) + t.eps;
    p = p + s.neg_step_size * __fdiv_rn(m, denom);
}

__device__ __forceinline__ void update_one(const AdamTable& t, int i, long long e, Scalars s) {
    float p = t.p[i][e], m = t.m[i][e], v = t.v[i][e];
    update(p, t.g[i][e], m, v, t, s);
    t.p[i][e] = p;
    t.m[i][e] = m;
    t.v[i][e] = v;
}

__global__ __launch_bounds__(128) void k_adam_advance(AdamTable t) {
    const int i = threadIdx.x;
    if (i < t.n) *t.step[i] = *t.step[i] + 1.0f;              // exact up to 2^24 steps
}

__global__ __launch_bounds__(kThreads) void k_adam(AdamTable t) {
    // which tensor: the last i with first_block[i] <= blockIdx.x (uniform: scalar loads from the argument segment)
    const int b = blockIdx.x;
    int lo = 0, hi = t.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first_block[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int i = lo;
    const long long chunk = b - t.first_block[i], count = t.count[i];
    float* __restrict__ P = t.p[i];
    const float* __restrict__ G = t.g[i];
    float* __restrict__ M = t.m[i];
    float* __restrict__ V = t.v[i];
    const unsigned mis = (unsigned)((uintptr_t)P & 15u);
    const bool vec = mis == ((uintptr_t)G & 15u) && mis == ((uintptr_t)M & 15u) && mis == ((uintptr_t)V & 15u);
    long long head = vec ? (long long)(((16u - mis) & 15u) >> 2) : 0;
    if (head > count) head = count;
    const long long begin = head + chunk * kChunk;             // 16-byte aligned element when `vec`
    long long end = begin + kChunk;
    if (end > count) end = count;
    const long long n_here = end > begin ? end - begin : 0;
    const long long n_vec = vec ? n_here / 4 : 0;              // whole float4 of this chunk

    // the loads go out first; the fp64 scalars are formed while they are in flight
    float4 p4[kVecPerThread], g4[kVecPerThread], m4[kVecPerThread], v4[kVecPerThread];
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
        const long long q = (long long)u * kThreads + threadIdx.x;
        if (q < n_vec) {
            const long long e = begin + 4 * q;
            p4[u] = *reinterpret_cast<const float4*>(P + e);
            g4[u] = *reinterpret_cast<const float4*>(G + e);
            m4[u] = *reinterpret_cast<const float4*>(M + e);
            v4[u] = *reinterpret_cast<const float4*>(V + e);
        }
    }

    __shared__ Scalars shared;
    if (threadIdx.x == 0) {
        const double step = (double)*t.step[i];                // already advanced (k_adam_advance)
        const double lr = t.lr_dev ? (double)*t.lr_dev : (double)t.lr;
        const double bc1 = 1.0 - pow(t.beta1, step), bc2 = 1.0 - pow(t.beta2, step);
        shared.bc2_sqrt = (float)sqrt(bc2);
        shared.neg_step_size = (float)-(lr / bc1);
    }
    __syncthreads();
    const Scalars s = shared;

#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
        const long long q = (long long)u * kThreads + threadIdx.x;
        if (q < n_vec) {
            const long long e = begin + 4 * q;
            update(p4[u].x, g4[u].x, m4[u].x, v4[u].x, t, s);
            update(p4[u].y, g4[u].y, m4[u].y, v4[u].y, t, s);
            update(p4[u].z, g4[u].z, m4[u].z, v4[u].z, t, s);
            update(p4[u].w, g4[u].w, m4[u].w, v4[u].w, t, s);
            *reinterpret_cast<float4*>(P + e) = p4[u];
            *reinterpret_cast<float4*>(M + e) = m4[u];
            *reinterpret_cast<float4*>(V + e) = v4[u];
        }
    }
    // what is left of this chunk one float at a time: its tail (< 4 elements) when vectorised, all of it otherwise
    for (long long e = begin + 4 * n_vec + threadIdx.x; e < end; e += kThreads) update_one(t, i, e, s);
    // the head in front of the first aligned element belongs to the tensor's first workgroup
    if (chunk == 0 && (long long)threadIdx.x < head) update_one(t, i, threadIdx.x, s);
}

}  // namespace
}  // namespace inerf

extern "C" int inerf_adam_step(const inerf_adam_args* a, void* stream) {
    using namespace inerf;
    if (!a || a->n_tensors < 0) return INERF_E_INVALID;
    if (a->n_tensors == 0) return INERF_OK;
    if (!a->params || !a->grads || !a->exp_avg || !a->exp_avg_sq || !a->steps || !a->counts) return INERF_E_INVALID;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps > 0.0)) return INERF_E_INVALID;
    // every tensor is checked before the first launch: a bad entry leaves the whole list untouched
    for (int i = 0; i < a->n_tensors; ++i) {
        if (!a->params[i] || !a->grads[i] || !a->exp_avg[i] || !a->exp_avg_sq[i] || !a->steps[i] || a->counts[i] <= 0) return INERF_E_INVALID;
        if (((uintptr_t)a->params[i] | (uintptr_t)a->grads[i] | (uintptr_t)a->exp_avg[i] | (uintptr_t)a->exp_avg_sq[i] | (uintptr_t)a->steps[i]) & 3u)
            return INERF_E_INVALID;
        if (a->counts[i] > (1ll << 40)) return INERF_E_UNSUPPORTED;
    }
    for (int base = 0; base < a->n_tensors; base += kMaxTensors) {
        AdamTable t{};
        t.n = a->n_tensors - base < kMaxTensors ? a->n_tensors - base : kMaxTensors;
        long long blocks = 0;
        for (int i = 0; i < t.n; ++i) {
            t.p[i] = a->params[base + i];
            t.g[i] = a->grads[base + i];
            t.m[i] = a->exp_avg[base + i];
            t.v[i] = a->exp_avg_sq[base + i];
            t.step[i] = a->steps[base + i];
            t.count[i] = a->counts[base + i];
            t.first_block[i] = (int)blocks;
            // (up to 3 head elements ride with the first workgroup: the chunks cover count - head <= count elements)
            blocks += (t.count[i] + kChunk - 1) / kChunk;
            if (blocks > 0x7fffffffll) return INERF_E_UNSUPPORTED;
        }
        t.first_block[t.n] = (int)blocks;
        t.lr = a->lr;
        t.lr_dev = a->lr_dev;
        t.beta1 = a->beta1;
        t.beta2 = a->beta2;
        t.one_minus_beta1 = (float)(1.0 - a->beta1);
        t.beta2_f = (float)a->beta2;
        t.one_minus_beta2 = (float)(1.0 - a->beta2);
        t.eps = (float)a->eps;
        hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(128), 0, (hipStream_t)stream, t);
        hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, t);
        const int rc = record(hipGetLastError());
        if (rc) return rc;
    }
    return INERF_OK;
}
