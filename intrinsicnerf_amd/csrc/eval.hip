// eval.hip - the SSR trainer's validation arithmetic on the device (trainer.py:1244-1245, training_utils.py:58-124):
//   inerf_sem_maps        : a frame's label map and entropy map from its semantic logits, one streaming launch
//   inerf_eval_accumulate : one pass over a frame's pixels into device-resident accumulators - the confusion table and the
//                           depth / rgb counts as int64, the depth and rgb error sums as fp64 - and, when the predicted label
//                           comes from logits, the two maps of inerf_sem_maps out of the same launch (sem_tile, one copy)
// Label.  The LOWEST INDEX THAT ATTAINS THE ROW'S MAXIMUM LOGIT.  The reference takes argmax(softmax(x)): the same index whenever
// the runner-up equals the maximum bitwise or lies below it by more than the fp32 rounding of the softmax can hide.  Where two
// logits differ by less than ~1e-7 (a row of zeros holding 1e-8 and 3e-8) torch answers 0 because the two softmax values round
// to the same float: that is rounding noise of the reference, not behaviour, and is not reproduced.  A row that holds a NaN or
// whose maximum is not finite gets label 0 and entropy NaN (torch: softmax turns the row NaN, argmax of an all-NaN row is 0); a
// row with a -inf entry and a finite maximum keeps its label and gets entropy NaN (-(-inf) * 0).
// Entropy.  Max-subtracted: d_i = x_i - m, e_i = expf(d_i) (accurate), S = sum e_i, T = sum e_i d_i, H = log S - T / S with S, T
// and the last line in fp64 - every e_i d_i is exact, both terms of H are non-negative, so H carries the ulp of expf and nothing else.
// Rows to lanes.  A row is 4 C bytes (112 at C = 28): one lane per row would touch 64 cache lines per load.  G = min(64,
// pow2ceil(C)) consecutive lanes read consecutive logits of one row, a wave takes 64 / G rows per step and 64 rows per tile; the
// (max, index) pair and (S, T) go through log2 G xor-shuffles, and a last shuffle hands row r of the tile to lane r, so the maps
// are stored - and the accumulators fed - one pixel per lane.
// Accumulation.  Bit-identical from run to run: every count goes through integer atomics (a sum of integers has no order),
// the confusion table privatised in LDS up to kLdsMaxClasses classes and sent to global atomics beyond; the fp64 sums go lane ->
// wave -> workgroup through fixed trees into one plain-stored row of partials per workgroup, and a second, tiny launch on the
// same stream adds the rows in index order to the running totals.  No workgroup waits for another inside a kernel, and no
// floating-point atomic exists here.  The grid is a function of n alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/inerf.h"
#include "sem_label.h"

namespace inerf {

int record(hipError_t e);

constexpr int kEvalThreads = 256;       // four waves, one 64-pixel tile each per trip
constexpr int kEvalMaxBlocks = 512;     // accumulate grid cap: a 320x240 frame is 300 workgroups, anything beyond 131 072 pixels loops
constexpr int kLdsMaxClasses = 64;      // C <= 64: the C x C table lives in LDS (<= 16 KB of uint32); above: global atomics
constexpr int kCounts = INERF_EVAL_COUNTS, kSums = INERF_EVAL_SUMS;

struct EvalArgs {
    SemIO sem;
    const float* pred_label;
    long long pred_label_stride;
    const float* true_label;
    long long true_label_stride;
    float ignore_label;
    const float* depth_pred;
    long long depth_pred_stride;
    const float* depth_trgt;
    long long depth_trgt_stride;
    const float* rgb_pred;
    long long rgb_pred_stride;
    const float* rgb_trgt;
    long long rgb_trgt_stride;
    unsigned long long* counts;     // the int64 table: conf[C * C], then kCounts counters
    double* partial;                // [gridDim.x, kSums]
};

enum { kTableNone = 0, kTableLds = 1, kTableGlobal = 2 };

__device__ __forceinline__ bool class_index(float v, int C) { return v >= 0.f && v < (float)C && v == floorf(v); }

// G: lanes per logits row, 0 = no logits (the predicted label is a column).  kTable: kTableNone = the maps alone.
template <int G, int kTable>
__global__ __launch_bounds__(kEvalThreads) void k_eval(EvalArgs a, long long n) {
    extern __shared__ unsigned s_conf[];            // [C * C], kTableLds only
    __shared__ unsigned s_cnt[kCounts];
    __shared__ double s_sum[kEvalThreads / 64][kSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.sem.n_classes;

    if (kTable != kTableNone) {
        if (kTable == kTableLds)
            for (int i = threadIdx.x; i < C * C; i += kEvalThreads) s_conf[i] = 0u;
        if (threadIdx.x < kCounts) s_cnt[threadIdx.x] = 0u;
        __syncthreads();
    }

    int cnt[kCounts] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sum[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

    for (long long tile = (long long)blockIdx.x * (kEvalThreads / 64) + wave; tile * 64 < n; tile += (long long)gridDim.x * (kEvalThreads / 64)) {
        const long long p = tile * 64 + lane;
        const bool live = p < n;
        float pred = __builtin_nanf("");
        if (G > 0) {
            float ent;
            sem_tile<(G > 0 ? G : 1)>(a.sem, tile * 64, n, lane, pred, ent);
            if (live && a.sem.label) a.sem.label[p * a.sem.label_stride] = pred;
            if (live && a.sem.entropy) a.sem.entropy[p * a.sem.entropy_stride] = ent;
        } else if (kTable != kTableNone && live && a.pred_label) {
            pred = a.pred_label[p * a.pred_label_stride];
        }
        if (kTable == kTableNone) continue;

        if (a.true_label) {
            const float t = live ? a.true_label[p * a.true_label_stride] : a.ignore_label;
            const bool valid = live && t != a.ignore_label;
            cnt[INERF_EVAL_N_NOT_IGNORED] += valid;
            const bool in = valid && class_index(t, C) && class_index(pred, C);
            const int idx = in ? (int)t * C + (int)pred : 0;            // row = true, column = predicted
            const unsigned long long who = __ballot(in);
            if (who) {
                // one class over a whole wave is the common case of a frame and the worst case of the atomic: one add of the count
                const int first = __ffsll((long long)who) - 1;
                const int idx0 = __shfl(idx, first);
                const bool same = __ballot(in && idx == idx0) == who;
                const bool adds = same ? lane == first : in;
                const unsigned by = same ? (unsigned)__popcll(who) : 1u;
                if (adds) {
                    if (kTable == kTableLds) atomicAdd(&s_conf[idx], by);
                    else atomicAdd(&a.counts[idx], (unsigned long long)by);
                }
            }
        }
        if (a.depth_pred) {
            const float dp = live ? a.depth_pred[p * a.depth_pred_stride] : 0.f;
            const float dt = live ? a.depth_trgt[p * a.depth_trgt_stride] : 0.f;
            cnt[INERF_EVAL_N_PIXELS] += live;
            cnt[INERF_EVAL_N_PRED_POSITIVE] += live && dp > 0.f;
            if (live && dt < 10.f && dt > 0.f && dp > 0.f) {
                // training_utils.py:101-109 in fp32, unfused, in its order: numpy's bits for everything but the logarithm
                const float ad = fabsf(__fsub_rn(dp, dt));
                const float sq = __fmul_rn(ad, ad);
                const float lg = __fsub_rn(logf(dp), logf(dt));
                const float thr = fmaxf(__fdiv_rn(dt, dp), __fdiv_rn(dp, dt));
                cnt[INERF_EVAL_N_MASK] += 1;
                cnt[INERF_EVAL_R1] += thr < 1.25f;
                cnt[INERF_EVAL_R2] += thr < 1.5625f;
                cnt[INERF_EVAL_R3] += thr < 1.953125f;
                sum[INERF_EVAL_ABS_REL] += (double)__fdiv_rn(ad, dt);
                sum[INERF_EVAL_ABS_DIFF] += (double)ad;
                sum[INERF_EVAL_SQ_REL] += (double)__fdiv_rn(sq, dt);
                sum[INERF_EVAL_SQ_DIFF] += (double)sq;
                sum[INERF_EVAL_SQ_LOG_DIFF] += (double)__fmul_rn(lg, lg);
            }
        }
        if (a.rgb_pred && live) {
            const float* __restrict__ x = a.rgb_pred + p * a.rgb_pred_stride;
            const float* __restrict__ y = a.rgb_trgt + p * a.rgb_trgt_stride;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = __fsub_rn(x[k], y[k]);
                sum[INERF_EVAL_RGB_SQ] += (double)__fmul_rn(d, d);
            }
            cnt[INERF_EVAL_N_RGB] += 3;
        }
    }
    if (kTable == kTableNone) return;

    // lane -> wave: xor trees, the same shape every run.  Integers through LDS atomics, the fp64 partials through their own slots
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {
        int v = cnt[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0 && v) atomicAdd(&s_cnt[k], (unsigned)v);
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        double v = sum[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_sum[wave][k] = v;
    }
    __syncthreads();
    // wave -> workgroup, then out: counts by integer atomics, the sums as this workgroup's plain-stored row
    if (threadIdx.x < kCounts && s_cnt[threadIdx.x]) atomicAdd(&a.counts[(long long)C * C + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + kSums) {
        const int k = threadIdx.x - 64;
        a.partial[(long long)blockIdx.x * kSums + k] = ((s_sum[0][k] + s_sum[1][k]) + s_sum[2][k]) + s_sum[3][k];
    }
    if (kTable == kTableLds)
        for (int i = threadIdx.x; i < C * C; i += kEvalThreads)
            if (s_conf[i]) atomicAdd(&a.counts[i], (unsigned long long)s_conf[i]);
}

// the second launch: the workgroups' rows in index order onto the running totals.  The rows are staged in LDS by the whole workgroup
// first: a lane that walked them in global memory would pay one L2 round trip per row (~40 us for a frame's 300 rows, measured)
__global__ __launch_bounds__(kEvalThreads) void k_eval_finish(const double* __restrict__ partial, int rows, double* __restrict__ sums) {
    __shared__ double s_part[kEvalMaxBlocks * kSums];
    for (int i = threadIdx.x; i < rows * kSums; i += kEvalThreads) s_part[i] = partial[i];      // rows <= kEvalMaxBlocks: eval_blocks()
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= kSums) return;
    double t = sums[k];
#pragma unroll 8
    for (int b = 0; b < rows; ++b) t += s_part[b * kSums + k];
    sums[k] = t;
}

static long long eval_blocks(long long n) {
    const long long b = (n + kEvalThreads - 1) / kEvalThreads;
    return b < kEvalMaxBlocks ? b : kEvalMaxBlocks;
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

template <int kTable>
static void launch_eval(int g, const EvalArgs& a, long long n, unsigned blocks, size_t lds, hipStream_t stream) {
#define INERF_EVAL_CASE(G) case G: hipLaunchKernelGGL((k_eval<G, kTable>), dim3(blocks), dim3(kEvalThreads), lds, stream, a, n); break;
    switch (g) {
        INERF_EVAL_CASE(0) INERF_EVAL_CASE(1) INERF_EVAL_CASE(2) INERF_EVAL_CASE(4) INERF_EVAL_CASE(8) INERF_EVAL_CASE(16)
        INERF_EVAL_CASE(32) INERF_EVAL_CASE(64)
    }
#undef INERF_EVAL_CASE
}

}  // namespace inerf

extern "C" int inerf_sem_maps(const float* logits, int64_t logits_stride, int64_t n, int n_classes, float* label, int64_t label_stride,
                              float* entropy, int64_t entropy_stride, void* stream) {
    using namespace inerf;
    if (n_classes < 1 || n_classes > INERF_MAX_CLASSES) return INERF_E_UNSUPPORTED;
    if (n < 0 || logits_stride < n_classes || (label && label_stride < 1) || (entropy && entropy_stride < 1)) return INERF_E_INVALID;
    if (n == 0 || (!label && !entropy)) return INERF_OK;
    if (!logits || misaligned(logits, 4) || misaligned(label, 4) || misaligned(entropy, 4)) return INERF_E_INVALID;
    const long long blocks = (n + kEvalThreads - 1) / kEvalThreads;
    if (blocks > 0x7fffffffLL) return INERF_E_UNSUPPORTED;
    EvalArgs a{};
    a.sem = SemIO{logits, (long long)logits_stride, n_classes, label, (long long)label_stride, entropy, (long long)entropy_stride};
    launch_eval<kTableNone>(lanes_per_row(n_classes), a, (long long)n, (unsigned)blocks, 0, (hipStream_t)stream);
    return record(hipGetLastError());
}

extern "C" int64_t inerf_eval_workspace_bytes(int64_t n) {
    return n <= 0 ? 0 : (int64_t)(inerf::eval_blocks(n) * inerf::kSums * sizeof(double));
}

extern "C" int inerf_eval_accumulate(const inerf_eval_args* args, void* stream) {
    using namespace inerf;
    if (!args) return INERF_E_INVALID;
    const bool sem = args->logits != nullptr, labels = args->true_label != nullptr, depth = args->depth_pred != nullptr,
               rgb = args->rgb_pred != nullptr;
    const int C = args->n_classes;
    if (C < 1 || C > INERF_MAX_CLASSES) return INERF_E_UNSUPPORTED;
    if (args->n < 0) return INERF_E_INVALID;
    if (sem && (args->logits_stride < C || (args->out_label && args->out_label_stride < 1) || (args->out_entropy && args->out_entropy_stride < 1)))
        return INERF_E_INVALID;
    if (labels && (args->true_label_stride < 1 || (!sem && (!args->pred_label || args->pred_label_stride < 1)))) return INERF_E_INVALID;
    if (depth && (!args->depth_trgt || args->depth_pred_stride < 1 || args->depth_trgt_stride < 1)) return INERF_E_INVALID;
    if (rgb && (!args->rgb_trgt || args->rgb_pred_stride < 3 || args->rgb_trgt_stride < 3)) return INERF_E_INVALID;
    if (args->n == 0) return INERF_OK;
    if (args->n > 0x7fffffffLL) return INERF_E_UNSUPPORTED;                        // the per-workgroup counters are 32-bit
    if (!args->counts || !args->sums || misaligned(args->counts, 8) || misaligned(args->sums, 8)) return INERF_E_INVALID;
    if (!args->workspace || misaligned(args->workspace, 8) || args->workspace_bytes < inerf_eval_workspace_bytes(args->n)) return INERF_E_WORKSPACE;
    const void* floats[] = {args->logits, args->pred_label, args->out_label, args->out_entropy, args->true_label, args->depth_pred,
                            args->depth_trgt, args->rgb_pred, args->rgb_trgt};
    for (const void* f : floats)
        if (misaligned(f, 4)) return INERF_E_INVALID;

    EvalArgs a{};
    a.sem = SemIO{args->logits, (long long)args->logits_stride, C, args->out_label, (long long)args->out_label_stride,
                  args->out_entropy, (long long)args->out_entropy_stride};
    a.pred_label = sem ? nullptr : args->pred_label;
    a.pred_label_stride = args->pred_label_stride;
    a.true_label = args->true_label;
    a.true_label_stride = args->true_label_stride;
    a.ignore_label = (float)args->ignore_label;
    a.depth_pred = args->depth_pred; a.depth_pred_stride = args->depth_pred_stride;
    a.depth_trgt = args->depth_trgt; a.depth_trgt_stride = args->depth_trgt_stride;
    a.rgb_pred = args->rgb_pred; a.rgb_pred_stride = args->rgb_pred_stride;
    a.rgb_trgt = args->rgb_trgt; a.rgb_trgt_stride = args->rgb_trgt_stride;
    a.counts = reinterpret_cast<unsigned long long*>(args->counts);
    a.partial = static_cast<double*>(args->workspace);
    const unsigned blocks = (unsigned)eval_blocks(args->n);
    const int g = sem ? lanes_per_row(C) : 0;
    if (C <= kLdsMaxClasses)
        launch_eval<kTableLds>(g, a, (long long)args->n, blocks, sizeof(unsigned) * (size_t)C * C, (hipStream_t)stream);
    else
        launch_eval<kTableGlobal>(g, a, (long long)args->n, blocks, 0, (hipStream_t)stream);
    const int rc = record(hipGetLastError());
    if (rc != INERF_OK) return rc;
    hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(kEvalThreads), 0, (hipStream_t)stream, a.partial, (int)blocks, args->sums);
    return record(hipGetLastError());
}
