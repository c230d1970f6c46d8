// losses.hip - the training losses of both trainers, one forward and one backward launch per step:
//   compute_intrinsic_loss and its helpers   object_level/run_nerf_helpers.py:15-86, SSR/training/training_utils.py:127-207
//   img2mse on the image and on the cluster target   run_nerf.py:976,987,1006,1012; trainer.py:923,936,985-986
//   nn.CrossEntropyLoss(ignore_index=-1)(logits, label-1)   trainer.py:858-865,927,939
// The reference evaluates them as ~60 elementwise / reduction ATen ops per level (and as many again in autograd) on
// 1 024 - 2 048 rays: pure launch latency.  Here a step's terms - coarse and fine level together - are ONE launch, and their
// gradients ONE more.
//
// Forward: a single workgroup of 16 waves strides over the rays; every lane keeps its 14 partial sums in fp64, a 6-step
// butterfly adds them inside the wave, the 16 wave sums go through LDS and are added in wave order.  No atomics, no second
// workgroup, so nothing to hand over inside the launch and no counter to zero before it: at the batch sizes of a training step
// (N <= 4 096: ~45 floats per ray and level) the launch is latency, not bandwidth.  Larger N is correct, just not parallel.
// Backward: one thread per ray and level gathers what the ray contributes to - its own chroma / residual / intensity / image /
// cluster / cross-entropy terms, its near pair and its far pair - and writes its rows.  A pure gather: bit-identical run to run.
//
// Arithmetic: every per-ray expression is the reference's, in its order, in fp32 (true divisions, no contraction); only the
// sums over rays are carried in fp64, which is at least as accurate as ATen's pairwise fp32 sums.
//
// The [N,1] mask of the object-level trainer (run_nerf.py:703 `images[...,-1:]`): `exp(...)[split] * mask1[split,1] *
// mask2[split,1]` broadcasts to a [split, split] matrix W[i,j] = e_j m1_i m2_i, so torch.mean(W * norm_2) =
// mean_i(m1_i m2_i) * mean_j(e_j norm_2_j).  INERF_LOSS_MASK_OUTER computes that product of two means; the matrix never exists.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout.h"

namespace inerf {

int record(hipError_t e);

namespace {

constexpr int kFwdThreads = 1024;
constexpr int kFwdWaves = kFwdThreads / 64;
constexpr int kBwdThreads = 256;
constexpr int kSums = 14;
// the partial sums of one level
enum : int { kChromaR, kChromaG, kResidual, kSparsity, kShading, kFar, kGtSum, kAlbedoSum, kImage, kCluster, kCe, kCeCount,
             kMaskNear, kMaskFar };
// state[l*16 + ...] behind the nine terms
enum : int { kStateMeanDiff = 9, kStateMaskNear = 10, kStateMaskFar = 11, kStateCeCount = 12 };

struct LossLevel {
    const float* albedo;
    const float* shading;
    const float* residual;
    const float* rgb;
    const float* logits;
    float* d_albedo;
    float* d_shading;
    float* d_residual;
    float* d_rgb;
    float* d_logits;
};

struct LossParams {
    long long n, split, off, split2, off2;
    int n_levels, n_classes, ce_offset;
    bool labels, outer;
    const float* gt;
    const float* mask;            // pair key as a float mask ...
    const long long* key_labels;  // ... or as int64 labels
    const float* target;
    const long long* ce_labels;
    const float* weights;
    const float* grad_total;
    const float* grad_terms;
    LossLevel level[2];
    float* state;
};

struct Chroma {
    float r, g, sum;
};

// compute_chroma_loss / compute_chroma_weight: sum = c0 + c1 + c2 + 1e-5, r = c0 / sum, g = c1 / sum
__device__ __forceinline__ Chroma chroma_of(const float* __restrict__ c) {
    Chroma o;
    o.sum = ((c[0] + c[1]) + c[2]) + 1e-5f;
    o.r = c[0] / o.sum;
    o.g = c[1] / o.sum;
    return o;
}

__device__ __forceinline__ float sq(float x) { return x * x; }

struct PairWeight {
    float w_chroma;     // exp(-60 d2) [* mask product]
    float w_shading;    // d2 [* mask product]
    float mask;         // the mask product itself (outer form: summed on its own)
};

// compute_chroma_weight of the pair (i, j) of gt colours; the mask product applied per ray unless the outer form is asked for
__device__ __forceinline__ PairWeight pair_weight(const LossParams& p, long long i, long long j) {
    const Chroma c1 = chroma_of(p.gt + 3 * i), c2 = chroma_of(p.gt + 3 * j);
    const float d2 = sq(c1.r - c2.r) + sq(c1.g - c2.g);
    const float e = expf(-60.0f * d2);
    PairWeight o;
    if (p.labels) {
        o.mask = p.key_labels[i] == p.key_labels[j] ? 1.0f : 0.0f;
        o.w_chroma = e * o.mask;
        o.w_shading = d2;                                   // training_utils.py:150: the mask is commented out
    } else {
        const float m1 = p.mask[i], m2 = p.mask[j];
        o.mask = m1 * m2;
        o.w_chroma = p.outer ? e : e * m1 * m2;
        o.w_shading = p.outer ? d2 : d2 * m1 * m2;
    }
    return o;
}

__device__ __forceinline__ float norm2_of(const float* __restrict__ a, const float* __restrict__ b) {
    return (sq(a[0] - b[0]) + sq(a[1] - b[1])) + sq(a[2] - b[2]);
}

// label of ray i for the cross-entropy, -1 when the ray is ignored
__device__ __forceinline__ int ce_label(const LossParams& p, long long i) {
    const long long lab = p.ce_labels[i] + p.ce_offset;
    return lab >= 0 && lab < p.n_classes ? (int)lab : -1;
}

// max and log(sum exp(x - max)) of a logits row (log_softmax as ATen evaluates it)
__device__ __forceinline__ void row_stats(const float* __restrict__ row, int c, float& mx, float& sum) {
    mx = row[0];
    for (int k = 1; k < c; ++k) mx = fmaxf(mx, row[k]);
    sum = 0.f;
    for (int k = 0; k < c; ++k) sum += expf(row[k] - mx);
}

__global__ __launch_bounds__(kFwdThreads) void k_intrinsic_loss(LossParams p) {
    __shared__ double red[kFwdWaves][kSums];
    __shared__ double fin[kSums];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float total = 0.f;                                       // thread 0 only
    for (int l = 0; l < p.n_levels; ++l) {
        const LossLevel& lv = p.level[l];
        double acc[kSums];
#pragma unroll
        for (int v = 0; v < kSums; ++v) acc[v] = 0.0;
        for (long long i = tid; i < p.n; i += kFwdThreads) {
            const float* a = lv.albedo + 3 * i;
            const float* g = p.gt + 3 * i;
            const Chroma ca = chroma_of(a), cg = chroma_of(g);
            acc[kChromaR] += sq(ca.r - cg.r);
            acc[kChromaG] += sq(ca.g - cg.g);
            const float* r = lv.residual + 3 * i;
            acc[kResidual] += (sq(r[0]) + sq(r[1])) + sq(r[2]);
            acc[kGtSum] += (g[0] + g[1]) + g[2];
            acc[kAlbedoSum] += (a[0] + a[1]) + a[2];
            if (lv.rgb) acc[kImage] += norm2_of(lv.rgb + 3 * i, g);
            if (p.target) acc[kCluster] += norm2_of(a, p.target + 3 * i);
            if (lv.logits) {
                const int lab = ce_label(p, i);
                if (lab >= 0) {
                    const float* row = lv.logits + i * p.n_classes;
                    float mx, sum;
                    row_stats(row, p.n_classes, mx, sum);
                    acc[kCe] += -((row[lab] - mx) - logf(sum));
                    acc[kCeCount] += 1.0;
                }
            }
            if (i < p.split) {
                const long long j = i + p.off;
                const PairWeight w = pair_weight(p, i, j);
                acc[kSparsity] += w.w_chroma * norm2_of(a, lv.albedo + 3 * j);
                acc[kShading] += w.w_shading * sq(lv.shading[i] - lv.shading[j]);
                acc[kMaskNear] += w.mask;
            }
            if (i < p.split2) {
                const long long j = i + p.off2;
                const PairWeight w = pair_weight(p, i, j);
                acc[kFar] += w.w_chroma * norm2_of(a, lv.albedo + 3 * j);
                acc[kMaskFar] += w.mask;
            }
        }
#pragma unroll
        for (int v = 0; v < kSums; ++v) {
            double x = acc[v];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            if (lane == 0) red[wave][v] = x;
        }
        __syncthreads();
        if (tid < kSums) {
            double s = 0.0;
            for (int w = 0; w < kFwdWaves; ++w) s += red[w][tid];         // wave order: the same sum every run
            fin[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            const double n = (double)p.n, n3 = 3.0 * n, sp = (double)p.split, sp2 = (double)p.split2;
            // an empty mean is 0 / 0 = NaN, as torch.mean of an empty tensor
            const double mask_near = fin[kMaskNear] / sp, mask_far = fin[kMaskFar] / sp2;
            const double mean_diff = fin[kGtSum] / n3 - fin[kAlbedoSum] / n3;
            float t[INERF_LOSS_STATE_FLOATS];
            for (int k = 0; k < INERF_LOSS_STATE_FLOATS; ++k) t[k] = 0.f;
            t[INERF_LOSS_TERM_CHROMA] = (float)(fin[kChromaR] / n) + (float)(fin[kChromaG] / n);
            t[INERF_LOSS_TERM_RESIDUAL] = (float)(fin[kResidual] / n3);
            t[INERF_LOSS_TERM_SPARSITY] = (float)(p.outer ? mask_near * (fin[kSparsity] / sp) : fin[kSparsity] / sp);
            t[INERF_LOSS_TERM_SHADING] = (float)(p.outer ? mask_near * (fin[kShading] / sp) : fin[kShading] / sp);
            t[INERF_LOSS_TERM_FAR] = (float)(p.outer ? mask_far * (fin[kFar] / sp2) : fin[kFar] / sp2);
            t[INERF_LOSS_TERM_INTENSITY] = (float)(mean_diff * mean_diff);
            if (lv.rgb) t[INERF_LOSS_TERM_IMAGE] = (float)(fin[kImage] / n3);
            if (p.target) t[INERF_LOSS_TERM_CLUSTER] = (float)(fin[kCluster] / n3);
            if (lv.logits) t[INERF_LOSS_TERM_SEMANTIC] = (float)(fin[kCe] / fin[kCeCount]);
            t[kStateMeanDiff] = (float)mean_diff;
            t[kStateMaskNear] = (float)mask_near;
            t[kStateMaskFar] = (float)mask_far;
            t[kStateCeCount] = (float)fin[kCeCount];
            for (int k = 0; k < INERF_LOSS_STATE_FLOATS; ++k) p.state[l * INERF_LOSS_STATE_FLOATS + k] = t[k];
            for (int k = 0; k < INERF_LOSS_TERMS; ++k) {
                const bool present = k < INERF_LOSS_TERM_IMAGE || (k == INERF_LOSS_TERM_IMAGE && lv.rgb) ||
                                     (k == INERF_LOSS_TERM_CLUSTER && p.target) || (k == INERF_LOSS_TERM_SEMANTIC && lv.logits);
                if (present) total += (p.weights ? p.weights[k] : 1.0f) * t[k];
            }
        }
        __syncthreads();                                     // red / fin are reused by the next level
    }
    if (tid == 0) p.state[p.n_levels * INERF_LOSS_STATE_FLOATS] = total;
}

__global__ __launch_bounds__(kBwdThreads) void k_intrinsic_loss_bwd(LossParams p) {
    const long long i = (long long)blockIdx.x * kBwdThreads + threadIdx.x;
    const int l = blockIdx.y;
    if (i >= p.n) return;
    const LossLevel& lv = p.level[l];
    const float* st = p.state + l * INERF_LOSS_STATE_FLOATS;
    float c[INERF_LOSS_TERMS];
    const float gt = p.grad_total ? p.grad_total[0] : 0.f;
#pragma unroll
    for (int k = 0; k < INERF_LOSS_TERMS; ++k)
        c[k] = gt * (p.weights ? p.weights[k] : 1.0f) + (p.grad_terms ? p.grad_terms[l * INERF_LOSS_STATE_FLOATS + k] : 0.f);
    const float n = (float)p.n, n3 = 3.0f * n;

    const float* a = lv.albedo + 3 * i;
    const float* g = p.gt + 3 * i;
    float da[3];
    {   // chroma: d/da of mean((ra - rg)^2) + mean((ga - gg)^2), ra = a0 / sum, ga = a1 / sum
        const Chroma ca = chroma_of(a), cg = chroma_of(g);
        const float er = c[INERF_LOSS_TERM_CHROMA] * (2.0f * (ca.r - cg.r) / n);
        const float eg = c[INERF_LOSS_TERM_CHROMA] * (2.0f * (ca.g - cg.g) / n);
        da[0] = (er * (1.0f - ca.r) - eg * ca.g) / ca.sum;
        da[1] = (eg * (1.0f - ca.g) - er * ca.r) / ca.sum;
        da[2] = (-er * ca.r - eg * ca.g) / ca.sum;
    }
    {   // intensity: (rgb_mean - albedo_mean)^2, every albedo entry weighs 1 / 3N in the mean
        const float di = c[INERF_LOSS_TERM_INTENSITY] * (-2.0f * st[kStateMeanDiff] / n3);
        da[0] += di; da[1] += di; da[2] += di;
    }
    if (p.target) {
        const float* t = p.target + 3 * i;
        const float k = c[INERF_LOSS_TERM_CLUSTER] * 2.0f / n3;
#pragma unroll
        for (int q = 0; q < 3; ++q) da[q] += k * (a[q] - t[q]);
    }
    float ds = 0.f;
    // near pair: ray i < split is the first of (i, i + off), ray i >= off the second of (i - off, i); the weights come from gt alone
    if (i < p.split || i >= p.off) {
        const long long first = i < p.split ? i : i - p.off, partner = i < p.split ? i + p.off : i - p.off;
        const PairWeight w = pair_weight(p, first, first + p.off);
        const float outer = p.outer ? st[kStateMaskNear] : 1.0f;
        const float* b = lv.albedo + 3 * partner;
        const float ka = c[INERF_LOSS_TERM_SPARSITY] * outer * w.w_chroma * 2.0f / (float)p.split;
#pragma unroll
        for (int q = 0; q < 3; ++q) da[q] += ka * (a[q] - b[q]);
        ds = c[INERF_LOSS_TERM_SHADING] * outer * w.w_shading * 2.0f / (float)p.split * (lv.shading[i] - lv.shading[partner]);
    }
    // far pair, inside the first half: (i, i + off2) for i < split2
    if (i < p.split2 || (i >= p.off2 && i < p.split)) {
        const long long first = i < p.split2 ? i : i - p.off2, partner = i < p.split2 ? i + p.off2 : i - p.off2;
        const PairWeight w = pair_weight(p, first, first + p.off2);
        const float outer = p.outer ? st[kStateMaskFar] : 1.0f;
        const float* b = lv.albedo + 3 * partner;
        const float ka = c[INERF_LOSS_TERM_FAR] * outer * w.w_chroma * 2.0f / (float)p.split2;
#pragma unroll
        for (int q = 0; q < 3; ++q) da[q] += ka * (a[q] - b[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) lv.d_albedo[3 * i + q] = da[q];
    lv.d_shading[i] = ds;
    {
        const float* r = lv.residual + 3 * i;
        const float k = c[INERF_LOSS_TERM_RESIDUAL] * 2.0f / n3;
#pragma unroll
        for (int q = 0; q < 3; ++q) lv.d_residual[3 * i + q] = k * r[q];
    }
    if (lv.rgb) {
        const float* x = lv.rgb + 3 * i;
        const float k = c[INERF_LOSS_TERM_IMAGE] * 2.0f / n3;
#pragma unroll
        for (int q = 0; q < 3; ++q) lv.d_rgb[3 * i + q] = k * (x[q] - g[q]);
    }
    if (lv.logits) {
        const int lab = ce_label(p, i);
        const float* row = lv.logits + i * p.n_classes;
        float* d = lv.d_logits + i * p.n_classes;
        if (lab < 0) {
            for (int k = 0; k < p.n_classes; ++k) d[k] = 0.f;       // an ignored ray takes no gradient (also when every ray is)
        } else {
            float mx, sum;
            row_stats(row, p.n_classes, mx, sum);
            const float k0 = c[INERF_LOSS_TERM_SEMANTIC] / st[kStateCeCount];
            for (int k = 0; k < p.n_classes; ++k) d[k] = k0 * (expf(row[k] - mx) / sum - (k == lab ? 1.0f : 0.0f));
        }
    }
}

// argument checks shared by both entry points; fills `p`
int loss_params(const inerf_loss_args* a, bool backward, LossParams& p) {
    if (!a || a->n_rays < 0 || (a->n_levels != 1 && a->n_levels != 2)) return INERF_E_INVALID;
    if (a->flags & ~(INERF_LOSS_KEY_LABELS | INERF_LOSS_MASK_OUTER)) return INERF_E_INVALID;
    if ((a->flags & INERF_LOSS_KEY_LABELS) && (a->flags & INERF_LOSS_MASK_OUTER)) return INERF_E_INVALID;   // labels have no [n,1] form
    if (a->n_rays > (1ll << 30)) return INERF_E_UNSUPPORTED;
    const bool have_rgb = a->level[0].rgb != nullptr, have_logits = a->level[0].logits != nullptr;
    if (a->n_rays > 0) {
        if (!a->gt_rgb || !a->pair_key) return INERF_E_INVALID;
        for (int l = 0; l < a->n_levels; ++l) {
            const inerf_loss_level& lv = a->level[l];
            if (!lv.albedo || !lv.shading || !lv.residual) return INERF_E_INVALID;
            if ((lv.rgb != nullptr) != have_rgb || (lv.logits != nullptr) != have_logits) return INERF_E_INVALID;
            if (backward && (!lv.d_albedo || !lv.d_shading || !lv.d_residual || (have_rgb && !lv.d_rgb) || (have_logits && !lv.d_logits)))
                return INERF_E_INVALID;
        }
        if (have_logits && (!a->ce_labels || a->n_classes < 1)) return INERF_E_INVALID;
        if (have_logits && a->n_classes > INERF_LOSS_MAX_CLASSES) return INERF_E_UNSUPPORTED;
    }
    if (!a->state || a->state_bytes < inerf_intrinsic_loss_workspace_bytes(a->n_rays, a->n_levels)) return INERF_E_WORKSPACE;
    p.n = a->n_rays;
    p.split = p.n / 2;
    p.off = p.n - p.split;
    p.split2 = p.split / 2;
    p.off2 = p.split - p.split2;
    p.n_levels = a->n_levels;
    p.n_classes = a->n_classes;
    p.ce_offset = a->ce_label_offset;
    p.labels = (a->flags & INERF_LOSS_KEY_LABELS) != 0;
    p.outer = (a->flags & INERF_LOSS_MASK_OUTER) != 0;
    p.gt = a->gt_rgb;
    p.mask = p.labels ? nullptr : static_cast<const float*>(a->pair_key);
    p.key_labels = p.labels ? static_cast<const long long*>(a->pair_key) : nullptr;
    p.target = a->cluster_target;
    p.ce_labels = reinterpret_cast<const long long*>(a->ce_labels);
    p.weights = a->weights;
    p.grad_total = a->grad_total;
    p.grad_terms = a->grad_terms;
    for (int l = 0; l < 2; ++l) {
        const inerf_loss_level& s = a->level[l];
        p.level[l] = LossLevel{s.albedo, s.shading, s.residual, s.rgb, s.logits, s.d_albedo, s.d_shading, s.d_residual, s.d_rgb, s.d_logits};
    }
    p.state = a->state;
    return INERF_OK;
}

}  // namespace
}  // namespace inerf

extern "C" int64_t inerf_intrinsic_loss_workspace_bytes(int64_t n_rays, int n_levels) {
    if (n_rays < 0 || (n_levels != 1 && n_levels != 2)) return INERF_E_INVALID;
    return (int64_t)(n_levels + 1) * INERF_LOSS_STATE_FLOATS * (int64_t)sizeof(float);
}

extern "C" int inerf_intrinsic_loss(const inerf_loss_args* args, void* stream) {
    using namespace inerf;
    LossParams p;
    const int rc = loss_params(args, false, p);
    if (rc) return rc;
    // (an empty batch is launched too: its terms are the NaNs of torch's empty means)
    hipLaunchKernelGGL(k_intrinsic_loss, dim3(1), dim3(kFwdThreads), 0, (hipStream_t)stream, p);
    return record(hipGetLastError());
}

extern "C" int inerf_intrinsic_loss_backward(const inerf_loss_args* args, void* stream) {
    using namespace inerf;
    LossParams p;
    const int rc = loss_params(args, true, p);
    if (rc) return rc;
    if (p.n == 0) return INERF_OK;
    const long long blocks = (p.n + kBwdThreads - 1) / kBwdThreads;
    hipLaunchKernelGGL(k_intrinsic_loss_bwd, dim3((unsigned)blocks, (unsigned)p.n_levels), dim3(kBwdThreads), 0, (hipStream_t)stream, p);
    return record(hipGetLastError());
}
