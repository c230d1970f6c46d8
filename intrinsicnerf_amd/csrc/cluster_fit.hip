// cluster_fit.hip - mean-shift fitting of the albedo clusters, every class of a manager at once:
//   Cluster_Manager.update_center   SSR/training/cluster.py:52-70   (one Cluster per semantic class, None when empty)
//   Cluster.update_center           cluster.py:138-152              (mapping, bandwidth, MeanShift(bin_seeding=True))
//   choose_anchors                  cluster.py:156-182              (voxel filter: the anchors of the lookup, cluster.hip)
//   mapping_color_np / inv_mapping  cluster.py:316-322, 335-341
// and, underneath, sklearn's estimate_bandwidth (k-th neighbour distance of a 5 000-point subsample), get_bin_seeds,
// _mean_shift_single_seed and the merge of MeanShift.fit.
//
// Pipeline (one stream, no host synchronisation; every grid is sized from n_pixels, kernels read the device-side counts):
//   1. stable partition of the pixels by class (per-chunk class counts, an exclusive scan, a ranked scatter);
//   2. mapping into (I/3*f, g/I, b/I), fp32 without contraction, non-finite values flagged;
//   3. bandwidth: one workgroup per subsample row computes the fp64 distances to the class's subsample and selects the
//      k-th smallest by a bitwise search over the fp64 bit patterns (exact, no sort); a fixed-order mean per class;
//   4. bin seeds: a hash table of (class, round(p/bw)) keeps the first pixel of every bin; the flagged pixels are
//      compacted with the partition of step 1, so the seeds come in the order sklearn's dict produces them;
//   5. mean shift: the points of each class are binned into cells of edge bw*(1+1e-4) (a hash table of cells, the
//      points copied cell by cell), so a step reads 27 cells.  One 256-thread workgroup runs a seed's whole trajectory.
//      Coordinates are summed as 2^-30 fixed-point int64: the sums are exact, so the mean is independent of the order
//      in which the cell's points were scattered (the only atomics that decide placement) - bit-identical runs;
//   6. merge: bitonic sort of (class, count desc, centre desc), then per class the greedy suppression within bw in
//      that order; labels = fp64 nearest surviving centre, lowest index on ties;
//   7. anchors: a hash table of (class, voxel) keeps the minimum of (dist bits, rank) per voxel; the occupied voxels
//      are sorted into (class, voxel) C-order; the centres go back through the inverse mapping.
// Integer atomics only (counts, table claims, min of packed keys): outputs do not depend on scheduling.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "layout.h"

namespace inerf {

int record(hipError_t e);

namespace {

constexpr int kChunk = 1024;           // pixels per partition chunk (one wave walks it in 16 steps of 64)
constexpr int kScanBlock = 1024;       // elements per block of the exclusive scan (256 threads x 4)
constexpr int kMaxSample = 8192;       // subsample size the k-th neighbour kernel holds in registers (32 per thread)
constexpr int kMaxClasses = 255;       // the class sits in 8 bits of the sort keys
constexpr long long kMaxPixels = (1ll << 24) - 1;   // counts sit in 24 bits of the sort keys
constexpr int kMaxIter = 300;          // MeanShift(max_iter=300)
constexpr float kCoordLimit = 256.f;   // |mapped coordinate| bound of the fixed-point sums and the packed bin keys
constexpr double kFix = 1073741824.0;  // 2^30
constexpr double kCellGrow = 1.0001;   // cell edge / bw: a point within bw of the mean is at most one cell away per axis
constexpr int kOff = 1 << 17;          // bias of the packed 18-bit bin / cell coordinates
constexpr unsigned long long kEmpty64 = ~0ull;
constexpr unsigned kEmpty32 = ~0u;

// status bits (out_status[0])
constexpr int kStatNonFinite = 1, kStatRange = 2, kStatSample = 4;

struct ClassInfo {
    double bw;          // bandwidth after band_factor and the 0.01 floor (0 for an empty class)
    double cell;        // cell edge of the mean-shift grid
    int floor_bound;    // 1: bw is the Python float 0.01 (sklearn then bins and seeds in fp32), 0: an np.float64 (fp64)
    int seeds_are_points;
    int pad0, pad1;
};

struct Work {
    int n, K, nchunks, H;
    int* counts;            // [(K+1) * nchunks], scanned in place
    int* scan_tmp;          // block sums of the scans
    int* cls_begin;         // [K+2]
    int* perm;              // [n] pixel index of partition position q
    int* cls;               // [n] class of position q (K = outside every class)
    float4* mapped;         // [n] mapped colour of position q
    int* key32;             // [n] per-position key of the second partition (seed flags); later: labels
    int* seeds;             // [n] partition positions of the seeds, class by class
    int* seed_begin;        // [K+2]
    double* kth;            // [S] k-th neighbour distance of every subsample row
    ClassInfo* info;        // [K]
    unsigned long long* hkey;   // [H] bin / cell keys (64-bit), then the voxel keys (32-bit, aliased)
    int* hval;              // [H] bin table: first rank; cell table: count
    int* hstart;            // [H] cell table: first point (scanned counts)
    int* hcursor;           // [H] cell table: fill cursor
    unsigned long long* vval;   // [H] voxel table: min (dist bits << 32 | rank)
    float4* cellpts;        // [n] points in cell order
    float4* cand;           // [n] (key bits, x, y, z) of every seed's centre; sorted
    int* cand_begin;        // [K+1]
    int* surv;              // [n] candidate index of every survivor, at the class's candidate offset
    int* nsurv;             // [K]
    int* center_begin;      // [K+1]
    float4* centers;        // [n] surviving centres (mapped), back to back
    unsigned long long* vlist;  // [n] occupied voxels (class << 52 | voxel << 32 | rank); sorted
    int* counters;          // [4]: 0 = occupied voxels
    int* status;            // [4] caller's
};

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

__device__ __forceinline__ unsigned long long hash64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// class of a position range table: largest c in [0, K] with begin[c] <= q (begin has K+2 entries, begin[K+1] = total)
__device__ __forceinline__ int find_class(const int* begin, int K, int q) {
    int lo = 0, hi = K + 1;            // invariant: begin[lo] <= q < begin[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (begin[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- 1. stable partition (also used for the seeds)
// key of element i: from int64 labels (null: class 0), or from an int32 key array; anything outside [0, K) -> K
__device__ __forceinline__ int part_key(const long long* lab, const int* key32, int K, int i) {
    long long v = key32 ? (long long)key32[i] : (lab ? lab[i] : 0ll);
    return (v >= 0 && v < K) ? (int)v : K;
}

// one wave per chunk of kChunk elements; pass 0 counts, pass 1 scatters (counts already scanned)
template <bool kScatter>
__global__ __launch_bounds__(64) void k_partition(const long long* __restrict__ lab, const int* __restrict__ key32, int n, int K,
                                                  int nchunks, int* __restrict__ counts, int* __restrict__ out_idx,
                                                  int* __restrict__ out_cls, const int* __restrict__ remap) {
    __shared__ int run[kMaxClasses + 2];
    const int lane = lane_id();
    const int chunk = blockIdx.x;
    for (int c = lane; c <= K; c += 64) run[c] = 0;
    __syncthreads();
    const int base = chunk * kChunk;
    for (int s = 0; s < kChunk; s += 64) {
        const int i = base + s + lane;
        const bool valid = i < n;
        const int key = valid ? part_key(lab, key32, K, i) : -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int first = __ffsll((long long)todo) - 1;
            const int c = __shfl(key, first);
            const unsigned long long members = __ballot(key == c) & todo;
            todo &= ~members;
            const int r = run[c];
            if (kScatter && key == c) {
                const unsigned long long below = members & ((1ull << lane) - 1ull);
                const int pos = counts[c * nchunks + chunk] + r + __popcll(below);
                out_idx[pos] = remap ? remap[i] : i;
                if (out_cls) out_cls[pos] = c;
            }
            __syncthreads();
            if (lane == 0) run[c] = r + __popcll(members);
            __syncthreads();
        }
    }
    if (!kScatter)
        for (int c = lane; c <= K; c += 64) counts[c * nchunks + chunk] = run[c];
}

// begin[c] = scanned counts at (c, chunk 0); begin[K+1] = n
__global__ void k_part_begin(const int* __restrict__ counts, int nchunks, int K, int n, int* __restrict__ begin) {
    for (int c = threadIdx.x; c <= K + 1; c += blockDim.x) begin[c] = c <= K ? counts[c * nchunks] : n;
}

// ---------------------------------------------------------------- exclusive scan of int32 (multi-level, fixed order)
__global__ __launch_bounds__(256) void k_scan_block(int* __restrict__ data, int n, int* __restrict__ sums) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * kScanBlock + t * 4;
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = b0 + j < n ? data[b0 + j] : 0; s += v[j]; }
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                   // Hillis-Steele inclusive scan of the thread totals
        const int add = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (b0 + j < n) data[b0 + j] = run;
        run += v[j];
    }
    if (t == 255 && sums) sums[blockIdx.x] = part[255];
}

__global__ __launch_bounds__(256) void k_scan_add(int* __restrict__ data, int n, const int* __restrict__ sums) {
    const long long i = (long long)blockIdx.x * kScanBlock + threadIdx.x;
    const int add = sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i + 256 * j < n) data[i + 256 * j] += add;
}

long long scan_tmp_ints(long long n) {
    long long t = 0;
    while (n > kScanBlock) { n = (n + kScanBlock - 1) / kScanBlock; t += n; }
    return t + 1;
}

void scan_exclusive(int* data, long long n, int* tmp, hipStream_t st) {
    const long long blocks = (n + kScanBlock - 1) / kScanBlock;
    if (blocks <= 1) {
        hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(256), 0, st, data, (int)n, (int*)nullptr);
        return;
    }
    hipLaunchKernelGGL(k_scan_block, dim3((unsigned)blocks), dim3(256), 0, st, data, (int)n, tmp);
    scan_exclusive(tmp, blocks, tmp + blocks, st);
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)blocks), dim3(256), 0, st, data, (int)n, (const int*)tmp);
}

void partition(const Work& w, const long long* lab, const int* key32, const int* remap, int* out_idx, int* out_cls, int* begin,
               hipStream_t st) {
    hipLaunchKernelGGL(k_partition<false>, dim3(w.nchunks), dim3(64), 0, st, lab, key32, w.n, w.K, w.nchunks, w.counts,
                       (int*)nullptr, (int*)nullptr, remap);
    scan_exclusive(w.counts, (long long)(w.K + 1) * w.nchunks, w.scan_tmp, st);
    hipLaunchKernelGGL(k_partition<true>, dim3(w.nchunks), dim3(64), 0, st, lab, key32, w.n, w.K, w.nchunks, w.counts, out_idx,
                       out_cls, remap);
    hipLaunchKernelGGL(k_part_begin, dim3(1), dim3(256), 0, st, (const int*)w.counts, w.nchunks, w.K, w.n, begin);
}

// ---------------------------------------------------------------- 2. mapping (cluster.py:316-322, numpy fp32)
__global__ void k_map(const float* __restrict__ pixels, Work w, const float* __restrict__ factor) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n) return;
    const int c = w.cls[q];
    if (c >= w.K) return;
    const int p = w.perm[q];
    const float r = pixels[3ll * p], g = pixels[3ll * p + 1], b = pixels[3ll * p + 2];
    const float I = __fadd_rn(__fadd_rn(r, g), b);
    const float d0 = __fmul_rn(__fdiv_rn(I, 3.0f), factor[c]);
    const float d1 = __fdiv_rn(g, I), d2 = __fdiv_rn(b, I);
    w.mapped[q] = make_float4(d0, d1, d2, 0.f);
    const bool finite = isfinite(d0) && isfinite(d1) && isfinite(d2);
    if (!finite) atomicOr(w.status, kStatNonFinite);
    else if (!(fabsf(d0) < kCoordLimit && fabsf(d1) < kCoordLimit && fabsf(d2) < kCoordLimit)) atomicOr(w.status, kStatRange);
}

// ---------------------------------------------------------------- 3. bandwidth (estimate_bandwidth, kd-tree fp64)
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// one workgroup per subsample row j (all classes' rows back to back)
__global__ __launch_bounds__(256) void k_kth(Work w, const int* __restrict__ sidx, const int* __restrict__ sbegin, double quantile) {
    __shared__ int red[4];
    const int j = blockIdx.x;
    const int c = find_class(sbegin, w.K - 1, j);      // sbegin has K+1 entries: classes 0..K-1
    const int s0 = sbegin[c], S = sbegin[c + 1] - s0;
    const int n_c = w.cls_begin[c + 1] - w.cls_begin[c];
    if (S <= 0 || n_c <= 0) return;
    auto point = [&](int i) {
        int r = sidx[s0 + i];
        if (r < 0 || r >= n_c) { if (threadIdx.x == 0) atomicOr(w.status, kStatSample); r = r < 0 ? 0 : n_c - 1; }
        return w.mapped[w.cls_begin[c] + r];
    };
    const float4 me = point(j - s0);
    const double mx = me.x, my = me.y, mz = me.z;
    constexpr int kPer = kMaxSample / 256;
    unsigned long long d[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int i = threadIdx.x + 256 * u;
        d[u] = ~0ull;
        if (i < S) {
            const float4 o = point(i);
            const double dx = mx - (double)o.x, dy = my - (double)o.y, dz = mz - (double)o.z;
            const double r2 = __dadd_rn(__dadd_rn(__dadd_rn(0.0, __dmul_rn(dx, dx)), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            d[u] = (unsigned long long)__double_as_longlong(r2);     // non-negative: the bit pattern orders like the value
        }
    }
    // n_neighbors = max(1, int(len(X) * quantile)); x_(k) = the largest v with #{x < v} < k, built bit by bit
    long long kk = (long long)((double)S * quantile);
    const int k = kk < 1 ? 1 : (kk > S ? S : (int)kk);
    unsigned long long ans = 0;
    for (int bit = 62; bit >= 0; --bit) {
        const unsigned long long t = ans | (1ull << bit);
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < kPer; ++u) cnt += d[u] < t ? 1 : 0;
        if (block_sum_int(cnt, red) < k) ans = t;
    }
    if (threadIdx.x == 0) w.kth[j] = sqrt(__longlong_as_double((long long)ans));
}

// one wave per class: fixed-order mean of the k-th distances, band_factor and the 0.01 floor
__global__ __launch_bounds__(64) void k_bandwidth(Work w, const int* __restrict__ sbegin, double band_factor, double* __restrict__ out_bw) {
    const int c = blockIdx.x;
    const int s0 = sbegin[c], S = sbegin[c + 1] - s0;
    const int n_c = w.cls_begin[c + 1] - w.cls_begin[c];
    double s = 0.0;
    for (int i = lane_id(); i < S; i += 64) s = __dadd_rn(s, w.kth[s0 + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = __dadd_rn(s, __shfl_xor(s, o));
    if (lane_id() != 0) return;
    ClassInfo ci{};
    if (n_c > 0 && S <= 0) atomicOr(w.status, kStatSample);
    if (n_c > 0) {
        const double bw = S > 0 ? __dmul_rn(s / (double)S, band_factor) : 0.0;
        ci.floor_bound = bw < 0.01 ? 1 : 0;                 // max(bandwidth * band_factor, 0.01)
        ci.bw = ci.floor_bound ? 0.01 : bw;
        ci.cell = ci.bw * kCellGrow;
    }
    w.info[c] = ci;
    if (out_bw) out_bw[c] = ci.bw;
}

// ---------------------------------------------------------------- 4. bin seeds (get_bin_seeds, min_bin_freq=1)
__device__ __forceinline__ long long bin_coord(float x, const ClassInfo& ci) {
    // np.round(point / bin_size): fp32 when bin_size is the Python float 0.01, fp64 when it is an np.float64
    if (ci.floor_bound) return (long long)rintf(__fdiv_rn(x, (float)ci.bw));
    return (long long)rint(__ddiv_rn((double)x, ci.bw));
}

__device__ __forceinline__ unsigned long long pack_key(int c, long long a, long long b, long long d) {
    return ((unsigned long long)c << 54) | ((unsigned long long)(a + kOff) << 36) | ((unsigned long long)(b + kOff) << 18) |
           (unsigned long long)(d + kOff);
}

// insert (or find) key; returns the slot
__device__ __forceinline__ int table_slot(unsigned long long* keys, int H, unsigned long long key, bool insert) {
    unsigned long long h = hash64(key) & (unsigned long long)(H - 1);
    for (int probe = 0; probe < H; ++probe) {
        const unsigned long long cur = keys[h];
        if (cur == key) return (int)h;
        if (cur == kEmpty64) {
            if (!insert) return -1;
            const unsigned long long prev = atomicCAS(keys + h, kEmpty64, key);
            if (prev == kEmpty64 || prev == key) return (int)h;
        }
        h = (h + 1) & (unsigned long long)(H - 1);
    }
    return -1;
}

template <bool kFlag>
__global__ void k_bins(Work w) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n) return;
    const int c = w.cls[q];
    if (c >= w.K) { if (kFlag) w.key32[q] = w.K; return; }
    const ClassInfo ci = w.info[c];
    const float4 p = w.mapped[q];
    const unsigned long long key = pack_key(c, bin_coord(p.x, ci), bin_coord(p.y, ci), bin_coord(p.z, ci));
    const int rank = q - w.cls_begin[c];
    const int slot = table_slot(w.hkey, w.H, key, !kFlag);
    if (!kFlag) {
        if (slot >= 0) atomicMin(w.hval + slot, rank);
    } else {
        w.key32[q] = (slot >= 0 && w.hval[slot] == rank) ? c : w.K;     // first pixel of its bin: a seed
    }
}

// ---------------------------------------------------------------- 5. mean shift
__device__ __forceinline__ long long cell_coord(double x, double cell) { return (long long)floor(__ddiv_rn(x, cell)); }

template <int kPass>      // 0: count, 1: scatter
__global__ void k_cells(Work w) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n) return;
    const int c = w.cls[q];
    if (c >= w.K) return;
    const double cell = w.info[c].cell;
    const float4 p = w.mapped[q];
    const unsigned long long key = pack_key(c, cell_coord(p.x, cell), cell_coord(p.y, cell), cell_coord(p.z, cell));
    const int slot = table_slot(w.hkey, w.H, key, kPass == 0);
    if (slot < 0) return;
    if (kPass == 0) atomicAdd(w.hval + slot, 1);
    else w.cellpts[w.hstart[slot] + atomicAdd(w.hcursor + slot, 1)] = p;
}

__device__ __forceinline__ long long fix(float x) { return __double2ll_rn((double)x * kFix); }

__device__ __forceinline__ long long block_sum_ll(long long v, long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const long long s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

// candidate key word: class in bits 24..31, 0xFFFFFF - count in bits 0..23 (ascending = class asc, count desc); ~0 = dropped
__device__ __forceinline__ float key_word(int c, int count) {
    const unsigned k = count > 0 ? ((unsigned)c << 24) | (unsigned)(0xFFFFFF - count) : kEmpty32;
    return __uint_as_float(k);
}

__global__ __launch_bounds__(256) void k_meanshift(Work w) {
    __shared__ long long red[4];
    __shared__ int cstart[27], ccount[27];
    const int T = w.seed_begin[w.K];
    for (int t = blockIdx.x; t < T; t += gridDim.x) {
        const int c = find_class(w.seed_begin, w.K, t);
        const ClassInfo ci = w.info[c];
        const int q = w.seeds[t];
        const float4 p = w.mapped[q];
        double m[3];
        if (ci.seeds_are_points) {              // as many bins as points: sklearn seeds with the points themselves
            m[0] = p.x; m[1] = p.y; m[2] = p.z;
        } else {
            const long long b[3] = {bin_coord(p.x, ci), bin_coord(p.y, ci), bin_coord(p.z, ci)};
            for (int a = 0; a < 3; ++a)         // bin_seeds (fp32) * bin_size: fp32 product for the Python float, fp64 otherwise
                m[a] = ci.floor_bound ? (double)__fmul_rn((float)b[a], (float)ci.bw) : __dmul_rn((double)(float)b[a], ci.bw);
        }
        const double r2max = __dmul_rn(ci.bw, ci.bw);
        const double stop = 1e-3 * ci.bw;
        float mean[3] = {0.f, 0.f, 0.f};
        int count = 0;
        for (int it = 0;; ++it) {
            __syncthreads();
            if (threadIdx.x < 27) {
                const int dx = threadIdx.x % 3 - 1, dy = (threadIdx.x / 3) % 3 - 1, dz = threadIdx.x / 9 - 1;
                const unsigned long long key = pack_key(c, cell_coord(m[0], ci.cell) + dx, cell_coord(m[1], ci.cell) + dy,
                                                        cell_coord(m[2], ci.cell) + dz);
                const int slot = table_slot(w.hkey, w.H, key, false);
                cstart[threadIdx.x] = slot >= 0 ? w.hstart[slot] : 0;
                ccount[threadIdx.x] = slot >= 0 ? w.hval[slot] : 0;
            }
            __syncthreads();
            long long sx = 0, sy = 0, sz = 0;
            int cnt = 0;
            for (int cc = 0; cc < 27; ++cc) {
                const int s0 = cstart[cc], nn = ccount[cc];
                for (int i = threadIdx.x; i < nn; i += 256) {
                    const float4 o = w.cellpts[s0 + i];
                    const double dx = (double)o.x - m[0], dy = (double)o.y - m[1], dz = (double)o.z - m[2];
                    const double r2 = __dadd_rn(__dadd_rn(__dadd_rn(0.0, __dmul_rn(dx, dx)), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                    if (r2 <= r2max) { sx += fix(o.x); sy += fix(o.y); sz += fix(o.z); ++cnt; }
                }
            }
            sx = block_sum_ll(sx, red); sy = block_sum_ll(sy, red); sz = block_sum_ll(sz, red);
            const int n_in = (int)block_sum_ll(cnt, red);
            count = n_in;
            if (n_in == 0) break;                       // no point within bw: the seed is dropped
            const double den = (double)n_in * kFix;
            const float nm[3] = {(float)((double)sx / den), (float)((double)sy / den), (float)((double)sz / den)};
            const double ex = (double)nm[0] - m[0], ey = (double)nm[1] - m[1], ez = (double)nm[2] - m[2];
            const double shift = sqrt(ex * ex + ey * ey + ez * ez);
            for (int a = 0; a < 3; ++a) { mean[a] = nm[a]; m[a] = nm[a]; }
            if (shift <= stop || it == kMaxIter) break;
        }
        if (threadIdx.x == 0) w.cand[t] = make_float4(key_word(c, count), mean[0], mean[1], mean[2]);
    }
}

// ---------------------------------------------------------------- bitonic sort (ascending, in place, device-side length)
// Every comparison puts the smaller element at the lower index, so positions >= len act as +infinity and are never touched.
__device__ __forceinline__ bool cand_less(const float4& a, const float4& b) {
    const unsigned ka = __float_as_uint(a.x), kb = __float_as_uint(b.x);
    if (ka != kb) return ka < kb;
    if (a.y != b.y) return a.y > b.y;       // centre tuple descending
    if (a.z != b.z) return a.z > b.z;
    return a.w > b.w;
}
__device__ __forceinline__ bool elem_less(const float4& a, const float4& b) { return cand_less(a, b); }
__device__ __forceinline__ bool elem_less(unsigned long long a, unsigned long long b) { return a < b; }

template <typename E>
__global__ __launch_bounds__(256) void k_bitonic(E* __restrict__ data, const int* __restrict__ len_ptr, int len_offset, int k, int j, int flip) {
    const int len = len_ptr[len_offset];
    const long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long lo, hi;
    if (flip) {              // first step of a merge of size k: mirror partner
        const long long half = k >> 1;
        const long long blk = pair / half, off = pair % half;
        lo = blk * k + off;
        hi = blk * k + (k - 1 - off);
    } else {
        const long long blk = pair / j, off = pair % j;
        lo = blk * 2 * j + off;
        hi = lo + j;
    }
    if (hi >= len) return;
    const E a = data[lo], b = data[hi];
    if (elem_less(b, a)) { data[lo] = b; data[hi] = a; }
}

template <typename E>
void bitonic_sort(E* data, const int* len_ptr, int len_offset, long long cap, hipStream_t st) {
    long long P = 1;
    while (P < cap) P <<= 1;
    const unsigned blocks = (unsigned)((P / 2 + 255) / 256);
    for (long long k = 2; k <= P; k <<= 1) {
        hipLaunchKernelGGL(k_bitonic<E>, dim3(blocks), dim3(256), 0, st, data, len_ptr, len_offset, (int)k, (int)(k >> 1), 1);
        for (long long j = k >> 2; j >= 1; j >>= 1)
            hipLaunchKernelGGL(k_bitonic<E>, dim3(blocks), dim3(256), 0, st, data, len_ptr, len_offset, (int)k, (int)j, 0);
    }
}

// ---------------------------------------------------------------- 6. merge, labels
__device__ __forceinline__ int cand_class(const float4& e) {
    const unsigned k = __float_as_uint(e.x);
    return k == kEmpty32 ? INT_MAX : (int)(k >> 24);
}

// cand_begin[c] = first sorted candidate of class >= c (c = 0..K)
__global__ void k_cand_begin(Work w) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > w.K) return;
    int lo = 0, hi = w.seed_begin[w.K];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cand_class(w.cand[mid]) < c) lo = mid + 1; else hi = mid;
    }
    w.cand_begin[c] = lo;
}

// one workgroup per class: greedy suppression in sorted order (MeanShift.fit: each still-unique centre removes every
// other centre within bw); `alive` is the class's range of key32
__global__ __launch_bounds__(256) void k_merge(Work w) {
    __shared__ int next_alive;
    const int c = blockIdx.x;
    const int b = w.cand_begin[c], e = w.cand_begin[c + 1];
    int* alive = w.key32;
    for (int i = b + threadIdx.x; i < e; i += 256) alive[i] = 1;
    const double r2max = __dmul_rn(w.info[c].bw, w.info[c].bw);
    int ns = 0;
    int i = b;
    while (true) {
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x == 0) next_alive = INT_MAX;
        __syncthreads();
        if (i + (int)threadIdx.x < e && alive[i + threadIdx.x]) atomicMin(&next_alive, i + (int)threadIdx.x);
        __syncthreads();
        const int s = next_alive;
        if (s == INT_MAX) {
            if (i + 256 >= e) break;
            i += 256;
            continue;
        }
        if (threadIdx.x == 0) w.surv[b + ns] = s;
        ++ns;
        const float4 cs = w.cand[s];
        for (int j = s + 1 + threadIdx.x; j < e; j += 256) {
            if (!alive[j]) continue;
            const float4 o = w.cand[j];
            const double dx = (double)o.y - (double)cs.y, dy = (double)o.z - (double)cs.z, dz = (double)o.w - (double)cs.w;
            const double r2 = __dadd_rn(__dadd_rn(__dadd_rn(0.0, __dmul_rn(dx, dx)), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            if (r2 <= r2max) alive[j] = 0;
        }
        i = s + 1;
    }
    if (threadIdx.x == 0) w.nsurv[c] = ns;
}

__global__ void k_center_begin(Work w, int* __restrict__ out_center_begin) {
    if (threadIdx.x != 0) return;
    int run = 0;
    for (int c = 0; c < w.K; ++c) {
        w.center_begin[c] = run;
        if (out_center_begin) out_center_begin[c] = run;
        run += w.nsurv[c];
    }
    w.center_begin[w.K] = run;
    if (out_center_begin) out_center_begin[w.K] = run;
}

// survivors -> back to back centres: mapped (for the labels and the caller) and inverse-mapped rgb (cluster.py:335-341)
__global__ void k_centers_out(Work w, const float* __restrict__ factor, float* __restrict__ out_rgb, float* __restrict__ out_mapped,
                              int* __restrict__ out_count) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= w.center_begin[w.K]) return;
    const int c = find_class(w.center_begin, w.K - 1, o);
    const float4 e = w.cand[w.surv[w.cand_begin[c] + o - w.center_begin[c]]];
    w.centers[o] = make_float4(e.y, e.z, e.w, 0.f);
    const float I = __fdiv_rn(__fmul_rn(e.y, 3.0f), factor[c]);
    const float g = __fmul_rn(e.z, I), b = __fmul_rn(e.w, I);
    const float r = __fsub_rn(__fsub_rn(I, g), b);
    auto clamp01 = [](float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); };
    if (out_rgb) { out_rgb[3ll * o] = clamp01(r); out_rgb[3ll * o + 1] = clamp01(g); out_rgb[3ll * o + 2] = clamp01(b); }
    if (out_mapped) { out_mapped[3ll * o] = e.y; out_mapped[3ll * o + 1] = e.z; out_mapped[3ll * o + 2] = e.w; }
    if (out_count) out_count[o] = 0xFFFFFF - (int)(__float_as_uint(e.x) & 0xFFFFFF);
}

// labels_: nearest surviving centre in fp64, the lowest index on ties; stored in key32 (partition order)
__global__ void k_labels(Work w, int* __restrict__ out_pixel_label) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n) return;
    const int c = w.cls[q];
    if (c >= w.K) { if (out_pixel_label) out_pixel_label[w.perm[q]] = -1; return; }
    const float4 p = w.mapped[q];
    const int b = w.center_begin[c], e = w.center_begin[c + 1];
    double best = 0.0;
    int arg = -1;
    for (int i = b; i < e; ++i) {
        const float4 o = w.centers[i];
        const double dx = (double)p.x - (double)o.x, dy = (double)p.y - (double)o.y, dz = (double)p.z - (double)o.z;
        const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        if (arg < 0 || r2 < best) { best = r2; arg = i - b; }
    }
    w.key32[q] = arg;
    if (out_pixel_label) out_pixel_label[w.perm[q]] = arg;
}

// ---------------------------------------------------------------- 7. anchors (choose_anchors, cluster.py:156-182)
__device__ __forceinline__ int voxel_axis(float x) {
    const float v = __fdiv_rn(x, 0.01f);                 // (pixels / leaf_size).long(): fp32 division, truncation
    long long id = (long long)v;
    return (int)(id < 0 ? 0 : (id > 99 ? 99 : id));
}
__device__ __forceinline__ float voxel_term(int id, float x) {
    // id * leaf_size + half_leaf_size - pixel, squared (fp32, torch's scalar promotion)
    const float ctr = __fadd_rn(__fmul_rn((float)id, 0.01f), 0.005f);
    const float d = __fsub_rn(ctr, x);
    return __fmul_rn(d, d);
}

template <int kPass>      // 0: min per voxel, 1: collect occupied voxels
__global__ void k_voxels(Work w) {
    unsigned* keys = reinterpret_cast<unsigned*>(w.hkey);
    if (kPass == 1) {
        const int h = blockIdx.x * blockDim.x + threadIdx.x;
        if (h >= w.H || keys[h] == kEmpty32) return;
        const unsigned long long v = w.vval[h];
        const int slot = atomicAdd(w.counters, 1);
        w.vlist[slot] = ((unsigned long long)keys[h] << 32) | (v & 0xFFFFFFFFull);
        return;
    }
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n) return;
    const int c = w.cls[q];
    if (c >= w.K) return;
    const float4 p = w.mapped[q];
    const int ix = voxel_axis(p.x), iy = voxel_axis(p.y), iz = voxel_axis(p.z);
    const float dist = __fadd_rn(__fadd_rn(voxel_term(ix, p.x), voxel_term(iy, p.y)), voxel_term(iz, p.z));
    const unsigned key = ((unsigned)c << 20) | (unsigned)((ix * 100 + iy) * 100 + iz);
    const unsigned long long val = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)(q - w.cls_begin[c]);
    unsigned h = (unsigned)(hash64(key) & (unsigned long long)(w.H - 1));
    for (int probe = 0; probe < w.H; ++probe) {
        unsigned cur = keys[h];
        if (cur == kEmpty32) {
            const unsigned prev = atomicCAS(keys + h, kEmpty32, key);
            cur = prev == kEmpty32 ? key : prev;
        }
        if (cur == key) { atomicMin(w.vval + h, val); return; }
        h = (h + 1) & (unsigned)(w.H - 1);
    }
}

// anchor_begin[c] = first sorted voxel of class >= c
__global__ void k_anchor_begin(Work w, int* __restrict__ out_anchor_begin) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > w.K) return;
    int lo = 0, hi = w.counters[0];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)(w.vlist[mid] >> 52) < c) lo = mid + 1; else hi = mid;
    }
    out_anchor_begin[c] = lo;
}

__global__ void k_anchors_out(Work w, float* __restrict__ out_anchors, long long* __restrict__ out_links) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= w.counters[0]) return;
    const unsigned long long v = w.vlist[a];
    const int c = (int)(v >> 52);
    const int q = w.cls_begin[c] + (int)(v & 0xFFFFFFFFull);
    const float4 p = w.mapped[q];
    out_anchors[3ll * a] = p.x; out_anchors[3ll * a + 1] = p.y; out_anchors[3ll * a + 2] = p.z;
    out_links[a] = w.key32[q];
}

// seeds_are_points per class (get_bin_seeds: as many bins as points -> the points themselves)
__global__ void k_seed_info(Work w) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.K) return;
    const int n_c = w.cls_begin[c + 1] - w.cls_begin[c];
    w.info[c].seeds_are_points = n_c > 0 && (w.seed_begin[c + 1] - w.seed_begin[c]) == n_c;
}

__global__ void k_class_stats(Work w, int* __restrict__ stats) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.K) return;
    stats[4 * c + 0] = w.cls_begin[c + 1] - w.cls_begin[c];
    stats[4 * c + 1] = w.seed_begin[c + 1] - w.seed_begin[c];
    stats[4 * c + 2] = w.cand_begin[c + 1] - w.cand_begin[c];
    stats[4 * c + 3] = w.nsurv[c];
}

// ---------------------------------------------------------------- workspace
long long pow2_at_least(long long v) { long long p = 1; while (p < v) p <<= 1; return p; }

// the workspace, carved in one fixed order; with base == nullptr only the size is computed
long long layout(long long n, int K, long long n_sample, char* base, Work* w) {
    long long bytes = 0;
    auto take = [&](auto*& ptr, long long count) {
        using T = std::remove_reference_t<decltype(*ptr)>;
        if (base) ptr = reinterpret_cast<T*>(base + bytes);
        bytes += ((long long)sizeof(T) * (count > 0 ? count : 1) + 255) & ~255ll;
    };
    Work tmp{};
    Work& d = w ? *w : tmp;
    const long long nchunks = (n + kChunk - 1) / kChunk;
    const long long H = pow2_at_least(2 * n < 1024 ? 1024 : 2 * n);
    const long long ncount = (K + 1) * nchunks;
    take(d.counts, ncount);
    take(d.scan_tmp, scan_tmp_ints(ncount > H ? ncount : H));
    take(d.cls_begin, K + 2);
    take(d.perm, n);
    take(d.cls, n);
    take(d.mapped, n);
    take(d.key32, n);
    take(d.seeds, n);
    take(d.seed_begin, K + 2);
    take(d.kth, n_sample);
    take(d.info, K);
    take(d.hkey, H);
    take(d.hval, H);
    take(d.hstart, H);
    take(d.hcursor, H);
    take(d.vval, H);
    take(d.cellpts, n);
    take(d.cand, n);
    take(d.cand_begin, K + 1);
    take(d.surv, n);
    take(d.nsurv, K);
    take(d.center_begin, K + 1);
    take(d.centers, n);
    take(d.vlist, n);
    take(d.counters, 4);
    return bytes;
}

}  // namespace
}  // namespace inerf

extern "C" int64_t inerf_cluster_fit_workspace_bytes(int64_t n_pixels, int n_classes, int64_t n_sample_idx) {
    using namespace inerf;
    if (n_pixels < 1 || n_pixels > kMaxPixels || n_classes < 1 || n_classes > kMaxClasses || n_sample_idx < 0) return INERF_E_INVALID;
    return layout(n_pixels, n_classes, n_sample_idx, nullptr, nullptr);
}

extern "C" int inerf_cluster_fit(const inerf_cluster_fit_args* a, void* stream) {
    using namespace inerf;
    if (!a) return INERF_E_INVALID;
    const long long n = a->n_pixels;
    const int K = a->n_classes;
    if (n < 1 || K < 1 || !a->pixels || !a->sample_idx || !a->sample_begin || !a->factor || !a->status || !a->out_center_begin ||
        !a->out_anchor_begin || !a->out_bandwidth || a->n_sample_idx < 0 || !(a->quantile > 0.0 && a->quantile <= 1.0) ||
        !(a->band_factor > 0.0 && a->band_factor < 1e30))
        return INERF_E_INVALID;
    if (n > kMaxPixels || K > kMaxClasses) return INERF_E_UNSUPPORTED;
    if (a->max_class_samples > kMaxSample || a->max_class_samples < 0) return INERF_E_UNSUPPORTED;
    if (a->n_sample_idx > 0 && (!a->out_centers || !a->out_anchors || !a->out_links)) return INERF_E_INVALID;
    const long long need = inerf_cluster_fit_workspace_bytes(n, K, a->n_sample_idx);
    if (!a->workspace || a->workspace_bytes < need) return INERF_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    Work w{};
    w.n = (int)n; w.K = K; w.nchunks = (int)((n + kChunk - 1) / kChunk);
    w.H = (int)pow2_at_least(2 * n < 1024 ? 1024 : 2 * n);
    w.status = a->status;
    layout(n, K, a->n_sample_idx, static_cast<char*>(a->workspace), &w);
    const unsigned nb = (unsigned)((n + 255) / 256), hb = (unsigned)((w.H + 255) / 256);
    const unsigned kb = (unsigned)((K + 1 + 255) / 256);
    const long long S = a->n_sample_idx;
    hipError_t err = hipSuccess;
    auto chk = [&](hipError_t e) { if (err == hipSuccess) err = e; };
    chk(hipMemsetAsync(w.status, 0, 4 * sizeof(int), st));
    chk(hipMemsetAsync(w.counters, 0, 16, st));

    // 1. stable partition by class; 2. mapping
    partition(w, reinterpret_cast<const long long*>(a->labels), nullptr, nullptr, w.perm, w.cls, w.cls_begin, st);
    hipLaunchKernelGGL(k_map, dim3(nb), dim3(256), 0, st, a->pixels, w, a->factor);
    // 3. bandwidth
    if (S > 0) hipLaunchKernelGGL(k_kth, dim3((unsigned)S), dim3(256), 0, st, w, a->sample_idx, a->sample_begin, a->quantile);
    hipLaunchKernelGGL(k_bandwidth, dim3(K), dim3(64), 0, st, w, a->sample_begin, a->band_factor, a->out_bandwidth);
    // 4. bin seeds: first pixel of each (class, bin), compacted in partition order
    chk(hipMemsetAsync(w.hkey, 0xFF, 8ll * w.H, st));
    chk(hipMemsetAsync(w.hval, 0x7F, 4ll * w.H, st));
    hipLaunchKernelGGL(k_bins<false>, dim3(nb), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_bins<true>, dim3(nb), dim3(256), 0, st, w);
    partition(w, nullptr, w.key32, nullptr, w.seeds, nullptr, w.seed_begin, st);
    hipLaunchKernelGGL(k_seed_info, dim3(kb), dim3(256), 0, st, w);
    // 5. cells of the mean-shift grid, then the trajectories
    chk(hipMemsetAsync(w.hkey, 0xFF, 8ll * w.H, st));
    chk(hipMemsetAsync(w.hval, 0, 4ll * w.H, st));
    chk(hipMemsetAsync(w.hcursor, 0, 4ll * w.H, st));
    hipLaunchKernelGGL(k_cells<0>, dim3(nb), dim3(256), 0, st, w);
    chk(hipMemcpyAsync(w.hstart, w.hval, 4ll * w.H, hipMemcpyDeviceToDevice, st));
    scan_exclusive(w.hstart, w.H, w.scan_tmp, st);
    hipLaunchKernelGGL(k_cells<1>, dim3(nb), dim3(256), 0, st, w);
    const unsigned ms_blocks = (unsigned)(n < 4096 ? n : 4096);
    hipLaunchKernelGGL(k_meanshift, dim3(ms_blocks), dim3(256), 0, st, w);
    // 6. merge and labels
    bitonic_sort(w.cand, w.seed_begin, K, n, st);
    hipLaunchKernelGGL(k_cand_begin, dim3(kb), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_merge, dim3(K), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_center_begin, dim3(1), dim3(64), 0, st, w, a->out_center_begin);
    hipLaunchKernelGGL(k_centers_out, dim3(nb), dim3(256), 0, st, w, a->factor, a->out_centers,
                       a->out_mapped_centers, a->out_center_counts);
    hipLaunchKernelGGL(k_labels, dim3(nb), dim3(256), 0, st, w, a->out_pixel_label);
    // 7. anchors
    chk(hipMemsetAsync(w.hkey, 0xFF, 4ll * w.H, st));
    chk(hipMemsetAsync(w.vval, 0xFF, 8ll * w.H, st));
    hipLaunchKernelGGL(k_voxels<0>, dim3(nb), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_voxels<1>, dim3(hb), dim3(256), 0, st, w);
    bitonic_sort(w.vlist, w.counters, 0, n, st);
    hipLaunchKernelGGL(k_anchor_begin, dim3(kb), dim3(256), 0, st, w, a->out_anchor_begin);
    hipLaunchKernelGGL(k_anchors_out, dim3(nb), dim3(256), 0, st, w, a->out_anchors, reinterpret_cast<long long*>(a->out_links));
    if (a->out_class_stats) hipLaunchKernelGGL(k_class_stats, dim3(kb), dim3(256), 0, st, w, a->out_class_stats);
    chk(hipGetLastError());
    return record(err);
}
