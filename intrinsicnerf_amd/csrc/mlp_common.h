// mlp_common.h - shared between the two encode+MLP kernels (mlp.hip: exact fp32 MFMA; mlp_f16.hip:
// f16 hi/lo split operands) and their launcher.
#pragma once
#include <hip/hip_runtime.h>

#include "grid.h"
#include "layout.h"

namespace inerf {

// The probe's cull margin.  The probe culls a point when s < -kappa S.  kappa = 8 x the largest r = |s - sigma| / S: as ONE
// constant, kProbeKappa, the power of two above 8 x the worst r of the networks it was fitted to (profiles/gate_probe_margin.txt) - or, with a
// GateMargin state, 8 x the largest r the listed trunk has measured on THIS packed network's own candidates, once it has seen enough of them.
constexpr float kProbeKappa = 0x1p-6f;              // before a network has been observed, and wherever no state is given
constexpr float kProbeKappaFloor = 0x1p-9f;         // the smallest 8 r of the project's networks (1.56e-3), rounded up to a power of two
constexpr float kProbeFactor = 8.0f;
// Listed points measured before r_max is believed.  On the bench frame r over all listed points of a pass is within 2 x r over its first n
// from n = 2^10 on (profiles/gate_margin_bench.txt section 2); 2^20 is deliberately more: within 1.13 x in both passes, more than any
// small launch lists (those stay on the constant), and reached inside the first sub-range launch of a frame.
constexpr unsigned long long kProbeMinObserved = 1ull << 20;

// INERF_GATE_STATE_BYTES of include/inerf.h: device memory, zero-initialised, one per packed blob.  Written by the kernels alone.
struct GateMargin {
    float r_max;                    // >= 0: the largest finite |s - sigma| / S of a listed point (atomicMax on its bits)
    float kappa_in_use;             // the margin of the launch in flight (k_gate_margin_begin)
    unsigned long long observed;    // listed points measured so far
    unsigned int launches;          // launches that have used this state
    unsigned int reserved[3];
};
static_assert(sizeof(GateMargin) == 32, "INERF_GATE_STATE_BYTES");

// the one statement of the rule (host: inerf_gate_kappa, which the CPU tests pin; device: k_gate_margin_begin)
__host__ __device__ inline float gate_kappa(float r_max, unsigned long long observed, unsigned long long min_observed) {
    const bool finite = r_max - r_max == 0.0f;      // neither NaN nor an infinity
    if (!(observed >= min_observed) || !finite) return kProbeKappa;
    const float k = kProbeFactor * r_max;
    return k > kProbeKappaFloor ? k : kProbeKappaFloor;
}

struct MlpParams {
    const float* wts;       // packed blob
    const float* rays;      // [N,11]
    const float* z;         // [N,S]
    float* raw;             // [N*S, channels]
    int32_t* status;        // optional device word(s) for INERF_STATUS_* bits
    int status_rays;        // 0: one word; > 0: one word per that many rays (inerf_encode_mlp_chunked)
    float* save;            // training forward: activation buffer (layout.h SaveSlot), else nullptr
    float* act_max;         // training forward, optional: device float that receives max |activation| (caller zeroes it)
    float* sem_scratch;     // inference, optional scratch (sem_scratch_bytes): SSR - per-workgroup slots of the channel-split semantic head; object-level 128-point tile - the parked position encoding (sem_scratch_bytes)
    int64_t save_off[SAVE_SLOTS];   // float offsets of the slots for this launch's n_points
    int64_t bits_off;       // float offset of the ReLU-mask area (layout.h relu_bits_offset)
    NetLayout L;
    int n_points;           // N*S  (< 2^31, checked on the host)
    int n_samples;
    int n_tiles;
    int channels;
    int n_classes;
    int endpoint;
    int l_xyz, l_dir;
    float xyz_div;
    // density gate (mlp_f16_t128.hip; object-level f16x3 inference with INERF_FLAG_GATE_COLOUR): a launch is walked in sub-ranges of whole rays
    int ray0;               // global index of this sub-range's first ray: the range words (status_rays) are indexed by global ray
    unsigned char* gate_rec;        // one 1 KB record (h7: 256 f16 hi | 256 f16 lo) per surviving point, in reservation order
    int* gate_idx;                  // ... and its point index within the sub-range
    unsigned int* gate_count;       // the sub-range's survivor count (zeroed by the launcher)
    // ... with INERF_FLAG_GATE_PROBE: the probe kernel's candidates, which the listed trunk walks (appended: the fields above keep their offsets)
    int* cand_idx;                  // point index within the sub-range per candidate, in reservation order
    unsigned int* cand_count;       // the sub-range's candidate count (zeroed by the launcher)
    float* probe_out;               // tests only, optional: [n_points, 2] = (s, S) of the probe per point
    // occupancy grid (mlp_f16_t128.hip kGridTrunk; appended likewise): point gp of the launch is lattice index ray0 + gp of `grid`
    GridSpec grid;
    float grid_dist;                // occ = 1 - exp(-relu(sigma) * grid_dist)
    float* occ;                     // [n_points]
    float* sigma_out;               // [n_points] or nullptr
    // the probe's cull margin per packed network (appended likewise): nullptr = the constant kProbeKappa and no (s, S) list
    GateMargin* gate_state;         // caller-owned, zeroed when the network is packed; the listed trunk measures |s - sigma| / S into it
    float* cand_ss;                 // (s, S) of the probe per candidate, in the order of cand_idx
};

struct GatePlan {
    int64_t rays_per_sub, n_sub;        // sub-ranges of whole rays
    int64_t idx_off, count_off, bytes;  // workspace: records at 0, point indices, one counter per sub-range (fused: neither records nor indices)
    int64_t cand_off, cand_count_off;   // ... the probe's candidate list and its counter per sub-range
    int64_t cand_ss_off;                // ... and the candidates' (s, S), 8 B per point of a sub-range (read only with a GateMargin state)
};
bool mlp_gate_fused(uint32_t flags);                                   // the probe path without records: INERF_FLAG_GATE_PROBE unless INERF_GATE_FUSED=0
GatePlan mlp_gate_plan(int64_t n_rays, int n_samples, bool fused);     // `fused`: 12 B per point of a sub-range instead of 1 040
bool mlp_gate_applies(const inerf_net_desc& net, uint32_t flags);      // which launches the flag changes anything for
int launch_mlp_f16x3_gated(const MlpParams& p, int64_t n_rays, void* gate_ws, bool probe, hipStream_t stream);

// Staggered start of the input-gradient chain.  Every workgroup walks the same stages at the same pace, so the whole chip asks HBM for the same kind of rows at the same moment - 64 KB per CU x 256 CUs is
// 6 000 cycles of HBM whatever the kernel does meanwhile.  A start offset of ((b ^ (b >> 3)) & 7) x units x 2 048 cycles spreads
// those bursts over an eighth of a tile each: chain 2.20 -> 2.04 ms on 393 216 points.
// (No effect on the training forward, whose two workgroups per CU drift apart by themselves: 2.13 vs 2.12 ms.)
#ifdef __HIPCC__
__device__ __forceinline__ void stagger_start(int units) {
    const int b = blockIdx.x;
    for (int d = ((b ^ (b >> 3)) & 7) * units; d > 0; --d) __builtin_amdgcn_s_sleep(32);
}
#endif
int stagger_units(int n_tiles, int grid);       // 0 when a workgroup has fewer than four tiles

// Training entry points: an activation / gradient slot ([n_points, 256] fp32) is addressed through one buffer descriptor
// (32-bit range), so one evaluation kept for a backward pass is limited to this many sample points; callers split larger
// batches into several evaluations (kernels.mlp_train does: parameter gradients add up).
constexpr int64_t kMaxTrainPoints = 4000000;

int device_cus();                 // CU count of the CURRENT device (cached per device id)
int current_device();             // hipGetDevice, 0 on error
int tile_blocks();

// "Has this been done for the current device?" - function attributes (dynamic LDS size) belong to the device a kernel
// is loaded on, and a process may drive several (the Python launchers switch devices per call), so every launcher keeps
// one of these per kernel variant instead of a process-wide bool.  Lock-free; a race only repeats an idempotent call.
struct PerDeviceOnce {
    unsigned long long done[4] = {0, 0, 0, 0};          // bit d of word d/64: devices 0..255
    bool first() {
        const int d = current_device() & 255;
        const unsigned long long bit = 1ull << (d & 63);
        if (__atomic_load_n(&done[d >> 6], __ATOMIC_ACQUIRE) & bit) return false;
        return true;
    }
    void mark() {
        const int d = current_device() & 255;
        __atomic_fetch_or(&done[d >> 6], 1ull << (d & 63), __ATOMIC_RELEASE);
    }
};
int record(hipError_t e);
int launch_mlp_f32(MlpParams& p, int64_t n_points, bool ssr, hipStream_t stream);
int launch_mlp_f16x3(MlpParams& p, int64_t n_points, bool ssr, hipStream_t stream);   // p.save != nullptr: saving variant
int launch_mlp_f16x3_t128(MlpParams& p, int64_t n_points, bool ssr, hipStream_t stream);      // inference on the 128-point tile (mlp_f16_t128.hip)
int launch_grid_trunk_f16x3(MlpParams& p, int64_t n_points, bool ssr, hipStream_t stream);    // ... its occupancy-grid mode: position, trunk, sigma
bool mlp_f16x3_takes_t128(bool ssr, bool save, bool endpoint, int n_classes);                   // which launches take it
int64_t enc_cache_bytes_t128(int64_t n_points);                                                 // object-level inference on the 128-point tile: the parked encoding
int64_t sem_scratch_bytes_t128(int64_t n_points);                                               // ... and the SSR form's scratch (classes > 0)
int64_t sem_scratch_bytes(const inerf_net_desc& net, int64_t n_points, bool endpoint);   // 0 when the launch would not use one

}  // namespace inerf
