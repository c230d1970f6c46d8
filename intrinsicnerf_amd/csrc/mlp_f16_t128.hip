// mlp_f16_t128.hip - the inference form of the split-f16 encode+MLP kernel on a 128-POINT tile (round 6).
//
// Why: in k_encode_mlp_f16x3_dual (mlp_f16.hip) every wave pulls 4 KiB of weight fragments from L2 per 12 MFMAs - 2.65 MB per
// 64-point tile, 43 B/clk/CU at the full matrix rate against an L2 that delivers ~56 B/clk/CU with every CU asking - and the
// matrix pipe waits for them a third of the time (profiles/r01_mfma_mix_microbench.txt, r06_weight_stream_*.txt).  Here ONE workgroup of
// EIGHT waves walks 128 points through the same 14 GEMMs: a wave owns 32 output channels x all 128 points of a 256-wide layer
// (1 row block x 4 point blocks), so a weight fragment feeds four point blocks instead of two - 2 KiB per 12 MFMAs, half the
// L2 -> CU stream - and the operand reads that double instead (8 ds_read_b128 per 12 MFMAs) go to LDS, whose 256 B/clk for
// that instruction is a quarter used.  151,552 B of LDS, one workgroup per CU, two waves per SIMD (<= 256 registers each).
//
// Object-level network and the SSR network with <= 32 classes (no endpoint feature).
// Same arithmetic, same summation order per output element as the 64-point kernels (the packed blob is the same one: wave
// w8 reads row block w8 & 1 of packing wave w8 >> 1):  the results are bit-identical to k_encode_mlp_f16x3_dual's.  To keep
// that true for the two heads whose hidden layers stay in registers (albedo | shading hidden, view-dependent hidden: their
// output sums are formed per 64- / 32-channel group, in group order), those two layers keep the 64-point kernel's wave tile -
// channel group w8 & 3 x point half w8 >> 2 - and stream their weights twice per tile (15 % of the FLOPs).
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "mlp_f16_dev.h"
#include "mlp_f16_heads.h"
#include "mlp_f16_pp.h"

#ifndef INERF_T128_PEEL
#define INERF_T128_PEEL 1       // (0: development builds for A/B runs)
#endif
#ifndef INERF_GATE_TRUNK_PARK
#define INERF_GATE_TRUNK_PARK 1 // (0: development builds for A/B runs - the gated trunk evaluates the encoder again at the skip layer)
#endif

namespace inerf {

constexpr int kPtsT = 128;                       // points per tile
constexpr int kPlaneT = kPtsT * kRowD;           // halfs per plane (rows of 296 halfs = 592 B: conflict-free ds_read_b128)
constexpr int kLdsBytesT = 2 * kPlaneT * 2;      // 151,552
constexpr int kSemScratchBytesT = 8 * 2 * 16 * 64 * 4;      // SSR: per workgroup 64 KiB - per wave [2 point blocks][16 registers][64 lanes] floats

// Object-level inference: the tile's position encoding (columns 0..63 of both planes: 32 KiB) parked in an L2-resident slot per workgroup
// between the first layer and the skip layer, which needs it again after the layers in between overwrote it in place - 4 LDS reads + 4
// stores + 4 loads + 4 LDS writes of 16 bytes per thread instead of a second evaluation of the encoder (~540 VALU instructions and 42
// two-byte LDS writes per thread; the kernel is bound by instruction issue: profiles/r06_pp_pipeline.txt).  The same bits.
constexpr int kEncCacheBytesT = 2 * kPtsT * kEncCols * 2;      // 32,768 per workgroup
int64_t enc_cache_bytes_t128(int64_t n_points) {
    const int64_t tiles = (n_points + kPtsT - 1) / kPtsT;
    return (tiles < device_cus() ? tiles : device_cus()) * (int64_t)kEncCacheBytesT;
}

// Gated trunk (kMode == kGateTrunk below): the same 32 KiB parked in LDS instead.  The trunk kernel never runs the heads, so while its
// layers run the 32 direction columns and the 8 pad halfs behind them (columns 256..295, 80 B per row and plane) are dead: five of a
// row's eight sixteen-byte pieces go there, the other three into an extension area behind the two planes - piece (j - 5) of
// [plane][row][3].  That is the CU's whole LDS: 151,552 + 12,288 = 163,840 B (the trunk kernel's launch size only).
constexpr int kParkRowPieces = (kDirCols + 8) / 8;                       // 5: columns 256..295 of the piece's own row and plane
constexpr int kParkExtPieces = kEncCols / 8 - kParkRowPieces;            // 3
constexpr int kParkExtBytes = 2 * kPtsT * kParkExtPieces * 16;           // 12,288
constexpr int kLdsBytesTrunk = kLdsBytesT + (INERF_GATE_TRUNK_PARK ? kParkExtBytes : 0);
static_assert(kLdsBytesTrunk <= 160 * 1024, "the parked encoding must fit the CU's LDS");
static_assert(kColDirD + 8 * kParkRowPieces <= kRowD && kParkRowPieces > 0 && kParkExtPieces >= 0, "parked pieces stay inside their row");

int64_t sem_scratch_bytes_t128(int64_t n_points) {
    const int64_t tiles = (n_points + kPtsT - 1) / kPtsT;
    return (tiles < device_cus() ? tiles : device_cus()) * (int64_t)kSemScratchBytesT;
}

// kSsr: the SSR network (Semantic_NeRF, semantic_nerf.py:74-181) with at most 32 classes and no endpoint feature: xyz / 10 in the
// encoder, and between the albedo|shading head and the feature layer the semantic head - hidden layer (128 channels) split over the
// waves like the view-dependent one (32-channel group cg x 64-point half ph: semantic_linear.0.0 streamed twice per 128 points; the
// 64-point kernel streams it twice per 64), the wave's hidden channels stay in registers as B operands of the logits product
// (layout.h sem2q), and its PARTIAL logits (32 classes x 64 points over 32 hidden channels: 32 accumulator registers) are parked in
// the wave's own L2-resident scratch slot (MlpParams.sem_scratch: 8 KiB per wave - an explicit spill placed where nothing waits for
// it; held in registers across the feature and view layers they cost 48 spilled registers inside those loops) until the tile's planes
// are dead, where the four partials of a point meet in LDS and are added in group order.
// kSave (object-level network): the training forward - every layer's output also leaves as operand fragments of the weight-gradient
// products, the ReLU masks of h0..h7 as bits (mlp_f16.hip, k_encode_mlp_f16x3_dual<true, ..>): the SAME bytes at the same addresses
// as the 64-point kernel writes (a 128-point tile is two of the slots' 64-point tiles; this wave's 32 channels are one channel block
// of a fragment, one of the two mask words of a lane), so the chain and the weight-gradient kernels read either forward's buffer.
// kPipe (object-level inference, INERF_F16_KERNEL=pp): the trunk as a software pipeline over the tile's two 64-point halves - each half's
// epilogue is issued between the MFMAs of the other half's GEMM (mlp_f16_pp.h).  Same values, same summation order: bit-identical results.
//
// kMode (density gate, object-level inference: DESIGN.md 3.1c) - the ONE tile body serves three kernels, so the gated pair computes
// with the same instructions in the same order as the whole kernel:
//   kWhole      encode, trunk, heads: everything of a tile, as above
//   kGateTrunk  encode (position only: nothing here reads the direction columns), trunk with the encoding parked in LDS for the skip layer
//               (kPark below), then only sigma: raw[pt] = (0, 0, 0, sigma, 0 ...).  A point SURVIVES when !(sigma <= 0) (a NaN survives);
//               the tile's survivors are counted by ballot, one lane reserves their contiguous record range with one atomicAdd on
//               MlpParams.gate_count, and each survivor's h7 row leaves exactly as the epilogue left it in the planes (256 f16 hi |
//               256 f16 lo = 1 KB, sixteen-byte stores) together with its point index
//   kGateHeads  walks ceil(*gate_count / 128) tiles of records: rows back into the planes, the direction encoding again from point
//               index -> ray, then the heads; the ten colour channels go to raw[index].  Rows past the count are computed on the last
//               record and not stored.  The range guard is per POINT here (a tile holds points of rays from anywhere in the launch).
//   kGateProbe  (INERF_FLAG_GATE_PROBE) settles sigma's SIGN for most points at a third of the trunk's matrix work: position encoding and the
//               eight layers on hi operands alone (ONE product per MAC, activations rounded to nearest into the hi plane; the lo plane
//               holds nothing but a copy of the encoding, which the skip layer reads there), then s = the alpha product on hi operands
//               and S = the same product on |weights| and |bias|.  raw[pt] = (0, 0, 0, s, 0 ...); a point is a CANDIDATE when
//               !(s < -kProbeKappa * S) (a NaN or an infinity is one): its index goes into a list, reserved like the records.  Every
//               other point's exact sigma is negative (the margin: profiles/gate_probe_margin.txt), which is all the frame needs of it.
//   kGateTrunk with kListed: persistent over ceil(*cand_count / 128) tiles of the candidate list - a row's point comes from the list, its
//               exact sigma is scattered into that point's raw row, its record carries the original index (the heads kernel is the same).
//               A point's column of every GEMM depends on that point alone: the same bits as the unlisted trunk's.
//   kGridTrunk  (occupancy grid of mesh extraction, both networks: inerf_occupancy_grid) kGateTrunk up to and including sigma on the points of
//               a lattice: point gp is lattice index ray0 + gp (grid_point(), grid.h; SSR: / xyz_div), and all that leaves is
//               occ[gp] = 1 - exp(-relu(sigma) grid_dist) and, when asked for, sigma_out[gp] - no raw rows, no records, no atomics.
//   kGateWhole  (always kListed; the probe path's second launch unless INERF_GATE_FUSED=0) the listed trunk and the gated heads in ONE tile body:
//               a listed row's h7 goes from the planes straight into the heads - no record, no survivor list.  Position encoding parked in LDS
//               like the gated trunk's; the direction encoding (and the point's range words) is written once the parked pieces have left the
//               direction columns, in front of layer 7's GEMM.  Exact sigma goes to the candidate's raw row always, the ten colour channels
//               only when !(sigma <= 0): every other candidate keeps the probe's zeros, and raises no range flag behind h7 (its heads were not
//               evaluated at all when they were a launch of their own).  Survivors are counted per workgroup: one atomicAdd at kernel exit.
enum : int { kWhole = 0, kGateTrunk = 1, kGateHeads = 2, kGateProbe = 3, kGridTrunk = 4, kGateWhole = 5 };
constexpr int kGateRecordBytes = 2 * kWidth * 2;      // 1 024
// (the probe's margin, kProbeKappa or a GateMargin state's kappa_in_use: mlp_common.h)

// The margin of the launch in flight: p.gate_state's kappa_in_use (written by k_gate_margin_begin in front of the launch's first probe kernel
// on the stream, the same for every sub-range), read once per kernel like the counts; without a state the constant.
__device__ __forceinline__ float probe_kappa(const MlpParams& p) {
    if (!p.gate_state) return kProbeKappa;
    const unsigned bits = *reinterpret_cast<const volatile unsigned*>(&p.gate_state->kappa_in_use);
    return __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_readfirstlane((int)bits));
}

}  // namespace inerf
#include "mlp_f16_gate.h"       // the pieces the gate's kernels share: encoder, parking, probe trunk, raw rows, slots
namespace inerf {

template <bool kSsr, bool kSave, bool kPipe, int kMode, bool kListed = false>
__device__ __forceinline__ void encode_mlp_t128_tiles(const MlpParams& p) {
    static_assert(!(kSsr && kSave), "the saving form is the object-level network's");
    static_assert(!kPipe || (!kSsr && !kSave), "the pipelined trunk is the object-level inference form");
    static_assert(kMode == kWhole || kMode == kGridTrunk || (!kSsr && !kSave && !kPipe), "the density gate is the object-level inference form's");
    static_assert(kMode != kGridTrunk || (!kSave && !kPipe), "the occupancy grid is an inference form");
    static_assert(kListed ? kMode == kGateTrunk || kMode == kGateWhole : kMode != kGateWhole, "the candidate list feeds the gated trunk, alone or with the heads behind it");
    constexpr bool kNoDirAtEncode = kMode == kGateTrunk || kMode == kGateProbe || kMode == kGridTrunk || kMode == kGateWhole;
    constexpr bool kPointGuard = kMode == kGateHeads || kMode == kGateWhole;      // the heads' range guard is per point (rows from anywhere in the launch)
    constexpr int kParts = 512 / kPtsT;
    // the wide GEMMs' first products take a zero C operand instead of 64 v_mov in front of every GEMM (wide_gemm_h PEEL): +1.3 % same-box,
    // same bits (profiles/r06_peel_ab.txt); the saving form keeps the explicit zeroing like the two-workgroup one
    constexpr bool kPeel = INERF_T128_PEEL && !kSave;
    extern __shared__ __attribute__((aligned(16))) _Float16 ldst[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..7
    const int cg = wave & 3, ph = wave >> 2;                        // heads' hidden layers: channel group x point half
    const NetLayout& L = p.L;

    _Float16* const xw = ldst + (lane & 31) * kRowD;
    const _Float16* const xr = xw + 8 * (lane >> 5);                       // wide GEMM operand reads (+ column)
    _Float16* const xd = xw + 4 * (lane >> 5) + 32 * wave;                 // wide stores: this wave's 32 channels

    WeightBuf wb;
    wb.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wts), 0, L.total_floats * 4, 0x00020000);
    wb.voff = lane * 16;
    // this wave's 32-channel stream of a 256-wide layer: row block (wave & 1) of packing wave (wave >> 1), k-blocks 4 KiB apart
    auto frag32 = [&](const GemmSlot& s, int kbt) { return (s.w + (wave >> 1) * kbt * 2 * 2 * 256) * 4 + (wave & 1) * 2048; };
    auto frag256 = [&](const GemmSlot& s, int kbt) { return (s.w + cg * kbt * 2 * 2 * 256) * 4; };       // 64-channel group cg
    auto frag128 = [&](const GemmSlot& s, int kbt) { return (s.w + cg * kbt * 1 * 2 * 256) * 4; };       // 32-channel group cg of a 128-wide layer

    WidePreH<1> pre1;
    WidePreH<2> pre2;
    if constexpr (kMode == kGateHeads)      prefetch_w<2>(pre2, wb, frag256(L.as1, 16));
    else if constexpr (kMode == kGateProbe) prefetch_w<1, 4096, 2048, 1>(pre1, wb, frag32(L.trunk[0], 4));
    else                                    prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[0], 4));
    // gated heads: the survivor count of this sub-launch (written by the trunk kernel in front of it on the stream; never more than its points)
    int n_rec = 0;
    if constexpr (kMode == kGateHeads) {
        n_rec = __builtin_amdgcn_readfirstlane((int)*reinterpret_cast<const volatile unsigned*>(p.gate_count));
        n_rec = n_rec < p.n_points ? n_rec : p.n_points;
    }
    // listed trunk: the candidate count of this sub-launch (written by the probe kernel in front of it on the stream), likewise
    if constexpr (kListed) {
        n_rec = __builtin_amdgcn_readfirstlane((int)*reinterpret_cast<const volatile unsigned*>(p.cand_count));
        n_rec = n_rec < p.n_points ? n_rec : p.n_points;
    }
    float kappa = kProbeKappa;                    // probe: the margin of this launch
    if constexpr (kMode == kGateProbe) kappa = probe_kappa(p);
    // listed trunk with a GateMargin state: r = |s - sigma| / S of every listed point - this lane's running maximum (lanes 0..15 hold rows)
    // and this wave's count of measured rows, across the tile loop; they leave at kernel exit
    float r_seen = 0.0f;
    int n_seen = 0;
    int n_kept = 0;                               // listed whole kernel: this wave's survivors, likewise
    const int n_tiles = kMode == kGateHeads || kListed ? (n_rec + kPtsT - 1) / kPtsT : p.n_tiles;
    auto pad_of = [&](int r) { return pad_words(ldst, r); };      // (gated heads: the point's range flags)
    float amax = 0.0f;                            // running maxima of |scaled value| (encoder inputs / layer outputs): the f16 range guard
    f16x2 amax2 = {(_Float16)0.0f, (_Float16)0.0f};
    const int n_tiles64 = (p.n_points + kTilePoints - 1) / kTilePoints;      // the save slots' tiles

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int lane_t = tid;                         // (laundered per tile: keeps the lane_t parts of per-tile offsets out of the loop-invariant set,
        asm volatile("" : "+v"(lane_t));          // and `lane_t` itself out of the registers that live across the tile loop)
        lane_t &= 63;
        if constexpr (!kSave) {                   // inference: the f16 range guard is per tile (flag_f16_range); training forwards keep the
            amax = 0.0f;                          // launch's maximum (act_max; their status is one word)
            amax2 = f16x2{(_Float16)0.0f, (_Float16)0.0f};
        }
        // ---------------- encode -> hi/lo planes (xyz: columns 0..63, dir: columns 256..287) ----------------
        auto encode = [&](bool with_dir, bool with_pos = kMode != kGateHeads) {
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
            const int pt = tid_o % kPtsT, part = tid_o / kPtsT;
            int gp = tile * kPtsT + pt;
            if constexpr (kMode == kGateHeads) gp = p.gate_idx[gp < n_rec ? gp : n_rec - 1];      // the record's point
            if constexpr (kListed) gp = p.cand_idx[gp < n_rec ? gp : n_rec - 1];                  // the candidate (rows past the count: the last one)
            gp = gp < p.n_points ? gp : p.n_points - 1;
            int n_samples = p.n_samples;           // (laundered: the division's reciprocal, as a loop invariant, is one more register held - and
            asm volatile("" : "+s"(n_samples));    // at this kernel's 256 spilled - across the whole tile)
            const int ray = gp / n_samples;
            const float* __restrict__ r = p.rays + (size_t)ray * INERF_RAY_FLOATS;
            _Float16* row = ldst + pt * kRowD;
            constexpr auto kStore = kMode == kGateProbe ? &hi_store_parked<kPlaneT> : &split_store<kPlaneT>;
            if constexpr (kMode != kGateHeads)        // (the gated heads' rows arrive with h7 in these columns; the grid's point is a lattice point)
                if (with_pos) encode_position<kSsr, kParts, 2, kStore, kPlaneT, kMode == kGridTrunk>(p, r, gp, part, row, amax);
            if constexpr (kMode == kGateWhole) if (!with_pos) amax = 0.0f;      // (the direction's own maximum: the probe's flag speaks for the position)
            if constexpr (kMode != kGateTrunk && kMode != kGateProbe && kMode != kGridTrunk) if (with_dir) {      // (gated trunk: compiled out - the heads kernel encodes its survivors' directions)
                const int fd = kParts - 1 - part;
                if (fd < p.l_dir) {
                    const float s = (float)(1 << fd);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float sn, cs;
                        fast_sincosf(r[8 + c] * s, &sn, &cs);
                        split_store<kPlaneT>(row + kColDirD + 3 + 6 * fd + c, sn, amax);
                        split_store<kPlaneT>(row + kColDirD + 6 + 6 * fd + c, cs, amax);
                    }
                }
                if (part == 3) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) split_store<kPlaneT>(row + kColDirD + c, r[8 + c], amax);
                    for (int c = 3 + 6 * p.l_dir; c < kDirCols; ++c) { row[kColDirD + c] = (_Float16)0.0f; row[kPlaneT + kColDirD + c] = (_Float16)0.0f; }
                }
            }
            if constexpr (kPointGuard) if (with_dir) {      // this thread's word of the point's range flags: written by every tile, so never stale
                pad_of(pt)[part] = !(amax <= kF16Safe);
                amax = 0.0f;
            }
        };
        if constexpr (kMode == kGateHeads) {
            // this wave's sixteen rows (the rows its own lanes read last in the tile before: no barrier needed in front), a whole 1 KB
            // record per instruction: lane = sixteen-byte piece, pieces 0..31 the hi plane's columns, 32..63 the lo plane's
            u32x4 v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                int rec = tile * kPtsT + 16 * wave + j;
                rec = rec < n_rec ? rec : n_rec - 1;
                v[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.gate_rec + (size_t)rec * kGateRecordBytes) + lane_t);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j)
                *reinterpret_cast<u32x4*>(ldst + (lane_t >> 5) * kPlaneT + (16 * wave + j) * kRowD + 8 * (lane_t & 31)) = v[j];
        }
#ifdef INERF_ABL_NO_ENCODE      // (timing ablation of a development build: the first tile's encoding stays in LDS; results are wrong)
        if (tile == (int)blockIdx.x)
#endif
        encode(!kNoDirAtEncode);
        __syncthreads();
        // park the encoding for the skip layer (piece q = tid + 512 i of the tile's 2 048 sixteen-byte pieces: plane q / 1024, row (q % 1024) / 8)
        const bool enc_cached = !kSsr && !kSave && kMode == kWhole && p.sem_scratch != nullptr;
        const __amdgpu_buffer_rsrc_t enc_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            p.sem_scratch, 0, enc_cached ? (int)((unsigned)gridDim.x * (unsigned)kEncCacheBytesT) : 0, 0x00020000);
        auto enc_piece = [&](int i) {
            const int q = (tid & 511) + 512 * i;
            return ldst + (q >> 10) * kPlaneT + ((q & 1023) >> 3) * kRowD + (q & 7) * 8;
        };
        if constexpr (!kSsr && !kSave) {
            if (enc_cached) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(enc_piece(i)), enc_rsrc,
                                                           (int)blockIdx.x * kEncCacheBytesT + (tid + 512 * i) * 16, 0, 0);
            }
        }
        // gated trunk: the same pieces parked in LDS (park_encoding, mlp_f16_gate.h)
        constexpr bool kPark = (kMode == kGateTrunk || kMode == kGridTrunk || kMode == kGateWhole) && INERF_GATE_TRUNK_PARK;
        static_assert(kMode != kGateWhole || kPark, "the listed whole kernel has no second encoder pass: its direction columns hold the parked pieces");
        if constexpr (kPark) park_encoding<2, 512>(ldst, tid, false);
        auto encode_again = [&]() {         // the encoding back into columns 0..63 (sc0: past the vector L1, whose lines of an earlier tile may be stale)
            if constexpr (kPark) {
                park_encoding<2, 512>(ldst, tid, true);
                return;
            }
            if constexpr (!kSsr && !kSave) {
                if (enc_cached) {
                    u32x4 v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        v[i] = __builtin_amdgcn_raw_buffer_load_b128(enc_rsrc, (int)blockIdx.x * kEncCacheBytesT + (tid + 512 * i) * 16, 0, 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(enc_piece(i)) = v[i];
                    return;
                }
            }
            encode(false);
        };
        // training forward: the encoding as operand fragments of dW = dZ^T enc (pts_linears.0 and .5's encoding columns), straight from
        // the planes before the first layer's output lands there: per 64-point half a 64-channel fragment slot, one channel block per
        // wave (waves 0..3 = half x block); waves 4, 5: the view encoding of half 0 / 1 (32 channels, one block)
        if constexpr (kSave) {
            int lane_e = lane_t;
            asm volatile("" : "+v"(lane_e));
            if (wave < 4) {
                const int half = wave >> 1, blk = wave & 1;
                FragDst d;
                d.rsrc = __builtin_amdgcn_make_buffer_rsrc(p.save + p.save_off[SAVE_ENC], 0, (int)((unsigned)n_tiles64 * (unsigned)(kFragTileBytes / 4)), 0x00020000);
                d.voff = (unsigned)(2 * tile + half) * (unsigned)(kFragTileBytes / 4) + (unsigned)blk * (2u * kFragBytes) + (unsigned)lane_e * 16u;
                planes_to_frag<1, kRowD, kPlaneT, 2>(xr + half * 64 * kRowD + 32 * blk, plane_selector(lane_e), d);
            } else if (wave < 6) {
                const int half = wave - 4;
                FragDst d;
                d.rsrc = __builtin_amdgcn_make_buffer_rsrc(p.save + p.save_off[SAVE_DIR], 0, (int)((unsigned)n_tiles64 * (unsigned)(kFragTileBytes / 8)), 0x00020000);
                d.voff = (unsigned)(2 * tile + half) * (unsigned)(kFragTileBytes / 8) + (unsigned)lane_e * 16u;
                planes_to_frag<1, kRowD, kPlaneT, 1>(xr + half * 64 * kRowD + kColDirD, plane_selector(lane_e), d);
            }
        }

        // a 256-wide layer in place: GEMM over columns [0, 16*KBT) | barrier | store to columns [0, 256) | barrier
        f32x16 am1[1][4];
        f32x4 bias1[1][4];
        float inv1;
        // ReLU masks of h0..h7 for the input-gradient chain (layout.h relu_bits_offset) and the layers' fragment slots (layout.h SaveSlot)
        const __amdgpu_buffer_rsrc_t bits_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            p.save + (kSave ? p.bits_off : 0), 0, kSave ? (int)((unsigned)n_tiles64 * (unsigned)kReluBitTileBytes) : 0, 0x00020000);
        auto frag_dst = [&](int slot, int half, int first_block) {
            FragDst d;
            d.rsrc = __builtin_amdgcn_make_buffer_rsrc(p.save + (kSave ? p.save_off[slot] : 0), 0,
                                                       kSave ? (int)((unsigned)n_tiles64 * (unsigned)kFragTileBytes) : 0, 0x00020000);
            d.voff = (unsigned)(2 * tile + half) * (unsigned)kFragTileBytes + (unsigned)first_block * (2u * kFragBytes) + (unsigned)lane_t * 16u;
            return d;
        };
        auto store256 = [&](const GemmSlot& s, bool relu, int frag_slot, auto&& prefetch_next, auto bits_tag) {
            load_bias<1>(bias1, inv1, wb, (s.b + 32 * wave) * 4, (s.b + kWidth) * 4, lane_t);
            prefetch_next();
            constexpr bool kBits = kSave && decltype(bits_tag)::value;
            // this wave's 32 channels = row block (wave & 1) of the 64-channel group (wave >> 1): word (wave & 1) of that group's lane pair
            const BitsDst bd = {bits_rsrc, kBits ? ((((2 * tile) * kReluBitLayers + (frag_slot - SAVE_H0)) * 4 + (wave >> 1)) * 64 + lane_t) * 8 + 4 * (wave & 1) : 0};
#ifndef INERF_ABL_NO_BARRIER    // (timing ablation of a development build: the layer barriers gone - racy, results are wrong)
            __syncthreads();                       // every wave has read the layer's input
#endif
            wide_store_h<1, kRowD, kPlaneT, false, kBits, 4, !kSave>(am1, inv1, bias1, xd, relu, amax2, nullptr, 0, 0, 0, nullptr, &bd);
#ifndef INERF_ABL_NO_BARRIER
            __syncthreads();
#endif
            if constexpr (kSave)                   // this wave's 32 channels of all 128 points (the layer is complete behind the barrier)
                if (frag_slot >= 0) {
                    int lane_o = lane_t;           // (laundered: the selector is rebuilt per layer instead of living in 8 registers)
                    asm volatile("" : "+v"(lane_o));
                    const Selector sel = plane_selector(lane_o);
                    planes_to_frag<1, kRowD, kPlaneT>(xr + 32 * wave, sel, frag_dst(frag_slot, 0, wave));
                    planes_to_frag<1, kRowD, kPlaneT>(xr + 64 * kRowD + 32 * wave, sel, frag_dst(frag_slot, 1, wave));
                }
        };
        constexpr std::true_type kWithBits{};
        constexpr std::false_type kNoBits{};
        auto pf32 = [&](const GemmSlot& s, int kbt) { return [&, kbt]() { prefetch_w<1, 4096>(pre1, wb, frag32(s, kbt)); }; };
        auto pf32_at = [&](const GemmSlot& s, int kbt, int kb_first) {
            return [&, kbt, kb_first]() { prefetch_w<1, 4096>(pre1, wb, frag32(s, kbt) + kb_first * 4096); };
        };
        auto pf256 = [&](const GemmSlot& s, int kbt) { return [&, kbt]() { prefetch_w<2>(pre2, wb, frag256(s, kbt)); }; };

        // ---------------- trunk ----------------
        if constexpr (kMode == kGateHeads) {
            // (h7 came with the records)
        } else if constexpr (kPipe) {
            // halves A (rows 0..63) and B (rows 64..127); accX: the half's accumulators of its latest GEMM, epilogued during the other half's next one
            f32x16 accA[2], accB[2];
            f32x4 bias[1][4];                      // of the layer whose epilogue the next step carries (requested a barrier + a k-block ahead)
            float inv = 0.0f;
            const _Float16* const xrB = xr + 64 * kRowD;
            _Float16* const xdB = xd + 64 * kRowD;
            auto bias_of = [&](const GemmSlot& s, f32x4 (&b)[1][4], float& iv) { load_bias<1>(b, iv, wb, (s.b + 32 * wave) * 4, (s.b + kWidth) * 4, lane_t); };
            // layer 0 (K = the 64 encoding columns): G(0,A) | G(0,B) || E(0,A)
            pp_step<4, 0, true, kRowD, kPlaneT>(pre1, wb, frag32(L.trunk[0], 4), xr, 0, accA, accB, inv, bias[0], xdB, amax2);
            bias_of(L.trunk[0], bias, inv);
            prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[0], 4));
            __syncthreads();                       // every wave has read the encoding of half A
            pp_step<4, 8, true, kRowD, kPlaneT>(pre1, wb, frag32(L.trunk[0], 4), xrB, 0, accB, accA, inv, bias[0], xd, amax2);
            prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[1], 16));
            __syncthreads();
#pragma unroll 1
            for (int layer = 1; layer < kDepth; ++layer) {
                const GemmSlot& s = L.trunk[layer];
                if (layer != kSkipInput) {
                    // A(l): G(l,A) || E(l-1,B);  B(l): G(l,B) || E(l,A)
                    pp_step<16, 8, true, kRowD, kPlaneT>(pre1, wb, frag32(s, 16), xr, 0, accA, accB, inv, bias[0], xdB, amax2);
                    bias_of(s, bias, inv);
                    prefetch_w<1, 4096>(pre1, wb, frag32(s, 16));
                    __syncthreads();
                    pp_step<16, 8, true, kRowD, kPlaneT>(pre1, wb, frag32(s, 16), xrB, 0, accB, accA, inv, bias[0], xd, amax2);
                    if (layer + 1 == kSkipInput) prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[kSkipInput], 20) + 4 * 4096);
                    else if (layer + 1 < kDepth) prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[layer + 1], 16));
                    __syncthreads();
                } else {
                    // pts_linears[5] over cat([pts, h]): the h part (k-blocks 4..19 of the stream) of both halves, then the encoding again in
                    // columns 0..63 (both halves' h4 are consumed), then the encoding part on top of the same accumulators
                    pp_step<16, 8, true, kRowD, kPlaneT>(pre1, wb, frag32(s, 20) + 4 * 4096, xr, 0, accA, accB, inv, bias[0], xdB, amax2);      // || E(4,B)
                    bias_of(s, bias, inv);
                    prefetch_w<1, 4096>(pre1, wb, frag32(s, 20) + 4 * 4096);
                    __syncthreads();
                    pp_step<16, 0, true, kRowD, kPlaneT>(pre1, wb, frag32(s, 20) + 4 * 4096, xrB, 0, accB, accA, inv, bias[0], xd, amax2);
                    prefetch_w<1, 4096>(pre1, wb, frag32(s, 20));
                    __syncthreads();
                    encode_again();
                    __syncthreads();
                    pp_step<4, 0, false, kRowD, kPlaneT>(pre1, wb, frag32(s, 20), xr, 0, accA, accB, inv, bias[0], xdB, amax2);
                    prefetch_w<1, 4096>(pre1, wb, frag32(s, 20));
                    __syncthreads();               // every wave has read the encoding of half A: E(5,A) may overwrite it
                    pp_step<4, 8, false, kRowD, kPlaneT>(pre1, wb, frag32(s, 20), xrB, 0, accB, accA, inv, bias[0], xd, amax2);                 // || E(5,A)
                    prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[kSkipInput + 1], 16));
                    __syncthreads();
                }
            }
            prefetch_w<2>(pre2, wb, frag256(L.as1, 16));                      // (outside the layer loop: assigned inside it the 32 registers are loop-carried)
            pp_epilogue<kRowD, kPlaneT>(accB, inv, bias[0], xdB, amax2);      // E(7,B): nothing left to run it under
            __syncthreads();
        } else if constexpr (kMode == kGateProbe) {
            // the skip layer's encoding from its copy in the lo plane (nothing overwrites it)
            probe_trunk<1>(pre1, wb, L, frag32, xr, xd, wave, lane_t, amax2, [&]() { return xr + kPlaneT; });
        } else {
            wide_gemm_h<1, 4, 0, kRowD, kPlaneT, true, 4096, 4, 2048, kPeel>(pre1, wb, frag32(L.trunk[0], 4), xr, 0, 0, lane_t, am1);
            store256(L.trunk[0], true, SAVE_H0, pf32(L.trunk[1], 16), kWithBits);
    #pragma unroll 1
            for (int layer = 1; layer < kSkipInput; ++layer) {
                wide_gemm_h<1, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, kPeel>(pre1, wb, frag32(L.trunk[layer], 16), xr, 0, 0, lane_t, am1);
                if (layer + 1 < kSkipInput) store256(L.trunk[layer], true, SAVE_H0 + layer, pf32(L.trunk[layer + 1], 16), kWithBits);
                else                        store256(L.trunk[layer], true, SAVE_H0 + layer, pf32_at(L.trunk[kSkipInput], 20, 4), kWithBits);
            }
            {   // pts_linears[5] over cat([pts, h]): h-part (k-blocks 4..19 of the stream), then the encoding again
                const GemmSlot& s = L.trunk[kSkipInput];
                wide_gemm_h<1, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, kPeel>(pre1, wb, frag32(s, 20) + 4 * 4096, xr, 0, 0, lane_t, am1);
                prefetch_w<1, 4096>(pre1, wb, frag32(s, 20));
                __syncthreads();
                encode_again();
                __syncthreads();
                wide_gemm_h<1, 4, 0, kRowD, kPlaneT, false, 4096, 4>(pre1, wb, frag32(s, 20), xr, 0, 0, lane_t, am1);
                store256(s, true, SAVE_H0 + kSkipInput, pf32(L.trunk[6], 16), kWithBits);
            }
            wide_gemm_h<1, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, kPeel>(pre1, wb, frag32(L.trunk[6], 16), xr, 0, 0, lane_t, am1);
            store256(L.trunk[6], true, SAVE_H0 + 6, pf32(L.trunk[7], 16), kWithBits);
            // listed whole kernel: the direction columns and the pad words are free since the copy-back (two layers' barriers ago) and nothing
            // reads them before the heads (layer 7's barriers ahead) - the direction encoding and the point's range words, as the gated heads do
            if constexpr (kMode == kGateWhole) encode(true, false);
            wide_gemm_h<1, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, kPeel>(pre1, wb, frag32(L.trunk[7], 16), xr, 0, 0, lane_t, am1);
            if constexpr (kMode == kGateTrunk || kMode == kGridTrunk) store256(L.trunk[7], true, SAVE_H7, pf32(L.trunk[0], 4), kWithBits);
            else                               store256(L.trunk[7], true, SAVE_H7, pf256(L.as1, 16), kWithBits);
        }

        // listed kernels with a GateMargin state: the probe's error on list entry `at` (this lane's row when `valid`), in correctly rounded
        // operations; a NaN density, an infinite s or S == 0 is not counted and cannot poison the maximum
        auto measure_margin = [&](bool valid, int at, float sigma) {
            if (p.gate_state) {                        // (uniform)
                bool seen = false;
                if (valid) {
                    const float2 ss = *reinterpret_cast<const float2*>(p.cand_ss + 2 * (size_t)at);
                    const float e = __fdiv_rn(fabsf(__fsub_rn(ss.x, sigma)), ss.y);
                    seen = ss.y > 0.0f && e - e == 0.0f;
                    if (seen) r_seen = fmaxf(r_seen, e);
                }
                n_seen += __popcll(__ballot(seen));
            }
        };

        // ---------------- density gate: sigma (probe: s and S), the raw rows, the survivors' records or the candidate list ----------------
        if constexpr (kMode == kGateTrunk || kMode == kGateProbe) {
            const int pt16 = tile * kPtsT + 16 * wave;
            const _Float16* const xs_g = ldst + (16 * wave + (lane_t & 15)) * kRowD + 8 * (lane_t >> 4);
            float sigma, scale = 0.0f;                 // lanes 0..15: this wave's points
            if constexpr (kMode == kGateProbe) skinny_probe_h<8>(wb, L.alpha.w * 4, L.alpha.b * 4, (L.alpha.b + 16) * 4, xs_g, lane_t, sigma, scale);
            else sigma = skinny_gemm_h<8, kPlaneT>(wb, L.alpha.w * 4, L.alpha.b * 4, (L.alpha.b + 16) * 4, xs_g, lane_t)[0];
            const bool valid = lane_t < 16 && pt16 + lane_t < (kListed ? n_rec : p.n_points);
            const bool keep[1] = {valid && (kMode == kGateProbe ? !(sigma < -kappa * scale) : !(sigma <= 0.0f))};
            const unsigned kept[1] = {(unsigned)__builtin_amdgcn_readfirstlane((unsigned)__ballot(keep[0]))};
            post_count(ldst, wave, kept[0], lane_t);
            int my_point[1] = {pt16 + lane_t};         // the row's point within the sub-range
            if constexpr (kListed) {                   // exact sigma into the candidate's raw row, whose other ten channels the probe zeroed
                my_point[0] = p.cand_idx[valid ? pt16 + lane_t : 0];
                if (valid) __builtin_nontemporal_store(sigma, p.raw + (size_t)my_point[0] * p.channels + 3);
                measure_margin(valid, pt16 + lane_t, sigma);
            } else {
                store_sigma_rows(p, pt16, sigma, lane_t);
            }
            if constexpr (kMode == kGateProbe)
                if (p.probe_out && valid) {            // tests: (s, S) per point
                    p.probe_out[2 * (size_t)(pt16 + lane_t)] = sigma;
                    p.probe_out[2 * (size_t)(pt16 + lane_t) + 1] = scale;
                }
            const float s_row[1] = {sigma}, big_s_row[1] = {scale};
            const int slot0 = reserve_slots<1>(ldst, kMode == kGateProbe ? p.cand_count : p.gate_count, kMode == kGateProbe ? p.cand_idx : p.gate_idx,
                                               keep, kept, my_point, wave, lane_t, tid, kMode == kGateProbe ? p.cand_ss : nullptr, s_row, big_s_row);
            if constexpr (kMode == kGateTrunk) {
                int slot = slot0;
                for (unsigned m = kept[0]; m != 0u; m &= m - 1u, ++slot) {      // one 1 KB record per instruction: lane = sixteen-byte piece of the row, hi plane | lo plane
                    const int j = __builtin_ctz(m);
                    const u32x4 v = *reinterpret_cast<const u32x4*>(ldst + (lane_t >> 5) * kPlaneT + (16 * wave + j) * kRowD + 8 * (lane_t & 31));
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p.gate_rec + (size_t)slot * kGateRecordBytes) + lane_t);
                }
            }
            // The range guard is the PROBE's: it sees every point of the sub-range, a candidate included, in tiles of consecutive rays, and
            // its hi-only activations are within 1e-3 of the exact ones - with the threshold a factor 8.7 below f16's maximum the exact
            // trunk cannot overflow on a point the probe did not flag.  A listed tile holds points of rays from anywhere in the sub-range:
            // a per-tile flag here would mark the words of rays whose own points are in range (and have their chunks rendered again).
            if constexpr (!kListed) flag_f16_range(p, tile * kPtsT, kPtsT, amax, amax2, lane_t);
            __syncthreads();                       // the rows are read: the next tile's encode may overwrite them
            continue;
        }

        // ---------------- occupancy grid: sigma as above, then the activation of extract_colour_mesh.py:172-175 ----------------
        if constexpr (kMode == kGridTrunk) {
            const int pt16 = tile * kPtsT + 16 * wave;
            const _Float16* const xs_g = ldst + (16 * wave + (lane_t & 15)) * kRowD + 8 * (lane_t >> 4);
            const float sigma = skinny_gemm_h<8, kPlaneT>(wb, L.alpha.w * 4, L.alpha.b * 4, (L.alpha.b + 16) * 4, xs_g, lane_t)[0];      // lanes 0..15: this wave's points
            if (lane_t < 16 && pt16 + lane_t < p.n_points) {
                float occ = __fsub_rn(1.0f, expf(-__fmul_rn(fmaxf(sigma, 0.0f), p.grid_dist)));      // as the compositing kernel's alpha (ray_ops.hip)
                if (sigma != sigma) occ = sigma;                                                      // relu(NaN) stays NaN in torch
                __builtin_nontemporal_store(occ, p.occ + pt16 + lane_t);
                if (p.sigma_out) __builtin_nontemporal_store(sigma, p.sigma_out + pt16 + lane_t);
            }
            flag_f16_range(p, tile * kPtsT, kPtsT, amax, amax2, lane_t);
            __syncthreads();                       // the rows are read: the next tile's encode may overwrite them
            continue;
        }

        // ---------------- heads ----------------
        const bool sem = kSsr && L.sem_rbs > 0;
        // (gated heads: the row's record, whose point is looked up where the row is written)
        const int my_pt = tile * kPtsT + 16 * wave + (lane_t & 15);
        const bool my_valid = my_pt < (kPointGuard ? n_rec : p.n_points);
        float* const out_row = p.raw + (size_t)(my_valid && !kPointGuard ? my_pt : 0) * p.channels;
        // gated heads, the per-point range guard: every check is of ONE layer (amax2 starts from zero again behind it), and only a wave
        // that saw a value out of range looks up which of its lanes' points it belongs to - from the hi halves themselves, which are
        // what amax2 is the maximum of
        auto out_of_range = [&]() { return __any(!((float)amax2[0] <= kF16Safe) || !((float)amax2[1] <= kF16Safe)) != 0; };
        auto flag_operands = [&](const auto& hi_ops) {      // register operands [q][pb]: point (lane & 31) of point block pb of half ph
            if (out_of_range()) {
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    bool bad = false;
#pragma unroll
                    for (int q = 0; q < (int)std::extent_v<std::remove_reference_t<decltype(hi_ops)>>; ++q)
#pragma unroll
                        for (int i = 0; i < 8; ++i) bad |= !(fabsf((float)hi_ops[q][pb][i]) <= kF16Safe);
                    if (bad) pad_of((lane_t & 31) + 32 * pb + 64 * ph)[0] = 1;
                }
            }
            amax2 = f16x2{(_Float16)0.0f, (_Float16)0.0f};
        };
        // (operand addresses of the heads from the per-tile laundered lane_t index: as loop invariants they are two more spilled registers)
        const _Float16* const xs = ldst + (16 * wave + (lane_t & 15)) * kRowD + 8 * (lane_t >> 4);   // skinny operand reads: this wave's 16 points

        // albedo + shading: hidden layer (this wave: channel group cg of point half ph) -> registers -> partial output sums
        f32x4 part_as[2], part_res[2];
        const _Float16* const xr_h = ldst + ((lane_t & 31) + 64 * ph) * kRowD + 8 * (lane_t >> 5);
        {
            f32x16 am2[2][2];
            f32x4 bias2[2][4];
            float inv2;
            wide_gemm_h<2, 16, 0, kRowD, kPlaneT, true, 4096, 2, 2048, kPeel>(pre2, wb, frag256(L.as1, 16), xr_h, 0, 0, lane_t, am2);
            load_bias<2>(bias2, inv2, wb, (L.as1.b + 64 * cg) * 4, (L.as1.b + kWidth) * 4, lane_t);
            if (sem) prefetch_w<1>(pre1, wb, frag128(L.sem1, 16));
            else     prefetch_w<1, 4096>(pre1, wb, frag32(L.feat, 16));
            f16x8 hi[4][2], lo[4][2];
            if constexpr (kPointGuard) amax2 = f16x2{(_Float16)0.0f, (_Float16)0.0f};
            to_operands<2, false, 2, !kSave>(am2, inv2, bias2, amax2, hi, lo);
            if constexpr (kPointGuard) flag_operands(hi);
            if constexpr (kSave) {                // the hidden layer as operand fragments, transposed out of the registers (it never touches LDS):
                int lane_o = lane_t;              // channel group cg of point half ph = the 64-point kernel's wave cg of tile 2 * tile + ph
                asm volatile("" : "+v"(lane_o));
                operands_to_frag<2>(hi, lo, accumulator_selector(lane_o), frag_dst(SAVE_AS1H, ph, 2 * cg));
            }
            regop_gemm<4>(wb, (L.as2r.w + cg * 4 * 2 * 256) * 4, hi, lo, part_as);
        }
        // semantic head (semantic_nerf.py:150-152): hidden = relu(semantic_linear.0.0 h7), this wave's 32 channels x 64 points -> registers
        // -> partial logits of the (one) 32-class block, kept until the exchange at the end of the tile
        const __amdgpu_buffer_rsrc_t sem_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            p.sem_scratch, 0, kSsr ? (int)((unsigned)gridDim.x * (unsigned)kSemScratchBytesT) : 0, 0x00020000);
        const int sem_slot = ((int)blockIdx.x * 8 + wave) * (kSemScratchBytesT / 8) + lane_t * 16;      // + (pb * 4 + g) * 1024
        if constexpr (kSsr) {
            if (sem) {
                f32x16 sem_part[2];
                f32x16 ams[1][2];
                f32x4 biass[1][4];
                float invs;
                wide_gemm_h<1, 16, 0, kRowD, kPlaneT, true, 2048, 2, 2048, kPeel>(pre1, wb, frag128(L.sem1, 16), xr_h, 0, 0, lane_t, ams);
                load_bias<1>(biass, invs, wb, (L.sem1.b + 32 * cg) * 4, (L.sem1.b + kHalf) * 4, lane_t);
                prefetch_w<1, 4096>(pre1, wb, frag32(L.feat, 16));
                f16x8 hi[2][2], lo[2][2];
                to_operands<1>(ams, invs, biass, amax2, hi, lo);
                regop_gemm_full<2, 2>(wb, (L.sem2q.w + cg * 2 * 2 * 256) * 4, hi, lo, sem_part);
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 v = {sem_part[pb][4 * g], sem_part[pb][4 * g + 1], sem_part[pb][4 * g + 2], sem_part[pb][4 * g + 3]};
                        // (whole offset in the VGPR operand: a 16-byte buffer store with a register SGPR offset gets no hazard wait state, tests/test_isa_audit_cpu.py)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), sem_rsrc, sem_slot + (pb * 4 + g) * 1024, 0, 0);
                    }
            }
        }
        // feature (no activation) in place of h7, then the view-dependent layer over [feature | dir] -> registers
        wide_gemm_h<1, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, kPeel>(pre1, wb, frag32(L.feat, 16), xr, 0, 0, lane_t, am1);
        // sigma, last of h7's readers (here, not in front of the heads: four registers fewer across their GEMM loops)
        f32x4 sig4 = {0.0f, 0.0f, 0.0f, 0.0f};      // (gated heads: the trunk kernel wrote sigma)
        if constexpr (kMode != kGateHeads) sig4 = skinny_gemm_h<8, kPlaneT>(wb, L.alpha.w * 4, L.alpha.b * 4, (L.alpha.b + 16) * 4, xs, lane_t);
        {
            WidePreH<1> prev;
            store256(L.feat, false, SAVE_FEAT, [&]() { prefetch_w<1>(prev, wb, frag128(L.views, 18)); }, kNoBits);
            if constexpr (kPointGuard) {      // this wave's 32 feature channels of its lanes' four points, complete in the planes behind the barrier
                if (out_of_range()) {
#pragma unroll
                    for (int pb = 0; pb < 4; ++pb) {
                        const int r = (lane_t & 31) + 32 * pb;
                        const _Float16* src = ldst + r * kRowD + 32 * wave + 16 * (lane_t >> 5);
                        const f16x8 f0 = *reinterpret_cast<const f16x8*>(src), f1 = *reinterpret_cast<const f16x8*>(src + 8);
                        bool bad = false;
#pragma unroll
                        for (int i = 0; i < 8; ++i) bad |= !(fabsf((float)f0[i]) <= kF16Safe) || !(fabsf((float)f1[i]) <= kF16Safe);
                        if (bad) pad_of(r)[0] = 1;
                    }
                }
                amax2 = f16x2{(_Float16)0.0f, (_Float16)0.0f};
            }
            f32x16 amv[1][2];
            f32x4 biasv[1][4];
            float invv;
            wide_gemm_h<1, 18, 0, kRowD, kPlaneT, true, 2048, 2, 2048, kPeel>(prev, wb, frag128(L.views, 18), xr_h, 0, 0, lane_t, amv);
            load_bias<1>(biasv, invv, wb, (L.views.b + 32 * cg) * 4, (L.views.b + kHalf) * 4, lane_t);
            if constexpr (kMode == kGateHeads) prefetch_w<2>(pre2, wb, frag256(L.as1, 16));
            else                               prefetch_w<1, 4096>(pre1, wb, frag32(L.trunk[0], 4));
            f16x8 hi[2][2], lo[2][2];
            to_operands<1, false, 2, !kSave>(amv, invv, biasv, amax2, hi, lo);
            if constexpr (kPointGuard) flag_operands(hi);
            if constexpr (kSave) {                // 128 channels: a four-block fragment slot, block cg of point half ph
                int lane_o = lane_t;
                asm volatile("" : "+v"(lane_o));
                FragDst d;
                d.rsrc = __builtin_amdgcn_make_buffer_rsrc(p.save + p.save_off[SAVE_VH], 0, (int)((unsigned)n_tiles64 * (unsigned)(kFragTileBytes / 2)), 0x00020000);
                d.voff = (unsigned)(2 * tile + ph) * (unsigned)(kFragTileBytes / 2) + (unsigned)cg * (2u * kFragBytes) + (unsigned)lane_o * 16u;
                operands_to_frag<1, 4>(hi, lo, accumulator_selector(lane_o), d);
            }
            regop_gemm<2>(wb, (L.resr.w + cg * 2 * 2 * 256) * 4, hi, lo, part_res);
        }
        __syncthreads();                           // feature / dir columns are dead: the exchange area may be written
        bool my_flagged = false;                   // gated heads: the four flag words of this lane's row (their last writer is behind the barrier; the
        if constexpr (kPointGuard) {               // next tile's encode writes them again right behind the next one)
            const u32x4 f = *reinterpret_cast<const u32x4*>(pad_of(16 * wave + (lane_t & 15)));
            my_flagged = (f[0] | f[1] | f[2] | f[3]) != 0u;
        }
        if (lane_t < 32) {
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                float* ex = reinterpret_cast<float*>(ldst + (lane_t + 32 * pb + 64 * ph) * kRowD + kColExD) + 8 * cg;
                *reinterpret_cast<f32x4*>(ex) = part_as[pb];
                *reinterpret_cast<f32x4*>(ex + 4) = part_res[pb];
            }
        }
        // the four partial logit blocks of a point (one per 32-channel group of the hidden layer), 32 floats each, in dead columns that
        // neither the heads' exchange area (hi plane, bytes 128..255) nor the next tile's encode (bytes 0..127 and 512..575) touch:
        // groups 0 / 1 at bytes 256..383 / 384..511 of the row in the hi plane, groups 2 / 3 at bytes 128..255 / 256..383 in the lo plane
        auto sem_ex = [&](int g, int r) {
            return reinterpret_cast<float*>(ldst) + (g < 2 ? 64 + 32 * g : kPlaneT / 2 + 32 * (g - 1)) + r * (kRowD / 2);
        };
        if constexpr (kSsr) {
            if (sem) {      // this wave's partial logits back from its slot (sc0: past the vector L1, whose lines of an earlier tile may be stale;
                            // fetched here, not ahead of the barrier: held across it they were spilled to scratch) and into the exchange area:
                            // accumulator register 4 g + i = class 8 g + 4 (lane >> 5) + i of point (lane & 31) of point block pb of this wave's half
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    u32x4 sem_v[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) sem_v[g] = __builtin_amdgcn_raw_buffer_load_b128(sem_rsrc, sem_slot + (pb * 4 + g) * 1024, 0, 1);
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *reinterpret_cast<u32x4*>(sem_ex(cg, 64 * ph + 32 * pb + (lane_t & 31)) + 8 * g + 4 * (lane_t >> 5)) = sem_v[g];
                }
            }
        }
        __syncthreads();
        if constexpr (kSsr) {
            if (sem) {      // this wave's 16 points x 32 classes: lane = (point, 8 classes); the four partials in group order (deterministic)
                const int r = 16 * wave + (lane_t & 15), c8 = 8 * (lane_t >> 4);
                f32x4 s0 = *reinterpret_cast<const f32x4*>(sem_ex(0, r) + c8), s1 = *reinterpret_cast<const f32x4*>(sem_ex(0, r) + c8 + 4);
#pragma unroll
                for (int g = 1; g < 4; ++g) {
                    s0 += *reinterpret_cast<const f32x4*>(sem_ex(g, r) + c8);
                    s1 += *reinterpret_cast<const f32x4*>(sem_ex(g, r) + c8 + 4);
                }
                const float sem_inv2 = wb.scalar((L.sem2.b + 16 * L.sem_rbs) * 4);
                const f32x4 b0 = wb.vec4((L.sem2.b + c8) * 4, 0), b1 = wb.vec4((L.sem2.b + c8 + 4) * 4, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (my_valid && c8 + i < p.n_classes) __builtin_nontemporal_store(__builtin_fmaf(s0[i], sem_inv2, b0[i]), out_row + INERF_BASE_CHANNELS + c8 + i);
                    if (my_valid && c8 + 4 + i < p.n_classes) __builtin_nontemporal_store(__builtin_fmaf(s1[i], sem_inv2, b1[i]), out_row + INERF_BASE_CHANNELS + c8 + 4 + i);
                }
            }
        }
        // a wave's 16 points x 11 floats are 704 CONTIGUOUS bytes of raw: they leave as 44 sixteen-byte pieces (lanes 0..43, staged in
        // dead columns of the lo plane), every 64-byte sector written once by one instruction
        const bool whole_rows = !kPointGuard && p.channels == INERF_BASE_CHANNELS && tile * kPtsT + kPtsT <= p.n_points &&
                                (reinterpret_cast<uintptr_t>(p.raw) & 15) == 0;
        auto stage_row = [&](int r) { return reinterpret_cast<float*>(ldst + kPlaneT + r * kRowD + 128); };      // lo plane, bytes 256..299 of row r
        if (lane_t < 16 && my_valid) {
            const float* ex = reinterpret_cast<const float*>(ldst + (16 * wave + lane_t) * kRowD + kColExD);
            f32x4 as4 = {0.0f, 0.0f, 0.0f, 0.0f}, res4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                as4 += *reinterpret_cast<const f32x4*>(ex + 8 * w);
                res4 += *reinterpret_cast<const f32x4*>(ex + 8 * w + 4);
            }
            const f32x4 b_as = wb.vec4(L.as2.b * 4, 0), b_res = wb.vec4(L.res.b * 4, 0);
            const float inv_as = wb.scalar((L.as2.b + 16) * 4), inv_res = wb.scalar((L.res.b + 16) * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                as4[i] = __builtin_fmaf(as4[i], inv_as, b_as[i]);
                res4[i] = __builtin_fmaf(res4[i], inv_res, b_res[i]);
            }
            const float a0 = sigmoid_ref_h(as4[0]), a1 = sigmoid_ref_h(as4[1]), a2 = sigmoid_ref_h(as4[2]);
            const float sh = sigmoid_ref_h(as4[3]);
            const float r0 = sigmoid_ref_h(res4[0]), r1 = sigmoid_ref_h(res4[1]), r2 = sigmoid_ref_h(res4[2]);
            const float c0 = __fadd_rn(__fmul_rn(a0, sh), r0), c1 = __fadd_rn(__fmul_rn(a1, sh), r1), c2 = __fadd_rn(__fmul_rn(a2, sh), r2);   // run_nerf_helpers.py:320
            if constexpr (kMode == kGateHeads) {      // the survivor's ten colour channels, to the row of its point; its range flag, to the word of its ray
                const int pt = p.gate_idx[my_pt];
                float* const row = p.raw + (size_t)pt * p.channels;
                __builtin_nontemporal_store(c0, row + 0); __builtin_nontemporal_store(c1, row + 1); __builtin_nontemporal_store(c2, row + 2);
                __builtin_nontemporal_store(a0, row + 4); __builtin_nontemporal_store(a1, row + 5); __builtin_nontemporal_store(a2, row + 6);
                __builtin_nontemporal_store(sh, row + 7);
                __builtin_nontemporal_store(r0, row + 8); __builtin_nontemporal_store(r1, row + 9); __builtin_nontemporal_store(r2, row + 10);
                if (my_flagged && p.status)
                    atomicOr(p.status + (p.status_rays > 0 ? (p.ray0 + pt / p.n_samples) / p.status_rays : 0), INERF_STATUS_F16_RANGE);
            } else if constexpr (kMode == kGateWhole) {      // the candidate's exact sigma always; colours and range flag only where the gated heads would have run
                const int pt = p.cand_idx[my_pt];
                float* const row = p.raw + (size_t)pt * p.channels;
                __builtin_nontemporal_store(sig4[0], row + 3);
                if (!(sig4[0] <= 0.0f)) {
                    __builtin_nontemporal_store(c0, row + 0); __builtin_nontemporal_store(c1, row + 1); __builtin_nontemporal_store(c2, row + 2);
                    __builtin_nontemporal_store(a0, row + 4); __builtin_nontemporal_store(a1, row + 5); __builtin_nontemporal_store(a2, row + 6);
                    __builtin_nontemporal_store(sh, row + 7);
                    __builtin_nontemporal_store(r0, row + 8); __builtin_nontemporal_store(r1, row + 9); __builtin_nontemporal_store(r2, row + 10);
                    if (my_flagged && p.status)
                        atomicOr(p.status + (p.status_rays > 0 ? (p.ray0 + pt / p.n_samples) / p.status_rays : 0), INERF_STATUS_F16_RANGE);
                }
            } else if (whole_rows) {
                float* st = stage_row(16 * wave + lane_t);
                *reinterpret_cast<f32x4*>(st) = f32x4{c0, c1, c2, sig4[0]};
                *reinterpret_cast<f32x4*>(st + 4) = f32x4{a0, a1, a2, sh};
                st[8] = r0; st[9] = r1; st[10] = r2;
            } else {
                __builtin_nontemporal_store(c0, out_row + 0);
                __builtin_nontemporal_store(c1, out_row + 1);
                __builtin_nontemporal_store(c2, out_row + 2);
                __builtin_nontemporal_store(sig4[0], out_row + 3);
                __builtin_nontemporal_store(a0, out_row + 4); __builtin_nontemporal_store(a1, out_row + 5); __builtin_nontemporal_store(a2, out_row + 6);
                __builtin_nontemporal_store(sh, out_row + 7);
                __builtin_nontemporal_store(r0, out_row + 8); __builtin_nontemporal_store(r1, out_row + 9); __builtin_nontemporal_store(r2, out_row + 10);
            }
        }
        if (whole_rows && lane_t < 44) {      // (LDS is in order within a wave: the sixteen lanes' rows are there)
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * lane_t + i, pt = e / INERF_BASE_CHANNELS;
                v[i] = stage_row(16 * wave + pt)[e - INERF_BASE_CHANNELS * pt];
            }
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.raw + (size_t)(tile * kPtsT + 16 * wave) * INERF_BASE_CHANNELS) + lane_t);
        }
        if constexpr (kMode == kGateWhole) {       // this wave's survivors, and the probe's error on its sixteen rows
            const bool valid = lane_t < 16 && my_valid;
            n_kept += __popcll(__ballot(valid && !(sig4[0] <= 0.0f)));
            measure_margin(valid, my_pt, sig4[0]);
        }
        if constexpr (!kPointGuard) flag_f16_range(p, tile * kPtsT, kPtsT, amax, amax2, lane_t);
        // (the next tile's encode writes bytes 0..127 and 512..575 of the rows, both planes: clear of the exchange area (hi plane, bytes
        // 128..255) and of the staging rows (lo plane, bytes 256..299) this tile's last readers may still be in)
    }
    if constexpr (kListed) {
        if (p.gate_state) {      // (uniform) one atomicMax per wave, one 64-bit atomicAdd per workgroup (the counts meet in pad words 0..7: every
                                 // tile's last readers of them are behind its closing barrier)
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) r_seen = fmaxf(r_seen, __shfl_xor(r_seen, o));
            if (lane == 0) {
                if (r_seen > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(&p.gate_state->r_max), __builtin_bit_cast(unsigned int, r_seen));
                pad_words(ldst, wave)[0] = n_seen;
            }
            __syncthreads();
            if (tid == 0) {
                unsigned long long total = 0;
#pragma unroll
                for (int g = 0; g < 8; ++g) total += (unsigned long long)pad_words(ldst, g)[0];
                if (total > 0) atomicAdd(&p.gate_state->observed, total);
            }
        }
        if constexpr (kMode == kGateWhole) {      // the workgroup's survivors, the same way: one atomicAdd on the sub-range's count
            __syncthreads();                      // (thread 0 has read the counts above)
            if (lane == 0) pad_words(ldst, wave)[0] = n_kept;
            __syncthreads();
            if (tid == 0) {
                unsigned int total = 0;
#pragma unroll
                for (int g = 0; g < 8; ++g) total += (unsigned int)pad_words(ldst, g)[0];
                if (total > 0) atomicAdd(p.gate_count, total);
            }
        }
    }
    if (kSave && p.act_max) {
        float m = split_upper_bound(amax, amax2) * (1.0f / kActScale);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0 && m == m) atomicMax(reinterpret_cast<unsigned int*>(p.act_max), __builtin_bit_cast(unsigned int, m));
    }
}

template <bool kSsr, bool kSave = false, bool kPipe = false>
__global__ __launch_bounds__(512, 2) void k_encode_mlp_f16x3_t128(const MlpParams p) {
    encode_mlp_t128_tiles<kSsr, kSave, kPipe, kWhole>(p);
}
__global__ __launch_bounds__(512, 2) void k_mlp_gate_trunk_f16x3(const MlpParams p) { encode_mlp_t128_tiles<false, false, false, kGateTrunk>(p); }
__global__ __launch_bounds__(512, 2) void k_mlp_gate_heads_f16x3(const MlpParams p) { encode_mlp_t128_tiles<false, false, false, kGateHeads>(p); }
__global__ __launch_bounds__(512, 2) void k_mlp_gate_probe_f16(const MlpParams p) { encode_mlp_t128_tiles<false, false, false, kGateProbe>(p); }
__global__ __launch_bounds__(512, 2) void k_mlp_gate_trunk_listed_f16x3(const MlpParams p) { encode_mlp_t128_tiles<false, false, false, kGateTrunk, true>(p); }
__global__ __launch_bounds__(512, 2) void k_mlp_gate_whole_listed_f16x3(const MlpParams p) { encode_mlp_t128_tiles<false, false, false, kGateWhole, true>(p); }
template <bool kSsr>
__global__ __launch_bounds__(512, 2) void k_grid_trunk_f16x3(const MlpParams p) { encode_mlp_t128_tiles<kSsr, false, false, kGridTrunk>(p); }

}  // namespace inerf
#include "mlp_f16_probe.h"      // k_mlp_gate_probe_wg2_f16: the probe as two four-wave workgroups per CU
namespace inerf {

// ---- the density gate's launcher ----
// A launch is walked in sub-ranges of whole rays.  With the probe: probe kernel, then the listed whole kernel, on the same stream - the candidate
// list holds one index per point of a sub-range, so it cannot overflow, and nothing else is kept per point but the probe's (s, S).
// The record paths (the gate alone: trunk kernel, heads kernel; INERF_GATE_FUSED=0: probe, listed trunk, heads) hold one 1 KB record per POINT of
// a sub-range - every point surviving is the worst case - so the record buffer cannot overflow either.  Points per sub-range come from a byte
// budget of records, INERF_GATE_BYTES / 1 028, on every path (a sub-range is the same whichever path walks it); unset, the record paths take
// 2 GiB = 2 M points = 64 tiles per CU per trunk launch (DESIGN.md 3.1c on the tail that implies), the fused path kGateFusedPoints.
constexpr int64_t kGateFusedPoints = (int64_t)1 << 27;      // 12 B per point: at most 1.5 GiB of list and (s, S); a count of points stays an int
static int64_t gate_budget_points(bool fused) {
    int64_t bytes = (int64_t)2 << 30;
    if (const char* e = getenv("INERF_GATE_BYTES")) {
        const double v = atof(e);
        if (v >= 1.0) bytes = v < 6.0e10 ? (int64_t)v : (int64_t)6.0e10;
    } else if (fused) {
        return kGateFusedPoints;
    }
    return bytes / (kGateRecordBytes + 4);
}

// the probe path without records (the listed whole kernel) unless INERF_GATE_FUSED=0
bool mlp_gate_fused(uint32_t flags) {
    const char* const e = getenv("INERF_GATE_FUSED");
    return (flags & INERF_FLAG_GATE_PROBE) && !(e && e[0] == '0');
}

bool mlp_gate_applies(const inerf_net_desc& net, uint32_t flags) {
    return net.precision == INERF_PREC_F16X3 && net.variant == INERF_VARIANT_OBJECT && !(flags & INERF_FLAG_ENDPOINT) && !getenv("INERF_F16_KERNEL");
}

GatePlan mlp_gate_plan(int64_t n_rays, int n_samples, bool fused) {
    GatePlan g{};
    if (n_rays <= 0 || n_samples < 1) return g;
    const int64_t fit = gate_budget_points(fused) / n_samples;
    g.rays_per_sub = fit < 1 ? 1 : fit < n_rays ? fit : n_rays;
    g.n_sub = (n_rays + g.rays_per_sub - 1) / g.rays_per_sub;
    const int64_t pts = g.rays_per_sub * n_samples;
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    // (fused: no record region and no survivor list - the counters come first)
    g.idx_off = fused ? 0 : up(pts * kGateRecordBytes);
    g.count_off = fused ? 0 : g.idx_off + up(pts * 4);
    // (the probe's candidate list and counters come behind the budgeted part: the sub-ranges are the same with and without the probe)
    g.cand_off = g.count_off + up(g.n_sub * 4);
    g.cand_count_off = g.cand_off + up(pts * 4);
    g.cand_ss_off = g.cand_count_off + up(g.n_sub * 4);
    g.bytes = g.cand_ss_off + up(pts * 8);
    return g;
}

// kProbeMinObserved, or INERF_PROBE_MIN_OBS from the environment (tests)
static unsigned long long probe_min_observed() {
    if (const char* e = getenv("INERF_PROBE_MIN_OBS")) {
        const double v = atof(e);
        if (v >= 0.0) return v < 1.8e19 ? (unsigned long long)v : ~0ull;
    }
    return kProbeMinObserved;
}

// One thread in front of a launch's first probe kernel: the margin every sub-range of the launch uses.  What the listed trunks of this launch
// measure moves r_max and observed, not kappa_in_use.
__global__ void k_gate_margin_begin(GateMargin* st, unsigned long long min_observed) {
    st->kappa_in_use = gate_kappa(st->r_max, st->observed, min_observed);
    st->launches += 1u;
}

// `probe` (INERF_FLAG_GATE_PROBE): probe kernel -> listed whole kernel per sub-range (INERF_GATE_FUSED=0: probe kernel -> listed trunk -> heads)
// instead of trunk -> heads.  With p0.gate_state the probe's margin is that state's (k_gate_margin_begin), the probe lists its candidates' (s, S)
// and the listed kernel measures them against the exact sigma.
int launch_mlp_f16x3_gated(const MlpParams& p0, int64_t n_rays, void* gate_ws, bool probe, hipStream_t stream) {
    const bool fused = mlp_gate_fused(probe ? INERF_FLAG_GATE_PROBE : 0u);
    const GatePlan g = mlp_gate_plan(n_rays, p0.n_samples, fused);
    char* const ws = static_cast<char*>(gate_ws);
    unsigned int* const counts = reinterpret_cast<unsigned int*>(ws + g.count_off);
    unsigned int* const cand_counts = reinterpret_cast<unsigned int*>(ws + g.cand_count_off);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)g.n_sub * 4, stream);
    if (e == hipSuccess && probe) e = hipMemsetAsync(cand_counts, 0, (size_t)g.n_sub * 4, stream);
    if (e != hipSuccess) return record(e);
    static PerDeviceOnce attr_set;
    if (attr_set.first()) {
        const struct { void (*kernel)(const MlpParams); int lds_bytes; } kernels[] = {
            {k_mlp_gate_trunk_f16x3, kLdsBytesTrunk}, {k_mlp_gate_heads_f16x3, kLdsBytesT}, {k_mlp_gate_probe_f16, kLdsBytesT},
            {k_mlp_gate_trunk_listed_f16x3, kLdsBytesTrunk}, {k_mlp_gate_probe_wg2_f16, kLdsBytesProbeWg2},
            {k_mlp_gate_whole_listed_f16x3, kLdsBytesTrunk}};
        for (const auto& k : kernels) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes);
            if (e != hipSuccess) return record(e);
        }
        attr_set.mark();
    }
    // the probe's form: two four-wave workgroups per CU (mlp_f16_probe.h); INERF_PROBE_WG=1: the eight-wave workgroup (the same bits)
    const char* const wg_env = getenv("INERF_PROBE_WG");
    const bool probe_wg2 = !(wg_env && wg_env[0] == '1');
    GateMargin* const margin = probe ? p0.gate_state : nullptr;
    if (margin) hipLaunchKernelGGL(k_gate_margin_begin, dim3(1), dim3(1), 0, stream, margin, probe_min_observed());
    for (int64_t s = 0; s < g.n_sub; ++s) {
        const int64_t r0 = s * g.rays_per_sub, nr = n_rays - r0 < g.rays_per_sub ? n_rays - r0 : g.rays_per_sub;
        MlpParams p = p0;
        p.rays += r0 * INERF_RAY_FLOATS;
        p.z += r0 * p0.n_samples;
        p.raw += r0 * p0.n_samples * p0.channels;
        p.ray0 = (int)r0;
        p.n_points = (int)(nr * p0.n_samples);
        p.n_tiles = (p.n_points + kPtsT - 1) / kPtsT;
        p.gate_rec = fused ? nullptr : reinterpret_cast<unsigned char*>(ws);
        p.gate_idx = fused ? nullptr : reinterpret_cast<int*>(ws + g.idx_off);
        p.gate_count = counts + s;
        p.cand_idx = reinterpret_cast<int*>(ws + g.cand_off);
        p.cand_count = cand_counts + s;
        p.gate_state = margin;
        p.cand_ss = margin ? reinterpret_cast<float*>(ws + g.cand_ss_off) : nullptr;
        if (p.probe_out) p.probe_out = p0.probe_out + 2 * r0 * p0.n_samples;
        const int grid = p.n_tiles < device_cus() ? p.n_tiles : device_cus();
        if (probe) {
            if (probe_wg2) {
                const int grid2 = p.n_tiles < 2 * device_cus() ? p.n_tiles : 2 * device_cus();
                hipLaunchKernelGGL(k_mlp_gate_probe_wg2_f16, dim3(grid2), dim3(kProbeWg2Threads), kLdsBytesProbeWg2, stream, p);
            } else {
                hipLaunchKernelGGL(k_mlp_gate_probe_f16, dim3(grid), dim3(512), kLdsBytesT, stream, p);
            }
            // (persistent: the tile count is on the device)
            hipLaunchKernelGGL(fused ? k_mlp_gate_whole_listed_f16x3 : k_mlp_gate_trunk_listed_f16x3, dim3(grid), dim3(512), kLdsBytesTrunk, stream, p);
        } else {
            hipLaunchKernelGGL(k_mlp_gate_trunk_f16x3, dim3(grid), dim3(512), kLdsBytesTrunk, stream, p);      // (+ the parked encoding's extension area)
        }
        if (!fused) hipLaunchKernelGGL(k_mlp_gate_heads_f16x3, dim3(grid), dim3(512), kLdsBytesT, stream, p);      // (persistent: its tile count is on the device)
    }
    e = hipGetLastError();
    if (e == hipSuccess && getenv("INERF_GATE_LOG")) {      // debug: the survivor share of this launch (synchronises - not for timed runs)
        std::vector<unsigned int> h((size_t)g.n_sub), hc((size_t)g.n_sub, 0u);
        e = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = hipMemcpy(h.data(), counts, h.size() * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && probe) e = hipMemcpy(hc.data(), cand_counts, hc.size() * 4, hipMemcpyDeviceToHost);
        unsigned long long kept = 0, cand = 0;
        for (unsigned int c : h) kept += c;
        for (unsigned int c : hc) cand += c;
        const double pts = (double)(n_rays * p0.n_samples);
        fprintf(stderr, "inerf gate: %lld rays x %d samples in %lld sub-launches, %llu of %lld points survive (%.4f)", (long long)n_rays,
                p0.n_samples, (long long)g.n_sub, kept, (long long)(n_rays * p0.n_samples), (double)kept / pts);
        if (probe) fprintf(stderr, ", %llu are the probe's candidates (%.4f)", cand, (double)cand / pts);
        if (margin) {
            GateMargin m{};
            if (e == hipSuccess) e = hipMemcpy(&m, margin, sizeof m, hipMemcpyDeviceToHost);
            fprintf(stderr, ", margin %.6g (r_max %.6g over %llu listed points, launch %u)", (double)m.kappa_in_use, (double)m.r_max, m.observed, m.launches);
        }
        fprintf(stderr, "\n");
    }
    return record(e);
}

}  // namespace inerf

extern "C" float inerf_gate_kappa(float r_max, int64_t observed, int64_t min_observed) {
    return inerf::gate_kappa(r_max, observed < 0 ? 0ull : (unsigned long long)observed, min_observed < 0 ? 0ull : (unsigned long long)min_observed);
}
extern "C" int64_t inerf_gate_min_observed(void) {
    const unsigned long long v = inerf::probe_min_observed();
    return v > (unsigned long long)INT64_MAX ? INT64_MAX : (int64_t)v;
}

namespace inerf {

// The occupancy grid's launch: like the gated trunk's - one eight-wave workgroup per CU with the parked encoding's extension area, persistent over the tiles.
int launch_grid_trunk_f16x3(MlpParams& p, int64_t n_points, bool ssr, hipStream_t stream) {
    p.n_tiles = (int)((n_points + kPtsT - 1) / kPtsT);
    const int grid = p.n_tiles < device_cus() ? p.n_tiles : device_cus();
    void (*kern)(const MlpParams) = ssr ? k_grid_trunk_f16x3<true> : k_grid_trunk_f16x3<false>;
    static PerDeviceOnce attr_sets[2];
    if (attr_sets[ssr].first()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytesTrunk);
        if (e != hipSuccess) return record(e);
        attr_sets[ssr].mark();
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), kLdsBytesTrunk, stream, p);
    return record(hipGetLastError());
}

int launch_mlp_f16x3_t128(MlpParams& p, int64_t n_points, bool ssr, hipStream_t stream) {
    p.n_tiles = (int)((n_points + kPtsT - 1) / kPtsT);
    const int grid = p.n_tiles < device_cus() ? p.n_tiles : device_cus();
    const bool save = p.save != nullptr;
    if (ssr && save) return INERF_E_UNSUPPORTED;
    const char* form = getenv("INERF_F16_KERNEL");
    const bool pipe = !ssr && !save && form && form[0] == 'p';        // the pipelined trunk (opt-in)
    void (*kern)(const MlpParams) = ssr ? k_encode_mlp_f16x3_t128<true> : save ? k_encode_mlp_f16x3_t128<false, true>
                                  : pipe ? k_encode_mlp_f16x3_t128<false, false, true> : k_encode_mlp_f16x3_t128<false>;
    static PerDeviceOnce attr_sets[4];
    PerDeviceOnce& attr_set = attr_sets[ssr ? 1 : save ? 2 : pipe ? 3 : 0];
    if (attr_set.first()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytesT);
        if (e != hipSuccess) return record(e);
        attr_set.mark();
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), kLdsBytesT, stream, p);
    return record(hipGetLastError());
}

}  // namespace inerf
