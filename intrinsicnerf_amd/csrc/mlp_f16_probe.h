// mlp_f16_probe.h - the density gate's probe as TWO workgroups per CU (included by mlp_f16_t128.hip behind its tile constants).
//
// k_mlp_gate_probe_f16 holds the CU with one workgroup of eight waves in the same phase: its nine hi-only epilogues, eighteen barriers,
// the encoder and the tail are all serial to the MFMAs (the matrix pipe is busy about half the time).  The probe reads and writes the hi
// plane alone, so a 128-point tile needs 75,776 B of LDS + 6,144 B for the parked encoding = 81,920 B, and TWO tiles are exactly the
// CU's 163,840 B.  Here FOUR waves walk a 128-point tile: wave w owns the 64 output channels of packing wave w (both of its 32-channel
// row blocks, the blob's default k-block stride) x all 128 points - 128 accumulator registers, 8 MFMAs per 4 ds_read_b128 and 2 weight
// loads.  Per 128 points the L2 -> CU weight stream is the eight-wave probe's (128 KB per 256-wide layer), the LDS operand reads are
// half of it.  The second workgroup's GEMM fills the matrix pipe while this one is in an epilogue, at a barrier or in the encoder.
//
// Same products in the same k order with the same instruction, the same epilogue per value: (s, S) per point are the eight-wave
// probe's bits.  The encoding is parked like the gated trunk's (kParkRowPieces: five of a row's eight sixteen-byte pieces in the dead
// columns 256..295 of the row, three in an extension area behind the plane) and copied back between two barriers at the skip layer.
#pragma once

namespace inerf {

constexpr int kProbeWg2Threads = 256;
constexpr int kProbeWg2ExtBytes = kPtsT * kParkExtPieces * 16;            // 6,144
constexpr int kLdsBytesProbeWg2 = kPlaneT * 2 + kProbeWg2ExtBytes;        // 81,920
static_assert(2 * kLdsBytesProbeWg2 <= 160 * 1024, "two probe workgroups share the CU's LDS");

__device__ __forceinline__ void mlp_gate_probe_wg2_tiles(const MlpParams& p) {
    constexpr int kParts = kProbeWg2Threads / kPtsT;      // 2
    extern __shared__ __attribute__((aligned(16))) _Float16 ldst[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..3
    const NetLayout& L = p.L;

    _Float16* const xw = ldst + (tid & 31) * kRowD;
    const _Float16* const xr = xw + 8 * ((tid & 63) >> 5);                 // wide GEMM operand reads (+ column)
    _Float16* const xd = xw + 4 * ((tid & 63) >> 5) + 64 * wave;           // wide stores: this wave's 64 channels

    WeightBuf wb;
    wb.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wts), 0, L.total_floats * 4, 0x00020000);
    wb.voff = (tid & 63) * 16;
    // this wave's 64-channel stream of a 256-wide layer: packing wave `wave`, k-blocks 4 KiB apart, row blocks 2 KiB apart (hi fragments alone)
    auto frag64 = [&](const GemmSlot& s, int kbt) { return (s.w + wave * kbt * 2 * 2 * 256) * 4; };
    WidePreH<2> pre;
    prefetch_w<2, 4096, 2048, 1>(pre, wb, frag64(L.trunk[0], 4));
    const float kappa = probe_kappa(p);          // the margin of this launch

    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        int lane_t = tid;                         // (laundered per tile, like the eight-wave form's)
        asm volatile("" : "+v"(lane_t));
        lane_t &= 63;
        float amax = 0.0f;                        // the tile's running maxima: the f16 range guard
        f16x2 amax2 = {(_Float16)0.0f, (_Float16)0.0f};
        // ---------------- encode -> hi plane (xyz: columns 0..63) ----------------
        {
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
            const int pt = tid_o % kPtsT, part = tid_o / kPtsT;
            int gp = tile * kPtsT + pt;
            gp = gp < p.n_points ? gp : p.n_points - 1;
            const int ray = gp / p.n_samples;
            const float* __restrict__ r = p.rays + (size_t)ray * INERF_RAY_FLOATS;
            _Float16* row = ldst + pt * kRowD;
            encode_position<false, kParts, kParts - 1, &hi_store, 0>(p, r, gp, part, row, amax);
        }
        __syncthreads();
        park_encoding<1, kProbeWg2Threads>(ldst, tid, false);      // (before layer 0's epilogue overwrites the encoding)

        // ---------------- trunk: the skip layer's encoding back in columns 0..63 between two barriers ----------------
        probe_trunk<2>(pre, wb, L, frag64, xr, xd, wave, lane_t, amax2, [&]() {
            __syncthreads();                       // every wave has read h4
            park_encoding<1, kProbeWg2Threads>(ldst, tid, true);
            __syncthreads();
            return xr;
        });

        // ---------------- s and S, the raw rows, the candidate list: this wave's 32 points as two groups of 16 ----------------
        // (group 2 wave + h is wave 2 wave + h of the eight-wave form: the same counts in the same pad words, the list in point order)
        bool keep[2];
        unsigned kept[2];
        float s_row[2], big_s_row[2];              // lanes 0..15: the groups' (s, S)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int pt16 = tile * kPtsT + 32 * wave + 16 * h;
            const _Float16* const xs_g = ldst + (32 * wave + 16 * h + (lane_t & 15)) * kRowD + 8 * (lane_t >> 4);
            float& sigma = s_row[h];
            float& scale = big_s_row[h];
            skinny_probe_h<8>(wb, L.alpha.w * 4, L.alpha.b * 4, (L.alpha.b + 16) * 4, xs_g, lane_t, sigma, scale);
            const bool valid = lane_t < 16 && pt16 + lane_t < p.n_points;
            keep[h] = valid && !(sigma < -kappa * scale);
            kept[h] = __builtin_amdgcn_readfirstlane((unsigned)__ballot(keep[h]));
            store_sigma_rows(p, pt16, sigma, lane_t);
            if (p.probe_out && valid) {            // tests: (s, S) per point
                p.probe_out[2 * (size_t)(pt16 + lane_t)] = sigma;
                p.probe_out[2 * (size_t)(pt16 + lane_t) + 1] = scale;
            }
        }
        post_count(ldst, 2 * wave, kept[0], lane_t);         // (behind both groups' rows: posted per group in the loop the frame takes 0.5 ms
        post_count(ldst, 2 * wave + 1, kept[1], lane_t);     // longer - profiles/gate_dedup_bench.txt)
        const int pt32 = tile * kPtsT + 32 * wave;
        const int point[2] = {pt32 + lane_t, pt32 + 16 + lane_t};
        reserve_slots<2>(ldst, p.cand_count, p.cand_idx, keep, kept, point, wave, lane_t, tid, p.cand_ss, s_row, big_s_row);
        flag_f16_range(p, tile * kPtsT, kPtsT, amax, amax2, lane_t);
        __syncthreads();                           // the rows and the pad words are read: the next tile's encode and parking may overwrite them
    }
}

__global__ __launch_bounds__(kProbeWg2Threads, 2) void k_mlp_gate_probe_wg2_f16(const MlpParams p) { mlp_gate_probe_wg2_tiles(p); }

}  // namespace inerf
