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
    auto pad_of = [&](int r) { return reinterpret_cast<int*>(ldst + r * kRowD + kWidth + kDirCols); };

    WidePreH<2> pre;
    auto pf = [&](const GemmSlot& s, int kbt, int kb_first) { prefetch_w<2, 4096, 2048, 1>(pre, wb, frag64(s, kbt) + kb_first * 4096); };
    pf(L.trunk[0], 4, 0);

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
            const float zz = __builtin_nontemporal_load(p.z + gp);
            float x[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(r[c], __fmul_rn(r[3 + c], zz));      // run_nerf.py:488
            auto hi_store = [&](_Float16* dst, float v) {      // hi_store_parked's value and maximum, the plane alone
                const float t = v * kActScale;
                dst[0] = (_Float16)t;
                amax = fmaxf(amax, fabsf(t));
            };
            for (int f = part; f < p.l_xyz; f += kParts) {
                const float s = (float)(1 << f);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float sn, cs;
                    fast_sincosf(x[c] * s, &sn, &cs);
                    hi_store(row + 3 + 6 * f + c, sn);
                    hi_store(row + 6 + 6 * f + c, cs);
                }
            }
            if (part == kParts - 1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) hi_store(row + c, x[c]);
                for (int c = 3 + 6 * p.l_xyz; c < kEncCols; ++c) row[c] = (_Float16)0.0f;
            }
        }
        __syncthreads();
        // the encoding parked for the skip layer before layer 0's epilogue overwrites it (every wave's copy is read in front of that
        // layer's first barrier): a thread parks and restores the SAME four pieces - piece j = tid & 7 of rows tid >> 3 + 32 i - so the
        // parked copy needs no barrier of its own.  The pad words it covers hold the candidate counts only behind layer 7.
        auto park_copy = [&](bool restore) {
            int t = tid;
            asm volatile("" : "+v"(t));
            const int r = t >> 3, j = t & 7;
            const bool in_row = j < kParkRowPieces;
            _Float16* const cols = ldst + r * kRowD + j * 8;
            _Float16* const parked = in_row ? cols + kColDirD : ldst + kPlaneT + (r * kParkExtPieces + (j - kParkRowPieces)) * 8;
            u32x4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const _Float16* const a = cols + i * 32 * kRowD;
                const _Float16* const b = parked + (in_row ? i * 32 * kRowD : i * 32 * kParkExtPieces * 8);
                v[i] = *reinterpret_cast<const u32x4*>(restore ? b : a);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                _Float16* const a = cols + i * 32 * kRowD;
                _Float16* const b = parked + (in_row ? i * 32 * kRowD : i * 32 * kParkExtPieces * 8);
                *reinterpret_cast<u32x4*>(restore ? a : b) = v[i];
            }
        };
        park_copy(false);

        // ---------------- trunk: one product per MAC, the hi plane in place ----------------
        f32x16 am[2][4];
        f32x4 bias[2][4];
        float inv;
        auto store_hi = [&](const GemmSlot& s, const GemmSlot& next, int kbt, int kb_first) {
            load_bias<2>(bias, inv, wb, (s.b + 64 * wave) * 4, (s.b + kWidth) * 4, lane_t);
            pf(next, kbt, kb_first);
            __syncthreads();                       // every wave has read the layer's input
            wide_store_h<2, kRowD, kPlaneT, false, false, 4, true, true>(am, inv, bias, xd, true, amax2, nullptr, 0, 0, 0);
            __syncthreads();
        };
        wide_gemm_h<2, 4, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag64(L.trunk[0], 4), xr, 0, 0, lane_t, am);
        store_hi(L.trunk[0], L.trunk[1], 16, 0);
#pragma unroll 1
        for (int layer = 1; layer < kSkipInput; ++layer) {
            wide_gemm_h<2, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag64(L.trunk[layer], 16), xr, 0, 0, lane_t, am);
            if (layer + 1 < kSkipInput) store_hi(L.trunk[layer], L.trunk[layer + 1], 16, 0);
            else                        store_hi(L.trunk[layer], L.trunk[kSkipInput], 20, 4);
        }
        {   // pts_linears[5] over cat([pts, h]): the h part (k-blocks 4..19 of the stream), then the encoding back in columns 0..63
            const GemmSlot& s = L.trunk[kSkipInput];
            wide_gemm_h<2, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag64(s, 20) + 4 * 4096, xr, 0, 0, lane_t, am);
            pf(s, 20, 0);
            __syncthreads();                       // every wave has read h4
            park_copy(true);
            __syncthreads();
            wide_gemm_h<2, 4, 0, kRowD, kPlaneT, false, 4096, 4, 2048, false, 1>(pre, wb, frag64(s, 20), xr, 0, 0, lane_t, am);
            store_hi(s, L.trunk[6], 16, 0);
        }
        wide_gemm_h<2, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag64(L.trunk[6], 16), xr, 0, 0, lane_t, am);
        store_hi(L.trunk[6], L.trunk[7], 16, 0);
        wide_gemm_h<2, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag64(L.trunk[7], 16), xr, 0, 0, lane_t, am);
        store_hi(L.trunk[7], L.trunk[0], 4, 0);

        // ---------------- s and S, the raw rows, the candidate list: this wave's 32 points as two groups of 16 ----------------
        // (group 2 wave + h is wave 2 wave + h of the eight-wave form: the same counts in the same pad words, the list in point order)
        bool keep[2];
        unsigned kept[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int pt16 = tile * kPtsT + 32 * wave + 16 * h;
            const _Float16* const xs_g = ldst + (32 * wave + 16 * h + (lane_t & 15)) * kRowD + 8 * (lane_t >> 4);
            float sigma, scale;                    // lanes 0..15: the group's points
            skinny_probe_h<8>(wb, L.alpha.w * 4, L.alpha.b * 4, (L.alpha.b + 16) * 4, xs_g, lane_t, sigma, scale);
            const bool valid = lane_t < 16 && pt16 + lane_t < p.n_points;
            keep[h] = valid && !(sigma < -kProbeKappa * scale);
            kept[h] = __builtin_amdgcn_readfirstlane((unsigned)__ballot(keep[h]));
            // raw: the group's 16 points x 11 floats as 44 sixteen-byte pieces (like the whole kernel's), s in channel 3 of zeros
            float piece[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * (lane_t < 44 ? lane_t : 43) + i, pt = e / INERF_BASE_CHANNELS;
                const float s_pt = __shfl(sigma, pt);
                piece[i] = e - INERF_BASE_CHANNELS * pt == 3 ? s_pt : 0.0f;
            }
            if (p.channels == INERF_BASE_CHANNELS && pt16 + 16 <= p.n_points && (reinterpret_cast<uintptr_t>(p.raw) & 15) == 0) {
                if (lane_t < 44)
                    __builtin_nontemporal_store(f32x4{piece[0], piece[1], piece[2], piece[3]},
                                                reinterpret_cast<f32x4*>(p.raw + (size_t)pt16 * INERF_BASE_CHANNELS) + lane_t);
            } else if (valid) {
                float* const out_row = p.raw + (size_t)(pt16 + lane_t) * p.channels;
#pragma unroll
                for (int c = 0; c < INERF_BASE_CHANNELS; ++c) __builtin_nontemporal_store(c == 3 ? sigma : 0.0f, out_row + c);
            }
            if (p.probe_out && valid) {            // tests: (s, S) per point
                p.probe_out[2 * (size_t)(pt16 + lane_t)] = sigma;
                p.probe_out[2 * (size_t)(pt16 + lane_t) + 1] = scale;
            }
        }
        if (lane_t == 0) {
            pad_of(2 * wave)[0] = __popc(kept[0]);
            pad_of(2 * wave + 1)[0] = __popc(kept[1]);
        }
        __syncthreads();                           // the eight counts are there
        int before = 0, total = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int c = pad_of(g)[0];
            total += c;
            before += g < 2 * wave ? c : 0;
        }
        if (tid == 0) pad_of(8)[0] = total > 0 ? (int)atomicAdd(p.cand_count, (unsigned)total) : 0;
        __syncthreads();
        // (<= the launch's points - this wave's candidates: inside the list)
        const int slot0 = __builtin_amdgcn_readfirstlane(pad_of(8)[0] + before);
        const int slot1 = slot0 + __popc(kept[0]);
        const int pt32 = tile * kPtsT + 32 * wave;
        if (keep[0]) p.cand_idx[slot0 + __popc(kept[0] & ((1u << lane_t) - 1u))] = pt32 + lane_t;
        if (keep[1]) p.cand_idx[slot1 + __popc(kept[1] & ((1u << lane_t) - 1u))] = pt32 + 16 + lane_t;
        flag_f16_range(p, tile * kPtsT, kPtsT, amax, amax2, lane_t);
        __syncthreads();                           // the rows and the pad words are read: the next tile's encode and parking may overwrite them
    }
}

__global__ __launch_bounds__(kProbeWg2Threads, 2) void k_mlp_gate_probe_wg2_f16(const MlpParams p) { mlp_gate_probe_wg2_tiles(p); }

}  // namespace inerf
