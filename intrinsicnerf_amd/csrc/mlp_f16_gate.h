// mlp_f16_gate.h - device code the density gate's kernels share (included by mlp_f16_t128.hip behind its tile constants):
// the one tile body of mlp_f16_t128.hip (whole, gated trunk listed or not, gated heads, eight-wave probe) and the probe as two workgroups per
// CU (mlp_f16_probe.h).  Every piece here exists ONCE: the forms' results agree bit for bit because they run the same text.
#pragma once

namespace inerf {

// the 16 pad bytes behind a row's direction columns (hi plane; no GEMM uses what it reads there).  Gated trunk and probe: rows 0..7 hold the
// survivor counts of the tile's eight groups of 16 points, row 8 the tile's first slot.  Gated heads: row r holds four words, non-zero when
// point r left the f16 range
__device__ __forceinline__ int* pad_words(_Float16* ldst, int r) { return reinterpret_cast<int*>(ldst + r * kRowD + kWidth + kDirCols); }

// Position encoding of point gp into columns 0..63 of `row`: x = o + d z of ray r, or (kGrid, the occupancy grid: r unused) lattice point
// ray0 + gp of p.grid (grid.h); thread `part` of the point's kParts takes every kParts-th frequency, part kXyzPart the raw xyz and the zero
// fill.  Store: split_store (hi | lo), hi_store_parked (hi | the same in the lo plane) or hi_store (the hi plane alone: kLoPlane = 0, nothing
// behind the hi plane is zeroed either).
template <bool kSsr, int kParts, int kXyzPart, auto Store, int kLoPlane, bool kGrid = false>
__device__ __forceinline__ void encode_position(const MlpParams& p, const float* __restrict__ r, int gp, int part, _Float16* row, float& amax) {
    float x[3];
    if constexpr (kGrid) {
        grid_point(p.grid, p.ray0 + gp, x);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (kSsr && p.xyz_div != 1.0f) x[c] = __fdiv_rn(x[c], p.xyz_div);          // semantic_nerf.py:64
    } else {
        const float zz = __builtin_nontemporal_load(p.z + gp);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = __fadd_rn(r[c], __fmul_rn(r[3 + c], zz));                            // run_nerf.py:488
            if (kSsr && p.xyz_div != 1.0f) x[c] = __fdiv_rn(x[c], p.xyz_div);          // semantic_nerf.py:64
        }
    }
    for (int f = part; f < p.l_xyz; f += kParts) {
        const float s = (float)(1 << f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sn, cs;
            fast_sincosf(x[c] * s, &sn, &cs);
            Store(row + 3 + 6 * f + c, sn, amax);
            Store(row + 6 + 6 * f + c, cs, amax);
        }
    }
    if (part == kXyzPart) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Store(row + c, x[c], amax);
        for (int c = 3 + 6 * p.l_xyz; c < kEncCols; ++c) {
            row[c] = (_Float16)0.0f;
            if constexpr (kLoPlane != 0) row[kLoPlane + c] = (_Float16)0.0f;
        }
    }
}

// The tile's encoding (columns 0..63 of kPlanes planes) parked in LDS for the skip layer (kParkRowPieces: five of a row's eight sixteen-byte
// pieces in the dead columns 256..295 of the piece's own row and plane, three in the extension area behind the planes - [plane][row][3]) before
// layer 0's epilogue overwrites it; every wave's copy is read in front of that layer's first barrier.  A thread parks and restores the SAME
// four pieces - piece j = tid & 7 of row tid >> 3 and the rows kThreads / 8 apart, plane by plane - so the parked copy needs no barrier of its
// own.  The pad words it covers hold the counts only behind layer 7.  (Addresses from a laundered index, rebuilt at the skip layer instead of
// held across five layers.)
template <int kPlanes, int kThreads>
__device__ __forceinline__ void park_encoding(_Float16* ldst, int tid, bool restore) {
    constexpr int kPerPlane = 4 / kPlanes, kRows = kThreads / 8;
    static_assert(kPerPlane * kRows == kPtsT, "four pieces per thread cover the tile's rows of every plane");
    int t = tid;
    asm volatile("" : "+v"(t));
    const int r = t >> 3, j = t & 7;
    const bool in_row = j < kParkRowPieces;
    _Float16* const cols = ldst + r * kRowD + j * 8;
    _Float16* const parked = in_row ? cols + kColDirD : ldst + kPlanes * kPlaneT + (r * kParkExtPieces + (j - kParkRowPieces)) * 8;
    u32x4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int at_cols = (i / kPerPlane) * kPlaneT + (i % kPerPlane) * kRows * kRowD;
        const _Float16* const a = cols + at_cols;
        const _Float16* const b = parked + (in_row ? at_cols : ((i / kPerPlane) * kPtsT + (i % kPerPlane) * kRows) * kParkExtPieces * 8);
        v[i] = *reinterpret_cast<const u32x4*>(restore ? b : a);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int at_cols = (i / kPerPlane) * kPlaneT + (i % kPerPlane) * kRows * kRowD;
        _Float16* const a = cols + at_cols;
        _Float16* const b = parked + (in_row ? at_cols : ((i / kPerPlane) * kPtsT + (i % kPerPlane) * kRows) * kParkExtPieces * 8);
        *reinterpret_cast<u32x4*>(restore ? a : b) = v[i];
    }
}

// The probe's trunk: one product per MAC, the hi plane in place - wave `wave` owns 32 RB output channels x all 128 points (RB = 1: eight waves,
// RB = 2: four).  frag(slot, k-blocks): the wave's weight stream of a 256-wide layer, whose first fragments `pre` holds on entry (and holds
// again, of layer 0, on return).  skip_encoding(): where the skip layer's encoding is read (called behind the GEMM over h4).
template <int RB, class Frag, class SkipEncoding>
__device__ __forceinline__ void probe_trunk(WidePreH<RB>& pre, const WeightBuf& wb, const NetLayout& L, Frag&& frag, const _Float16* xr, _Float16* xd,
                                            int wave, int lane_t, f16x2& amax2, SkipEncoding&& skip_encoding) {
    f32x16 am[RB][4];
    f32x4 bias[RB][4];
    float inv;
    auto pf = [&](const GemmSlot& s, int kbt, int kb_first) { prefetch_w<RB, 4096, 2048, 1>(pre, wb, frag(s, kbt) + kb_first * 4096); };
    auto store_hi = [&](const GemmSlot& s, const GemmSlot& next, int kbt, int kb_first) {
        load_bias<RB>(bias, inv, wb, (s.b + 32 * RB * wave) * 4, (s.b + kWidth) * 4, lane_t);
        pf(next, kbt, kb_first);
        __syncthreads();                       // every wave has read the layer's input
        wide_store_h<RB, kRowD, kPlaneT, false, false, 4, true, true>(am, inv, bias, xd, true, amax2, nullptr, 0, 0, 0);
        __syncthreads();
    };
    wide_gemm_h<RB, 4, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag(L.trunk[0], 4), xr, 0, 0, lane_t, am);
    store_hi(L.trunk[0], L.trunk[1], 16, 0);
#pragma unroll 1
    for (int layer = 1; layer < kSkipInput; ++layer) {
        wide_gemm_h<RB, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag(L.trunk[layer], 16), xr, 0, 0, lane_t, am);
        if (layer + 1 < kSkipInput) store_hi(L.trunk[layer], L.trunk[layer + 1], 16, 0);
        else                        store_hi(L.trunk[layer], L.trunk[kSkipInput], 20, 4);
    }
    {   // pts_linears[5] over cat([pts, h]): the h part (k-blocks 4..19 of the stream), then the encoding part on top of the same accumulators
        const GemmSlot& s = L.trunk[kSkipInput];
        wide_gemm_h<RB, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag(s, 20) + 4 * 4096, xr, 0, 0, lane_t, am);
        pf(s, 20, 0);
        wide_gemm_h<RB, 4, 0, kRowD, kPlaneT, false, 4096, 4, 2048, false, 1>(pre, wb, frag(s, 20), skip_encoding(), 0, 0, lane_t, am);
        store_hi(s, L.trunk[6], 16, 0);
    }
    wide_gemm_h<RB, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag(L.trunk[6], 16), xr, 0, 0, lane_t, am);
    store_hi(L.trunk[6], L.trunk[7], 16, 0);
    wide_gemm_h<RB, 16, 0, kRowD, kPlaneT, true, 4096, 4, 2048, true, 1>(pre, wb, frag(L.trunk[7], 16), xr, 0, 0, lane_t, am);
    store_hi(L.trunk[7], L.trunk[0], 4, 0);
}

// raw rows of the 16 points from pt16 on (lanes 0..15 hold their sigma): 16 points x 11 floats as 44 sixteen-byte pieces (like the whole
// kernel's), sigma in channel 3 of zeros; four-byte stores where the rows are ragged, wider than 11 or not on a sixteen-byte boundary
__device__ __forceinline__ void store_sigma_rows(const MlpParams& p, int pt16, float sigma, int lane_t) {
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
    } else if (lane_t < 16 && pt16 + lane_t < p.n_points) {
        float* const out_row = p.raw + (size_t)(pt16 + lane_t) * p.channels;
#pragma unroll
        for (int c = 0; c < INERF_BASE_CHANNELS; ++c) __builtin_nontemporal_store(c == 3 ? sigma : 0.0f, out_row + c);
    }
}

// group g of the tile's eight groups of 16 points: its count (kept = the ballot of its lanes) into pad word g, for reserve_slots
__device__ __forceinline__ void post_count(_Float16* ldst, int g, unsigned kept, int lane_t) {
    if (lane_t == 0) pad_words(ldst, g)[0] = __popc(kept);
}

// Slots for the tile's kept points, in point order: a wave holds kGroups groups of 16 points (group kGroups * wave + h: lane l < 16 keeps
// point[h] when keep[h]; kept[h] = the ballot, posted).  The eight counts meet in pad words 0..7, thread 0 reserves the tile's contiguous range
// with ONE atomicAdd on `counter` (first slot: pad word 8), every kept point's index goes into `list`.  Returns this wave's first slot
// (<= the launch's points - this wave's kept points: inside the buffers).  Two barriers: every wave's rows are written behind the first.
// ss_list (the probe with a GateMargin state; else nullptr, a uniform branch): the kept point's (s, S) = (s[h], big_s[h]) into ss_list[slot], for
// the listed trunk to hold against the exact sigma.
template <int kGroups>
__device__ __forceinline__ int reserve_slots(_Float16* ldst, unsigned int* counter, int* list, const bool (&keep)[kGroups], const unsigned (&kept)[kGroups],
                                             const int (&point)[kGroups], int wave, int lane_t, int tid, float* ss_list = nullptr,
                                             const float* s = nullptr, const float* big_s = nullptr) {
    __syncthreads();                           // the eight counts are there
    int before = 0, total = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int c = pad_words(ldst, g)[0];
        total += c;
        before += g < kGroups * wave ? c : 0;
    }
    if (tid == 0) pad_words(ldst, 8)[0] = total > 0 ? (int)atomicAdd(counter, (unsigned)total) : 0;
    __syncthreads();
    const int slot0 = __builtin_amdgcn_readfirstlane(pad_words(ldst, 8)[0] + before);
    int slot = slot0;
#pragma unroll
    for (int h = 0; h < kGroups; ++h) {
        if (keep[h]) {
            const int at = slot + __popc(kept[h] & ((1u << lane_t) - 1u));
            list[at] = point[h];
            if (ss_list) *reinterpret_cast<float2*>(ss_list + 2 * (size_t)at) = float2{s[h], big_s[h]};
        }
        slot += __popc(kept[h]);
    }
    return slot0;
}

}  // namespace inerf
