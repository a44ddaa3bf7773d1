// csrc/raster_edges.hip — the per-tile raster half of the edge pass (formulation and slot layout: edge_slots.hpp; the tiles' lists are
// bin_edges.hip's): one workgroup per 16x16 tile as in raster.hip walks the tile's list in key (= draw) order; entries are triangles, edges,
// backdrop units and one COVER entry per (item, tile).
//
//   k_raster_edges<..> every lane evaluates every entry on its own samples: msaa 1 and 4, with or without stroke triangles.
//   k_raster_fill<..>  fill scenes at msaa 1: the same walk class-batched, with packed counters.
//   k_raster_rows<..>  fill scenes at msaa 1: the winding numbers accumulated in LDS, lanes over (entry, sample row).
// launch_raster_edges picks one of them per pass; the three are bit-equal where they overlap.
#include <type_traits>

#include "edge_slots.hpp"
#include "launch.hpp"
#include "raster_tile_list.hpp"

namespace crh {

// The late start (see "Occlusion" in k_raster_edges) of a list longer than one chunk is found before the walk: the chunks' keys and the first word
// of their slots from the END of the list — X, the last opaque cover over the whole tile none of whose item's triangles are in the
// list (keys ascend: a binary search), then R, the last cover before X that resets the whole tile. The walk begins behind R: walk_from,
// and checks at X that it overwrote every sample: verify_entry (absolute positions in the list; unchanged when there is no such pair).
// The sorted keys are in `keys` (LDS) or — sorted_in_place — in `segment`. (Device only, not CRH_D: ballots and lane reads have no host form.)
__device__ __forceinline__ void find_late_start(const uint8_t* slots, const uint32_t* segment, const uint32_t* keys, bool sorted_in_place, uint32_t n, uint32_t lane, uint32_t& walk_from, uint32_t& verify_entry) {
    auto key_of = [&](uint32_t i) -> uint32_t { return sorted_in_place ? __hip_atomic_load(segment + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : keys[i]; };
    uint32_t x_at = 0xFFFFFFFFu;
    for (uint32_t c0 = ((n - 1u) >> 6) << 6;; c0 -= 64u) {
        const uint32_t k = c0 + lane < n ? key_of(c0 + lane) : 0xFFFFFFFFu;
        uint32_t code = 0;
        if (c0 + lane < n) {
            const uint32_t flags = *reinterpret_cast<const uint32_t*>(slots + (size_t)k * 32u);
            code = ((flags >> 4) & 15u) == EK_SYNTH ? (flags >> 8) & 31u : 0u;
        }
        unsigned long long resets = __builtin_amdgcn_ballot_w64(code >= 4u + kCoverHull);
        if (x_at == 0xFFFFFFFFu) {
            unsigned long long candidates = __builtin_amdgcn_ballot_w64(code >= 4u + kCoverOpaque);
            while (candidates) {
                const uint32_t at = 63u - (uint32_t)__builtin_clzll(candidates);
                const SynthRec sr = load_uniform(reinterpret_cast<const SynthRec*>(slots + (size_t)__builtin_amdgcn_readlane(k, at) * 32u));
                uint32_t lo = 0, hi = n; // the number of keys below the item's synthetic slots
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (key_of(mid) < sr.synth_a) lo = mid + 1u;
                    else hi = mid;
                }
                if (lo == 0u || key_of(lo - 1u) < sr.first_slot) {
                    x_at = c0 + at;
                    resets &= (1ull << at) - 1ull;
                    break;
                }
                candidates &= ~(1ull << at);
            }
        }
        if (x_at != 0xFFFFFFFFu && resets) {
            walk_from = c0 + 64u - (uint32_t)__builtin_clzll(resets); // behind the last whole-tile reset before X
            verify_entry = x_at;
            break;
        }
        if (c0 == 0u) break;
    }
}

// ---------------------------------------------------------------------------------------------- k_raster_edges
// A 16-bit row mask -> the lane masks of the lane's sample slots. Lane (px, rq) owns row bit rq + 4b in slot b (msaa 1) or 4 rq + q in
// slot q (msaa 4); a slot's lane mask repeats each of its four row bits over a 16-lane group. Scalar unit only: s_bitreplicate doubles
// every bit of its 32-bit operand, a tree of 8 of them turns 16 bits into 4 x 64.
struct SlotMasks {
    unsigned long long m[4];
};
CRH_D unsigned long long bit_double(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long out;
    asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(out) : "s"(v));
    return out;
#else
    return v;
#endif
}
template <int S>
CRH_D SlotMasks slot_masks(uint32_t rows16) {
    if (S == 4) { // gather every sample's four row bits: bit 4 q + rq <- bit 4 rq + q (a 4 x 4 bit transpose)
        const uint32_t t = rows16;
        rows16 = (t & 0x8421u) | ((t & 0x0842u) << 3) | ((t & 0x0084u) << 6) | ((t & 0x0008u) << 9) | ((t >> 3) & 0x0842u) | ((t >> 6) & 0x0084u) | ((t >> 9) & 0x0008u);
    }
    const unsigned long long x2 = bit_double(rows16 & 0xFFFFu), x4 = bit_double((uint32_t)x2);
    const unsigned long long lo = bit_double((uint32_t)x4), hi = bit_double((uint32_t)(x4 >> 32));
    SlotMasks k;
    k.m[0] = bit_double((uint32_t)lo), k.m[1] = bit_double((uint32_t)(lo >> 32)), k.m[2] = bit_double((uint32_t)hi), k.m[3] = bit_double((uint32_t)(hi >> 32));
    return k;
}

#ifndef CRH_EDGE_TILE_WAVES
#define CRH_EDGE_TILE_WAVES 5 // measured 4: 0.321, 5: 0.322, 6: 0.331 (spills), 8: 0.421 ms on the benchmark scene
#endif
// (A second argument — the maximum — was tried to leave register room for the binning kernels beside this one: at a cap of four the
// compiler takes 106 registers and nothing else fits either; and a maximum above the hardware's eight makes LLVM drop the whole attribute.)
#ifndef CRH_COL_LDS_SAMPLES
#define CRH_COL_LDS_SAMPLES 2 // msaa 4: samples of a lane whose colours live in LDS between the covers (k_raster_edges); dashed scene, raster alone: 0 (round 4) 1.60, 2: 1.545, 3: 1.572, 4 (four workgroups per CU): 1.80 - 1.87 ms
#endif
#ifndef CRH_STROKE_TILE_WAVES
#define CRH_STROKE_TILE_WAVES 5 // dashed strokes, msaa 4 (ms): 1 (145 registers): 2.96, 4: 2.34, 5: 2.24, 6: 2.83, 8: 5.05 — the kernel waits, it does not issue
#endif
// One workgroup per 16x16 tile, laid out exactly as k_raster_tile (raster.hip): msaa 1 = one wavefront, four pixel rows per lane;
// msaa 4 = four wavefronts, one pixel row x four samples per lane. Per sample the lane keeps the winding counter, the hull winding of
// the item being drawn and the colour; entries are walked in key order (= draw order).
// LONG: the late start also for lists of several chunks (selected by the host for frames whose tiles hold many entries on average).
template <int S, int ROWS, bool STROKES, bool LONG, bool XFMT = false> // XFMT: the frame formats 3-8 (raster_common.hpp store_px)
__global__ __launch_bounds__(64 * (4 / ROWS)) __attribute__((amdgpu_waves_per_eu((STROKES || S == 4) ? CRH_STROKE_TILE_WAVES : CRH_EDGE_TILE_WAVES))) void k_raster_edges(SceneDev s, RasterParams r) {
    const uint32_t bid = blockIdx.x; // the workgroup's place in the frame's tile order
    extern __shared__ uint32_t sort_buffer[];
    __shared__ float4 entry_buffer[4 / ROWS][64 * 3];
    __shared__ uint8_t compact_table[STROKES ? 4 / ROWS : 1][STROKES ? 256 : 4]; // (lane, slot) codes of the samples a stroke triangle has to decide
    // msaa 4 (round 5): a lane's sixteen colour floats — read and written at COVER entries only — live in LDS between the covers (a private
    // 64-byte place per lane: no barrier, no bank conflict), so that the stroke fragment stages get the register file (the dashed scene's
    // kernel kept 124 bytes per lane in scratch memory, 30 frames' worth of scratch stores per launch)
    // (... of kColLdsSamples of its four samples: with all four a workgroup takes 33.7 KB of LDS at the usual sort capacity, four instead of
    // five fit a CU, and the kernel is slower than with its spills — 1.87 against 1.60 ms on the dashed scene; with two, 1.545: the kernel is
    // bound by the vector instructions of the dash evaluation, not by its scratch traffic)
    constexpr bool kColLds = S == 4;
    constexpr int kColLdsSamples = CRH_COL_LDS_SAMPLES;
    __shared__ float4 col_lds[kColLds ? 4 / ROWS : 1][kColLds ? ROWS * kColLdsSamples * 64 : 1];
    uint32_t tx, ty;
    if (!tile_of_place(r, bid, tx, ty)) return;
    const uint32_t tile = ty * r.tiles_x + tx;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* __restrict__ keys = sort_buffer + wave * r.sort_capacity;
    const uint32_t px = lane & 15u, rq = lane >> 4;
    const uint32_t first_row = 4u * ROWS * wave;
    const uint32_t gx = tx * kTile + px;
    const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile);
    const int tpx = (int)(tx * kTile), tpy = (int)(ty * kTile);
    float sx[S], sy0[S];
    if (S == 1) {
        sx[0] = (float)px + 0.5f;
        sy0[0] = (float)(first_row + rq) + 0.5f;
    } else {
        const float ox[4] = {0.375f, 0.875f, 0.125f, 0.625f}, oy[4] = {0.125f, 0.375f, 0.625f, 0.875f};
#pragma unroll
        for (int q = 0; q < S; ++q) {
            sx[q] = (float)px + ox[q & 3];
            sy0[q] = (float)(first_row + rq) + oy[q & 3];
        }
    }
    const uint32_t row_shift = first_row + rq; // triangles: bit row_shift + 4b of a 16-bit pixel-row mask

    // bit  bit_of(b, q)  of a 16-bit mask shifted right by edge_shift
    int winding[ROWS][S], hullw[ROWS][S];
    float col[ROWS][S][4];
#pragma unroll
    for (int b = 0; b < ROWS; ++b)
#pragma unroll
        for (int q = 0; q < S; ++q) {
            winding[b][q] = 0;
            hullw[b][q] = 0;
            col[b][q][0] = col[b][q][1] = col[b][q][2] = col[b][q][3] = 0.0f;
        }
    if (r.load_existing) {
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
            if (gx < r.width && gy < r.height) {
                const float4 d = load_px<XFMT>(r, gx, gy);
#pragma unroll
                for (int q = 0; q < S; ++q) col[b][q][0] = d.x, col[b][q][1] = d.y, col[b][q][2] = d.z, col[b][q][3] = d.w;
            }
        }
    }
    auto col_fetch = [&]() { // the lane's colours: LDS -> registers (in front of what blends or stores them)
        if constexpr (kColLds) {
#pragma unroll
            for (int b = 0; b < ROWS; ++b)
#pragma unroll
                for (int q = 0; q < kColLdsSamples; ++q) {
                    const float4 v = col_lds[threadIdx.x >> 6][(uint32_t)(b * kColLdsSamples + q) * 64u + (threadIdx.x & 63u)];
                    col[b][q][0] = v.x, col[b][q][1] = v.y, col[b][q][2] = v.z, col[b][q][3] = v.w;
                }
        }
    };
    auto col_keep = [&]() { // registers -> LDS (the registers are free again until the next cover)
        if constexpr (kColLds) {
#pragma unroll
            for (int b = 0; b < ROWS; ++b)
#pragma unroll
                for (int q = 0; q < kColLdsSamples; ++q) col_lds[threadIdx.x >> 6][(uint32_t)(b * kColLdsSamples + q) * 64u + (threadIdx.x & 63u)] = make_float4(col[b][q][0], col[b][q][1], col[b][q][2], col[b][q][3]);
        }
    };
    col_keep();
    constexpr uint32_t kLdsSortMax = kSortBytesMax / (4u * (4u / ROWS));
    uint32_t list_begin, n;
    tile_list_range(r, tile, kLdsSortMax, list_begin, n);
#ifdef CRH_ABLATE
    if (r.debug & 64u) n = 0;
    if ((r.debug & 524288u) && n > 64u) n = 0;   // only the lists that fit one chunk
    if ((r.debug & 1048576u) && n <= 64u) n = 0; // only the longer ones
#endif
    uint32_t my_key = 0xFFFFFFFFu;
    const bool sorted_in_place = n > kLdsSortMax;
    uint32_t* const segment = r.tile_list + list_begin;
    if (sorted_in_place) {
        sort_list_in_place(segment, n, threadIdx.x, 64u * (4u / ROWS));
    } else if (n <= 64u) {
        if (lane < n) my_key = r.tile_list[list_begin + lane];
        if (n > 1u) my_key = sort_keys_in_lanes(my_key, lane, n <= 8u ? 8u : (n <= 16u ? 16u : (n <= 32u ? 32u : 64u))); // a network as deep as the list needs (the keys sit in the leading lanes)
    } else {
        sort_list_in_lds(keys, segment, n, lane);
    }

    const uint8_t* slots = r.slots;
    const int wmask = (int)r.winding_mask;
    // Cooperative row evaluation of an edge entry: lane j < 16 evaluates the wave's sample row j (msaa 1: pixel row j; msaa 4: local
    // row j / 4, sample j % 4) at the left tile boundary, lane 16 the backdrop row q0 of the tile (k_bin_edges); one ballot per question.
    const uint32_t row_j = lane & 15u;
    const float ry_row = lane == 16u ? (S == 1 ? 0.5f : 0.125f)
                                     : (S == 1 ? (float)row_j + 0.5f : (float)(first_row + (row_j >> 2)) + ((float)(row_j & 3u) * 0.25f + 0.125f));
    const float sy_row = ty0 + ry_row;
    uint32_t walk_from = 0, verify_entry = 0xFFFFFFFFu; // absolute positions in the list
    constexpr bool kLongLateStart = LONG; // (a variant of its own: compiled into the kernel of the 10 000 path scene — few tiles beyond one chunk — it cost 8 %: 0.234 -> 0.255 ms)
    if (kLongLateStart && n > 64u && !r.load_existing) find_late_start(slots, segment, keys, sorted_in_place, n, lane, walk_from, verify_entry);
    uint32_t first_j = walk_from & 63u;
    bool again_from_the_top = false;
    for (uint32_t q0 = kLongLateStart ? walk_from & ~63u : 0u; q0 < n; q0 += 64u) {
        if (sorted_in_place)
            my_key = q0 + lane < n ? __hip_atomic_load(segment + q0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xFFFFFFFFu;
        else if (n > 64u)
            my_key = q0 + lane < n ? keys[q0 + lane] : 0xFFFFFFFFu;
        const uint32_t count = min(64u, n - q0);
        // ---- entry setup, vectorised across the chunk: lane j prepares entry j
        float4 e0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e1 = e0, e2 = e0;
        bool hull_over_tile = false, replaces_tile = false; // this lane's entry is a cover that resets every sample / an opaque cover over the whole tile
        uint32_t item_first = 0, item_synth_a = 0;
        if (lane < count) {
            const uint8_t* slot = slots + (size_t)my_key * 32u;
            const uint32_t flags = *reinterpret_cast<const uint32_t*>(slot);
            const uint32_t kind = (flags >> 4) & 15u;
            if (kind == EK_EDGE) {
                const EdgeRec er = *reinterpret_cast<const EdgeRec*>(slot);
                const float c = er.bx * (ty0 - er.lo_y) + er.nay * (tx0 - er.lo_x);
                const bool xr = er.lo_x <= tx0 && tx0 < er.hi_x; // the edge crosses the line of the left tile boundary
                e0 = make_float4(c, er.bx, er.nay, 0.0f);
                e1 = make_float4(fminf(er.lo_y, er.hi_y), fmaxf(er.lo_y, er.hi_y), 0.0f, __uint_as_float(flags | (xr ? 0x1000u : 0u)));
            } else if (kind == EK_SYNTH) {
                const SynthRec sr = *reinterpret_cast<const SynthRec*>(slot);
                e0 = make_float4(sr.r, sr.g, sr.b, sr.a);
                e1.w = __uint_as_float(flags);
                const uint32_t code_all = (flags >> 8) & 31u;
                hull_over_tile = code_all >= 4u + kCoverHull;
                replaces_tile = code_all >= 4u + kCoverOpaque;
                item_first = sr.first_slot, item_synth_a = sr.synth_a;
            } else {
                const PrimCoverage mine = *reinterpret_cast<const PrimCoverage*>(slot);
                const int bx0 = max((int)mine.box.x, tpx) - tpx, bx1 = min((int)mine.box.y, tpx + kTile - 1) - tpx;
                const int by0 = max((int)mine.box.z, tpy) - tpy, by1 = min((int)mine.box.w, tpy + kTile - 1) - tpy;
                const uint32_t col_bits = bx1 >= bx0 ? (2u << bx1) - (1u << bx0) : 0u, row_bits = by1 >= by0 ? (2u << by1) - (1u << by0) : 0u;
                float cc[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) cc[i] = mine.bx[i] * (ty0 - mine.lo_y[i]) + mine.nay[i] * (tx0 - mine.lo_x[i]);
                e0 = make_float4(cc[0], cc[1], cc[2], __uint_as_float(col_bits | (row_bits << 16)));
                e1 = make_float4(mine.bx[0], mine.bx[1], mine.bx[2], __uint_as_float(flags));
                e2 = make_float4(mine.nay[0], mine.nay[1], mine.nay[2], __uint_as_float(mine.desc));
            }
        }
        float4* __restrict__ entries = entry_buffer[wave];
        __builtin_amdgcn_wave_barrier();
        entries[lane * 3u + 0u] = e0;
        entries[lane * 3u + 1u] = e1;
        entries[lane * 3u + 2u] = e2;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#ifdef CRH_ABLATE
        if (r.debug & 128u) continue;
#endif
        // sample (b, q) of this lane inside a set-up triangle? (k_raster_tile's coverage: packed edge functions, box bits)
        auto coverage = [&](const float4& ea4, const float4& eb4, const float4& ec4, uint32_t flags, bool (&inside)[ROWS][S]) {
            const uint32_t bits = __float_as_uint(ea4.w);
            const float c0 = ea4.x, c1 = ea4.y, c2 = ea4.z, bx_0 = eb4.x, bx_1 = eb4.y, bx_2 = eb4.z, nay_0 = ec4.x, nay_1 = ec4.y, nay_2 = ec4.z;
            const uint32_t lane_rows = ((bits >> px) & 1u) ? (bits >> 16) >> row_shift : 0u;
            const int thr0 = 1 - (int)(flags & 1u), thr1 = 1 - (int)((flags >> 1) & 1u), thr2 = 1 - (int)((flags >> 2) & 1u);
            float ha[S], hb[S], hc[S];
#pragma unroll
            for (int q = 0; q < S; ++q) {
                ha[q] = fmaf(sx[q], nay_0, c0);
                hb[q] = fmaf(sx[q], nay_1, c1);
                hc[q] = fmaf(sx[q], nay_2, c2);
            }
#pragma unroll
            for (int cmb = 0; cmb < ROWS * S; cmb += 2) {
                const int b0 = cmb / S, k0 = cmb % S, b1 = (cmb + 1) / S, k1 = (cmb + 1) % S;
                const f32x2 y = {sy0[k0] + (float)(4 * b0), sy0[k1] + (float)(4 * b1)};
                const f32x2 ea = fma2(y, splat2(bx_0), f32x2{ha[k0], ha[k1]});
                const f32x2 eb = fma2(y, splat2(bx_1), f32x2{hb[k0], hb[k1]});
                const f32x2 ec = fma2(y, splat2(bx_2), f32x2{hc[k0], hc[k1]});
                inside[b0][k0] = (__float_as_int(ea[0]) >= thr0) & (__float_as_int(eb[0]) >= thr1) & (__float_as_int(ec[0]) >= thr2) & ((lane_rows & (1u << (4 * b0))) != 0u);
                inside[b1][k1] = (__float_as_int(ea[1]) >= thr0) & (__float_as_int(eb[1]) >= thr1) & (__float_as_int(ec[1]) >= thr2) & ((lane_rows & (1u << (4 * b1))) != 0u);
            }
        };
        // Two nested loops over the chunk's entries: the inner one runs over what only changes the winding counters (triangles, edges,
        // backdrops) and stops at a cover entry, which the outer loop body handles — the ONE place where the colour registers are
        // written. (With the colour updated inside a multi-way dispatch, every iteration ended with two dozen register copies.)
        // Occlusion. If the list holds an opaque cover over the whole tile (X, the last one; none of its item's triangles in the tile), what was
        // drawn before X only matters through the winding a sample may still carry when X tests it (an item whose hull boundary crosses the
        // tile can leave one just outside its hull). The winding is zero everywhere behind a cover that resets the whole tile (R, the last one
        // before X): the list is started behind R with cleared counters — exact for the winding; the colours it misses are all overwritten by
        // X unless some sample fails X's stencil test, and then (verify_at) the tile is done again from the top.
        uint32_t j = kLongLateStart ? first_j : 0u, verify_at = (kLongLateStart && verify_entry - q0 < 64u) ? verify_entry - q0 : 0xFFFFFFFFu; // (a list of several chunks: found above)
        first_j = 0;
        if (n <= 64u && !r.load_existing) { // (the whole list is in this chunk, and the tile starts from a known colour)
            unsigned long long candidates = __builtin_amdgcn_ballot_w64(replaces_tile);
            const unsigned long long resets = __builtin_amdgcn_ballot_w64(hull_over_tile);
            while (candidates) {
                const uint32_t at = 63u - (uint32_t)__builtin_clzll(candidates);
                const uint32_t first_slot = __builtin_amdgcn_readlane(item_first, at), synth_a = __builtin_amdgcn_readlane(item_synth_a, at);
                // the bin kernel vouched for the item's edges; its triangles are binned by another wavefront: one of them in this tile has a key
                // in [first_slot, synth_a), and keys ascend
                const uint32_t below = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(lane < count && my_key < synth_a));
                if (below == 0u || __builtin_amdgcn_readlane(my_key, below - 1u) < first_slot) {
                    const unsigned long long before = resets & ((1ull << at) - 1ull);
                    j = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u; // behind the last whole-tile reset before X
                    verify_at = j ? at : 0xFFFFFFFFu;
                    break;
                }
                candidates &= ~(1ull << at);
            }
        }
        while (j < count) {
        for (; j < count; ++j) {
            const uint32_t prim = __builtin_amdgcn_readlane(my_key, j);
            const float4 ea4 = entries[j * 3u + 0u], eb4 = entries[j * 3u + 1u], ec4 = entries[j * 3u + 2u];
            const uint32_t flags = __builtin_amdgcn_readfirstlane(__float_as_uint(eb4.w));
            const uint32_t kind = (flags >> 4) & 15u;
            if (kind == EK_COVER_TRI || (kind == EK_SYNTH && ((flags >> 8) & 31u) >= 4u)) break; // a cover: the outer loop's business
#ifdef CRH_ABLATE // tools/ablate_edges.sh: what does each class of entries cost?
            if ((r.debug & 256u) && lane == 0u) atomicAdd(&r.overflow[8 + (kind == EK_EDGE ? ((flags & kEdgeHull) ? 1 : 0) : (kind == EK_SYNTH ? 2 : 3))], 1u);
            if ((r.debug & 8u) && kind == EK_EDGE) continue;
            if ((r.debug & 16u) && kind == EK_SYNTH) continue;
            if ((r.debug & 32u) && kind != EK_EDGE && kind != EK_SYNTH) continue;
#endif
            // Every class updates the state it owns in place, unconditionally per sample (a select with the old value where nothing
            // changes): state that is modified under a wave-uniform inner branch, or merged behind the dispatch, costs the compiler a
            // dozen register copies per entry at the join.
            if (kind == EK_EDGE) {
                // w(p) += sigma * [ Y_k g(p) + A_k ],  A_k = xr (g(q_k) - g(q_0)) - Y_k g(q_k)   (see the header of this file)
                const float c0 = ea4.x, ebx = ea4.y, enay = ea4.z, ymin = eb4.x, ymax = eb4.y;
                const int thr = 1 - (int)(flags & kEdgeTl);
                // the 16 sample rows of the wave + q0, one row per lane: g at the left tile boundary and the half-open y range
                const float eq = fmaf(ry_row, ebx, fmaf(0.0f, enay, c0));
                const unsigned long long gq_all = __builtin_amdgcn_ballot_w64(__float_as_int(eq) >= thr);
                const unsigned long long y_all = __builtin_amdgcn_ballot_w64((ymin <= sy_row) & (sy_row < ymax));
                const uint32_t gq = (uint32_t)gq_all & 0xFFFFu, ym = (uint32_t)y_all & 0xFFFFu;
                const uint32_t g0 = ((uint32_t)gq_all >> 16) & 1u ? 0xFFFFu : 0u, xr = (flags & 0x1000u) ? 0xFFFFu : 0u;
                const uint32_t a_plus = xr & gq & ~g0 & ~ym;                      // A = +1
                const uint32_t a_minus = (xr & ~gq & g0) | (ym & gq & (~xr | g0)); // A = -1
                const int unit = (flags & kEdgeSigmaPos) ? 1 : -1;               // sigma
                if (ROWS == 1 && (ym | a_plus | a_minus) == 0u) continue;        // msaa 4: none of this wavefront's four pixel rows is in reach
                const SlotMasks ys = slot_masks<S>(ym);
                float h[S];
#pragma unroll
                for (int q = 0; q < S; ++q) h[q] = fmaf(sx[q], enay, c0);
                int d[ROWS][S];
#pragma unroll
                for (int cmb = 0; cmb < ROWS * S; cmb += 2) {
                    const int b0 = cmb / S, k0 = cmb % S, b1 = (cmb + 1) / S, k1 = (cmb + 1) % S;
                    const f32x2 y = {sy0[k0] + (float)(4 * b0), sy0[k1] + (float)(4 * b1)};
                    const f32x2 ev = fma2(y, splat2(ebx), f32x2{h[k0], h[k1]});
                    if constexpr (LONG) { // the y range per sample as a bit of ym on the VECTOR unit: this variant's counters say the scalar unit is the busier one (70 % against 63 %)
                        const uint32_t y_shift = S == 1 ? rq : 4u * rq;
                        d[b0][k0] = (__float_as_int(ev[0]) >= thr ? unit : 0) & __builtin_amdgcn_sbfe((int)ym, y_shift + (S == 1 ? 4u * b0 : (uint32_t)k0), 1u);
                        d[b1][k1] = (__float_as_int(ev[1]) >= thr ? unit : 0) & __builtin_amdgcn_sbfe((int)ym, y_shift + (S == 1 ? 4u * b1 : (uint32_t)k1), 1u);
                    } else {
                    d[b0][k0] = ((__float_as_int(ev[0]) >= thr) & __builtin_amdgcn_inverse_ballot_w64(ys.m[S == 1 ? b0 : k0])) ? unit : 0;
                    d[b1][k1] = ((__float_as_int(ev[1]) >= thr) & __builtin_amdgcn_inverse_ballot_w64(ys.m[S == 1 ? b1 : k1])) ? unit : 0;
                    }
                }
                if (a_plus | a_minus) { // the edge crosses the left tile boundary (or runs left of it): row constants (on the deltas, not on the state)
                    const uint32_t lane_shift = S == 1 ? rq : 4u * rq; // sample (b, q) of lane (px, rq) is row bit rq + 4b (msaa 1) / 4 rq + q (msaa 4)
                    const uint32_t psh = (unit > 0 ? a_plus : a_minus) >> lane_shift, nsh = (unit > 0 ? a_minus : a_plus) >> lane_shift;
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int q = 0; q < S; ++q) {
                            const int p = S == 1 ? 4 * b : q;
                            d[b][q] += (int)((psh >> p) & 1u) - (int)((nsh >> p) & 1u);
                        }
                }
                { // both sets of counters, each with its (scalar) share of the delta — one multiply-add per counter: a branch on the edge's
                  // kind around the additions left the compiler a dozen register copies per entry where the two sides meet
                    const int to_hull = (flags & kEdgeHull) ? 1 : 0, to_fill = 1 - to_hull;
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int q = 0; q < S; ++q) {
                            hullw[b][q] = __mul24(d[b][q], to_hull) + hullw[b][q];
                            winding[b][q] = __mul24(d[b][q], to_fill) + winding[b][q];
                        }
                }
            } else if (kind == EK_SYNTH) { // a whole-tile backdrop of the fill (codes 0, 1) or hull (2, 3) winding
                const uint32_t code = (flags >> 8) & 31u;
                const int vw = code < 2u ? ((code & 1u) ? -1 : 1) : 0, vh = code < 2u ? 0 : ((code & 1u) ? -1 : 1);
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        winding[b][q] += vw;
                        hullw[b][q] += vh;
                    }
            } else {
            // ---- curve and stroke triangles, as k_raster_tile
            if (ROWS == 1) { // msaa 4: this wavefront owns four of the tile's sixteen pixel rows — a sliver's box seldom reaches them all
                const uint32_t row_bits = __builtin_amdgcn_readfirstlane(__float_as_uint(ea4.w)) >> 16;
                if (((row_bits >> first_row) & 15u) == 0u) continue;
            }
            const PrimFragment frag = load_uniform(reinterpret_cast<const PrimFragment*>(slots + (size_t)prim * 32u + 64u));
            bool inside[ROWS][S];
            coverage(ea4, eb4, ec4, flags, inside);
            {
            const int delta = (flags & 8u) ? 1 : -1; // front (ccw on screen) increments, back decrements (renderer.rs:577-582)
            const float dx0 = tx0 - frag.v0x, dy0 = ty0 - frag.v0y;
            if (kind <= KIND_RC) { // the four implicit-curve tests (shaders.wgsl:236-266), one straight-line variant per kind
                auto curve = [&](auto kind_tag) {
                    constexpr uint32_t K = decltype(kind_tag)::value;
                    constexpr int NA = K == KIND_IQ ? 2 : (K == KIND_RC ? 4 : 3); // attributes the kind interpolates
                    float hx[NA][S]; // attribute planes, tile relative: the row-independent inner fma
#pragma unroll
                    for (int t = 0; t < NA; ++t) {
                        const float ac = fmaf(dy0, frag.gy[t], fmaf(dx0, frag.gx[t], frag.a0[t]));
#pragma unroll
                        for (int q = 0; q < S; ++q) hx[t][q] = fmaf(sx[q], frag.gx[t], ac);
                    }
#pragma unroll
                    for (int b = 0; b < ROWS; ++b) {
                        bool row_touched = false;
#pragma unroll
                        for (int q = 0; q < S; ++q) row_touched = row_touched | inside[b][q];
                        if (!__any(row_touched)) continue; // curve triangles are small: most rows of the tile are not touched
#pragma unroll
                        for (int q = 0; q < S; ++q) {
                            const float y = sy0[q] + (float)(4 * b);
                            float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                            for (int t = 0; t < NA; ++t) a[t] = fmaf(y, frag.gy[t], hx[t][q]);
                            const float lhs = (K == KIND_IQ || K == KIND_RQ) ? a[0] * a[0] : a[0] * a[0] * a[0];
                            const float rhs = K == KIND_IQ ? a[1] : (K == KIND_RC ? a[1] * a[2] * a[3] : a[1] * a[2]);
                            winding[b][q] += (inside[b][q] && lhs - rhs <= 0.0f) ? delta : 0;
                        }
                    }
                };
                if (kind == KIND_IQ)
                    curve(std::integral_constant<uint32_t, KIND_IQ>{});
                else if (kind == KIND_IC)
                    curve(std::integral_constant<uint32_t, KIND_IC>{});
                else if (kind == KIND_RQ)
                    curve(std::integral_constant<uint32_t, KIND_RQ>{});
                else
                    curve(std::integral_constant<uint32_t, KIND_RC>{});
            } else if (STROKES) { // KIND_LINE / KIND_JOINT: the stroke fragment stages (shaders.wgsl:268-300)
                // A stroke triangle is a sliver: a few percent of the wave's 256 samples are inside it, and what is decided per sample
                // (dash pattern walk, caps, the joint's atan2) is long and branchy. So the samples to decide — inside the triangle, stencil
                // still zero: Equal(0) -> IncrementWrap, both faces (renderer.rs:571-576) — are COMPACTED: their (lane, slot) codes go to
                // an LDS table in dense order, lane d decides the d-th of them, and the verdicts return through a ballot.
                unsigned long long cand[ROWS * S];
                uint32_t base[ROWS * S], total = 0;
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        cand[b * S + q] = __builtin_amdgcn_ballot_w64(inside[b][q] && (winding[b][q] & wmask) == 0);
                        base[b * S + q] = total;
                        total += (uint32_t)__popcll(cand[b * S + q]);
                    }
#ifdef CRH_ABLATE
                if (r.debug & 512u) total = 0u; // tools/ablate_edges.sh: the stroke triangles' coverage without their fragment stages
#endif
                if (total != 0u) {
                    uint8_t* const table = compact_table[wave];
                    uint32_t rank[ROWS * S];
                    __builtin_amdgcn_wave_barrier(); // the previous entry's readers of the table are through
#pragma unroll
                    for (int k = 0; k < ROWS * S; ++k) {
                        rank[k] = base[k] + __builtin_amdgcn_mbcnt_hi((uint32_t)(cand[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cand[k], 0u));
                        if ((cand[k] >> lane) & 1ull) table[rank[k]] = (uint8_t)(lane | ((uint32_t)k << 6));
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const crh_dynamic_stroke_descriptor dsc = load_uniform(&s.descriptors[__builtin_amdgcn_readfirstlane(__float_as_uint(ec4.w))]);
                    const uint32_t caps = dsc.caps, count_dashed_join = dsc.count_dashed_join;
                    const uint32_t flat_u = frag.flat_u;
                    const float end_y = frag.end_y;
                    const bool dashed = (count_dashed_join & 4u) != 0u;
                    float ac[3]; // the attribute planes, tile relative
#pragma unroll
                    for (int t = 0; t < 3; ++t) ac[t] = fmaf(dy0, frag.gy[t], fmaf(dx0, frag.gx[t], frag.a0[t]));
                    for (uint32_t first = 0; first < total; first += 64u) {
                        const uint32_t d = first + lane;
                        const bool live = d < total;
                        const uint32_t code = live ? table[d] : 0u;
                        const uint32_t src = code & 63u, slot = code >> 6; // whose sample: lane (px, rq), slot (b, q)
                        const uint32_t spx = src & 15u, srq = src >> 4;
                        float x, y; // exactly sx[q] and sy0[q] + 4 b of that lane
                        if (S == 1) {
                            x = (float)spx + 0.5f;
                            y = ((float)(first_row + srq) + 0.5f) + (float)(4u * slot);
                        } else {
                            const float ox = slot == 0u ? 0.375f : (slot == 1u ? 0.875f : (slot == 2u ? 0.125f : 0.625f));
                            const float oy = slot == 0u ? 0.125f : (slot == 1u ? 0.375f : (slot == 2u ? 0.625f : 0.875f));
                            x = (float)spx + ox;
                            y = (float)(first_row + srq) + oy;
                        }
                        const float a0 = fmaf(y, frag.gy[0], fmaf(x, frag.gx[0], ac[0])), a1 = fmaf(y, frag.gy[1], fmaf(x, frag.gx[1], ac[1]));
                        const float a2 = fmaf(y, frag.gy[2], fmaf(x, frag.gx[2], ac[2]));
                        bool fill = false;
                        if (live) {
                            if (kind == KIND_LINE) {
                                if (dashed)
                                    fill = stroke_dashed(dsc, a0, a1);
                                else if ((flat_u & 65536u) != 0u)
                                    fill = cap_test(a0, a1 - end_y, caps >> 4);
                                else if (a1 < 0.0f)
                                    fill = cap_test(a0, -a1, caps);
                                else
                                    fill = true;
                            } else {
                                const float radius = sqrtf(a0 * a0 + a1 * a1);
                                const uint32_t join = count_dashed_join & 3u;
                                fill = join == 1u ? (flat_u & 65536u) != 0u : (join == 2u ? radius <= 0.5f : true);
                                if (fill && dashed) fill = stroke_dashed_joint(dsc, radius, a0, a1, a2);
                            }
                        }
                        const unsigned long long filled = __builtin_amdgcn_ballot_w64(fill);
#pragma unroll
                        for (int b = 0; b < ROWS; ++b)
#pragma unroll
                            for (int q = 0; q < S; ++q) {
                                const uint32_t at = rank[b * S + q] - first; // < 64 iff this pass decided the sample
                                const bool mine = ((cand[b * S + q] >> lane) & 1ull) != 0ull && at < 64u;
                                winding[b][q] += (mine && ((filled >> (at & 63u)) & 1ull) != 0ull) ? 1 : 0;
                            }
                    }
                }
            }
            } // curve / stroke triangles
            } // triangles
        } // run of entries that only change the winding counters
        if (j >= count) break;
        {
            // ---- entry j is a cover: color_cover (renderer.rs:340-354, 736-754) — blend where the winding is not zero, zero the winding
            //      of the covered samples; premultiplied "over" (shaders.wgsl:304-309, blending of examples/showcase/main.rs:32-43)
            const uint32_t prim = __builtin_amdgcn_readlane(my_key, j);
            const float4 ea4 = entries[j * 3u + 0u], eb4 = entries[j * 3u + 1u], ec4 = entries[j * 3u + 2u];
            const uint32_t flags = __builtin_amdgcn_readfirstlane(__float_as_uint(eb4.w));
            const uint32_t kind = (flags >> 4) & 15u;
            ++j;
#ifdef CRH_ABLATE
            if ((r.debug & 256u) && lane == 0u) atomicAdd(&r.overflow[8 + (kind == EK_SYNTH ? 2 : 3)], 1u);
            if ((r.debug & 16u) && kind == EK_SYNTH) continue;
            if ((r.debug & 32u) && kind != EK_SYNTH) continue;
#endif
            bool blend[ROWS][S];
            float cs0, cs1, cs2, cs3;
            col_fetch();
            if (kind == EK_SYNTH) { // COVER over the samples inside the hull, one unit of both backdrops folded in
                const uint32_t code = 4u + (((flags >> 8) & 31u) - 4u) % 9u;
                const int bd = (int)((code - 4u) % 3u) - 1, hbd = (int)((code - 4u) / 3u) - 1;
                cs0 = ea4.x, cs1 = ea4.y, cs2 = ea4.z, cs3 = ea4.w;
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        const int w = winding[b][q] + bd;
                        const bool in_hull = hullw[b][q] + hbd != 0;
                        blend[b][q] = in_hull && (w & wmask) != 0;
                        winding[b][q] = in_hull ? 0 : w;
                        hullw[b][q] = 0;
                    }
                if (j - 1u == verify_at) { // X of the late start: does it overwrite every sample? (it does unless a sample inherited a winding)
                    bool every = true;
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int q = 0; q < S; ++q) every = every && blend[b][q];
                    verify_at = 0xFFFFFFFFu;
                    if (__builtin_amdgcn_ballot_w64(every) != ~0ull || (r.debug & 33554432u) != 0u) { // no (or debug bit 25, tests: never trusted): the colours behind it matter — the whole list, from cleared state
#pragma unroll
                        for (int b = 0; b < ROWS; ++b)
#pragma unroll
                            for (int q = 0; q < S; ++q) {
                                winding[b][q] = 0, hullw[b][q] = 0;
                                col[b][q][0] = col[b][q][1] = col[b][q][2] = col[b][q][3] = 0.0f;
                            }
                        col_keep();
                        j = 0;
                        if (kLongLateStart && n > 64u) { // the first chunk has to be set up again
                            verify_entry = 0xFFFFFFFFu;
                            again_from_the_top = true;
                            break;
                        }
                        continue;
                    }
                }
            } else { // a triangle of a folded hull strip, drawn as the reference draws it
                const PrimFragment frag = load_uniform(reinterpret_cast<const PrimFragment*>(slots + (size_t)prim * 32u + 64u));
                bool inside[ROWS][S];
                coverage(ea4, eb4, ec4, flags, inside);
                cs0 = frag.a0[0], cs1 = frag.a0[1], cs2 = frag.a0[2], cs3 = frag.a0[3];
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        blend[b][q] = inside[b][q] && (winding[b][q] & wmask) != 0;
                        winding[b][q] = inside[b][q] ? 0 : winding[b][q];
                    }
            }
            // an opaque source over finite colours: src + dst * (1 - 1) is the source (r.occlude: every colour of the pass is tame; a source
            // component that is -0 would come out as +0 through the arithmetic, so it takes the arithmetic): a select per channel, no multiply-add
            const bool replace = r.occlude != 0u && cs3 == 1.0f && __float_as_uint(cs0) != 0x80000000u && __float_as_uint(cs1) != 0x80000000u && __float_as_uint(cs2) != 0x80000000u;
            if (replace) {
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        col[b][q][0] = blend[b][q] ? cs0 : col[b][q][0];
                        col[b][q][1] = blend[b][q] ? cs1 : col[b][q][1];
                        col[b][q][2] = blend[b][q] ? cs2 : col[b][q][2];
                        col[b][q][3] = blend[b][q] ? cs3 : col[b][q][3];
                    }
            } else {
            const float one_minus_a = 1.0f - cs3;
#pragma unroll
            for (int b = 0; b < ROWS; ++b)
#pragma unroll
                for (int q = 0; q < S; ++q) { // unconditional, in place (a select with the old value where nothing blends)
                    const float n0 = cs0 + col[b][q][0] * one_minus_a, n1 = cs1 + col[b][q][1] * one_minus_a;
                    const float n2 = cs2 + col[b][q][2] * one_minus_a, n3 = cs3 + col[b][q][3] * one_minus_a;
                    col[b][q][0] = blend[b][q] ? n0 : col[b][q][0];
                    col[b][q][1] = blend[b][q] ? n1 : col[b][q][1];
                    col[b][q][2] = blend[b][q] ? n2 : col[b][q][2];
                    col[b][q][3] = blend[b][q] ? n3 : col[b][q][3];
                }
            }
            if (rounds_writes<XFMT>(r)) { // an Rgba8Unorm attachment keeps 8 bits of what the blender writes (idempotent on the others)
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int q = 0; q < S; ++q)
#pragma unroll
                        for (int ch = 0; ch < 4; ++ch) col[b][q][ch] = attachment<XFMT>(r, ch, col[b][q][ch]);
            }
            col_keep();
        }
        } // entries of the chunk
        if (kLongLateStart && again_from_the_top) { // (X of the late start did not overwrite every sample: the whole list, chunk 0 first)
            again_from_the_top = false;
            q0 = 0u - 64u;
        }
    }
    // ---- MSAA resolve (box average) + RGBA8 unorm store
    col_fetch();
#pragma unroll
    for (int b = 0; b < ROWS; ++b) {
        const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
        if (gx < r.width && gy < r.height) {
            const float inv = 1.0f / (float)S;
            float avg[4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                float sum = 0.0f;
#pragma unroll
                for (int q = 0; q < S; ++q) sum = sum + col[b][q][ch];
                avg[ch] = sum * inv;
            }
            store_px<XFMT>(r, gx, gy, avg[0], avg[1], avg[2], avg[3]);
        }
    }
}
// (A RESIDENT grid — as many workgroups as stay on the machine at four wavefronts per SIMD, each looping over the places bid, bid + gridDim.x, ...
// of a falling tile order, so that the next frame's binning and tessellation workgroups find room beside it — was measured in round 4: dealt
// statically, the tiles balance worse than under the hardware's dynamic dispatch (0.29 - 0.31 against 0.22 ms), the loop around the kernel
// body costs 5 - 12 % by itself, and the front lanes gain nothing. Not kept.)

// ---------------------------------------------------------------------------------------------- k_raster_fill (round 5)
// The per-sample kernel of fill scenes at msaa 1 (no stroke triangles), with the walk re-stated (renderer.rs:304-318, 340-354, 565-582;
// shaders.wgsl:233-266, 304-309; vertex.rs:28-35): what k_raster_edges<1, 4, false, *> draws, entry for entry and bit for bit, but
//   * CLASS-BATCHED: a chunk's sorted entries are cut into groups  N* C  (N: edges, backdrop units, curve triangles; C: one cover). Inside a
//     group the N entries only add integers to the winding counters, so they commute: one ballot per class for the whole chunk, then per
//     group a homogeneous loop per class over the class mask (scalar bit scans) — no per-entry read of the entry's flags through LDS into a
//     scalar register and no chain of uniform branches per entry (round 4's ablation priced that dispatch at 15 vector + 45 scalar
//     instructions per walked entry, half of the kernel's scalar work). A group's backdrop units are summed on the scalar unit (population
//     counts of their masks) and applied with one add per sample row.
//   * PACKED COUNTERS: a sample keeps  fill + 65536 * hull  in ONE register (k_raster_rows' cell; exact while a tile's list has fewer than
//     32 768 entries — every entry moves either counter by ONE at most: an edge's Y g(p) + A is -1, 0 or 1, a backdrop unit, a curve triangle's
//     accept bit and each of a COVER's two folded units are one —; the host keeps frames that have shown a list of 16 384 entries on k_raster_edges,
//     since a list in place may grow to c + c / 2 + 64 <= 24 638 entries unmeasured, tests/test_gpu_packed_cells.py). A fill
//     edge or a curve triangle adds its accept bit with ONE add-with-carry (the compare's lane mask is the carry), four registers less per lane.
//   * The sample rows an edge's y range or a triangle's box leaves out are folded into the compare as a sign bit (two cheap vector
//     instructions per row) instead of lane masks built on the scalar unit (fifteen scalar instructions per entry: by the measured issue
//     rates, tools/valu_rate.hip, a scalar instruction costs a SIMD as much as a compare); a triangle's three edge tests are one saturating
//     subtract each, a three-way minimum and ONE compare.
// LONG: as k_raster_edges (the late start found across the chunks of a long list).
CRH_D int add_lane_bit(int v, unsigned long long mask) { // v + (this lane's bit of mask): the mask is the carry-in (in place: no copy at a loop's back edge)
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long carry;
    asm("v_addc_co_u32 %0, %1, %0, 0, %2" : "+v"(v), "=s"(carry) : "s"(mask));
#endif
    return v;
}
CRH_D int sub_lane_bit(int v, unsigned long long mask) { // v - (this lane's bit of mask)
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long carry;
    asm("v_subb_co_u32 %0, %1, %0, 0, %2" : "+v"(v), "=s"(carry) : "s"(mask));
#endif
    return v;
}
// "over" on the lanes of mask[b] only (sample row b), the others keep their colour: the blends run under the masks as the EXEC mask — no
// select per channel —, dst = src + dst * (1 - alpha) as a multiply and an add (Rust does not contract), or dst = src for an opaque source.
// ONE asm statement for the four rows and for BOTH variants, the choice between them a uniform scalar branch inside it: the colour registers are
// updated in place. (Per row, the compiler moved them to temporaries and back. As one statement per variant under an if / else, the structurizer's
// flow block between the arms kept the sixteen colours alive beside the first arm's results: registers of their own for each arm, and copies where
// they meet — 36 moves a cover with the ones that followed from them.) Register operands only; EXEC is restored on both ways through.
CRH_D void blend_rows(float (&c)[4][4], const unsigned long long (&mask)[4], float s0, float s1, float s2, float s3, float one_minus_a, uint32_t replace) { // replace: 0 or 1, uniform
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long saved;
    const uint32_t variant = __builtin_amdgcn_readfirstlane(replace); // (a scalar register for the compare; the callers decide it on scalars, so this is no instruction)
    asm volatile("s_mov_b64 %[saved], exec\n\t"
                 "s_cmp_lg_u32 %[variant], 0\n\t"
                 "s_cbranch_scc1 .Lblend_replace_%=\n\t"
                 "s_mov_b64 exec, %[m0]\n\t"
                 "v_mul_f32 %[c00], %[c00], %[oma]\n\t"
                 "v_mul_f32 %[c01], %[c01], %[oma]\n\t"
                 "v_mul_f32 %[c02], %[c02], %[oma]\n\t"
                 "v_mul_f32 %[c03], %[c03], %[oma]\n\t"
                 "v_add_f32 %[c00], %[s0], %[c00]\n\t"
                 "v_add_f32 %[c01], %[s1], %[c01]\n\t"
                 "v_add_f32 %[c02], %[s2], %[c02]\n\t"
                 "v_add_f32 %[c03], %[s3], %[c03]\n\t"
                 "s_mov_b64 exec, %[m1]\n\t"
                 "v_mul_f32 %[c10], %[c10], %[oma]\n\t"
                 "v_mul_f32 %[c11], %[c11], %[oma]\n\t"
                 "v_mul_f32 %[c12], %[c12], %[oma]\n\t"
                 "v_mul_f32 %[c13], %[c13], %[oma]\n\t"
                 "v_add_f32 %[c10], %[s0], %[c10]\n\t"
                 "v_add_f32 %[c11], %[s1], %[c11]\n\t"
                 "v_add_f32 %[c12], %[s2], %[c12]\n\t"
                 "v_add_f32 %[c13], %[s3], %[c13]\n\t"
                 "s_mov_b64 exec, %[m2]\n\t"
                 "v_mul_f32 %[c20], %[c20], %[oma]\n\t"
                 "v_mul_f32 %[c21], %[c21], %[oma]\n\t"
                 "v_mul_f32 %[c22], %[c22], %[oma]\n\t"
                 "v_mul_f32 %[c23], %[c23], %[oma]\n\t"
                 "v_add_f32 %[c20], %[s0], %[c20]\n\t"
                 "v_add_f32 %[c21], %[s1], %[c21]\n\t"
                 "v_add_f32 %[c22], %[s2], %[c22]\n\t"
                 "v_add_f32 %[c23], %[s3], %[c23]\n\t"
                 "s_mov_b64 exec, %[m3]\n\t"
                 "v_mul_f32 %[c30], %[c30], %[oma]\n\t"
                 "v_mul_f32 %[c31], %[c31], %[oma]\n\t"
                 "v_mul_f32 %[c32], %[c32], %[oma]\n\t"
                 "v_mul_f32 %[c33], %[c33], %[oma]\n\t"
                 "v_add_f32 %[c30], %[s0], %[c30]\n\t"
                 "v_add_f32 %[c31], %[s1], %[c31]\n\t"
                 "v_add_f32 %[c32], %[s2], %[c32]\n\t"
                 "v_add_f32 %[c33], %[s3], %[c33]\n\t"
                 "s_branch .Lblend_done_%=\n"
                 ".Lblend_replace_%=:\n\t"
                 "s_mov_b64 exec, %[m0]\n\t"
                 "v_mov_b32 %[c00], %[s0]\n\t"
                 "v_mov_b32 %[c01], %[s1]\n\t"
                 "v_mov_b32 %[c02], %[s2]\n\t"
                 "v_mov_b32 %[c03], %[s3]\n\t"
                 "s_mov_b64 exec, %[m1]\n\t"
                 "v_mov_b32 %[c10], %[s0]\n\t"
                 "v_mov_b32 %[c11], %[s1]\n\t"
                 "v_mov_b32 %[c12], %[s2]\n\t"
                 "v_mov_b32 %[c13], %[s3]\n\t"
                 "s_mov_b64 exec, %[m2]\n\t"
                 "v_mov_b32 %[c20], %[s0]\n\t"
                 "v_mov_b32 %[c21], %[s1]\n\t"
                 "v_mov_b32 %[c22], %[s2]\n\t"
                 "v_mov_b32 %[c23], %[s3]\n\t"
                 "s_mov_b64 exec, %[m3]\n\t"
                 "v_mov_b32 %[c30], %[s0]\n\t"
                 "v_mov_b32 %[c31], %[s1]\n\t"
                 "v_mov_b32 %[c32], %[s2]\n\t"
                 "v_mov_b32 %[c33], %[s3]\n"
                 ".Lblend_done_%=:\n\t"
                 "s_mov_b64 exec, %[saved]"
                 : [c00] "+v"(c[0][0]), [c01] "+v"(c[0][1]), [c02] "+v"(c[0][2]), [c03] "+v"(c[0][3]), [c10] "+v"(c[1][0]), [c11] "+v"(c[1][1]), [c12] "+v"(c[1][2]), [c13] "+v"(c[1][3]), [c20] "+v"(c[2][0]), [c21] "+v"(c[2][1]), [c22] "+v"(c[2][2]), [c23] "+v"(c[2][3]), [c30] "+v"(c[3][0]), [c31] "+v"(c[3][1]), [c32] "+v"(c[3][2]), [c33] "+v"(c[3][3]), [saved] "=&s"(saved)
                 : [m0] "s"(mask[0]), [m1] "s"(mask[1]), [m2] "s"(mask[2]), [m3] "s"(mask[3]), [s0] "v"(s0), [s1] "v"(s1), [s2] "v"(s2), [s3] "v"(s3), [oma] "v"(one_minus_a), [variant] "s"(variant)
                 : "scc");
#else
    (void)c, (void)mask, (void)s0, (void)s1, (void)s2, (void)s3, (void)one_minus_a, (void)replace;
#endif
}
// bit `bit` of `rows` clear -> the sign bit set in x (a sample row that is left out fails every  x >= 0 / x >= 1  test): v_lshlrev_b32 + v_and_or_b32
CRH_D int reject_unless_row(int x, uint32_t not_rows, int bit) { return (int)(((not_rows << (31 - bit)) & 0x80000000u) | (uint32_t)x); }
// WAVES: wavefronts per SIMD the build is held to. Round 6: SEVEN (72 registers, no scratch memory), for every frame. Until then the kernel was built twice —
// five waves (91 registers, no scratch) and, for frames of long lists, six (80 registers, 20 B of scratch: a pair of scratch stores per wavefront, as many
// bytes as the tile it draws) — because LLVM's SLP vectorizer kept the lane-invariant operands of its v_pk_* instructions duplicated in register pairs for
// the whole kernel. Without that pass (build.py FILE_FLAGS) the kernel needs 76 registers at any occupancy, 72 when held to seven waves, and spills from
// eight on (64 registers, 12 B). Same box, S10k @ 4096^2 / 100 000 paths @ 8192^2, raster kernel alone and pipelined step in ms (profiles/r06_experiments.txt):
//   round 5 (SLP, 5 / 6 waves)  0.166, 0.302 / 1.008, 1.950      no SLP, held to 5 or 6   0.150, 0.298 - 0.306 / 0.977, 1.93 - 1.95
//   no SLP, held to 7           0.142, 0.289 - 0.293 / 0.920, 1.877                      held to 8 (spills)       0.142, 0.299 / 0.976, 1.956
#ifndef CRH_FILL_TILE_WAVES
#define CRH_FILL_TILE_WAVES 7
#endif
template <bool LONG, int WAVES = CRH_FILL_TILE_WAVES, bool XFMT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES))) void k_raster_fill(SceneDev s, RasterParams r) {
    constexpr int ROWS = 4;
    const uint32_t bid = blockIdx.x; // the workgroup's place in the frame's tile order
    extern __shared__ uint32_t sort_buffer[];
    __shared__ float4 entry_buffer[64 * 3];
    uint32_t tx, ty;
    if (!tile_of_place(r, bid, tx, ty)) return;
    const uint32_t tile = ty * r.tiles_x + tx;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* __restrict__ keys = sort_buffer;
    const uint32_t px = lane & 15u, rq = lane >> 4;
    const uint32_t gx = tx * kTile + px;
    const float tile_y0 = (float)(ty * kTile); // (the walk derives the tile's origin again per chunk, below)
    const int tpx = (int)(tx * kTile), tpy = (int)(ty * kTile);
    const float sx = (float)px + 0.5f, sy0 = (float)rq + 0.5f; // the lane's samples: column px, rows rq + 4 b
    int cell[ROWS];        // fill winding + 65536 * hull winding of sample row rq + 4 b
    float col[ROWS][4];
#pragma unroll
    for (int b = 0; b < ROWS; ++b) {
        cell[b] = 0;
        col[b][0] = col[b][1] = col[b][2] = col[b][3] = 0.0f;
    }
    if (r.load_existing) {
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + 4u * b + rq;
            if (gx < r.width && gy < r.height) {
                const float4 d = load_px<XFMT>(r, gx, gy);
                col[b][0] = d.x, col[b][1] = d.y, col[b][2] = d.z, col[b][3] = d.w;
            }
        }
    }
    constexpr uint32_t kLdsSortMax = kSortBytesMax / 4u;
    uint32_t list_begin, n;
    tile_list_range(r, tile, kLdsSortMax, list_begin, n);
#ifdef CRH_ABLATE
    if (r.debug & 64u) n = 0;
#endif
    uint32_t my_key = 0xFFFFFFFFu;
    const bool sorted_in_place = n > kLdsSortMax;
    uint32_t* const segment = r.tile_list + list_begin;
    if (sorted_in_place) {
        sort_list_in_place(segment, n, lane, 64u);
    } else if (n <= 64u) {
        if (lane < n) my_key = r.tile_list[list_begin + lane];
        if (n > 1u) my_key = sort_keys_in_lanes(my_key, lane, n <= 8u ? 8u : (n <= 16u ? 16u : (n <= 32u ? 32u : 64u))); // a network as deep as the list needs (the keys sit in the leading lanes)
    } else {
        sort_list_in_lds(keys, segment, n, lane);
    }

    const uint8_t* slots = r.slots;
    const uint32_t wmask = r.winding_mask;
    // Cooperative row evaluation of an edge entry: lane j < 16 evaluates sample row j at the left tile boundary, lane 16 the backdrop row q0
    const uint32_t row_j = lane & 15u;
    const float ry_row = lane == 16u ? 0.5f : (float)row_j + 0.5f;
    const float sy_row = tile_y0 + ry_row;
    uint32_t walk_from = 0, verify_entry = 0xFFFFFFFFu; // absolute positions in the list
    if (LONG && n > 64u && !r.load_existing) find_late_start(slots, segment, keys, sorted_in_place, n, lane, walk_from, verify_entry);
    uint32_t first_j = walk_from & 63u;
    bool again_from_the_top = false;
    for (uint32_t q0 = LONG ? walk_from & ~63u : 0u; q0 < n; q0 += 64u) {
        // The tile's origin as floats, derived from the scalar tile coordinates HERE, per chunk: as values of the whole kernel the compiler kept
        // them duplicated in vector register pairs (operands of packed adds) and, in the six-wave build, spilled those — 16 bytes per lane, one
        // pair of scratch stores per wavefront: as many bytes as the tile it draws (WRITE_SIZE 1.95 x the frame at 8192^2).
        uint32_t tx_here = tx, ty_here = ty;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(tx_here), "+s"(ty_here));
#endif
        const float tx0 = (float)(tx_here * kTile), ty0 = (float)(ty_here * kTile);
        // (loads at a clamped index and a select, not a load under a lane-dependent condition: the loop has no divergent branch, see the set-up)
        if (sorted_in_place) {
            const uint32_t k_at = __hip_atomic_load(segment + min(q0 + lane, n - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            my_key = q0 + lane < n ? k_at : 0xFFFFFFFFu;
        } else if (n > 64u) {
            const uint32_t k_at = keys[min(q0 + lane, n - 1u)];
            my_key = q0 + lane < n ? k_at : 0xFFFFFFFFu;
        }
        const uint32_t count = min(64u, n - q0);
        // ---- entry set-up, vectorised across the chunk: lane j prepares entry j (the records of k_raster_edges) and says what class it is.
        // WITHOUT a divergent branch: the three kinds of record are all decoded from the same 64 bytes and the results selected (the paths of
        // a three-way branch run one after the other anyway when a chunk holds all kinds). With it, this loop is a region of uniform branches
        // only, which the compiler leaves as written — behind ONE divergent branch it linearised the whole walk into guarded blocks with a
        // dozen register copies per entry where they meet.
        const uint32_t first_key = __builtin_amdgcn_readfirstlane(my_key);
        const uint32_t safe_key = lane < count ? my_key : first_key; // (a slot that exists: entry 0's)
        const uint4* slot16 = reinterpret_cast<const uint4*>(slots + (size_t)safe_key * 32u);
        const uint4 w0 = slot16[0], w1 = slot16[1];
        const uint32_t flags = w0.x, kind = (flags >> 4) & 15u;
        const bool is_edge = kind == EK_EDGE, is_synth = kind == EK_SYNTH;
        const uint4* tail16 = slot16 + ((is_edge || is_synth) ? 0 : 2); // the second half of a triangle's coverage record (the others read their own line again)
        const uint4 w2 = tail16[0], w3 = tail16[1];
        auto f = [](uint32_t v) { return __uint_as_float(v); };
        // a boundary edge (EdgeRec: flags, -, lo_x, lo_y | hi_x, hi_y, bx, nay)
        const float e_c = f(w1.z) * (ty0 - f(w0.w)) + f(w1.w) * (tx0 - f(w0.z));
        const bool xr = f(w0.z) <= tx0 && tx0 < f(w1.x); // the edge crosses the line of the left tile boundary
        const float e_ymin = fminf(f(w0.w), f(w1.y)), e_ymax = fmaxf(f(w0.w), f(w1.y));
        // a backdrop unit or a COVER (SynthRec: flags, first_slot, r, g | b, a, synth_a, -); a COVER's two folded backdrop units decoded here, once:
        // (code - 4) % 9 = bd + 1 + 3 (hbd + 1) -> eflags bits 16-17 and 18-19
        // (... with multiplications: a division the compiler would put behind a lane-dependent branch; exact for these small operands)
        const uint32_t code_p5 = ((flags >> 8) & 31u) + 5u, code9 = code_p5 - 9u * ((code_p5 * 57u) >> 9); // (code + 5) % 9, code + 5 <= 36
        const uint32_t code9_div3 = (code9 * 11u) >> 5, code9_mod3 = code9 - 3u * code9_div3;               // code9 <= 8
        // a curve triangle (PrimCoverage: flags, desc, box | lo_x[3], lo_y[3], bx[3], nay[3])
        const int px0 = (int)(w0.z & 0xFFFFu), px1 = (int)(w0.z >> 16), py0 = (int)(w0.w & 0xFFFFu), py1 = (int)(w0.w >> 16);
        const int bx0 = max(px0, tpx) - tpx, bx1 = min(px1, tpx + kTile - 1) - tpx;
        const int by0 = max(py0, tpy) - tpy, by1 = min(py1, tpy + kTile - 1) - tpy;
        const uint32_t col_bits = bx1 >= bx0 ? (2u << bx1) - (1u << bx0) : 0u, row_bits = by1 >= by0 ? (2u << by1) - (1u << by0) : 0u;
        const float cc0 = f(w2.z) * (ty0 - f(w1.w)) + f(w3.y) * (tx0 - f(w1.x));
        const float cc1 = f(w2.w) * (ty0 - f(w2.x)) + f(w3.z) * (tx0 - f(w1.y));
        const float cc2 = f(w3.x) * (ty0 - f(w2.y)) + f(w3.w) * (tx0 - f(w1.z));
        const float4 e0 = make_float4(is_edge ? e_c : (is_synth ? f(w0.z) : cc0), is_edge ? f(w1.z) : (is_synth ? f(w0.w) : cc1), is_edge ? f(w1.w) : (is_synth ? f(w1.x) : cc2),
                                      is_synth ? f(w1.y) : f(col_bits | (row_bits << 16)));
        const float4 e1 = make_float4(is_edge ? e_ymin : f(w2.z), is_edge ? e_ymax : f(w2.w), f(w3.x), 0.0f);
        const float4 e2 = make_float4(f(w3.y), f(w3.z), f(w3.w), 0.0f);
        // (bit 20: an opaque source none of whose components is -0 — `replace` below —, decided here so that the walk's branch on it is on a scalar)
        const bool opaque_source = f(w1.y) == 1.0f && w0.z != 0x80000000u && w0.w != 0x80000000u && w1.x != 0x80000000u;
        const uint32_t eflags = lane < count ? flags | (is_edge ? (xr ? 0x1000u : 0u) : (is_synth ? (code9_mod3 << 16) | (code9_div3 << 18) | (opaque_source ? 1u << 20 : 0u) : 0u)) : 15u << 4; // (no entry: no class)
        const uint32_t item_first = w0.y, item_synth_a = w1.z; // (read at COVER entries only)
        float4* __restrict__ entries = entry_buffer;
        __builtin_amdgcn_wave_barrier();
        entries[lane * 3u + 0u] = e0;
        entries[lane * 3u + 1u] = e1;
        entries[lane * 3u + 2u] = e2;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // ---- the chunk's classes, one ballot each
        const uint32_t ekind = (eflags >> 4) & 15u, ecode = (eflags >> 8) & 31u;
        const bool synth = ekind == EK_SYNTH;
        const unsigned long long m_cover = __builtin_amdgcn_ballot_w64(ekind == EK_COVER_TRI || (synth && ecode >= 4u));
        const unsigned long long m_edge = __builtin_amdgcn_ballot_w64(ekind == EK_EDGE);
        const unsigned long long m_tri = __builtin_amdgcn_ballot_w64(ekind >= KIND_IQ && ekind <= KIND_RC);
        const unsigned long long m_units = __builtin_amdgcn_ballot_w64(synth && ecode < 4u);       // backdrop units: fill +1 / -1 (codes 0, 1), hull +1 / -1 (2, 3)
        const unsigned long long m_odd = __builtin_amdgcn_ballot_w64(synth && (ecode & 1u) != 0u); // ... the -1 ones
        const unsigned long long m_hullu = __builtin_amdgcn_ballot_w64(synth && (ecode & 2u) != 0u); // ... the hull's
#ifdef CRH_ABLATE
        if (r.debug & 128u) continue;
#endif
        // sample row b of this lane inside a set-up triangle? (k_raster_tile's coverage — E_i = fma(y, bx_i, fma(x, nay_i, c_i)) accepted as
        // an integer >= 1 - top_left_i — as the lane mask of the samples inside: a saturating subtract per edge, a three-way minimum, the box
        // rows folded in as a sign bit, ONE compare)
        struct TriCoverage {
            float ha, hb, hc, bxa, bxb, bxc;
            int thr0, thr1, thr2;
            uint32_t not_rows; // bit 4 b clear: the lane's sample row b is inside the triangle's pixel box
        };
        auto tri_coverage = [&](const float4& ea4, const float4& eb4, const float4& ec4, uint32_t flags) {
            const uint32_t bits = __float_as_uint(ea4.w);
            TriCoverage t;
            t.not_rows = ((bits >> px) & 1u) ? ~((bits >> 16) >> rq) : ~0u;
            t.thr0 = 1 - (int)(flags & 1u), t.thr1 = 1 - (int)((flags >> 1) & 1u), t.thr2 = 1 - (int)((flags >> 2) & 1u);
            t.ha = fmaf(sx, ec4.x, ea4.x), t.hb = fmaf(sx, ec4.y, ea4.y), t.hc = fmaf(sx, ec4.z, ea4.z);
            t.bxa = eb4.x, t.bxb = eb4.y, t.bxc = eb4.z;
            return t;
        };
        auto inside_row = [&](const TriCoverage& t, int b) -> unsigned long long {
            const float y = sy0 + (float)(4 * b);
            const int xa = __builtin_elementwise_sub_sat(__float_as_int(fmaf(y, t.bxa, t.ha)), t.thr0);
            const int xb = __builtin_elementwise_sub_sat(__float_as_int(fmaf(y, t.bxb, t.hb)), t.thr1);
            const int xc = __builtin_elementwise_sub_sat(__float_as_int(fmaf(y, t.bxc, t.hc)), t.thr2);
            return __builtin_amdgcn_ballot_w64(reject_unless_row(min(xa, min(xb, xc)), t.not_rows, 4 * b) >= 0);
        };
        // Occlusion (k_raster_edges): X = the last opaque cover over the whole tile none of whose item's triangles are in the list; the walk starts
        // behind R, the last whole-tile reset in front of it, and X verifies that it overwrites every sample.
        uint32_t j0 = LONG ? first_j : 0u, verify_at = (LONG && verify_entry - q0 < 64u) ? verify_entry - q0 : 0xFFFFFFFFu;
        first_j = 0;
        if (n <= 64u && !r.load_existing) { // (the whole list is in this chunk, and the tile starts from a known colour)
            unsigned long long candidates = __builtin_amdgcn_ballot_w64(synth && ecode >= 4u + kCoverOpaque);
            const unsigned long long resets = __builtin_amdgcn_ballot_w64(synth && ecode >= 4u + kCoverHull);
            while (candidates) {
                const uint32_t at = 63u - (uint32_t)__builtin_clzll(candidates);
                const uint32_t first_slot = __builtin_amdgcn_readlane(item_first, at), synth_a = __builtin_amdgcn_readlane(item_synth_a, at);
                const uint32_t below = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(lane < count && my_key < synth_a));
                if (below == 0u || __builtin_amdgcn_readlane(my_key, below - 1u) < first_slot) {
                    const unsigned long long before = resets & ((1ull << at) - 1ull);
                    j0 = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u; // behind the last whole-tile reset before X
                    verify_at = j0 ? at : 0xFFFFFFFFu;
                    break;
                }
                candidates &= ~(1ull << at);
            }
        }
        const unsigned long long all = count >= 64u ? ~0ull : (1ull << count) - 1ull;
        unsigned long long rest = j0 >= 64u ? 0ull : all & (~0ull << j0);
        while (rest) {
            const unsigned long long covers = m_cover & rest;
            const uint32_t end = covers ? (uint32_t)__builtin_ctzll(covers) : 64u;
            const unsigned long long group = end >= 64u ? rest : rest & ((1ull << end) - 1ull); // the N entries in front of the next cover
            // ---- backdrop units of the group: summed on the scalar unit
            const unsigned long long units = group & m_units;
            if (units) {
                const int fill_units = (int)__popcll(units & ~m_hullu & ~m_odd) - (int)__popcll(units & ~m_hullu & m_odd);
                const int hull_units = (int)__popcll(units & m_hullu & ~m_odd) - (int)__popcll(units & m_hullu & m_odd);
                int add = fill_units + hull_units * 65536;
#ifdef CRH_ABLATE
                if (r.debug & 16u) add = 0;
#endif
#pragma unroll
                for (int b = 0; b < ROWS; ++b) cell[b] += add;
            }
            // ---- boundary edges:  w(p) += sigma * [ Y_k g(p) + A_k ],  A_k = xr (g(q_k) - g(q_0)) - Y_k g(q_k)   (see the header of this file)
            unsigned long long edges = group & m_edge;
#ifdef CRH_ABLATE
            if (r.debug & 8u) edges = 0ull;
#endif
            while (edges) {
                const uint32_t j = (uint32_t)__builtin_ctzll(edges);
                edges &= edges - 1ull;
                const float4 ea4 = entries[j * 3u + 0u];
                const float2 yr = *reinterpret_cast<const float2*>(&entries[j * 3u + 1u]);
                const uint32_t flags = __builtin_amdgcn_readlane(eflags, j);
                const float c0 = ea4.x, ebx = ea4.y, enay = ea4.z, ymin = yr.x, ymax = yr.y;
                const int thr = 1 - (int)(flags & kEdgeTl);
                // the 16 sample rows + q0, one row per lane: g at the left tile boundary and the half-open y range
                const float eq = fmaf(ry_row, ebx, fmaf(0.0f, enay, c0));
                const unsigned long long gq_all = __builtin_amdgcn_ballot_w64(__float_as_int(eq) >= thr);
                const unsigned long long y_all = __builtin_amdgcn_ballot_w64(ymin <= sy_row) & __builtin_amdgcn_ballot_w64(sy_row < ymax);
                const uint32_t gq = (uint32_t)gq_all & 0xFFFFu, ym = (uint32_t)y_all & 0xFFFFu;
                const bool g0 = (((uint32_t)gq_all >> 16) & 1u) != 0u, xr = (flags & 0x1000u) != 0u;
                // A_k = xr (g(q_k) - g(q_0)) - Y_k g(q_k), three cases:  !xr: -(ym & gq);  xr & !g0: +(gq & ~ym);  xr & g0: -(~gq | ym)
                const uint32_t ygq = ym & gq;
                const uint32_t a_plus = (xr && !g0) ? gq ^ ygq : 0u;
                const uint32_t a_minus = xr ? (g0 ? (gq ^ 0xFFFFu) | ym : 0u) : ygq;
                const bool positive = (flags & kEdgeSigmaPos) != 0u; // sigma
                const int weight = (flags & kEdgeHull) ? 65536 : 1;  // the half of the cell the edge's chain belongs to
                const int unit = positive ? weight : -weight;
                const float h = fmaf(sx, enay, c0);
                const f32x2 y01 = {sy0, sy0 + 4.0f}, y23 = {sy0 + 8.0f, sy0 + 12.0f};
                const f32x2 ev01 = fma2(y01, splat2(ebx), f32x2{h, h}), ev23 = fma2(y23, splat2(ebx), f32x2{h, h});
                // Straight-line code from here (an if / else per property of the edge — hull or fill, sigma, "spans all rows" — came back from the
                // compiler as guarded blocks with the four counters copied at every join): the lanes whose sample row b takes the edge's unit,
                // Y_k g(p), with the rows outside the y range failing the compare through their sign bit
                const uint32_t not_ym = ~ym >> rq; // bit 4 b clear: the lane's sample row b is inside the edge's y range
                cell[0] += (reject_unless_row(__float_as_int(ev01[0]), not_ym, 0) >= thr) ? unit : 0;
                cell[1] += (reject_unless_row(__float_as_int(ev01[1]), not_ym, 4) >= thr) ? unit : 0;
                cell[2] += (reject_unless_row(__float_as_int(ev23[0]), not_ym, 8) >= thr) ? unit : 0;
                cell[3] += (reject_unless_row(__float_as_int(ev23[1]), not_ym, 12) >= thr) ? unit : 0;
                if (a_plus | a_minus) { // the edge crosses the left tile boundary (or runs left of it): row constants A_k sigma. Two bits per row —
                                        // 01: +1, 11: -1 — in one scalar word; the lane shifts its rows down and takes signed two-bit fields
                    const uint32_t up = positive ? a_plus : a_minus, down = positive ? a_minus : a_plus;
                    const int consts = (int)((((uint32_t)bit_double(up) & 0x55555555u) | (uint32_t)bit_double(down)) >> (2u * rq));
#pragma unroll
                    for (int b = 0; b < ROWS; ++b) cell[b] = __mul24(__builtin_amdgcn_sbfe(consts, 8u * b, 2u), weight) + cell[b];
                }
            }
            // ---- curve triangles: the four implicit-curve tests (shaders.wgsl:236-266), one straight-line variant per kind
            unsigned long long tris = group & m_tri;
#ifdef CRH_ABLATE
            if (r.debug & 32u) tris = 0ull;
#endif
            while (tris) {
                const uint32_t j = (uint32_t)__builtin_ctzll(tris);
                tris &= tris - 1ull;
                const uint32_t prim = __builtin_amdgcn_readlane(my_key, j);
                const uint32_t flags = __builtin_amdgcn_readlane(eflags, j);
                const PrimFragment frag = load_uniform(reinterpret_cast<const PrimFragment*>(slots + (size_t)prim * 32u + 64u));
                const float4 ea4 = entries[j * 3u + 0u], eb4 = entries[j * 3u + 1u], ec4 = entries[j * 3u + 2u];
                const uint32_t kind = (flags >> 4) & 15u;
                const TriCoverage cov = tri_coverage(ea4, eb4, ec4, flags);
                const int back = (flags & 8u) ? 0 : -1; // front (ccw on screen) increments, back decrements (renderer.rs:577-582)
                const uint32_t box_rows = __builtin_amdgcn_readfirstlane(__float_as_uint(ea4.w)) >> 16;
                const float dx0 = tx0 - frag.v0x, dy0 = ty0 - frag.v0y;
                auto curve = [&](auto kind_tag) {
                    constexpr uint32_t K = decltype(kind_tag)::value;
                    constexpr int NA = K == KIND_IQ ? 2 : (K == KIND_RC ? 4 : 3); // attributes the kind interpolates
                    float hx[NA]; // attribute planes, tile relative: the row-independent inner fma
#pragma unroll
                    for (int t = 0; t < NA; ++t) hx[t] = fmaf(sx, frag.gx[t], fmaf(dy0, frag.gy[t], fmaf(dx0, frag.gx[t], frag.a0[t])));
#pragma unroll
                    for (int b = 0; b < ROWS; ++b) {
                        if (((box_rows >> (4 * b)) & 15u) == 0u) continue; // none of the four sample rows 4 b .. 4 b + 3 is in the triangle's box
                        const unsigned long long inside = inside_row(cov, b);
                        if (inside == 0ull) continue; // curve triangles are small: most rows of the tile are not touched
                        const float y = sy0 + (float)(4 * b);
                        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                        for (int t = 0; t < NA; ++t) a[t] = fmaf(y, frag.gy[t], hx[t]);
                        const float lhs = (K == KIND_IQ || K == KIND_RQ) ? a[0] * a[0] : a[0] * a[0] * a[0];
                        const float rhs = K == KIND_IQ ? a[1] : (K == KIND_RC ? a[1] * a[2] * a[3] : a[1] * a[2]);
                        const unsigned long long filled = inside & __builtin_amdgcn_ballot_w64(lhs - rhs <= 0.0f);
                        cell[b] = add_lane_bit(cell[b] ^ back, filled) ^ back; // ~(~c + bit) = c - bit
                    }
                };
                // Four ifs side by side, not an if / else chain, and each on a copy of `kind` the compiler cannot see through (it would thread them back
                // into the chain): behind the structurizer an else arm is a second guarded block BEHIND the first, and the cells as they came in stay
                // alive beside the first arm's results for it — every arm then worked on copies: a move in front of each skipped row, four at the
                // loop's back edge and four more where the edge loop ends. A lone if that updates the cells joins them with themselves.
                auto is_kind = [&](uint32_t k) {
                    uint32_t mine = kind;
#if defined(__HIP_DEVICE_COMPILE__)
                    asm volatile("" : "+s"(mine));
#endif
                    return mine == k;
                };
                if (is_kind(KIND_IQ)) curve(std::integral_constant<uint32_t, KIND_IQ>{});
                if (is_kind(KIND_IC)) curve(std::integral_constant<uint32_t, KIND_IC>{});
                if (is_kind(KIND_RQ)) curve(std::integral_constant<uint32_t, KIND_RQ>{});
                if (is_kind(KIND_RC)) curve(std::integral_constant<uint32_t, KIND_RC>{});
            }
            if (end >= 64u) break; // (the group runs on into the next chunk)
            rest = end >= 63u ? 0ull : rest & (~0ull << (end + 1u));
            // ---- entry `end` is a cover: color_cover (renderer.rs:340-354, 736-754) — blend where the winding is not zero, zero the winding of
            //      the covered samples; premultiplied "over" (shaders.wgsl:304-309, blending of examples/showcase/main.rs:32-43)
            const uint32_t flags = __builtin_amdgcn_readlane(eflags, end);
            const uint32_t kind = (flags >> 4) & 15u;
#ifdef CRH_ABLATE
            if ((r.debug & 16u) && kind == EK_SYNTH) continue;
#endif
            unsigned long long blend[ROWS]; // lanes whose sample row b takes the source
            float cs0, cs1, cs2, cs3;
            // replace: an opaque source over finite colours — src + dst * (1 - 1) is the source (r.occlude: every colour of the pass is tame; a source
            // component that is -0 would come out as +0 through the arithmetic, so it takes the arithmetic)
            uint32_t replace; // (0 or 1, put together from scalar words: as a bool it came to the blend through a vector register)
            if (kind == EK_SYNTH) { // COVER over the samples inside the hull, one unit of both backdrops folded in
                replace = (r.occlude != 0u ? 1u : 0u) & (flags >> 20);
                const float4 ea4 = entries[end * 3u + 0u];
                const uint32_t code_all = (flags >> 8) & 31u;
                const int add = ((int)((flags >> 16) & 3u) - 1) + ((int)((flags >> 18) & 3u) - 1) * 65536;
                cs0 = ea4.x, cs1 = ea4.y, cs2 = ea4.z, cs3 = ea4.w;
                if (code_all >= 4u + kCoverHull) { // the whole tile lies inside the hull (no hull edge in the list, hull backdrop not zero): every sample is tested, every winding zeroed
#pragma unroll
                    for (int b = 0; b < ROWS; ++b) {
                        blend[b] = __builtin_amdgcn_ballot_w64((((uint32_t)(cell[b] + add)) & wmask) != 0u);
                        cell[b] = 0;
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < ROWS; ++b) {
                        const int t = cell[b] + add;
                        const int fill = __builtin_amdgcn_sbfe(t, 0u, 16u);
                        const unsigned long long in_hull = __builtin_amdgcn_ballot_w64(t != fill); // (65536 x the hull winding is what is left, whatever the sign of the fill's)
                        blend[b] = in_hull & __builtin_amdgcn_ballot_w64(((uint32_t)fill & wmask) != 0u);
                        cell[b] = __builtin_amdgcn_inverse_ballot_w64(in_hull) ? 0 : fill;
                    }
                }
                if (end == verify_at) { // X of the late start: does it overwrite every sample? (it does unless a sample inherited a winding)
                    verify_at = 0xFFFFFFFFu;
                    if ((blend[0] & blend[1] & blend[2] & blend[3]) != ~0ull || (r.debug & 33554432u) != 0u) { // no (or debug bit 25, tests: never trusted): the colours behind it matter — the whole list, from cleared state
#pragma unroll
                        for (int b = 0; b < ROWS; ++b) {
                            cell[b] = 0;
                            col[b][0] = col[b][1] = col[b][2] = col[b][3] = 0.0f;
                        }
                        if (LONG && n > 64u) { // the first chunk has to be set up again
                            verify_entry = 0xFFFFFFFFu;
                            again_from_the_top = true;
                            break;
                        }
                        rest = all;
                        continue;
                    }
                }
            } else { // a triangle of a folded hull strip, drawn as the reference draws it
                const uint32_t prim = __builtin_amdgcn_readlane(my_key, end);
                const PrimFragment frag = load_uniform(reinterpret_cast<const PrimFragment*>(slots + (size_t)prim * 32u + 64u));
                const float4 ea4 = entries[end * 3u + 0u], eb4 = entries[end * 3u + 1u], ec4 = entries[end * 3u + 2u];
                const TriCoverage cov = tri_coverage(ea4, eb4, ec4, flags);
                cs0 = frag.a0[0], cs1 = frag.a0[1], cs2 = frag.a0[2], cs3 = frag.a0[3];
                replace = __builtin_amdgcn_readfirstlane((r.occlude != 0u && cs3 == 1.0f && __float_as_uint(cs0) != 0x80000000u && __float_as_uint(cs1) != 0x80000000u && __float_as_uint(cs2) != 0x80000000u) ? 1u : 0u); // (the float compare is a vector instruction: back to a scalar here, on the rare path)
#pragma unroll
                for (int b = 0; b < ROWS; ++b) {
                    const unsigned long long inside = inside_row(cov, b);
                    const int fill = __builtin_amdgcn_sbfe(cell[b], 0u, 16u);
                    blend[b] = inside & __builtin_amdgcn_ballot_w64(((uint32_t)fill & wmask) != 0u);
                    cell[b] = __builtin_amdgcn_inverse_ballot_w64(inside) ? cell[b] - fill : cell[b]; // (the fill winding to zero, the hull's — zero in such items — as it is)
                }
            }
            const float one_minus_a = 1.0f - cs3;
            blend_rows(col, blend, cs0, cs1, cs2, cs3, one_minus_a, replace);
            if (rounds_writes<XFMT>(r)) { // an Rgba8Unorm attachment keeps 8 bits of what the blender writes (idempotent on the others)
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) col[b][ch] = attachment<XFMT>(r, ch, col[b][ch]);
            }
        } // groups of the chunk
        if (LONG && again_from_the_top) { // (X of the late start did not overwrite every sample: the whole list, chunk 0 first)
            again_from_the_top = false;
            q0 = 0u - 64u;
        }
    }
    // ---- RGBA8 unorm / binary16 store (the lane's column derived again from the scalar tile coordinate: kept from the top of the kernel it was the six-wave
    //      build's last spilled register)
    uint32_t tx_end = tx, all_lanes = ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(tx_end), "+s"(all_lanes)); // (opaque operands: neither value is the one computed at the top of the kernel and kept alive since)
    const uint32_t lane_end = __builtin_amdgcn_mbcnt_hi(all_lanes, __builtin_amdgcn_mbcnt_lo(all_lanes, 0u)); // the lane's number (= threadIdx.x: one wavefront per workgroup)
#else
    const uint32_t lane_end = threadIdx.x;
#endif
    const uint32_t gx_end = tx_end * kTile + (lane_end & 15u);
#pragma unroll
    for (int b = 0; b < ROWS; ++b) {
        const uint32_t gy = ty * kTile + 4u * b + rq;
        if (gx_end < r.width && gy < r.height) store_px<XFMT>(r, gx_end, gy, col[b][0], col[b][1], col[b][2], col[b][3]);
    }
}

// ---------------------------------------------------------------------------------------------- k_raster_rows (round 4)
// The same pass with the winding numbers ACCUMULATED IN LDS and the lanes spread over (entry, sample row) instead of every lane evaluating
// every entry on its own samples (renderer.rs:304-318, 340-354, 565-582; vertex.rs:28-35; shaders.wgsl:233-266, 304-309). msaa 1, no strokes.
//
// Along a sample row the contribution of an edge entry is a STEP function of the column: g_e = accepts(fma(ry, bx, fma(rx, nay, c))) is monotone
// in rx (round-to-nearest is monotone, twice), so  sigma * [Y_k g(j) + A_k]  is a row constant plus one unit from some switch column on.
// A lane that owns (edge, row) finds the switch column with five evaluations of the EXACT predicate (a lower bound over 16 columns) and makes
// two deposits into a 16 x 16 grid of the tile in DELTA form — the row constant at column 0, +-1 at the switch column; whole-tile backdrop
// units deposit a constant per row; a curve triangle is evaluated by lanes laid over its own pixel box (one sample per lane, the per-sample
// expressions of k_raster_edges) and deposits +-1 at (row, column) and -+1 at column + 1. A cell holds the fill winding in its low and the
// hull winding in its high 16 bits as ONE integer (fill + 65536 * hull): deposits and prefix sums are linear, the two are taken apart after
// the sum (exact while both stay below 2^15 in magnitude: a tile list of fewer than 32 768 entries cannot exceed it, longer ones go to
// k_raster_edges). What is serial is only what the reference orders: a tile's entries are cut into GROUPS  N* C+  (N: edges, backdrop
// units, curve triangles; C: cover entries — every item's covers follow all of its other entries in key order, and the N entries of an item
// without a cover in this tile simply stay in the winding, exactly as the stencil buffer keeps them); the deposits of up to kRowSlots groups
// go to as many grids at once (lanes packed across items: an item has three entries per tile on average), then the groups' cover entries are
// committed in order: the pixel owners (lane = row, four consecutive columns) read their four cells, prefix-sum along the row (three adds
// and two DPP steps inside the quad), add the winding left over from earlier items, test, blend, zero.
// tools/proto_edges.cpp (mode 2) proves the row form against oracle/raster.hpp on the CPU; the GPU parity suite checks this kernel.
#ifndef CRH_ROW_SLOTS
#define CRH_ROW_SLOTS 2
#endif
#ifndef CRH_ROW_TILE_WAVES
#define CRH_ROW_TILE_WAVES 6
#endif
constexpr uint32_t kRowSlots = CRH_ROW_SLOTS; // a power of two
CRH_D int quad_from(int v, int ctrl_0012_or_0101, bool shift_two) { // lane c of a quad <- lane c - 1 (c - 2); lanes without a source get their own value (masked by the caller)
#if defined(__HIP_DEVICE_COMPILE__)
    return shift_two ? __builtin_amdgcn_mov_dpp(v, 0x44, 0xF, 0xF, true) : __builtin_amdgcn_mov_dpp(v, 0x90, 0xF, 0xF, true);
#else
    return v;
#endif
}
// inclusive prefix sum over the wavefront with DPP modifiers (no LDS): Hillis-Steele inside the 16-lane rows (lanes without a source keep the
// identity 0), then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3
#if defined(__HIP_DEVICE_COMPILE__)
#define CRH_DPP(v_, ctrl_, rows_) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v_), ctrl_, rows_, 0xF, false))
#else
#define CRH_DPP(v_, ctrl_, rows_) (v_)
#endif
CRH_D uint32_t dpp_scan_add(uint32_t v) {
    v += CRH_DPP(v, 0x111, 0xF), v += CRH_DPP(v, 0x112, 0xF), v += CRH_DPP(v, 0x114, 0xF), v += CRH_DPP(v, 0x118, 0xF);
    v += CRH_DPP(v, 0x142, 0xA), v += CRH_DPP(v, 0x143, 0xC);
    return v;
}
// the first of the 16 columns of sample row y (x_j = j + 0.5) at which  accepts(E_j) != inv  — E = fma(y, bx, fma(x, nay, c)) is monotone in x,
// so the predicate switches at most once —, 16 if there is none: five evaluations of the exact predicate
CRH_D uint32_t switch_column(float y, float c, float bx, float nay, int thr, bool inv) {
    float lo = 0.0f;
#pragma unroll
    for (int step = 8; step >= 1; step >>= 1) {
        const float x = lo + ((float)step - 0.5f);
        const bool g = __float_as_int(fmaf(y, bx, fmaf(x, nay, c))) >= thr;
        lo = (g != inv) ? lo : lo + (float)step;
    }
    const bool g15 = __float_as_int(fmaf(y, bx, fmaf(15.5f, nay, c))) >= thr;
    return (lo == 15.0f && g15 == inv) ? 16u : (uint32_t)(int)lo;
}
// the first of 16 indices (as a float, 0 .. 15) at which a predicate that is monotone (false ... false true ... true) holds, 16 if none: five evaluations
template <class P>
CRH_D uint32_t first_of_16(P holds) {
    float lo = 0.0f;
#pragma unroll
    for (int step = 8; step >= 1; step >>= 1) lo = holds(lo + (float)(step - 1)) ? lo : lo + (float)step;
    return (lo == 15.0f && !holds(15.0f)) ? 16u : (uint32_t)(int)lo;
}
template <bool LONG, bool XFMT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CRH_ROW_TILE_WAVES))) void k_raster_rows(SceneDev s, RasterParams r) {
    const uint32_t bid = blockIdx.x;
    extern __shared__ uint32_t sort_buffer[];
    __shared__ float4 entry_buffer[64 * 3];
    __shared__ uint32_t grid[kRowSlots][16][16]; // [group slot][sample row][column], delta form, fill + 65536 * hull
    __shared__ float4 frag_buffer[64 * 3];       // a curve triangle's attribute planes relative to the tile: constants, x gradients, y gradients
    __shared__ uint8_t edge_list[64], tri_list[64], slot_of[64];
    __shared__ uint16_t pair_start[66];          // [rank of a triangle in the chunk] its first (triangle, row) pair; [number of triangles] all pairs
    __shared__ uint16_t edge_pair_start[66];     // the same for the boundary edges: their (edge, row) pairs — the rows of the edge's half-open y range
    __shared__ uint32_t vgrid[kRowSlots][16];    // [group slot][sample row] what begins at that row and holds for every column of it and of the rows below (delta form down the tile)
    uint32_t tx, ty;
    if (!tile_of_place(r, bid, tx, ty)) return;
    const uint32_t tile = ty * r.tiles_x + tx;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* __restrict__ keys = sort_buffer;
    // pixel owners: lane = (row k, quad c) owns the pixels (4c .. 4c + 3, k) of the tile: 16 bytes of a frame row
    const uint32_t row_k = lane >> 2, quad_c = lane & 3u;
    const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile);
    const int tpx = (int)(tx * kTile), tpy = (int)(ty * kTile);
    const uint32_t gx0 = tx * kTile + 4u * quad_c, gy = ty * kTile + row_k;
    const int quad_m1 = quad_c >= 1u ? -1 : 0, quad_m2 = quad_c >= 2u ? -1 : 0;
    int left[4]; // the winding the stencil buffer still holds from earlier items (non-zero only where an item's fill pokes out of its hull)
    bool left_any = false; // ... on some sample of the tile
    float col[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        left[i] = 0;
        col[i][0] = col[i][1] = col[i][2] = col[i][3] = 0.0f;
    }
    if (r.load_existing && gy < r.height) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (gx0 + (uint32_t)i < r.width) {
                const float4 d = load_px<XFMT>(r, gx0 + (uint32_t)i, gy);
                col[i][0] = d.x, col[i][1] = d.y, col[i][2] = d.z, col[i][3] = d.w;
            }
    }
    uint4* const my_cells = reinterpret_cast<uint4*>(&grid[0][row_k][4u * quad_c]); // + slot * 64 (uint4 units)
#pragma unroll
    for (uint32_t g = 0; g < kRowSlots; ++g) my_cells[g * 64u] = make_uint4(0u, 0u, 0u, 0u);
    if (lane < kRowSlots * 16u) (&vgrid[0][0])[lane] = 0u;
    // tile_list_range (raster_tile_list.hpp) written out, without its scalar pin: with the helper three of the four instantiations take one register less (99, 98, 99 for 100, 99, 100)
    const uint32_t list_begin = r.direct ? r.tile_base[tile] : r.tile_offset[tile];
    uint32_t n = (r.overflow[0] | r.overflow[5]) ? 0u : (r.direct ? r.tile_count[tile] : r.tile_offset[tile + 1] - list_begin);
    constexpr uint32_t kLdsSortMax = kSortBytesMax / 4u;
    if (n > r.sort_capacity && n <= kLdsSortMax) { // the host grows the sort buffer (overflow[3] = the longest list) and runs the frame again
        if (r.direct && threadIdx.x == 0u) atomicMax(&r.overflow[3], n);
        n = 0;
    } else if (n > kLdsSortMax && r.direct && threadIdx.x == 0u) {
        atomicMax(&r.overflow[3], n); // (the host takes frames that have shown a list of 16 384 entries away from this kernel: its cells hold two 16-bit fields, exact below 32 768 entries)
    }
    uint32_t my_key = 0xFFFFFFFFu;
    const bool sorted_in_place = n > kLdsSortMax;
    uint32_t* const segment = r.tile_list + list_begin;
    if (sorted_in_place) {
        sort_list_in_place(segment, n, threadIdx.x, 64u);
    } else if (n <= 64u) {
        if (lane < n) my_key = r.tile_list[list_begin + lane];
        // (a network as deep as the list needs: most tiles hold fewer than 32 entries — and many fewer than 8, the least sort_keys_in_lanes
        // (raster_tile_list.hpp) runs: with it the glyph scene's step measured a median of 0.615 ms against the parent's 0.603 - 0.612, same resource rows: profiles/tile_list_helpers.txt §3)
        const uint32_t depth = n <= 2u ? 2u : (n <= 4u ? 4u : (n <= 8u ? 8u : (n <= 16u ? 16u : (n <= 32u ? 32u : 64u))));
        if (n > 1u) {
#pragma unroll
            for (uint32_t kk = 2; kk <= 64u; kk <<= 1) {
                if (kk > depth) break;
#pragma unroll
                for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                    const uint32_t other = __shfl_xor(my_key, j, 64);
                    const bool keep_min = ((lane & j) == 0) == ((lane & kk) == 0);
                    my_key = keep_min ? min(my_key, other) : max(my_key, other);
                }
            }
        }
    } else {
        sort_list_in_lds(keys, segment, n, lane);
    }

    const uint8_t* slots = r.slots;
    const int wmask = (int)r.winding_mask;
    uint32_t walk_from = 0, verify_entry = 0xFFFFFFFFu;
    if (LONG && n > 64u && !r.load_existing) find_late_start(slots, segment, keys, sorted_in_place, n, lane, walk_from, verify_entry);
    uint32_t first_j = walk_from & 63u;
    bool again_from_the_top = false;
    bool prev_cover = true; // the entry in front of the chunk's first one was a cover (or there was none): the first entry opens a group
    uint32_t group_base = 0; // the group of the chunk's first entry (groups are numbered along the list; slot = group % kRowSlots)
    for (uint32_t q0 = LONG ? walk_from & ~63u : 0u; q0 < n; q0 += 64u) {
        if (sorted_in_place)
            my_key = q0 + lane < n ? __hip_atomic_load(segment + q0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xFFFFFFFFu;
        else if (n > 64u)
            my_key = q0 + lane < n ? keys[q0 + lane] : 0xFFFFFFFFu;
        const uint32_t count = min(64u, n - q0);
        // ---- entry setup, vectorised across the chunk: lane j prepares entry j (as k_raster_edges)
        float4 e0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e1 = e0, e2 = e0;
        bool hull_over_tile = false, replaces_tile = false;
        uint32_t item_first = 0, item_synth_a = 0;
        uint32_t cls = 0; // 1: edge-like (a boundary edge or a backdrop unit), 2: curve triangle, 3: cover
        float4 f0 = e0, f1 = e0, f2 = e0;
        uint32_t my_rows = 0; // a curve triangle: the sample rows of its box inside the tile; a boundary edge: the rows of its y range
        uint32_t v_row = 16u; // an edge-like entry: the row from which on it adds v_value to every sample of the tile (16: none)
        int v_value = 0;
        if (lane < count) {
            const uint8_t* slot = slots + (size_t)my_key * 32u;
            const uint32_t flags = *reinterpret_cast<const uint32_t*>(slot);
            const uint32_t kind = (flags >> 4) & 15u;
            if (kind == EK_EDGE) {
                const EdgeRec er = *reinterpret_cast<const EdgeRec*>(slot);
                const float c = er.bx * (ty0 - er.lo_y) + er.nay * (tx0 - er.lo_x);
                const bool xr = er.lo_x <= tx0 && tx0 < er.hi_x; // the edge crosses the line of the left tile boundary
                // The edge's contribution to sample (row k, column j), sigma * [Y_k g(k, j) + xr (g(q_k) - g(q_0)) - Y_k g(q_k)], in two parts:
                //   sigma Y_k (g(k, j) - g(q_k))   lives in the rows of the edge's half-open y range [ky0, ky1): one (edge, row) lane each, below;
                //   sigma xr (g(q_k) - g(q_0))     is the same for every column, and g(q_k) is monotone in k (bx >= 0): a unit from the row on at
                //                                  which the edge function at the left tile boundary switches — ONE deposit down the tile.
                const float ymin = fminf(er.lo_y, er.hi_y), ymax = fmaxf(er.lo_y, er.hi_y);
                const uint32_t ky0 = first_of_16([&](float k) { return ymin <= ty0 + (k + 0.5f); }), ky1 = first_of_16([&](float k) { return !(ty0 + (k + 0.5f) < ymax); });
                my_rows = ky1 > ky0 ? ky1 - ky0 : 0u;
                const int thr = 1 - (int)(flags & kEdgeTl);
                const float at_left = fmaf(0.0f, er.nay, c);
                const int sigma_field = ((flags & kEdgeSigmaPos) ? 1 : -1) * ((flags & kEdgeHull) ? 65536 : 1);
                if (xr && !(__float_as_int(fmaf(0.5f, er.bx, at_left)) >= thr)) { // g(q_0) = 0: the unit begins at the first row with g(q_k) = 1
                    v_row = first_of_16([&](float k) { return __float_as_int(fmaf(k + 0.5f, er.bx, at_left)) >= thr; });
                    v_value = sigma_field;
                }
                e0 = make_float4(c, er.bx, er.nay, 0.0f);
                e1 = make_float4(ymin, ymax, __uint_as_float(ky0), __uint_as_float(flags | (xr ? 0x1000u : 0u)));
                cls = 1u;
            } else if (kind == EK_SYNTH) {
                const SynthRec sr = *reinterpret_cast<const SynthRec*>(slot);
                e0 = make_float4(sr.r, sr.g, sr.b, sr.a);
                e1.w = __uint_as_float(flags);
                const uint32_t code_all = (flags >> 8) & 31u;
                hull_over_tile = code_all >= 4u + kCoverHull;
                replaces_tile = code_all >= 4u + kCoverOpaque;
                item_first = sr.first_slot, item_synth_a = sr.synth_a;
                cls = code_all >= 4u ? 3u : 1u;
                if (code_all < 4u) v_row = 0u, v_value = ((code_all & 1u) ? -1 : 1) * (code_all < 2u ? 1 : 65536); // a whole-tile backdrop unit of the fill (codes 0, 1) or hull (2, 3) winding
            } else {
                const PrimCoverage mine = *reinterpret_cast<const PrimCoverage*>(slot);
                const int bx0 = max((int)mine.box.x, tpx) - tpx, bx1 = min((int)mine.box.y, tpx + kTile - 1) - tpx;
                const int by0 = max((int)mine.box.z, tpy) - tpy, by1 = min((int)mine.box.w, tpy + kTile - 1) - tpy;
                const uint32_t col_bits = bx1 >= bx0 ? (2u << bx1) - (1u << bx0) : 0u, row_bits = by1 >= by0 ? (2u << by1) - (1u << by0) : 0u;
                float cc[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) cc[i] = mine.bx[i] * (ty0 - mine.lo_y[i]) + mine.nay[i] * (tx0 - mine.lo_x[i]);
                e0 = make_float4(cc[0], cc[1], cc[2], __uint_as_float(col_bits | (row_bits << 16)));
                e1 = make_float4(mine.bx[0], mine.bx[1], mine.bx[2], __uint_as_float(flags));
                e2 = make_float4(mine.nay[0], mine.nay[1], mine.nay[2], 0.0f);
                cls = kind == EK_COVER_TRI ? 3u : (kind <= KIND_RC ? 2u : 0u); // (stroke triangles: not in a pass this kernel draws)
                if (cls == 2u) { // the fragment half: attribute planes through vertex 0 -> relative to the tile (the expressions of k_raster_edges)
                    const PrimFragment* frag = reinterpret_cast<const PrimFragment*>(slot + 64);
                    const float4 a0 = *reinterpret_cast<const float4*>(frag->a0), gxv = *reinterpret_cast<const float4*>(frag->gx), gyv = *reinterpret_cast<const float4*>(frag->gy);
                    const float dx0 = tx0 - frag->v0x, dy0 = ty0 - frag->v0y;
                    f0 = make_float4(fmaf(dy0, gyv.x, fmaf(dx0, gxv.x, a0.x)), fmaf(dy0, gyv.y, fmaf(dx0, gxv.y, a0.y)), fmaf(dy0, gyv.z, fmaf(dx0, gxv.z, a0.z)),
                                     fmaf(dy0, gyv.w, fmaf(dx0, gxv.w, a0.w)));
                    f1 = gxv, f2 = gyv;
                    my_rows = col_bits ? (uint32_t)__popc(row_bits) : 0u;
                }
            }
        }
        float4* __restrict__ entries = entry_buffer;
        __builtin_amdgcn_wave_barrier();
        entries[lane * 3u + 0u] = e0;
        entries[lane * 3u + 1u] = e1;
        entries[lane * 3u + 2u] = e2;
        if (cls == 2u) frag_buffer[lane * 3u + 0u] = f0, frag_buffer[lane * 3u + 1u] = f1, frag_buffer[lane * 3u + 2u] = f2;
        // ---- where the walk starts (the late start of k_raster_edges, found the same way) ...
        uint32_t j_start = LONG ? first_j : 0u, verify_at = (LONG && verify_entry - q0 < 64u) ? verify_entry - q0 : 0xFFFFFFFFu;
        first_j = 0;
        if (n <= 64u && !r.load_existing) {
            unsigned long long candidates = __builtin_amdgcn_ballot_w64(replaces_tile);
            const unsigned long long resets = __builtin_amdgcn_ballot_w64(hull_over_tile);
            while (candidates) {
                const uint32_t at = 63u - (uint32_t)__builtin_clzll(candidates);
                const uint32_t first_slot = __builtin_amdgcn_readlane(item_first, at), synth_a = __builtin_amdgcn_readlane(item_synth_a, at);
                const uint32_t below = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(lane < count && my_key < synth_a));
                if (below == 0u || __builtin_amdgcn_readlane(my_key, below - 1u) < first_slot) {
                    const unsigned long long before = resets & ((1ull << at) - 1ull);
                    j_start = before ? 64u - (uint32_t)__builtin_clzll(before) : 0u;
                    verify_at = j_start ? at : 0xFFFFFFFFu;
                    break;
                }
                candidates &= ~(1ull << at);
            }
        }
        const unsigned long long edge_all = __builtin_amdgcn_ballot_w64(cls == 1u), tri_all = __builtin_amdgcn_ballot_w64(cls == 2u), cover_all = __builtin_amdgcn_ballot_w64(cls == 3u);
        { // the chunk's edge-like entries and its triangles in list order, and where each triangle's (triangle, row) pairs begin
            const unsigned long long below = (1ull << lane) - 1ull;
            const uint32_t edge_pairs_end = edge_all ? dpp_scan_add(cls == 1u ? my_rows : 0u) : 0u;
            if (cls == 1u) {
                const uint32_t rank = (uint32_t)__popcll(edge_all & below);
                edge_list[rank] = (uint8_t)lane;
                edge_pair_start[rank] = (uint16_t)(edge_pairs_end - my_rows);
            }
            if (lane == 63u) edge_pair_start[__popcll(edge_all)] = (uint16_t)edge_pairs_end;
            const uint32_t pairs_end = tri_all ? dpp_scan_add(cls == 2u ? my_rows : 0u) : 0u;
            if (cls == 2u) {
                const uint32_t rank = (uint32_t)__popcll(tri_all & below);
                tri_list[rank] = (uint8_t)lane;
                pair_start[rank] = (uint16_t)(pairs_end - my_rows);
            }
            if (lane == 63u) pair_start[__popcll(tri_all)] = (uint16_t)pairs_end;
        }
        bool chunk_again;
        do { // (run once; twice when X of the late start turns out not to overwrite every sample)
            chunk_again = false;
            // ---- ... which entries take part, their groups  N* C+  and the slot of each group's grid
            const unsigned long long live = j_start ? ~((1ull << j_start) - 1ull) : ~0ull; // (j_start < 64: a reset lies in front of it)
            const unsigned long long cover_mask = cover_all & live;
            const unsigned long long in_walk = (count == 64u ? ~0ull : (1ull << count) - 1ull) & live;
            // a group begins at an entry that is no cover and follows a cover (the chunk's first entry: follows the previous chunk's last)
            const unsigned long long after_cover = (cover_all << 1) | (((j_start == 0u && !prev_cover) ? 0ull : 1ull) << j_start);
            const unsigned long long begins = after_cover & ~cover_all & in_walk;
            {
                const unsigned long long upto = lane == 63u ? ~0ull : (2ull << lane) - 1ull;
                const uint32_t group = group_base + (uint32_t)__popcll(begins & upto);
                slot_of[lane] = (uint8_t)(group & (kRowSlots - 1u));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint32_t pos = j_start;
            while (pos < count) {
                // ---- a round: the entries of the next kRowSlots groups
                uint32_t round_end = count;
                {
                    unsigned long long later = pos >= 63u ? 0ull : begins & ~((2ull << pos) - 1ull); // groups that begin behind `pos`
#pragma unroll
                    for (uint32_t g = 1; g < kRowSlots; ++g) later &= later - 1ull; // drop kRowSlots - 1 of them (0 & -1 stays 0)
                    if (later) round_end = (uint32_t)__builtin_ctzll(later);
                }
                const unsigned long long below_pos = (1ull << pos) - 1ull, below_end = round_end == 64u ? ~0ull : (1ull << round_end) - 1ull;
#ifdef CRH_ABLATE // tools/count_rows.py: how often does each part of the kernel run?
                if ((r.debug & 256u) && lane == 0u) {
                    atomicAdd(&r.overflow[8], 1u);
                    atomicAdd(&r.overflow[10], (uint32_t)__popcll(edge_all & below_end & ~below_pos));
                    atomicAdd(&r.overflow[9], ((uint32_t)__popcll(edge_all & below_end & ~below_pos) + 3u) / 4u);
                    atomicAdd(&r.overflow[11], (uint32_t)__popcll(tri_all & below_end & ~below_pos));
                    atomicAdd(&r.overflow[13], (uint32_t)__popcll(cover_mask & below_end & ~below_pos));
                    if (pos == j_start && q0 == 0u) atomicAdd(&r.overflow[14], 1u);
                }
#endif
                // ---- deposits of the edge-like entries. (a) lane = entry: what an entry adds to whole rows (a backdrop unit; an edge's switch at the
                //      left tile boundary) goes down the tile in delta form; (b) lane = (edge, row of its y range), the pairs of the round's edges
                //      laid end to end: the switch column of the row, two deposits along it.
                if (v_row < 16u && ((below_end & ~below_pos) >> lane) & 1ull)
                    __hip_atomic_fetch_add(&vgrid[slot_of[lane]][v_row], (uint32_t)v_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint32_t e_lo = (uint32_t)__popcll(edge_all & below_pos), e_hi = (uint32_t)__popcll(edge_all & below_end); // (pos >= j_start: ranks among all of the chunk's)
                if (e_lo < e_hi) {
                    const uint32_t p_lo = __builtin_amdgcn_readfirstlane((uint32_t)edge_pair_start[e_lo]), p_hi = __builtin_amdgcn_readfirstlane((uint32_t)edge_pair_start[e_hi]);
                    uint32_t first_step = 1;
                    while (first_step * 2u < e_hi - e_lo) first_step *= 2u;
                    for (uint32_t p0 = p_lo; p0 < p_hi; p0 += 64u) {
#ifdef CRH_ABLATE
                        if ((r.debug & 256u) && lane == 0u) atomicAdd(&r.overflow[9], 1u);
#endif
                        const uint32_t pair = p0 + lane;
                        if (pair < p_hi) {
                            uint32_t rank = e_lo; // the last edge of the round whose pairs begin at or before `pair`
                            for (uint32_t step = first_step; step >= 1u; step >>= 1) {
                                const uint32_t cand = rank + step;
                                if (cand < e_hi && (uint32_t)edge_pair_start[min(cand, 64u)] <= pair) rank = cand;
                            }
                            const uint32_t idx = edge_list[rank];
                            const float4 ea4 = entries[idx * 3u + 0u], eb4 = entries[idx * 3u + 1u];
                            const uint32_t flags = __float_as_uint(eb4.w);
                            const uint32_t row = (__float_as_uint(eb4.z) + (pair - (uint32_t)edge_pair_start[rank])) & 15u;
                            const float ry = (float)row + 0.5f;
                            const float c0 = ea4.x, ebx = ea4.y, enay = ea4.z;
                            const int thr = 1 - (int)(flags & kEdgeTl);
                            const int gqk = __float_as_int(fmaf(ry, ebx, fmaf(0.0f, enay, c0))) >= thr ? 1 : 0;
                            const bool inv = enay < 0.0f; // g falls along the row: search the first column where it is 0
                            const uint32_t sw = switch_column(ry, c0, ebx, enay, thr, inv);
                            const int g_left = ((sw == 0u) != inv) ? 1 : 0;
                            const int sigma_field = ((flags & kEdgeSigmaPos) ? 1 : -1) * ((flags & kEdgeHull) ? 65536 : 1);
                            uint32_t* const cells = &grid[slot_of[idx]][row][0];
                            if (g_left != gqk) __hip_atomic_fetch_add(cells, (uint32_t)((g_left - gqk) * sigma_field), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (sw > 0u && sw < 16u) __hip_atomic_fetch_add(cells + sw, (uint32_t)(inv ? -sigma_field : sigma_field), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
                // ---- deposits of the curve triangles: lane = (triangle, sample row of its box). The columns of the row that lie inside the triangle
                //      are an interval — each edge function switches once along the row —, found with three searches; the lane then walks the
                //      interval, decides every sample with the implicit-curve test (shaders.wgsl:236-266, the expressions of k_raster_edges)
                //      and deposits +-delta where a run of accepted samples begins and ends. (Measured against the samples of all intervals laid
                //      end to end as tasks, one per lane: fewer instructions on large triangles, more phases — slower where this kernel is used.)
                const uint32_t t_lo = (uint32_t)__popcll(tri_all & below_pos), t_hi = (uint32_t)__popcll(tri_all & below_end);
                if (t_lo < t_hi) {
                    const uint32_t p_lo = __builtin_amdgcn_readfirstlane((uint32_t)pair_start[t_lo]), p_hi = __builtin_amdgcn_readfirstlane((uint32_t)pair_start[t_hi]);
                    uint32_t first_step = 1;
                    while (first_step * 2u < t_hi - t_lo) first_step *= 2u;
                    for (uint32_t p0 = p_lo; p0 < p_hi; p0 += 64u) {
#ifdef CRH_ABLATE
                        if ((r.debug & 256u) && lane == 0u) atomicAdd(&r.overflow[12], 1u), atomicAdd(&r.overflow[15], min(64u, p_hi - p0));
#endif
                        const uint32_t pair = p0 + lane;
                        const bool valid = pair < p_hi;
                        uint32_t rank = t_lo; // the last triangle of the round whose pairs begin at or before `pair`
                        for (uint32_t step = first_step; step >= 1u; step >>= 1) {
                            const uint32_t cand = rank + step;
                            if (cand < t_hi && (uint32_t)pair_start[min(cand, 64u)] <= pair) rank = cand;
                        }
                        const uint32_t idx = tri_list[rank];
                        const float4 ea4 = entries[idx * 3u + 0u], eb4 = entries[idx * 3u + 1u], ec4 = entries[idx * 3u + 2u];
                        const uint32_t flags = __float_as_uint(eb4.w), bits = __float_as_uint(ea4.w);
                        const uint32_t col_bits = bits & 0xFFFFu, row_bits = bits >> 16;
                        const uint32_t row = ((uint32_t)__builtin_ctz(row_bits | 0x10000u) + (pair - (uint32_t)pair_start[rank])) & 15u;
                        const float y = (float)row + 0.5f;
                        uint32_t c_lo = (uint32_t)__builtin_ctz(col_bits | 0x10000u), c_hi = c_lo + (uint32_t)__popc(col_bits);
                        {
                            const bool i0 = ec4.x < 0.0f, i1 = ec4.y < 0.0f, i2 = ec4.z < 0.0f;
                            const uint32_t s0 = switch_column(y, ea4.x, eb4.x, ec4.x, 1 - (int)(flags & 1u), i0);
                            const uint32_t s1 = switch_column(y, ea4.y, eb4.y, ec4.y, 1 - (int)((flags >> 1) & 1u), i1);
                            const uint32_t s2 = switch_column(y, ea4.z, eb4.z, ec4.z, 1 - (int)((flags >> 2) & 1u), i2);
                            c_lo = max(c_lo, max(i0 ? 0u : s0, max(i1 ? 0u : s1, i2 ? 0u : s2)));
                            c_hi = min(c_hi, min(i0 ? s0 : 16u, min(i1 ? s1 : 16u, i2 ? s2 : 16u)));
                        }
                        if (!valid || c_lo >= c_hi) c_lo = 1u, c_hi = 0u; // nothing to walk
                        const float4 fc = frag_buffer[idx * 3u + 0u], fx = frag_buffer[idx * 3u + 1u], fy = frag_buffer[idx * 3u + 2u];
                        const uint32_t kind = (flags >> 4) & 15u;
                        const bool square = kind == KIND_IQ || kind == KIND_RQ;
                        const int delta = (flags & 8u) ? 1 : -1; // front (ccw on screen) increments, back decrements (renderer.rs:577-582)
                        uint32_t* const cells = &grid[slot_of[idx]][row][0];
                        uint32_t j = c_lo;
                        float x = (float)c_lo + 0.5f;
                        bool prev = false;
                        while (__builtin_amdgcn_ballot_w64(j <= c_hi) != 0ull) { // (one column past the interval: a run that reaches its end is closed there)
                            if (j <= c_hi) {
                                const float a0 = fmaf(y, fy.x, fmaf(x, fx.x, fc.x)), a1 = fmaf(y, fy.y, fmaf(x, fx.y, fc.y));
                                const float a2 = fmaf(y, fy.z, fmaf(x, fx.z, fc.z)), a3 = fmaf(y, fy.w, fmaf(x, fx.w, fc.w));
                                const float sq = a0 * a0, m12 = a1 * a2;
                                const float lhs = square ? sq : sq * a0;
                                const float rhs = kind == KIND_IQ ? a1 : (kind == KIND_RC ? m12 * a3 : m12);
                                const bool acc = j < c_hi && lhs - rhs <= 0.0f;
                                if (acc != prev && j < 16u) __hip_atomic_fetch_add(cells + j, (uint32_t)(acc ? delta : -delta), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                prev = acc;
                            }
                            j += 1u;
                            x += 1.0f;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // ---- the covers of the round, in order: commit the group's grid, color_cover (renderer.rs:340-354, 736-754; shaders.wgsl:304-309)
                unsigned long long covers = cover_mask & below_end & ~below_pos;
                // a cover finds deposits in its group's grid iff the entry in front of it is no cover (the group's later covers find it committed)
                const unsigned long long dirty_covers = cover_all & ((~cover_all << 1) | ((j_start == 0u && !prev_cover) ? 1ull : 0ull));
                bool restart = false;
                while (covers) {
                    const uint32_t j = (uint32_t)__builtin_ctzll(covers);
                    covers &= covers - 1ull;
                    const float4 ea4 = entries[j * 3u + 0u], eb4 = entries[j * 3u + 1u], ec4 = entries[j * 3u + 2u];
                    const uint32_t flags = __builtin_amdgcn_readfirstlane(__float_as_uint(eb4.w));
                    const uint32_t kind = (flags >> 4) & 15u;
                    const bool dirty = ((dirty_covers >> j) & 1ull) != 0ull;
                    bool blend[4];
                    float cs0, cs1, cs2, cs3;
                    if (!dirty && !left_any && kind == EK_SYNTH) {
                        // Nothing was deposited for this cover and no sample carries a winding: fill = hull = 0 on the whole tile, so the hull test is
                        // "hbd != 0" and the stencil test "bd != 0 under the winding rule" for every sample alike (an item over the whole tile)
                        const uint32_t code = 4u + (((flags >> 8) & 31u) - 4u) % 9u;
                        const int bd = (int)((code - 4u) % 3u) - 1, hbd = (int)((code - 4u) / 3u) - 1;
                        const bool all = hbd != 0 && (bd & wmask) != 0;
                        if (j == verify_at) {
                            verify_at = 0xFFFFFFFFu;
                            if (!all || (r.debug & 33554432u) != 0u) {
                                restart = true;
                                break;
                            }
                        }
                        if (!all) continue; // (the winding stays zero either way)
                        cs0 = ea4.x, cs1 = ea4.y, cs2 = ea4.z, cs3 = ea4.w;
                        const bool replace = r.occlude != 0u && cs3 == 1.0f && __float_as_uint(cs0) != 0x80000000u && __float_as_uint(cs1) != 0x80000000u && __float_as_uint(cs2) != 0x80000000u;
                        const float one_minus_a = 1.0f - cs3;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            col[i][0] = replace ? cs0 : cs0 + col[i][0] * one_minus_a, col[i][1] = replace ? cs1 : cs1 + col[i][1] * one_minus_a;
                            col[i][2] = replace ? cs2 : cs2 + col[i][2] * one_minus_a, col[i][3] = replace ? cs3 : cs3 + col[i][3] * one_minus_a;
                        }
                        if (rounds_writes<XFMT>(r)) {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int ch = 0; ch < 4; ++ch) col[i][ch] = attachment<XFMT>(r, ch, col[i][ch]);
                        }
                        continue;
                    }
                    int p[4] = {0, 0, 0, 0};
                    if (dirty) {
                        uint4* const mine = my_cells + (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)slot_of[j]) * 64u;
                        const uint4 d = *mine;
                        *mine = make_uint4(0u, 0u, 0u, 0u);
                        uint32_t* const my_down = &vgrid[0][row_k] + (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)slot_of[j]) * 16u;
                        uint32_t down = *my_down; // what begins at this row for all columns: summed down the tile (the four lanes of a row hold the same)
                        *my_down = 0u;
                        down += CRH_DPP(down, 0x114, 0xF), down += CRH_DPP(down, 0x118, 0xF), down += CRH_DPP(down, 0x142, 0xA), down += CRH_DPP(down, 0x143, 0xC);
                        // prefix sum along the row: inside the lane, then over the four lanes of the row
                        const int total = (int)(d.x + d.y + d.z + d.w);
                        int scan = total + (quad_from(total, 0, false) & quad_m1);
                        scan = scan + (quad_from(scan, 0, true) & quad_m2);
                        p[0] = scan - total + (int)d.x + (int)down, p[1] = p[0] + (int)d.y, p[2] = p[1] + (int)d.z, p[3] = p[2] + (int)d.w;
                    }
                    if (kind == EK_SYNTH) { // COVER over the samples inside the hull, one unit of both backdrops folded in
                        const uint32_t code = 4u + (((flags >> 8) & 31u) - 4u) % 9u;
                        const int bd = (int)((code - 4u) % 3u) - 1, hbd = (int)((code - 4u) / 3u) - 1;
                        cs0 = ea4.x, cs1 = ea4.y, cs2 = ea4.z, cs3 = ea4.w;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int fill = __builtin_amdgcn_sbfe(p[i], 0u, 16u), hull = (p[i] - fill) >> 16;
                            const int w = left[i] + fill + bd;
                            const bool in_hull = hull + hbd != 0;
                            blend[i] = in_hull && (w & wmask) != 0;
                            left[i] = in_hull ? 0 : w;
                        }
                        if (j == verify_at) { // X of the late start: does it overwrite every sample? (it does unless a sample inherited a winding)
                            const bool every = blend[0] && blend[1] && blend[2] && blend[3];
                            verify_at = 0xFFFFFFFFu;
                            if (__builtin_amdgcn_ballot_w64(every) != ~0ull || (r.debug & 33554432u) != 0u) { // no (or debug bit 25): the colours behind it matter — the whole list, from cleared state
                                restart = true;
                                break;
                            }
                        }
                    } else { // a triangle of a folded hull strip, drawn as the reference draws it
                        const uint32_t prim = __builtin_amdgcn_readlane(my_key, j);
                        const PrimFragment frag = load_uniform(reinterpret_cast<const PrimFragment*>(slots + (size_t)prim * 32u + 64u));
                        const uint32_t bits = __builtin_amdgcn_readfirstlane(__float_as_uint(ea4.w));
                        const int thr0 = 1 - (int)(flags & 1u), thr1 = 1 - (int)((flags >> 1) & 1u), thr2 = 1 - (int)((flags >> 2) & 1u);
                        const float y = (float)row_k + 0.5f;
                        const bool row_in = ((bits >> (16u + row_k)) & 1u) != 0u;
                        cs0 = frag.a0[0], cs1 = frag.a0[1], cs2 = frag.a0[2], cs3 = frag.a0[3];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const uint32_t px = 4u * quad_c + (uint32_t)i;
                            const float x = (float)px + 0.5f;
                            const float ea = fmaf(y, eb4.x, fmaf(x, ec4.x, ea4.x)), eb = fmaf(y, eb4.y, fmaf(x, ec4.y, ea4.y)), ec = fmaf(y, eb4.z, fmaf(x, ec4.z, ea4.z));
                            const bool inside = row_in && ((bits >> px) & 1u) != 0u && (__float_as_int(ea) >= thr0) & (__float_as_int(eb) >= thr1) & (__float_as_int(ec) >= thr2);
                            const int w = left[i] + __builtin_amdgcn_sbfe(p[i], 0u, 16u);
                            blend[i] = inside && (w & wmask) != 0;
                            left[i] = inside ? 0 : w;
                        }
                    }
                    left_any = __builtin_amdgcn_ballot_w64((left[0] | left[1] | left[2] | left[3]) != 0) != 0ull;
                    // an opaque source over finite colours: src + dst * (1 - 1) is the source (r.occlude: every colour of the pass is tame; a
                    // source component that is -0 would come out as +0 through the arithmetic, so it takes the arithmetic)
                    const bool replace = r.occlude != 0u && cs3 == 1.0f && __float_as_uint(cs0) != 0x80000000u && __float_as_uint(cs1) != 0x80000000u && __float_as_uint(cs2) != 0x80000000u;
                    if (replace) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            col[i][0] = blend[i] ? cs0 : col[i][0];
                            col[i][1] = blend[i] ? cs1 : col[i][1];
                            col[i][2] = blend[i] ? cs2 : col[i][2];
                            col[i][3] = blend[i] ? cs3 : col[i][3];
                        }
                    }
                    // (a second if on a value the compiler cannot see through, not an else: as k_raster_fill's curve kinds — the else arm kept the
                    // sixteen colours alive beside the first arm's results, sixteen copies a cover where the arms meet)
                    uint32_t arithmetic = replace ? 0u : 1u;
#if defined(__HIP_DEVICE_COMPILE__)
                    asm volatile("" : "+v"(arithmetic));
#endif
                    if (arithmetic != 0u) {
                        const float one_minus_a = 1.0f - cs3;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float n0 = cs0 + col[i][0] * one_minus_a, n1 = cs1 + col[i][1] * one_minus_a;
                            const float n2 = cs2 + col[i][2] * one_minus_a, n3 = cs3 + col[i][3] * one_minus_a;
                            col[i][0] = blend[i] ? n0 : col[i][0];
                            col[i][1] = blend[i] ? n1 : col[i][1];
                            col[i][2] = blend[i] ? n2 : col[i][2];
                            col[i][3] = blend[i] ? n3 : col[i][3];
                        }
                    }
                    if (rounds_writes<XFMT>(r)) { // an Rgba8Unorm attachment keeps 8 bits of what the blender writes (idempotent on the others)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int ch = 0; ch < 4; ++ch) col[i][ch] = attachment<XFMT>(r, ch, col[i][ch]);
                    }
                }
                if (restart) { // (X of the late start did not overwrite every sample: everything again, from cleared state, the shortcut off)
                    left_any = false;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        left[i] = 0;
                        col[i][0] = col[i][1] = col[i][2] = col[i][3] = 0.0f;
                    }
#pragma unroll
                    for (uint32_t g = 0; g < kRowSlots; ++g) my_cells[g * 64u] = make_uint4(0u, 0u, 0u, 0u);
                    if (lane < kRowSlots * 16u) (&vgrid[0][0])[lane] = 0u;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    prev_cover = true, group_base = 0;
                    if (LONG && n > 64u) {
                        verify_entry = 0xFFFFFFFFu;
                        again_from_the_top = true;
                    } else {
                        j_start = 0;
                        chunk_again = true;
                    }
                    break;
                }
                pos = round_end;
            }
            if (!chunk_again && !again_from_the_top) {
                group_base += (uint32_t)__popcll(begins); // = the group of the chunk's last entry: it may go on in the next chunk
                prev_cover = ((cover_all >> (count - 1u)) & 1ull) != 0ull;
            }
            __builtin_amdgcn_wave_barrier(); // the lists and slots of this pass over the chunk are read: they may be rewritten
        } while (chunk_again);
        if (LONG && again_from_the_top) { // the whole list, chunk 0 first
            again_from_the_top = false;
            q0 = 0u - 64u;
        }
    }
    // ---- RGBA8 unorm / RGBA16F store: 16 (32) bytes of a frame row per lane
    if (gy < r.height) {
        if (r.format != CRH_FORMAT_RGBA16F && gx0 + 3u < r.width) {
            uint4 px;
            px.x = pack_px<XFMT>(r, col[0][0], col[0][1], col[0][2], col[0][3]), px.y = pack_px<XFMT>(r, col[1][0], col[1][1], col[1][2], col[1][3]);
            px.z = pack_px<XFMT>(r, col[2][0], col[2][1], col[2][2], col[2][3]), px.w = pack_px<XFMT>(r, col[3][0], col[3][1], col[3][2], col[3][3]);
            *reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(r.rgba8) + (size_t)gy * r.width + gx0) = px;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (gx0 + (uint32_t)i < r.width) store_px<XFMT>(r, gx0 + (uint32_t)i, gy, col[i][0], col[i][1], col[i][2], col[i][3]);
        }
    }
}
uint32_t launch_raster_edges(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx,
                         uint64_t raster_bytes, bool has_stroke) {
    if (!edge_pass_samples(samples)) return 0u;
    constexpr uint32_t kBlock = 1u << CRH_XCD_BLOCK_LOG2;
    const uint32_t blocks = ((r.tiles_x + kBlock - 1u) / kBlock) * ((r.tiles_y + kBlock - 1u) / kBlock);
    const dim3 grid((r.tile_order && r.order_places) ? r.order_places : ((blocks + 7u) / 8u) * kBlock * kBlock * 8u); // the places of the tile order (a multiple of 8: place b is drawn on XCD b mod 8)
    // fill scenes at msaa 1: the class-batched walk with packed counters (k_raster_fill); CRH_FILL_KERNEL=0 keeps k_raster_edges<1, 4, false, *> (A/B runs, tests: the two are bit-equal)
    const char* fill_env = getenv("CRH_FILL_KERNEL"); // (read per launch: tests switch it inside one process)
    const bool fill_kernel = !(fill_env && fill_env[0] == '0') && r.winding_mask <= 0xFFFFu && r.fill_cells != 0u;
    const bool xfmt = r.format > CRH_FORMAT_RGBA8_ATTACHMENT; // BGRA / sRGB targets: the XFMT instantiations (the same formulation)
#define CRH_LAUNCH_EDGES(S_, ROWS_, STROKES_, LONG_)                                                                                                    \
    do {                                                                                                                                              \
        if (xfmt)                                                                                                                                     \
            hipLaunchKernelGGL((k_raster_edges<S_, ROWS_, STROKES_, LONG_, true>), grid, dim3(64 * (4 / ROWS_)), (4 / ROWS_) * r.sort_capacity * 4u, stream, s, r); \
        else                                                                                                                                          \
            hipLaunchKernelGGL((k_raster_edges<S_, ROWS_, STROKES_, LONG_>), grid, dim3(64 * (4 / ROWS_)), (4 / ROWS_) * r.sort_capacity * 4u, stream, s, r); \
    } while (0)
    uint32_t variant = kRasterEdges;
    if (samples == 1 && !has_stroke && r.rows) {
        variant = r.long_lists ? kRasterRowsLong : kRasterRows; // the row-span kernel: winding numbers accumulated in LDS, lanes over (entry, sample row)
        if (r.long_lists && xfmt)
            hipLaunchKernelGGL((k_raster_rows<true, true>), grid, dim3(64), r.sort_capacity * 4u, stream, s, r);
        else if (r.long_lists)
            hipLaunchKernelGGL((k_raster_rows<true>), grid, dim3(64), r.sort_capacity * 4u, stream, s, r);
        else if (xfmt)
            hipLaunchKernelGGL((k_raster_rows<false, true>), grid, dim3(64), r.sort_capacity * 4u, stream, s, r);
        else
            hipLaunchKernelGGL((k_raster_rows<false>), grid, dim3(64), r.sort_capacity * 4u, stream, s, r);
    } else if (samples == 4) {
        if (has_stroke) CRH_LAUNCH_EDGES(4, 1, true, false); else CRH_LAUNCH_EDGES(4, 1, false, false);
    } else if (has_stroke) {
        CRH_LAUNCH_EDGES(1, 4, true, false);
    } else if (fill_kernel) {
        // (always the variant that looks for its late start across the chunks of a long list: measured on the 10 000 path scene — few lists
        // beyond one chunk — it is as fast as the one without, 0.1655 against 0.168 ms, and it is the build without scratch memory)
        // (... and ONE build for every frame: round 5's six-wave build for frames of long lists is gone with its reason, see CRH_FILL_TILE_WAVES)
        if (xfmt)
            hipLaunchKernelGGL((k_raster_fill<true, CRH_FILL_TILE_WAVES, true>), grid, dim3(64), r.sort_capacity * 4u, stream, s, r);
        else
            hipLaunchKernelGGL((k_raster_fill<true>), grid, dim3(64), r.sort_capacity * 4u, stream, s, r);
        variant = kRasterFill;
    } else if (r.long_lists) {
        CRH_LAUNCH_EDGES(1, 4, false, true);
        variant = kRasterEdgesLong;
    } else {
        CRH_LAUNCH_EDGES(1, 4, false, false);
    }
#undef CRH_LAUNCH_EDGES
    if (mark) mark(ctx, (samples == 1 && !has_stroke && r.rows) ? "raster_rows" : "raster_tiles", raster_bytes);
    return variant;
}

} // namespace crh
