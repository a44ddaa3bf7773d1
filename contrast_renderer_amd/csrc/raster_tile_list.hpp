// csrc/raster_tile_list.hpp — what every per-tile raster kernel does before it walks its tile's list: the tile of the workgroup's place,
// the list's range, and the sort into draw order (ascending keys) in one of three regimes. Written once for k_raster_tile / k_raster_blend
// (raster_tile_body.inc) and k_raster_edges, k_raster_fill, k_raster_rows (raster_edges.hip). Everything is forced inline: several of those
// kernels sit on a register boundary, and tools/resource_usage.py must show the same rows with a helper as with its lines written out.
// (CRH_D where a helper is plain arithmetic or guards its device code as ga.hpp's do; __device__ __forceinline__ for the three that are nothing but
// device code — threadIdx, barriers, fences, atomics — and have no host form to guard.)
#pragma once
#include "raster_common.hpp"

namespace crh {

// The tile of place `bid` in the frame's tile order; false: the place has no tile in this pass.
// XCD-aware: workgroup b runs on XCD b % 8 (each XCD has its own L2). The frame is cut into 8x8-tile blocks dealt to the XCDs in turn
// (spatially interleaved, so an unevenly filled frame still loads all eight), and an XCD walks a block's 64 tiles back to back: a primitive
// record shared by neighbouring tiles is fetched into one L2 instead of up to eight. The launchers pad the grid.
CRH_D bool tile_of_place(const RasterParams& r, uint32_t bid, uint32_t& tx, uint32_t& ty) {
    constexpr uint32_t kB = CRH_XCD_BLOCK_LOG2, kBlock = 1u << kB;
    const uint32_t turn = bid >> 3;
    const uint32_t blocks_x = (r.tiles_x + kBlock - 1u) >> kB, block = (turn >> (2u * kB)) * 8u + (bid & 7u);
    tx = (block % blocks_x) * kBlock + (turn & (kBlock - 1u)), ty = (block / blocks_x) * kBlock + ((turn >> kB) & (kBlock - 1u));
    if (r.tile_order) { // the host's order for this frame: every XCD's heavy tiles first (api.hip order_tiles_heavy_first)
        const uint32_t mine = r.tile_order[bid];
        if (mine == 0xFFFFFFFFu) return false;
        ty = mine / r.tiles_x, tx = mine - ty * r.tiles_x;
    }
    return !(tx >= r.tiles_x || ty >= r.tiles_y || ty < r.slab_ty0 || ty >= r.slab_ty1); // (beyond the frame, or not in this pass' slab of tile rows)
}

// The edge pass' list of a tile: its first entry in r.tile_list and its length n — 0 for a list the sort buffer cannot hold: the host grows the
// buffer (overflow[3] = the longest list; without lists in place, r.direct, the scan of the counts has published it) and runs the frame again.
// A list beyond lds_sort_max entries is sorted in place and reported too (the host keeps the longest list it has heard of: crh_frame::longest_list).
// (n is decided by selects on scalars only, and pinned to a scalar register: joined behind the lane-0 branch of the report, the compiler took
// it — and with it every branch of k_raster_fill's walk — for lane dependent.)
__device__ __forceinline__ void tile_list_range(const RasterParams& r, uint32_t tile, uint32_t lds_sort_max, uint32_t& list_begin, uint32_t& n) {
    list_begin = r.direct ? r.tile_base[tile] : r.tile_offset[tile];
    n = (r.overflow[0] | r.overflow[5]) ? 0u : (r.direct ? r.tile_count[tile] : r.tile_offset[tile + 1] - list_begin);
    const bool too_long = n > r.sort_capacity && n <= lds_sort_max;
    if (r.direct != 0u && (too_long || n > lds_sort_max) && threadIdx.x == 0u) atomicMax(&r.overflow[3], n);
    n = __builtin_amdgcn_readfirstlane(too_long ? 0u : n);
}

// ---- at most 64 entries: one key per lane, sorted in registers
// One compare-exchange step of a sorting network on the 64 lanes' u32 keys, partner inside the 16-lane row: the partner's key comes in as a DPP
// operand of v_min_u32 / v_max_u32 themselves (no LDS permute, no address arithmetic); keep_min: the lanes that keep the smaller key.
// (s_nop 1: a DPP operand written by the VALU instruction in front needs two wait states, and the assembler does not see into the asm.)
#if defined(__HIP_DEVICE_COMPILE__)
#define CRH_CX_DPP(key_, keep_min_, ctrl_)                                                                                                  \
    {                                                                                                                                       \
        uint32_t lo_, hi_;                                                                                                                  \
        asm("s_nop 1\n\tv_min_u32_dpp %0, %2, %2 " ctrl_ " row_mask:0xf bank_mask:0xf\n\tv_max_u32_dpp %1, %2, %2 " ctrl_ " row_mask:0xf bank_mask:0xf" \
            : "=&v"(lo_), "=&v"(hi_)                                                                                                        \
            : "v"(key_));                                                                                                                   \
        key_ = __builtin_amdgcn_inverse_ballot_w64(keep_min_) ? lo_ : hi_;                                                                   \
    }
#else
#define CRH_CX_DPP(key_, keep_min_, ctrl_) { (void)(keep_min_); }
#endif
// ... partner = lane ^ 4 = quad mirror of the half-row mirror: one DPP move, then as above
CRH_D uint32_t cx_xor4(uint32_t key, unsigned long long keep_min) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x141, 0xF, 0xF, false); // row_half_mirror
    uint32_t lo, hi;
    asm("s_nop 1\n\tv_min_u32_dpp %0, %2, %3 quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\tv_max_u32_dpp %1, %2, %3 quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf"
        : "=&v"(lo), "=&v"(hi)
        : "v"(t), "v"(key));
    return __builtin_amdgcn_inverse_ballot_w64(keep_min) ? lo : hi;
#else
    return key;
#endif
}
// ... partner in another row (lane ^ 16, ^ 31, ^ 32, ^ 63): through the LDS crossbar
CRH_D uint32_t cx_far(uint32_t key, uint32_t lane, uint32_t xor_mask, unsigned long long keep_min) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t other = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane ^ xor_mask) << 2), (int)key);
    return __builtin_amdgcn_inverse_ballot_w64(keep_min) ? min(key, other) : max(key, other);
#else
    return key;
#endif
}
// The normalised bitonic network (every merge begins with a mirror step, so all exchanges keep the minimum in the lower lane) over the first
// `depth` lanes — 8, 16, 32 or 64 (wave uniform) —, ascending; lanes without a key hold 0xFFFFFFFF.
CRH_D uint32_t sort_keys_in_lanes(uint32_t key, uint32_t lane, uint32_t depth) {
    constexpr unsigned long long kBit0 = 0x5555555555555555ull, kBit1 = 0x3333333333333333ull, kBit2 = 0x0F0F0F0F0F0F0F0Full, kBit3 = 0x00FF00FF00FF00FFull,
                                 kBit4 = 0x0000FFFF0000FFFFull, kBit5 = 0x00000000FFFFFFFFull; // lanes whose bit b is clear
    CRH_CX_DPP(key, kBit0, "quad_perm:[1,0,3,2]") // kk = 2
    CRH_CX_DPP(key, kBit1, "quad_perm:[3,2,1,0]") // kk = 4: mirror, 1
    CRH_CX_DPP(key, kBit0, "quad_perm:[1,0,3,2]")
    CRH_CX_DPP(key, kBit2, "row_half_mirror")     // kk = 8: mirror, 2, 1
    CRH_CX_DPP(key, kBit1, "quad_perm:[2,3,0,1]")
    CRH_CX_DPP(key, kBit0, "quad_perm:[1,0,3,2]")
    if (depth > 8u) {
        CRH_CX_DPP(key, kBit3, "row_mirror")      // kk = 16: mirror, 4, 2, 1
        key = cx_xor4(key, kBit2);
        CRH_CX_DPP(key, kBit1, "quad_perm:[2,3,0,1]")
        CRH_CX_DPP(key, kBit0, "quad_perm:[1,0,3,2]")
    }
    if (depth > 16u) {
        key = cx_far(key, lane, 31u, kBit4);      // kk = 32: mirror, 8, 4, 2, 1
        CRH_CX_DPP(key, kBit3, "row_ror:8")
        key = cx_xor4(key, kBit2);
        CRH_CX_DPP(key, kBit1, "quad_perm:[2,3,0,1]")
        CRH_CX_DPP(key, kBit0, "quad_perm:[1,0,3,2]")
    }
    if (depth > 32u) {
        key = cx_far(key, lane, 63u, kBit5);      // kk = 64: mirror, 16, 8, 4, 2, 1
        key = cx_far(key, lane, 16u, kBit4);
        CRH_CX_DPP(key, kBit3, "row_ror:8")
        key = cx_xor4(key, kBit2);
        CRH_CX_DPP(key, kBit1, "quad_perm:[2,3,0,1]")
        CRH_CX_DPP(key, kBit0, "quad_perm:[1,0,3,2]")
    }
    return key;
}

// A list longer than LDS holds — thousands of primitives over one tile (one Shape with 10^4 slivers through a point, hundreds of Shapes
// stacked): rare, so simple. A normalised bitonic network — every compare-exchange leaves the smaller key at the lower index — sorts any
// length: positions beyond n behave as +inf and are skipped. All n_threads threads of the tile's workgroup take part; keys move through L2
// (agent-scope atomics) so that every lane sees what the others wrote.
__device__ __forceinline__ void sort_list_in_place(uint32_t* segment, uint32_t n, uint32_t tid, uint32_t n_threads) {
    uint32_t padded = 1;
    while (padded < n) padded <<= 1;
    auto exchange = [&](uint32_t i, uint32_t partner) {
        if (partner < n) {
            const uint32_t a = __hip_atomic_load(segment + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t b = __hip_atomic_load(segment + partner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a > b) {
                __hip_atomic_store(segment + i, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(segment + partner, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    for (uint32_t k = 2; k <= padded; k <<= 1) {
        const uint32_t half = k >> 1;
        for (uint32_t p = tid; p < (padded >> 1); p += n_threads) { // the mirror step of the block of k
            const uint32_t block = p / half, t = p - block * half;
            exchange(block * k + t, block * k + k - 1u - t);
        }
        __threadfence();
        __syncthreads();
        for (uint32_t j = half >> 1; j > 0; j >>= 1) {
            for (uint32_t p = tid; p < (padded >> 1); p += n_threads) {
                const uint32_t i = 2u * j * (p / j) + (p % j);
                exchange(i, i + j);
            }
            __threadfence();
            __syncthreads();
        }
    }
}

// A list of 65 entries and more that the wave-private LDS buffer holds: src[0 .. n) -> keys[0 .. n) ascending (keys: the next power of two, at least 128, padded with 0xFFFFFFFF)
__device__ __forceinline__ void sort_list_in_lds(uint32_t* keys, const uint32_t* src, uint32_t n, uint32_t lane) {
    uint32_t padded = 128;
    while (padded < n) padded <<= 1;
    for (uint32_t i = lane; i < padded; i += 64u) keys[i] = i < n ? src[i] : 0xFFFFFFFFu;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t k = 2; k <= padded; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < padded; i += 64u) {
                const uint32_t partner = i ^ j;
                if (partner > i) {
                    const uint32_t a = keys[i], b = keys[partner];
                    if (((i & k) == 0) ? (a > b) : (a < b)) {
                        keys[i] = b;
                        keys[partner] = a;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
}

} // namespace crh
