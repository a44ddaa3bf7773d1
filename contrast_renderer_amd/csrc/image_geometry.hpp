// csrc/image_geometry.hpp — the workgroup geometries that the kernels of image_filter.hip share, each written once with its bank, coalescing
// and address-safety argument; a kernel's comment names its geometry and states only what is its own. Device code but for the grids. Row
// staging, chunk staging and row pairs (the two blurs); the tile and its halo (convolve, lighting, turbulence, displace); streaming
// (composite, colour filter, crop, statistics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "edge.hpp"

namespace crh {
namespace {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// (lo.u16[0], hi.u16[0]) and (lo.u16[1], hi.u16[1]) of two words: one v_perm_b32 each
__device__ __forceinline__ uint32_t low_halves(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x05040100u); }
__device__ __forceinline__ uint32_t high_halves(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }
// acc + v.u16[0] * q.u16[0] + v.u16[1] * q.u16[1] in 32 bits (v_dot2_u32_u16): two taps of one channel per instruction
__device__ __forceinline__ uint32_t dot2(uint32_t v, uint32_t q, uint32_t acc) { return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, v), __builtin_bit_cast(u16x2, q), acc, false); }
__device__ __forceinline__ uint32_t wave_of_workgroup() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); } // in an SGPR

constexpr int kBlurSegment = 256; // horizontal: output texels of one row per workgroup, one per lane
constexpr int kBlurApron = 192;   // CRH_MAX_BLUR_RADIUS: the most texels staged beyond the segment on either side (+ 1 for an odd radius' pad)
constexpr int kBlurColumns = 64;  // vertical: columns per workgroup, one per lane of a wave
constexpr int kBlurWaves = 4;     // vertical: waves per workgroup
constexpr int kBlurRows = 8;      // vertical: output rows per lane
constexpr int kBlurBlockRows = kBlurWaves * kBlurRows; // vertical: output rows per workgroup
constexpr int kBlurChunk = 32;    // vertical: intermediate rows staged in LDS at a time

// Row staging, 256 lanes. row[at] = the texel of `line` (n texels) at column first + at, at < count, by the edge (edge.hpp: wrapped, or zero
// under TRANSPARENT; every address wrapped or range-checked), split into two words of two 16-bit fields, r | b << 16 and g | a << 16; then
// the barrier. Lanes take consecutive texels: 256 consecutive words of global memory per turn, 8 bytes of LDS per lane at consecutive
// addresses. After it lane l reads row[l + const]: consecutive lanes, consecutive banks. The caller keeps count within row[].
__device__ __forceinline__ void stage_row(uint2* row, const uint32_t* line, int first, uint32_t count, uint32_t n, uint32_t edge) {
    for (uint32_t at = threadIdx.x; at < count; at += (uint32_t)kBlurSegment) {
        const uint32_t texel = edge_load<true>(line, first + (int)at, (int)n, edge);
        row[at] = make_uint2(texel & 0x00FF00FFu, (texel >> 8) & 0x00FF00FFu);
    }
    __syncthreads();
}

// Chunk staging, 4 waves, lanes along x. rows[s][lane] = texel (x, chunk + s) of the intermediate `tmp` (n rows of w texels of 8 bytes) by the
// edge, s < 32, between two barriers: the first lets every wave finish reading the chunk before. Wave v takes the rows v, v + 4, ...: a
// wave-uniform row, 64 consecutive 8-byte words of global memory and of LDS. Every row of the chunk is written — zeros beyond block_hi, the
// last row the workgroup reads, and in a column outside the image — so a reader may take any row of it. Every address is a wrapped or
// range-checked row times w plus a column below w.
__device__ __forceinline__ void stage_chunk(uint2 (*rows)[kBlurColumns], const uint2* tmp, uint32_t x, uint32_t w, uint32_t n, int chunk, int block_hi, uint32_t edge,
                                            uint32_t lane, uint32_t wave) {
    __syncthreads();
    for (int s = (int)wave; s < kBlurChunk; s += kBlurWaves) {
        uint2 t = make_uint2(0u, 0u);
        const int i = chunk + s;
        if (x < w && i <= block_hi) { // (edge_load's rule, written out: through the call the compiler arranges the two tests differently)
            if (edge != 0u) t = tmp[(size_t)edge_wrap_branching(i, (int)n, edge) * w + x];
            else if ((uint32_t)i < n) t = tmp[(size_t)i * w + x];
        }
        rows[s][lane] = t;
    }
    __syncthreads();
}

// Row pair. Two staged rows (i, i + 1) of a lane's column, each r | g << 16 and b | a << 16, regrouped by channel (four v_perm_b32); then
// pair_mad adds the pair to one output row's four sums with `taps` = the tap of row i | the tap of row i + 1 << 16, one v_dot2_u32_u16
// per channel: 36 vector instructions for the 64 multiply-adds of eight output rows.
struct RowPair { uint32_t r, g, b, a; };
__device__ __forceinline__ RowPair row_pair(uint2 t0, uint2 t1) { return RowPair{low_halves(t0.x, t1.x), high_halves(t0.x, t1.x), low_halves(t0.y, t1.y), high_halves(t0.y, t1.y)}; }
__device__ __forceinline__ void pair_mad(uint32_t (&acc)[4], RowPair p, uint32_t taps) {
    acc[0] = dot2(p.r, taps, acc[0]), acc[1] = dot2(p.g, taps, acc[1]), acc[2] = dot2(p.b, taps, acc[2]), acc[3] = dot2(p.a, taps, acc[3]);
}

// Tile. Grid (ceil(w / 64), ceil(h / (4 ROWS))), 256 lanes: the workgroup produces the tile of 64 x 4 ROWS texels at (i0, j0); lane l of
// wave v the ROWS outputs of column i0 + l, tile rows ROWS v .. ROWS v + ROWS - 1, so a wave's loads along a row and its stores are 64
// consecutive words. The wave is in an SGPR: whatever depends on the row alone is scalar arithmetic.
template <int ROWS>
struct Tile {
    static constexpr int W = 64, Waves = 4, Rows = ROWS, H = Waves * ROWS, Lanes = W * Waves;
    uint32_t lane, wave, i0, j0;
    __device__ __forceinline__ Tile() : lane(threadIdx.x & 63u), wave(wave_of_workgroup()), i0(blockIdx.x * (uint32_t)W), j0(blockIdx.y * (uint32_t)H) {}
    __device__ __forceinline__ uint32_t column() const { return i0 + lane; }                  // the lane's output column
    __device__ __forceinline__ uint32_t row() const { return j0 + wave * (uint32_t)ROWS; }    // the lane's first output row
    static dim3 grid(uint32_t w, uint32_t h) { return dim3((w + (uint32_t)W - 1u) / (uint32_t)W, (h + (uint32_t)H - 1u) / (uint32_t)H); } // <= 256 x 1024 at four rows per lane
};

// The halo of a tile: staged[q * PITCH + s] = convert(the source texel (x0 + s, y0 + q) by the edge), s < staged_w <= 128, q < staged_h,
// once; then the barrier. Wave v takes the staged rows v, v + 4, ... (a wave-uniform row: its wrap is scalar arithmetic), a lane the
// staged columns lane and lane + 64, whose wrap it computes once. T is the type the load is made in: uint32_t the texel, uint8_t its last
// byte alone, the alpha. Under TRANSPARENT row and column are clamped, so the load is unconditional — every source address is a wrapped
// or clamped row below h times w plus a wrapped or clamped column below w — and zero is selected outside. The tap loops after it have
// no wrap and no test of position. (The load is not a functor of the caller's: with one the compiler arranges the staging differently.)
template <int PITCH, typename T, typename Convert>
__device__ __forceinline__ void stage_tile(uint32_t* staged, uint32_t staged_w, uint32_t staged_h, const T* src, int x0, int y0, uint32_t w, uint32_t h, uint32_t edge, uint32_t lane, uint32_t wave,
                                           Convert&& convert) {
    int column[2];
    bool inside[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int x = x0 + (int)lane + t * 64; // the source column of staged column lane + 64 t
        column[t] = edge_wrap(x, (int)w, edge);
        inside[t] = edge != 0u || (uint32_t)x < w;
    }
    for (uint32_t q = wave; q < staged_h; q += 4u) {
        const int y = y0 + (int)q;
        const T* line = src + (size_t)edge_wrap(y, (int)h, edge) * w * (4u / sizeof(T));
        const bool row_inside = edge != 0u || (uint32_t)y < h;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t s = lane + (uint32_t)(t * 64);
            if (s < staged_w) {
                const uint32_t texel = line[(size_t)column[t] * (4u / sizeof(T)) + (4u / sizeof(T) - 1u)];
                staged[q * (uint32_t)PITCH + s] = convert(row_inside && inside[t] ? texel : 0u);
            }
        }
    }
    __syncthreads();
}

// Streaming: bytes in, bytes out, nothing shared. A workgroup of 256 lanes owns the row segment blockIdx.x of 256 V texels and strides over
// the rows blockIdx.y, blockIdx.y + gridDim.y, ...; a lane owns V consecutive texels of it, V = 4, 2 or 1: the most for which every row
// starts on a multiple of 4 V bytes, w % V == 0, so that the group is one aligned access of 4 V bytes and lies wholly inside the row or
// wholly outside it: every address is (row j < h) * w + (column i < w). The grid's rows are capped, the rows beyond strided over.
constexpr int kStreamLanes = 256;        // lanes per workgroup: one group of V texels of a row each
constexpr uint32_t kStreamBlocks = 8192; // the grid's cap: four rounds of 256 CUs x 8 workgroups (measured against 2048 and none: DESIGN.md)
template <int V> struct TexelGroup { typedef uint32_t type __attribute__((ext_vector_type(V))); }; // V texels: one access of 4 V bytes
template <int V> __device__ __forceinline__ uint32_t stream_column() { return (blockIdx.x * (uint32_t)kStreamLanes + threadIdx.x) * (uint32_t)V; } // the group's first; % V == 0

struct StreamGrid { uint32_t v, segments; dim3 grid; }; // segments <= 64
inline StreamGrid stream_grid(uint32_t w, uint32_t rows, uint32_t cap) {
    const uint32_t v = w % 4u == 0u ? 4u : w % 2u == 0u ? 2u : 1u;
    const uint32_t segments = (w + (uint32_t)kStreamLanes * v - 1u) / ((uint32_t)kStreamLanes * v);
    return StreamGrid{v, segments, dim3(segments, std::min(rows, std::max(1u, cap / segments)))};
}
// A second image shifted by x against the first: its group is one access of 4 V bytes too only where its rows and the shift keep it aligned,
// and then it lies wholly inside that image or wholly outside. (uint32_t)x % v is x mod v for a negative x as well: v divides 2^32.
inline uint32_t stream_wide(uint32_t v, uint32_t source_w, int32_t x) { return v > 1u && source_w % v == 0u && (uint32_t)x % v == 0u ? 1u : 0u; }
#define CRH_STREAM_DISPATCH(v, LAUNCH, ...) /* LAUNCH(V, ...) with V = v as a constant */ \
    do { if ((v) == 4u) LAUNCH(4, ##__VA_ARGS__); else if ((v) == 2u) LAUNCH(2, ##__VA_ARGS__); else LAUNCH(1, ##__VA_ARGS__); } while (0)

} // namespace
} // namespace crh
