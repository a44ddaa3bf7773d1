// csrc/image_filter.hip — every kernel of the image API (image.hip makes the calls, launch.hpp declares the launchers), one family after
// another. Each filter's rule is in its own header, shared with its host model; the edge rule is edge.hpp's, and the workgroup geometries
// that several families share are image_geometry.hpp's. Nothing here touches a raster kernel.
//   blur, variable blur                 k_image_blur_h / _v, k_image_variable_blur_h / _v   row and chunk staging, row pairs
//   composite, colour filter            k_image_composite, k_image_color_filter             streaming
//   morphology                          k_image_morph_h / _v                                doubling in LDS; van Herk / Gil-Werman
//   convolve, lighting                  k_image_convolve, k_image_lighting                  tile with a halo
//   turbulence, displace                k_image_turbulence, k_image_displace                tile
//   transform                           k_image_transform                                   block tile
//   distance field                      k_image_distance_v / _h                             column walks; a scan in LDS
//   resize                              k_image_resize_h / _v                               transposed chunks; row pairs from cache
//   crop, frame regions, statistics     k_image_crop, k_image_stats, k_image_stats_merge    streaming; a merge of partials
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "color_filter.hpp"
#include "composite.hpp"
#include "convolve.hpp"
#include "displace.hpp"
#include "distance.hpp"
#include "image_geometry.hpp"
#include "launch.hpp"
#include "lighting.hpp"
#include "morphology.hpp"
#include "regions.hpp"
#include "resize.hpp"
#include "transform.hpp"
#include "turbulence.hpp"
#include "variable_blur.hpp"

namespace crh {
namespace {
static_assert(kBlurRows == (int)kBlurTapPad, "a row pair may start one row early: the vertical table holds kBlurTapPad = rows per lane zeros on either side");
static_assert(kBlurApron == (int)kBlurMaxRadius && kBlurApron == (int)kVariableBlurMaxRadius, "the apron holds the largest radius of either blur");
} // namespace

// Horizontal pass. Grid (ceil(out_w / 256), src_h), 256 lanes: the workgroup stages the texels its segment of one row reads — the segment and
// an apron of radius + 1 on either side (stage_row) — then every lane forms its own output from LDS. The taps are read with a wave-uniform
// index, so they come through the scalar cache into SGPRs: taps[0] = q[0] as a 32-bit word (65536 when the axis is the identity),
// taps[1 + p] = q[2 p + 1] | q[2 p + 2] << 16, a pair of 16-bit taps (q[radius + 1] = 0 pads an odd radius: hence the apron's extra texel). The sum runs over tap PAIRS, q[k] (c(i - k) + c(i + k)): the two texels are added in
// their 16-bit fields (<= 510), the sums of taps k and k + 1 are regrouped by channel (v_perm_b32) and each channel takes both taps in one
// v_dot2_u32_u16: 12 vector instructions and four 8-byte LDS reads for 16 multiply-adds.
//   t = (sum_k q[|k|] c(i + k) + 128) >> 8 per channel, <= 65280; four of them are one 8-byte store.
// `origin`: the source column under output column 0 is -origin (the axis's radius for TRANSPARENT, else 0). `radius` is 0 when q[0] = 65536.
__global__ __launch_bounds__(kBlurSegment) void k_image_blur_h(const uint32_t* __restrict__ src, uint32_t src_w, uint2* __restrict__ tmp, uint32_t out_w, const uint32_t* __restrict__ taps,
                                                                uint32_t radius, uint32_t origin, uint32_t edge) {
    __shared__ uint2 row[kBlurSegment + 2 * (kBlurApron + 1)];
    const uint32_t j = blockIdx.y, o0 = blockIdx.x * (uint32_t)kBlurSegment, lane = threadIdx.x;
    const uint32_t* line = src + (size_t)j * src_w;
    const uint32_t apron = radius + 1u; // (radius <= kBlurApron: the host refuses more)
    stage_row(row, line, (int)o0 - (int)origin - (int)apron, (uint32_t)kBlurSegment + 2u * apron, src_w, edge);
    const uint32_t o = o0 + lane;
    if (o >= out_w) return;
    const uint32_t centre = lane + apron;
    const uint2 c = row[centre];
    const uint32_t q0 = taps[0];
    uint32_t r = __umul24(q0, c.x & 0xFFFFu), b = __umul24(q0, c.x >> 16), g = __umul24(q0, c.y & 0xFFFFu), a = __umul24(q0, c.y >> 16);
    for (uint32_t k = 1; k <= radius; k += 2) {
        const uint32_t q = taps[(k + 1u) >> 1];
        const uint2 l0 = row[centre - k], h0 = row[centre + k], l1 = row[centre - k - 1u], h1 = row[centre + k + 1u];
        const uint32_t rb0 = l0.x + h0.x, ga0 = l0.y + h0.y, rb1 = l1.x + h1.x, ga1 = l1.y + h1.y; // sums <= 510 in 16-bit fields
        r = dot2(low_halves(rb0, rb1), q, r), b = dot2(high_halves(rb0, rb1), q, b);
        g = dot2(low_halves(ga0, ga1), q, g), a = dot2(high_halves(ga0, ga1), q, a);
    }
    r = (r + 128u) >> 8, g = (g + 128u) >> 8, b = (b + 128u) >> 8, a = (a + 128u) >> 8;
    tmp[(size_t)j * out_w + o] = make_uint2(r | (g << 16), b | (a << 16));
}

// Vertical pass. Grid (ceil(out_w / 64), ceil(out_h / 32)), 4 waves: lanes run along x, so every global and LDS access of a wave is 64
// consecutive 4- or 8-byte words. The workgroup covers 32 output rows of 64 columns; wave w owns rows 8 w .. 8 w + 7 of them, eight rows per
// lane in 32 accumulators. The 32 + 2 radius intermediate rows the block reads are staged once, 32 rows (16 KiB) at a time (stage_chunk). The
// staged rows are taken in PAIRS (i, i + 1), which a lane adds to each of its eight rows (row_pair, pair_mad). `pairs` is the table
// F[n] | F[n - 1] << 16 of 16-bit taps, F = the symmetric q[|d|], d = -radius .. radius, between 8 zeros on either side: row i meets output
// row m with F[8 + 2 radius - (i - lo) + m] and row i + 1 with the word before, so the eight tap pairs of a row pair are eight consecutive
// words at a wave-uniform index — one scalar load, no branch — and a row outside an output's window meets a zero.
//   out = (sum_k q[|k|] t(i, j + k) + 2^23) >> 24 per channel; the sum is < 2^32 (65280 * 65536).
// `origin`: the intermediate row under output row 0 is -origin (the axis's radius for TRANSPARENT, else 0); tmp has tmp_h rows of out_w
// texels. radius = 0 with pairs = nullptr stands for q[0] = 65536 (the identity on this axis, which no 16-bit tap holds): out = (t + 128) >> 8.
__global__ __launch_bounds__(kBlurColumns * kBlurWaves) void k_image_blur_v(const uint2* __restrict__ tmp, uint32_t tmp_h, uint32_t* __restrict__ out, uint32_t out_w, uint32_t out_h,
                                                                            const uint32_t* __restrict__ pairs, uint32_t radius, uint32_t origin, uint32_t edge) {
    __shared__ uint2 rows[kBlurChunk][kBlurColumns];
    const uint32_t lane = threadIdx.x & 63u, wave = wave_of_workgroup();
    const uint32_t x = blockIdx.x * (uint32_t)kBlurColumns + lane;
    const int block_j0 = (int)(blockIdx.y * (uint32_t)kBlurBlockRows);
    const int j0 = block_j0 + (int)(wave * (uint32_t)kBlurRows); // this wave's first output row
    if (pairs == nullptr) { // the identity: a texel of the intermediate, rounded
        if (x >= out_w) return;
#pragma unroll
        for (int m = 0; m < kBlurRows && j0 + m < (int)out_h; ++m) {
            const uint2 t = edge_load<true>(tmp, j0 + m - (int)origin, (int)tmp_h, edge, out_w, x);
            out[(size_t)(j0 + m) * out_w + x] = (((t.x & 0xFFFFu) + 128u) >> 8) | ((((t.x >> 16) + 128u) >> 8) << 8) | ((((t.y & 0xFFFFu) + 128u) >> 8) << 16) | ((((t.y >> 16) + 128u) >> 8) << 24);
        }
        return;
    }
    const int R = (int)radius;
    // intermediate rows, as source rows (output row j is centred on j - origin): the block reads [block_lo, block_hi], this wave [lo, hi]
    const int last_row = min(block_j0 + kBlurBlockRows, (int)out_h) - 1;
    const int block_lo = block_j0 - (int)origin - R, block_hi = last_row - (int)origin + R;
    const int lo = j0 - (int)origin - R, hi = j0 + kBlurRows - 1 - (int)origin + R;
    uint32_t acc[kBlurRows][4];
#pragma unroll
    for (int m = 0; m < kBlurRows; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0u;
    for (int chunk = block_lo; chunk <= block_hi; chunk += kBlurChunk) {
        stage_chunk(rows, tmp, x, out_w, tmp_h, chunk, block_hi, edge, lane, wave);
        // this wave's rows of the chunk, [from, to], in pairs that start on an even row of the chunk (16 pairs: none leaves it). The pair's
        // first row may be lo - 1 and its second hi + 1: both meet zeros of the table (F's indices run from 0 to 2 R + 16).
        const int from = max(chunk, lo), to = min(min(chunk + kBlurChunk - 1, block_hi), hi); // wave-uniform
        for (int i = chunk + ((from - chunk) & ~1); i <= to; i += 2) {
            const RowPair pair = row_pair(rows[i - chunk][lane], rows[i + 1 - chunk][lane]);
            const uint32_t* q = pairs + (uint32_t)((int)kBlurTapPad + 2 * R - (i - lo)); // ascending in m
#pragma unroll
            for (int m = 0; m < kBlurRows; ++m) pair_mad(acc[m], pair, q[m]);
        }
    }
    if (x >= out_w) return;
#pragma unroll
    for (int m = 0; m < kBlurRows; ++m) {
        const int j = j0 + m;
        if (j >= (int)out_h) break;
        const uint32_t half = 1u << 23;
        out[(size_t)j * out_w + x] = ((acc[m][0] + half) >> 24) | (((acc[m][1] + half) >> 24) << 8) | (((acc[m][2] + half) >> 24) << 16) | (((acc[m][3] + half) >> 24) << 24);
    }
}

void launch_image_blur_h(const uint32_t* src, uint32_t src_w, uint32_t src_h, void* tmp, uint32_t out_w, const uint32_t* taps, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream) {
    const dim3 grid((out_w + (uint32_t)kBlurSegment - 1u) / (uint32_t)kBlurSegment, src_h); // from the output: src_h <= 16384 rows of the intermediate
    hipLaunchKernelGGL(k_image_blur_h, grid, dim3(kBlurSegment), 0, stream, src, src_w, static_cast<uint2*>(tmp), out_w, taps, radius, origin, edge);
}

void launch_image_blur_v(const void* tmp, uint32_t tmp_h, uint32_t* out, uint32_t out_w, uint32_t out_h, const uint32_t* pairs, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream) {
    const dim3 grid((out_w + (uint32_t)kBlurColumns - 1u) / (uint32_t)kBlurColumns, (out_h + (uint32_t)kBlurBlockRows - 1u) / (uint32_t)kBlurBlockRows);
    hipLaunchKernelGGL(k_image_blur_v, grid, dim3(kBlurColumns * kBlurWaves), 0, stream, static_cast<const uint2*>(tmp), tmp_h, out, out_w, out_h, pairs, radius, origin, edge);
}

namespace {
// sum_k q[|k|] row[centre + k] over one level's taps, acc = (r, b, g, a): the two texels of a tap are added in their 16-bit fields first.
// Called with q and R in SGPRs (a wave of one level: the taps come through the scalar cache, the loop does not diverge) or per lane.
__device__ __forceinline__ void variable_blur_row_sum(const uint2* row, uint32_t centre, const uint32_t* __restrict__ q, uint32_t R, uint32_t acc[4]) {
    const uint2 c = row[centre];
    variable_blur_mad(acc, q[0], VariableBlurFields{c.x, c.y});
    for (uint32_t k = 1; k <= R; ++k) {
        const uint2 l = row[centre - k], h = row[centre + k];
        variable_blur_mad(acc, q[k], VariableBlurFields{l.x + h.x, l.y + h.y});
    }
}

// One staged row i of the intermediate against a lane's kBlurRows output rows j0 + m: row m takes q_m[|i - (j0 + m)|] if that lies within
// its own radius (R[m] = -1: no such row or column) and nothing beyond. UNIFORM: every lane of the wave holds the same R and offset per
// row, so they are read from the first lane: scalar compares, scalar tap loads.
template <bool UNIFORM>
__device__ __forceinline__ void variable_blur_column_rows(const uint2 (*rows)[kBlurColumns], uint32_t lane, int chunk, int from, int to, int j0, const uint32_t* __restrict__ table, const int (&R)[kBlurRows],
                                                          const uint32_t (&offset)[kBlurRows], uint32_t (&acc)[kBlurRows][4]) {
    int Rm[kBlurRows];
    uint32_t om[kBlurRows];
#pragma unroll
    for (int m = 0; m < kBlurRows; ++m) Rm[m] = UNIFORM ? __builtin_amdgcn_readfirstlane(R[m]) : R[m], om[m] = UNIFORM ? __builtin_amdgcn_readfirstlane(offset[m]) : offset[m];
    for (int i = from; i <= to; ++i) {
        const uint2 t = rows[i - chunk][lane];
#pragma unroll
        for (int m = 0; m < kBlurRows; ++m) {
            const int d = abs(i - (j0 + m));
            if (d <= Rm[m]) variable_blur_mad(acc[m], table[om[m] + (uint32_t)d], VariableBlurFields{t.x, t.y});
        }
    }
}

// The same for a wave whose rows all hold ONE level (a mask of one value, the bands of a ramp along y): q = that level's taps and R its
// radius, in SGPRs. A pair of staged rows (i, i + 1) that lies wholly above the wave's rows, or wholly below them, and within R of all
// eight, meets them with consecutive taps q[a - 1 .. a + 7], each >= q[1] and so 16 bits wide: k_image_blur_v's inner loop (row_pair,
// pair_mad), the tap pairs packed from the scalar loads. The few rows beside or among the wave's own (and an odd one at a run's end) go
// one at a time as above.
__device__ __forceinline__ void variable_blur_column_one_level(const uint2 (*rows)[kBlurColumns], uint32_t lane, int chunk, int from, int to, int j0, const uint32_t* __restrict__ q, int R,
                                                               uint32_t (&acc)[kBlurRows][4]) {
    // the rows [from, to] in five runs, in any order (the sums are exact): [from, a0) one at a time, `na` rows from a0 in pairs above the
    // wave's rows, [a0 + na, b0) one at a time, `nb` rows from b0 in pairs below them, the rest one at a time
    const int a0 = min(max(j0 + kBlurRows - 1 - R, from), to + 1), na = max(min(to, j0 - 1) - a0 + 1, 0) & ~1;
    const int b0 = min(max(j0 + kBlurRows, from), to + 1), nb = max(min(to, j0 + R) - b0 + 1, 0) & ~1;
    const auto singles = [&](int lo, int hi) {
        for (int i = lo; i <= hi; ++i) {
            const uint2 t = rows[i - chunk][lane];
#pragma unroll
            for (int m = 0; m < kBlurRows; ++m) {
                const int d = abs(i - (j0 + m));
                if (d <= R) variable_blur_mad(acc[m], q[d], VariableBlurFields{t.x, t.y});
            }
        }
    };
    singles(from, a0 - 1);
    for (int i = a0; i < a0 + na; i += 2) { // row i is j0 - i + m >= 2 from row m, row i + 1 one less; j0 - i + 7 <= R
        const RowPair pair = row_pair(rows[i - chunk][lane], rows[i + 1 - chunk][lane]);
        const uint32_t* p = q + (j0 - i - 1);
#pragma unroll
        for (int m = 0; m < kBlurRows; ++m) pair_mad(acc[m], pair, p[m + 1] | p[m] << 16);
    }
    singles(a0 + na, b0 - 1);
    for (int i = b0; i < b0 + nb; i += 2) { // row i is i - j0 - m >= 1 from row m, row i + 1 one more; i + 1 - j0 <= R
        const RowPair pair = row_pair(rows[i - chunk][lane], rows[i + 1 - chunk][lane]);
        const uint32_t* p = q + (i - j0 - (kBlurRows - 1));
#pragma unroll
        for (int m = 0; m < kBlurRows; ++m) pair_mad(acc[m], pair, p[kBlurRows - 1 - m] | p[kBlurRows - m] << 16);
    }
    singles(b0 + nb, to);
}
} // namespace

// crh_image_variable_blur, horizontal pass. k_image_blur_h's geometry — grid (ceil(w / 256), h), 256 lanes, the segment and an apron
// staged in LDS (stage_row) — but the apron is the CALL's largest radius and every lane sums over its own level's taps: u = the mask's
// code at the lane's own texel, table[u] = offset << 8 | radius, the taps at table[offset ..]. A wave whose lanes all hold one level (a
// smooth mask, a ramp along y) takes its taps with a wave-uniform index, as k_image_blur_h does; any other wave loads them per lane and
// runs to its largest radius. Both give the same sums. The result keeps the source's size under every edge. No mask byte indexes outside
// the 256 entries; no radius reaches outside the apron (clamped here too).
__global__ __launch_bounds__(kBlurSegment) void k_image_variable_blur_h(const uint32_t* __restrict__ src, const uint32_t* __restrict__ mask, uint32_t w, uint2* __restrict__ tmp,
                                                                         const uint32_t* __restrict__ table, uint32_t apron, uint32_t shift, uint32_t edge) {
    __shared__ uint2 row[kBlurSegment + 2 * kBlurApron];
    const uint32_t j = blockIdx.y, o0 = blockIdx.x * (uint32_t)kBlurSegment, lane = threadIdx.x;
    const uint32_t* line = src + (size_t)j * w;
    apron = min(apron, (uint32_t)kBlurApron);
    stage_row(row, line, (int)o0 - (int)apron, (uint32_t)kBlurSegment + 2u * apron, w, edge); // (variable_blur_split's fields)
    const uint32_t o = o0 + lane;
    if (o >= w) return;
    const uint32_t u = variable_blur_level(mask[(size_t)j * w + o], shift);
    const uint32_t u0 = __builtin_amdgcn_readfirstlane(u);
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    if (__ballot(u != u0) == 0ull) {
        const uint32_t entry = table[u0];
        variable_blur_row_sum(row, lane + apron, table + variable_blur_offset(entry), min(variable_blur_radius(entry), apron), acc);
    } else {
        const uint32_t entry = table[u];
        variable_blur_row_sum(row, lane + apron, table + variable_blur_offset(entry), min(variable_blur_radius(entry), apron), acc);
    }
    const VariableBlurFields t = variable_blur_intermediate(acc);
    tmp[(size_t)j * w + o] = make_uint2(t.x, t.y);
}

// crh_image_variable_blur, vertical pass. k_image_blur_v's geometry — grid (ceil(w / 64), ceil(h / 32)), 4 waves, lanes along x, wave
// w owns output rows 8 w .. 8 w + 7 of the block's 32, eight rows per lane in 32 accumulators; the intermediate rows are staged 32 at
// a time in LDS (stage_chunk). Every (lane, row) has its own level, read from the mask at the output's own texel; the block
// stages the rows within its largest radius, a wave walks the rows within its own, and a lane's row takes a staged row only within that
// row's radius. Three tap paths, chosen per wave: one level in the whole wave (a uniform mask, the bands of a ramp along y) takes
// k_image_blur_v's inner loop on row pairs (variable_blur_column_one_level); one level per row across the lanes reads radii, offsets
// and taps through the scalar cache; any other wave loads a tap per lane. All three give the same sums.
//   out = (sum_k q_u[|k|] t(i, j + k) + 2^23) >> 24 per channel; the sum is < 2^32 (65280 * 65536).
__global__ __launch_bounds__(kBlurColumns * kBlurWaves) void k_image_variable_blur_v(const uint2* __restrict__ tmp, const uint32_t* __restrict__ mask, uint32_t* __restrict__ out, uint32_t w, uint32_t h,
                                                                                     const uint32_t* __restrict__ table, uint32_t shift, uint32_t edge) {
    __shared__ uint2 rows[kBlurChunk][kBlurColumns];
    __shared__ int wave_radius[kBlurWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = wave_of_workgroup();
    const uint32_t x = blockIdx.x * (uint32_t)kBlurColumns + lane;
    const int block_j0 = (int)(blockIdx.y * (uint32_t)kBlurBlockRows);
    const int j0 = block_j0 + (int)(wave * (uint32_t)kBlurRows); // this wave's first output row
    int R[kBlurRows], reach = -1;                                // (reach: the largest radius of this lane's rows)
    uint32_t offset[kBlurRows];
    bool uniform = true;
#pragma unroll
    for (int m = 0; m < kBlurRows; ++m) {
        const bool mine = x < w && j0 + m < (int)h;
        const uint32_t u = mine ? variable_blur_level(mask[(size_t)(j0 + m) * w + x], shift) : 0u;
        uniform = uniform && __ballot(mine && u != (uint32_t)__builtin_amdgcn_readfirstlane(u)) == 0ull; // (lane 0's column lies inside the image)
        const uint32_t entry = table[u];
        R[m] = mine ? (int)min(variable_blur_radius(entry), (uint32_t)kBlurApron) : -1;
        offset[m] = variable_blur_offset(entry);
        reach = max(reach, R[m]);
    }
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) reach = max(reach, __shfl_xor(reach, step));
    if (lane == 0u) wave_radius[wave] = reach;
    __syncthreads();
    int block_reach = wave_radius[0];
#pragma unroll
    for (int k = 1; k < kBlurWaves; ++k) block_reach = max(block_reach, wave_radius[k]);
    block_reach = __builtin_amdgcn_readfirstlane(block_reach), reach = __builtin_amdgcn_readfirstlane(reach);
    // one level in the whole wave: every row inside the image has the first row's tap set (and so its radius, the wave's reach)
    const uint32_t level_offset = __builtin_amdgcn_readfirstlane(offset[0]);
    bool one_level = uniform;
#pragma unroll
    for (int m = 1; m < kBlurRows; ++m) one_level = one_level && (j0 + m >= (int)h || (uint32_t)__builtin_amdgcn_readfirstlane(offset[m]) == level_offset);
    // intermediate rows: the block reads [block_lo, block_hi], this wave [lo, hi] (empty for a wave with no row: reach = -1)
    const int last_row = min(block_j0 + kBlurBlockRows, (int)h) - 1;
    const int block_lo = block_j0 - block_reach, block_hi = last_row + block_reach;
    const int lo = j0 - reach, hi = reach < 0 ? lo - 1 : min(j0 + kBlurRows, (int)h) - 1 + reach;
    uint32_t acc[kBlurRows][4];
#pragma unroll
    for (int m = 0; m < kBlurRows; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0u;
    // The staging loop once per path, the path chosen outside it: the three paths in one loop cost 134 VGPRs, apart the largest of them.
    // Every wave of the block runs the same chunks, so the barriers of the three copies pair up whichever copy a wave is in.
    const auto chunks = [&](auto&& accumulate) {
        for (int chunk = block_lo; chunk <= block_hi; chunk += kBlurChunk) {
            stage_chunk(rows, tmp, x, w, h, chunk, block_hi, edge, lane, wave);
            accumulate(chunk, max(chunk, lo), min(min(chunk + kBlurChunk - 1, block_hi), hi)); // [from, to]: wave-uniform, inside the chunk
        }
    };
    if (one_level) chunks([&](int chunk, int from, int to) { variable_blur_column_one_level(rows, lane, chunk, from, to, j0, table + level_offset, reach, acc); });
    else if (uniform) chunks([&](int chunk, int from, int to) { variable_blur_column_rows<true>(rows, lane, chunk, from, to, j0, table, R, offset, acc); });
    else chunks([&](int chunk, int from, int to) { variable_blur_column_rows<false>(rows, lane, chunk, from, to, j0, table, R, offset, acc); });
    if (x >= w) return;
#pragma unroll
    for (int m = 0; m < kBlurRows; ++m) {
        const int j = j0 + m;
        if (j >= (int)h) break;
        out[(size_t)j * w + x] = variable_blur_texel(acc[m]);
    }
}

void launch_image_variable_blur_h(const uint32_t* src, const uint32_t* mask, uint32_t w, uint32_t h, void* tmp, const uint32_t* table, uint32_t apron, uint32_t shift, uint32_t edge, hipStream_t stream) {
    const dim3 grid((w + (uint32_t)kBlurSegment - 1u) / (uint32_t)kBlurSegment, h);
    hipLaunchKernelGGL(k_image_variable_blur_h, grid, dim3(kBlurSegment), 0, stream, src, mask, w, static_cast<uint2*>(tmp), table, apron, shift, edge);
}

void launch_image_variable_blur_v(const void* tmp, const uint32_t* mask, uint32_t* out, uint32_t w, uint32_t h, const uint32_t* table, uint32_t shift, uint32_t edge, hipStream_t stream) {
    const dim3 grid((w + (uint32_t)kBlurColumns - 1u) / (uint32_t)kBlurColumns, (h + (uint32_t)kBlurBlockRows - 1u) / (uint32_t)kBlurBlockRows);
    hipLaunchKernelGGL(k_image_variable_blur_v, grid, dim3(kBlurColumns * kBlurWaves), 0, stream, static_cast<const uint2*>(tmp), mask, out, w, h, table, shift, edge);
}

// crh_image_composite. Streaming (image_geometry.hpp) over the backdrop and the result: 4 + 4 bytes read and 4 written per texel. The source
// is shifted by (x, y) against the result: its group is one load of 4 V bytes only where `source_wide` says so (stream_wide); otherwise V
// loads of 4 bytes. Every source address is formed behind
// the range check, in unsigned arithmetic: i - x and j - y wrap modulo 2^32 for any int32 shift, and the true difference lies in
// (-2^31 - 1, 2^31 + 16384), so the wrapped value is below the source's size (<= 16384) exactly when the true one is in range.
// The operator is four wave-uniform integers (composite.hpp CompositeFactors), the mode one branch outside the texel and channel loops.
template <int V>
__global__ __launch_bounds__(kStreamLanes) void k_image_composite(const uint32_t* __restrict__ backdrop, uint32_t w, uint32_t h, const uint32_t* __restrict__ source, uint32_t source_w,
                                                                      uint32_t source_h, uint32_t x, uint32_t y, uint32_t source_wide, uint32_t o, uint32_t mode, CompositeFactors f,
                                                                      uint32_t* __restrict__ out) {
    typedef typename TexelGroup<V>::type Group;
    const uint32_t i = stream_column<V>();
    if (i >= w) return; // (the whole group is outside)
    const uint32_t si = i - x;
    for (uint32_t j = blockIdx.y; j < h; j += gridDim.y) {
        const size_t at = (size_t)j * w + i;
        const uint32_t sj = j - y;
        const Group b = *reinterpret_cast<const Group*>(backdrop + at);
        Group s = 0u, r;
        if (sj < source_h) {
            const uint32_t* line = source + (size_t)sj * source_w;
            if (source_wide) {
                if (si < source_w) s = *reinterpret_cast<const Group*>(line + si);
            } else {
#pragma unroll
                for (int t = 0; t < V; ++t)
                    if (si + (uint32_t)t < source_w) s[t] = line[si + (uint32_t)t];
            }
        }
#define CRH_COMPOSITE_GROUP(M) \
    _Pragma("unroll") for (int t = 0; t < V; ++t) r[t] = composite_texel<M>(s[t], b[t], o, f)
        CRH_COMPOSITE_MODES(mode, CRH_COMPOSITE_GROUP)
#undef CRH_COMPOSITE_GROUP
        *reinterpret_cast<Group*>(out + at) = r;
    }
}

void launch_image_composite(const uint32_t* backdrop, uint32_t w, uint32_t h, const uint32_t* source, uint32_t source_w, uint32_t source_h, int32_t x, int32_t y, uint32_t o, uint32_t mode,
                            uint32_t op, uint32_t* out, hipStream_t stream) {
    const StreamGrid g = stream_grid(w, h, kStreamBlocks);
    const uint32_t wide = stream_wide(g.v, source_w, x);
    const CompositeFactors f = composite_factors(op);
#define CRH_COMPOSITE_LAUNCH(V) hipLaunchKernelGGL(k_image_composite<V>, g.grid, dim3(kStreamLanes), 0, stream, backdrop, w, h, source, source_w, source_h, (uint32_t)x, (uint32_t)y, wide, o, mode, f, out)
    CRH_STREAM_DISPATCH(g.v, CRH_COMPOSITE_LAUNCH);
#undef CRH_COMPOSITE_LAUNCH
}

namespace {
__device__ const UnpremultiplyTable k_unpremultiply{}; // color_filter.hpp's reciprocals, staged in LDS by every workgroup of the kernel below
} // namespace

// crh_image_color_filter. Streaming (image_geometry.hpp): 4 bytes read and 4 written per texel. The 16 coefficients and 4 biases are kernel arguments, wave-uniform (SGPRs); the
// matrix stage is 16 signed 24-bit multiply-adds per texel. The unpremultiply's 256 reciprocals and, with TABLES, the four 256-byte tables
// (as they are in memory: four byte planes, entry v of channel i at byte 256 i + v) are staged in LDS once per workgroup, one word per lane
// each, and read per texel with data-dependent indices: one 4-byte read for the alpha's reciprocal, four 1-byte reads for the tables.
// TABLES = false stages and reads no table and declares no LDS for one.
template <int V, bool TABLES>
__global__ __launch_bounds__(kStreamLanes) void k_image_color_filter(const uint32_t* __restrict__ src, uint32_t w, uint32_t h, ColorFilterCoefficients f,
                                                                         const uint32_t* __restrict__ tables, uint32_t* __restrict__ out) {
    typedef typename TexelGroup<V>::type Group;
    __shared__ uint32_t recip[256];
    __shared__ uint32_t lut[TABLES ? 256 : 1];
    recip[threadIdx.x] = k_unpremultiply.r[threadIdx.x];
    if (TABLES) lut[threadIdx.x] = tables[threadIdx.x];
    __syncthreads();
    const uint32_t i = stream_column<V>();
    if (i >= w) return; // (the whole group is outside)
    for (uint32_t j = blockIdx.y; j < h; j += gridDim.y) {
        const size_t at = (size_t)j * w + i;
        const Group s = *reinterpret_cast<const Group*>(src + at);
        Group r;
#pragma unroll
        for (int t = 0; t < V; ++t) r[t] = color_filter_texel<TABLES>(s[t], f, recip, reinterpret_cast<const uint8_t*>(lut));
        *reinterpret_cast<Group*>(out + at) = r;
    }
}

void launch_image_color_filter(const uint32_t* src, uint32_t w, uint32_t h, const ColorFilterCoefficients& f, const uint32_t* tables, uint32_t* out, hipStream_t stream) {
    const StreamGrid g = stream_grid(w, h, kStreamBlocks);
#define CRH_COLOR_FILTER_LAUNCH(V, TABLES) hipLaunchKernelGGL((k_image_color_filter<V, TABLES>), g.grid, dim3(kStreamLanes), 0, stream, src, w, h, f, tables, out)
    if (tables) CRH_STREAM_DISPATCH(g.v, CRH_COLOR_FILTER_LAUNCH, true);
    else CRH_STREAM_DISPATCH(g.v, CRH_COLOR_FILTER_LAUNCH, false);
#undef CRH_COLOR_FILTER_LAUNCH
}

namespace {
constexpr int kMorphSegment = 256; // horizontal: output texels of one row per workgroup, one per lane (k_image_blur_h's segment)
constexpr int kMorphApron = 192;   // CRH_MAX_MORPHOLOGY_RADIUS: texels staged beyond the segment on either side
constexpr int kMorphStaged = kMorphSegment + 2 * kMorphApron;                         // 640: the most texels a workgroup stages
constexpr int kMorphOwned = (kMorphStaged + kMorphSegment - 1) / kMorphSegment;        // 3: staged texels per lane
constexpr int kMorphColumns = 64;  // vertical: columns per workgroup, one per lane of its single wave
static_assert(kMorphApron == (int)kMorphologyMaxRadius, "the apron holds the largest radius");
} // namespace

// Horizontal pass, by doubling in LDS. Grid (ceil(out_w / 256), src_h), 256 lanes: the workgroup stages the L = 256 + 2 radius texels its
// segment of one row reads, each split into two words of two 16-bit fields (morphology.hpp), by edge.hpp's rule. Lane l owns the
// staged texels l, l + 256 and l + 512 and keeps them in registers. Step k turns m_k[i], the extreme of the 2^k texels from i on, into
// m_{k+1}[i] = op(m_k[i], m_k[i + 2^k]): per owned texel one 8-byte LDS read at lane + const (consecutive lanes, consecutive banks), two
// v_pk_min_u16 / v_pk_max_u16 and one 8-byte write into the other of two buffers, so a step needs one barrier. After p = floor(log2(2 radius + 1))
// steps (at most 8) the window of output o0 + l, the staged texels l .. l + 2 radius, is two overlapping spans of 2^p:
//   out = op(m_p[l], m_p[l + 2 radius + 1 - 2^p]).
// An m_k[i] whose span would pass the staged texels (i + 2^k > L) keeps its value of the step before; no span that an output reads contains
// one, because l + 2 radius + 1 <= L. Every LDS index is checked against L, every source address is formed from a wrapped or range-checked
// column. `origin`: the source column under output column 0 is -origin (the radius for a growing result, else 0). radius >= 1.
template <bool DILATE>
__global__ __launch_bounds__(kMorphSegment) void k_image_morph_h(const uint32_t* __restrict__ src, uint32_t src_w, uint32_t* __restrict__ out, uint32_t out_w, uint32_t radius, uint32_t origin,
                                                                  uint32_t edge) {
    __shared__ uint2 spans[2][kMorphStaged];
    const uint32_t j = blockIdx.y, o0 = blockIdx.x * (uint32_t)kMorphSegment, lane = threadIdx.x;
    const uint32_t* line = src + (size_t)j * src_w;
    const uint32_t window = 2u * radius + 1u, staged = (uint32_t)kMorphSegment + 2u * radius; // (radius <= kMorphApron: the host refuses more)
    const int first = (int)o0 - (int)origin - (int)radius; // the source column of staged texel 0
    MorphologyTexel own[kMorphOwned];
#pragma unroll
    for (int t = 0; t < kMorphOwned; ++t) {
        const uint32_t at = lane + (uint32_t)(t * kMorphSegment);
        const int i = first + (int)at;
        own[t] = morphology_split(at < staged ? edge_load(line, i, (int)src_w, edge) : 0u);
        if (at < staged) spans[0][at] = make_uint2(own[t].rb, own[t].ga);
    }
    __syncthreads();
    uint32_t span = 1u, from = 0u;
    for (; 2u * span <= window; span *= 2u, from ^= 1u) { // (wave- and workgroup-uniform: every lane meets every barrier)
#pragma unroll
        for (int t = 0; t < kMorphOwned; ++t) {
            const uint32_t at = lane + (uint32_t)(t * kMorphSegment);
            if (at + span < staged) {
                const uint2 next = spans[from][at + span];
                own[t] = morphology_extreme<DILATE>(own[t], MorphologyTexel{next.x, next.y});
            }
            if (at < staged) spans[from ^ 1u][at] = make_uint2(own[t].rb, own[t].ga);
        }
        __syncthreads();
    }
    const uint32_t o = o0 + lane;
    if (o >= out_w) return;
    const uint2 last = spans[from][lane + window - span]; // lane + window - span + span <= 255 + window = staged
    out[(size_t)j * out_w + o] = morphology_merge(morphology_extreme<DILATE>(own[0], MorphologyTexel{last.x, last.y}));
}

// Vertical pass, van Herk / Gil-Werman. Grid (ceil(out_w / 64), ceil(out_h / (2 radius + 1))), one wave: lanes run along x, so every global
// and LDS access of the wave is 64 consecutive words. The workgroup owns the W = 2 radius + 1 output rows j0 .. j0 + W - 1 of 64 columns; its
// pivot is the input row c under output row j0 + radius. A lane first walks its column UP from c, keeping the running extreme
// S[k] = op(in[c - k] .. in[c]) and storing each, packed, in LDS (row k, its own word: no lane reads another's, so no barrier); then DOWN
// from c with the running extreme P = op(in[c] .. in[c + m]): output row j0 + m has the window [c - (2 radius - m), c + m], so
//   out(j0 + m) = op(S[2 radius - m], P).
// 4 radius + 1 rows read and 3 (2 radius) + 1 texel comparisons for 2 radius + 1 outputs: two loads, three comparisons (six
// v_pk_min_u16 / v_pk_max_u16), one LDS write and one LDS read per texel at every radius. ROWS = the rows of S the LDS holds, >= W (the launcher picks
// the smallest of three instantiations, so a small radius does not pay the LDS of the largest). `in` has in_h rows of out_w texels;
// `origin`: the input row under output row 0 is -origin. The row index is wave-uniform: the wrap is scalar arithmetic, and its one remainder is
// taken at the pivot (edge.hpp's phase). radius >= 1.
template <bool DILATE, int ROWS>
__global__ __launch_bounds__(kMorphColumns) void k_image_morph_v(const uint32_t* __restrict__ in, uint32_t in_h, uint32_t* __restrict__ out, uint32_t out_w, uint32_t out_h, uint32_t radius,
                                                                  uint32_t origin, uint32_t edge) {
    __shared__ uint32_t suffix[ROWS][kMorphColumns];
    // rows loaded ahead of their use: the more LDS an instantiation takes, the fewer waves share a CU and the more each must keep in flight itself
    constexpr int kAhead = ROWS <= 33 ? 8 : ROWS <= 129 ? 16 : 32;
    const uint32_t lane = threadIdx.x, x = blockIdx.x * (uint32_t)kMorphColumns + lane;
    const uint32_t reach = min(2u * radius, (uint32_t)(ROWS - 1)); // = 2 radius (the launcher's choice of ROWS); the bound keeps every LDS index below ROWS
    const uint32_t j0 = blockIdx.y * (reach + 1u);
    const int c = (int)j0 - (int)origin + (int)radius;
    if (x >= out_w) return; // (no barrier below: a lane shares nothing with its neighbours)
    const uint32_t* column = in + x;
    const int n = (int)in_h, period = edge_period(n, edge);
    // Row i of the lane's column, (0, 0, 0, 0) outside the image under TRANSPARENT, by an unconditional load
    auto texel_of = [&](int i, int phase) { return morphology_split(edge_load_select(column, i, phase, n, edge, out_w)); };
    const int phase_c = edge_phase(c, n, edge); // the walk's one division; from here the phase moves by one with the row
    const MorphologyTexel centre = texel_of(c, phase_c);
    MorphologyTexel s = centre;
    suffix[0][lane] = morphology_merge(s);
    int phase = phase_c;
#pragma unroll kAhead
    for (uint32_t k = 1u; k <= reach; ++k) {
        phase = edge_phase_before(phase, period);
        s = morphology_extreme<DILATE>(s, texel_of(c - (int)k, phase));
        suffix[k][lane] = morphology_merge(s);
    }
    MorphologyTexel p = centre;
    const uint32_t rows = min(reach + 1u, out_h - j0); // (j0 < out_h by the grid)
    out[(size_t)j0 * out_w + x] = morphology_merge(morphology_extreme<DILATE>(p, morphology_split(suffix[reach][lane])));
    phase = phase_c;
#pragma unroll kAhead
    for (uint32_t m = 1u; m < rows; ++m) {
        phase = edge_phase_next(phase, period);
        p = morphology_extreme<DILATE>(p, texel_of(c + (int)m, phase));
        out[(size_t)(j0 + m) * out_w + x] = morphology_merge(morphology_extreme<DILATE>(p, morphology_split(suffix[reach - m][lane])));
    }
}

void launch_image_morph_h(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint32_t* out, uint32_t out_w, uint32_t op, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream) {
    const dim3 grid((out_w + (uint32_t)kMorphSegment - 1u) / (uint32_t)kMorphSegment, src_h); // src_h <= 16384 rows: below the grid's limit of 65535
    if (op == kMorphologyDilate) hipLaunchKernelGGL(k_image_morph_h<true>, grid, dim3(kMorphSegment), 0, stream, src, src_w, out, out_w, radius, origin, edge);
    else hipLaunchKernelGGL(k_image_morph_h<false>, grid, dim3(kMorphSegment), 0, stream, src, src_w, out, out_w, radius, origin, edge);
}

void launch_image_morph_v(const uint32_t* in, uint32_t in_h, uint32_t* out, uint32_t out_w, uint32_t out_h, uint32_t op, uint32_t radius, uint32_t origin, uint32_t edge, hipStream_t stream) {
    const uint32_t window = 2u * radius + 1u;
    const dim3 grid((out_w + (uint32_t)kMorphColumns - 1u) / (uint32_t)kMorphColumns, (out_h + window - 1u) / window); // <= 16384 / 3 + 1 row blocks
#define CRH_MORPH_V_LAUNCH(DILATE, ROWS) hipLaunchKernelGGL((k_image_morph_v<DILATE, ROWS>), grid, dim3(kMorphColumns), 0, stream, in, in_h, out, out_w, out_h, radius, origin, edge)
    if (op == kMorphologyDilate) {
        if (window <= 33u) CRH_MORPH_V_LAUNCH(true, 33);
        else if (window <= 129u) CRH_MORPH_V_LAUNCH(true, 129);
        else CRH_MORPH_V_LAUNCH(true, 2 * kMorphApron + 1);
    } else {
        if (window <= 33u) CRH_MORPH_V_LAUNCH(false, 33);
        else if (window <= 129u) CRH_MORPH_V_LAUNCH(false, 129);
        else CRH_MORPH_V_LAUNCH(false, 2 * kMorphApron + 1);
    }
#undef CRH_MORPH_V_LAUNCH
}

namespace {
#ifndef CRH_CONVOLVE_ROWS
#define CRH_CONVOLVE_ROWS 4 // (a build with -DCRH_CONVOLVE_ROWS=1, 2 or 8 is how DESIGN.md's comparison of the register blocking was measured)
#endif
typedef Tile<CRH_CONVOLVE_ROWS> ConvolveTile; // adjacent output rows per lane: a staged texel's bytes are extracted once for all of them
constexpr int kConvolveRows = ConvolveTile::Rows;
constexpr int kConvolveHalo = (int)kConvolveMaxOrder - 1;              // 14: the most texels staged beyond the tile per axis
constexpr int kConvolvePitch = ConvolveTile::W + kConvolveHalo;        // 78 words per staged row
constexpr int kConvolveStagedRows = ConvolveTile::H + kConvolveHalo;   // 30
constexpr int kConvolveTapRows = (int)kConvolveMaxOrder + 2 * (kConvolveRows - 1); // 21: the kernel's rows between kConvolveRows - 1 rows of zeros

// The kernel matrix as k_image_convolve reads it: rotated, so that k[(dy + kConvolveRows - 1) * 15 + dx] multiplies the window's texel
// (dx, dy) counted from the window's top left, and between rows of zeros, so that a lane's output row b takes row q - b + kConvolveRows - 1
// for the staged row q of its block whether or not that staged row lies in b's window. `bias` = ConvolveCoefficients::bias.
struct ConvolveTaps {
    int32_t k[kConvolveTapRows * (int)kConvolveMaxOrder];
    int32_t bias;
};
} // namespace

// crh_image_convolve: a 2-D stencil on a tile of 64 x 16 texels (image_geometry.hpp: Tile). The workgroup stages the (64 + order_x - 1) x
// (16 + order_y - 1) source texels its windows read in LDS, once (stage_tile); the load stage (the clamp to alpha and, with PRESERVE, the
// unpremultiply) is applied there, so the tap loop has no wrap, no clamp and no division. Then lane l of wave v produces the four outputs
// of column l, tile rows 4 v .. 4 v + 3: for each of the order_y + 3 staged rows under them and each kernel column it reads one word at
// lane + const (consecutive lanes, consecutive banks: no conflict at the pitch of 78), extracts its bytes once and adds it into the four
// outputs' sums with the coefficients of four rows of the padded table — 16 (with PRESERVE, 12) signed 24-bit multiply-adds per read. The
// coefficients are a kernel argument and every index into them is wave-uniform: scalar loads, scalar operands. LDS: 9360 B (+ 1 KiB of
// reciprocals with PRESERVE), so registers and the 32-wave cap, not LDS, bound the occupancy. LDS indices: row 4 v + q <= 12 + order_y + 2
// = (16 + order_y - 1) - 1, column l + dx <= 63 + order_x - 1 <= 77.
template <bool PRESERVE>
__global__ __launch_bounds__(ConvolveTile::Lanes) void k_image_convolve(const uint32_t* __restrict__ src, uint32_t w, uint32_t h, ConvolveTaps taps, uint32_t order_x, uint32_t order_y,
                                                                                    uint32_t target_x, uint32_t target_y, uint32_t edge, uint32_t* __restrict__ out) {
    __shared__ uint32_t staged[kConvolveStagedRows * kConvolvePitch];
    __shared__ uint32_t recip[PRESERVE ? 256 : 1];
    if (PRESERVE) {
        recip[threadIdx.x] = k_unpremultiply.r[threadIdx.x];
        __syncthreads();
    }
    const ConvolveTile tile;
    const uint32_t lane = tile.lane;
    const int i0 = (int)tile.i0, j0 = (int)tile.j0; // (below: orders <= 15, the host refuses more)
    stage_tile<kConvolvePitch>(staged, (uint32_t)ConvolveTile::W + order_x - 1u, (uint32_t)ConvolveTile::H + order_y - 1u, src, i0 - (int)target_x, j0 - (int)target_y, w, h, edge, lane,
                               tile.wave, [&](uint32_t texel) { return convolve_load<PRESERVE>(texel, recip); });
    const uint32_t y0 = tile.wave * (uint32_t)kConvolveRows; // the tile row of the lane's first output
    int32_t n[kConvolveRows][4];
#pragma unroll
    for (int b = 0; b < kConvolveRows; ++b)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) n[b][ch] = taps.bias;
    for (uint32_t q = 0; q < order_y + (uint32_t)(kConvolveRows - 1); ++q) {
        const uint32_t* line = staged + (y0 + q) * (uint32_t)kConvolvePitch + lane;
        const int32_t* row = taps.k + q * kConvolveMaxOrder; // output row b takes the table's row q - b + kConvolveRows - 1
        for (uint32_t dx = 0; dx < order_x; ++dx) {
            const uint32_t s = line[dx];
#pragma unroll
            for (int b = 0; b < kConvolveRows; ++b) convolve_mad<PRESERVE>(n[b], row[(uint32_t)(kConvolveRows - 1 - b) * kConvolveMaxOrder + dx], s);
        }
    }
    const uint32_t i = (uint32_t)i0 + lane;
    if (i >= w) return;
#pragma unroll
    for (int b = 0; b < kConvolveRows; ++b) {
        const uint32_t j = (uint32_t)j0 + y0 + (uint32_t)b;
        if (j >= h) break;
        const uint32_t centre = staged[(y0 + (uint32_t)b + target_y) * (uint32_t)kConvolvePitch + lane + target_x]; // the loaded texel under the output
        out[(size_t)j * w + i] = convolve_store<PRESERVE>(n[b], centre);
    }
}

void launch_image_convolve(const uint32_t* src, uint32_t w, uint32_t h, const ConvolveCoefficients& f, uint32_t order_x, uint32_t order_y, uint32_t target_x, uint32_t target_y, uint32_t edge,
                           bool preserve_alpha, uint32_t* out, hipStream_t stream) {
    ConvolveTaps taps = {};
    for (uint32_t dy = 0; dy < order_y; ++dy)
        for (uint32_t dx = 0; dx < order_x; ++dx)
            taps.k[(dy + (uint32_t)(kConvolveRows - 1)) * kConvolveMaxOrder + dx] = f.k[(order_y - 1u - dy) * order_x + (order_x - 1u - dx)];
    taps.bias = f.bias;
    const dim3 grid = ConvolveTile::grid(w, h), block(ConvolveTile::Lanes);
    if (preserve_alpha) hipLaunchKernelGGL(k_image_convolve<true>, grid, block, 0, stream, src, w, h, taps, order_x, order_y, target_x, target_y, edge, out);
    else hipLaunchKernelGGL(k_image_convolve<false>, grid, block, 0, stream, src, w, h, taps, order_x, order_y, target_x, target_y, edge, out);
}

namespace {
#ifndef CRH_LIGHTING_ROWS
#define CRH_LIGHTING_ROWS 4 // (a build with -DCRH_LIGHTING_ROWS=1, 2 or 8 is how DESIGN.md's comparison of the row blocking was measured)
#endif
#ifndef CRH_LIGHTING_FLAT_SKIP
#define CRH_LIGHTING_FLAT_SKIP 1 // (-DCRH_LIGHTING_FLAT_SKIP=0: a distant light's arithmetic on every texel, the comparison of DESIGN.md)
#endif
typedef Tile<CRH_LIGHTING_ROWS> LightingTile; // adjacent output rows per lane: the column sums of a staged row serve three of them
constexpr int kLightingRows = LightingTile::Rows;
constexpr int kLightingPitch = LightingTile::W + 2;      // 66 words per staged row: the tile and one texel of halo on each side
constexpr int kLightingStagedRows = LightingTile::H + 2; // 18
} // namespace

// crh_image_lighting: a 3 x 3 stencil on the alpha channel under binary64 arithmetic, on a tile of 64 x 16 texels (image_geometry.hpp:
// Tile). The workgroup stages the 66 x 18 alpha codes its gradients read in LDS, one word each, once (stage_tile), so the arithmetic never
// branches on position. Only the alpha byte of a source texel is loaded (one byte load at texel * 4 + 3). Then lane l of wave v produces the
// four outputs of column l, tile rows 4 v .. 4 v + 3, walking down the staged rows 4 v .. 4 v + 5: of each it reads the three codes at lane,
// lane + 1, lane + 2 (consecutive lanes, consecutive banks: no conflict at the pitch of 66) and keeps their difference (right - left) and
// their sum (left + 2 mid + right) for the three output rows that use them, so an output costs 3 LDS reads, not 9. gx and gy are integer
// sums of those; the rest is lighting_texel, specialised on (OP, LIGHT): a distant diffuse call carries no per-texel L and no power.
// Under a distant light the result depends on (gx, gy) alone, and lanes whose gradient is zero — most of any real layer — take the texel
// the host computed with the same function (f.flat); a wave in which every lane does skips the arithmetic. LDS: 4752 B, so registers and
// the 32-wave cap, not LDS, bound the occupancy. LDS indices: row 4 v + b + 2 <= 12 + 3 + 2 = 17, column l + 2 <= 65.
template <uint32_t OP, uint32_t LIGHT>
__global__ __launch_bounds__(LightingTile::Lanes) void k_image_lighting(const uint8_t* __restrict__ src, uint32_t w, uint32_t h, LightingConstants f, uint32_t edge,
                                                                                    uint32_t* __restrict__ out) {
    __shared__ uint32_t staged[kLightingStagedRows * kLightingPitch];
    const LightingTile tile;
    const uint32_t lane = tile.lane;
    const int i0 = (int)tile.i0, j0 = (int)tile.j0;
    stage_tile<kLightingPitch>(staged, (uint32_t)kLightingPitch, (uint32_t)kLightingStagedRows, src, i0 - 1, j0 - 1, w, h, edge, lane, tile.wave, [](uint32_t alpha) { return alpha; });
    const uint32_t y0 = tile.wave * (uint32_t)kLightingRows; // the tile row of the lane's first output
    const uint32_t i = (uint32_t)i0 + lane;
    // the staged rows above and on the first output: their differences, sums and the code under the output
    const uint32_t* line = staged + y0 * (uint32_t)kLightingPitch + lane;
    int diff_above = (int)line[2] - (int)line[0], sum_above = (int)(line[0] + 2u * line[1] + line[2]);
    line += kLightingPitch;
    int diff_here = (int)line[2] - (int)line[0], sum_here = (int)(line[0] + 2u * line[1] + line[2]);
    uint32_t alpha = line[1];
#pragma unroll
    for (int b = 0; b < kLightingRows; ++b) {
        line += kLightingPitch;
        const uint32_t below = line[1];
        const int diff_below = (int)line[2] - (int)line[0], sum_below = (int)(line[0] + 2u * below + line[2]);
        const int gx = diff_above + 2 * diff_here + diff_below, gy = sum_below - sum_above;
        const uint32_t j = (uint32_t)j0 + y0 + (uint32_t)b;
        if (i < w && j < h) {
            uint32_t texel;
            if (CRH_LIGHTING_FLAT_SKIP && LIGHT == kLightDistant && gx == 0 && gy == 0) texel = f.flat;
            else texel = lighting_texel<OP, LIGHT>(f, gx, gy, alpha, i, j);
            out[(size_t)j * w + i] = texel;
        }
        diff_above = diff_here, diff_here = diff_below, sum_above = sum_here, sum_here = sum_below, alpha = below;
    }
}

void launch_image_lighting(const uint32_t* src, uint32_t w, uint32_t h, const LightingConstants& f, uint32_t op, uint32_t light, uint32_t edge, uint32_t* out, hipStream_t stream) {
    const dim3 grid = LightingTile::grid(w, h), block(LightingTile::Lanes);
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(src);
#define CRH_LIGHTING_LAUNCH(OP, LIGHT) hipLaunchKernelGGL((k_image_lighting<OP, LIGHT>), grid, block, 0, stream, bytes, w, h, f, edge, out)
    if (op == kLightingDiffuse) {
        if (light == kLightDistant) CRH_LIGHTING_LAUNCH(kLightingDiffuse, kLightDistant);
        else if (light == kLightPoint) CRH_LIGHTING_LAUNCH(kLightingDiffuse, kLightPoint);
        else CRH_LIGHTING_LAUNCH(kLightingDiffuse, kLightSpot);
    } else {
        if (light == kLightDistant) CRH_LIGHTING_LAUNCH(kLightingSpecular, kLightDistant);
        else if (light == kLightPoint) CRH_LIGHTING_LAUNCH(kLightingSpecular, kLightPoint);
        else CRH_LIGHTING_LAUNCH(kLightingSpecular, kLightSpot);
    }
#undef CRH_LIGHTING_LAUNCH
}

namespace {
#ifndef CRH_TURBULENCE_ROWS
#define CRH_TURBULENCE_ROWS 4 // (a build with -DCRH_TURBULENCE_ROWS=1, 2 or 8 is how DESIGN.md's comparison of the row blocking is measured)
#endif
typedef Tile<CRH_TURBULENCE_ROWS> TurbulenceTile; // adjacent output rows per lane: one column half serves them all
constexpr int kTurbulenceRows = TurbulenceTile::Rows;
} // namespace

// crh_image_turbulence: procedural noise, bound by binary64 arithmetic and LDS gathers, on a tile of 64 x 16 texels (image_geometry.hpp:
// Tile). The workgroup first copies the call's tables into LDS: the gradients of the channels it
// evaluates, 16 bytes per (channel, lattice value) — 16 KB, or 12 KB when OPAQUE — and the 256 lattice bytes; lane t copies entry t of
// every channel and (the first wave) word t of the lattice. Then lane l of wave v produces the four outputs of column l, tile rows
// 4 v .. 4 v + 3. The octaves are the outer loop: per octave the lane computes its column's half of the cell once (floor, fractions,
// s-curve, the wrap when STITCH, lat[bx0] and lat[bx1]) and then, for each of its rows, the row's half (the same function), the four
// corner indices — once for all channels — and per channel four 16-byte gradients (ds_read_b128: consecutive lattice values lie in
// consecutive bank quads, so only lanes of one 16-lane group whose corners differ by a multiple of 16 collide) and the 21 operations of
// the interpolation. The sums of the rows stay in registers (rows x channels doubles). A lane outside the image computes like any other —
// every LDS index is masked to 8 bits — and does not store. Periods, their reciprocals and the ratio of octave o are the kernel
// arguments of octave 0 shifted or halved o times, which is exact. The specialisation without STITCH carries no wrap at all.
template <uint32_t KIND, bool OPAQUE, bool STITCH>
__global__ __launch_bounds__(TurbulenceTile::Lanes) void k_image_turbulence(const TurbulenceTables* __restrict__ tables, uint32_t w, uint32_t h, TurbulenceConstants f,
                                                                                          uint32_t* __restrict__ out) {
    constexpr int CH = OPAQUE ? 3 : 4;
    __shared__ __attribute__((aligned(16))) double gradient[CH * 512];
    __shared__ __attribute__((aligned(16))) uint8_t lattice[256];
    const TurbulenceTile tile;
    const uint32_t lane = tile.lane, wave = tile.wave;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const uint32_t e = ((uint32_t)k * 256u + threadIdx.x) * 2u;
        gradient[e] = tables->gradient[e], gradient[e + 1u] = tables->gradient[e + 1u];
    }
    if (wave == 0u) reinterpret_cast<uint32_t*>(lattice)[lane] = reinterpret_cast<const uint32_t*>(tables->lattice)[lane];
    __syncthreads();
    const uint32_t i = tile.column(), j0 = tile.row();
    double vx = (f.ox + (double)i) * f.fx, vy[kTurbulenceRows];
#pragma unroll
    for (int b = 0; b < kTurbulenceRows; ++b) vy[b] = (f.oy + (double)(j0 + (uint32_t)b)) * f.fy;
    TurbulenceSums<CH> sums[kTurbulenceRows] = {};
    double inv_ratio = 1.0, inv_px = f.inv_px, inv_py = f.inv_py;
    int32_t px = f.px, py = f.py;
    for (uint32_t o = 0; o < f.octaves; ++o) {
        const TurbulenceAxis x = turbulence_axis<STITCH>(vx, px, inv_px);
        const uint32_t a0 = lattice[x.b0], a1 = lattice[x.b1];
#pragma unroll
        for (int b = 0; b < kTurbulenceRows; ++b) {
            const TurbulenceAxis y = turbulence_axis<STITCH>(vy[b], py, inv_py);
            turbulence_add<KIND, CH>(lattice, gradient, a0, a1, x, y, inv_ratio, &sums[b]);
            vy[b] = vy[b] * 2.0;
        }
        vx = vx * 2.0;
        inv_ratio = inv_ratio * 0.5, inv_px = inv_px * 0.5, inv_py = inv_py * 0.5;
        px <<= 1, py <<= 1;
    }
    if (i < w) {
#pragma unroll
        for (int b = 0; b < kTurbulenceRows; ++b) {
            const uint32_t j = j0 + (uint32_t)b;
            if (j < h) out[(size_t)j * w + i] = turbulence_texel<KIND, CH>(sums[b]);
        }
    }
}

void launch_image_turbulence(const TurbulenceTables* tables, uint32_t w, uint32_t h, const TurbulenceConstants& f, uint32_t kind, bool opaque, uint32_t* out, hipStream_t stream) {
    const dim3 grid = TurbulenceTile::grid(w, h), block(TurbulenceTile::Lanes);
    const bool stitch = f.px != 0 || f.py != 0;
#define CRH_TURBULENCE_LAUNCH(KIND, OPAQUE)                                                                                                 \
    do {                                                                                                                                    \
        if (stitch) hipLaunchKernelGGL((k_image_turbulence<KIND, OPAQUE, true>), grid, block, 0, stream, tables, w, h, f, out);             \
        else hipLaunchKernelGGL((k_image_turbulence<KIND, OPAQUE, false>), grid, block, 0, stream, tables, w, h, f, out);                  \
    } while (0)
    if (kind == kTurbulenceFractalNoise) {
        if (opaque) CRH_TURBULENCE_LAUNCH(kTurbulenceFractalNoise, true);
        else CRH_TURBULENCE_LAUNCH(kTurbulenceFractalNoise, false);
    } else {
        if (opaque) CRH_TURBULENCE_LAUNCH(kTurbulenceTurbulence, true);
        else CRH_TURBULENCE_LAUNCH(kTurbulenceTurbulence, false);
    }
#undef CRH_TURBULENCE_LAUNCH
}

namespace {
#ifndef CRH_DISPLACE_ROWS
#define CRH_DISPLACE_ROWS 4 // (a build with -DCRH_DISPLACE_ROWS=1, 2 or 8 is how DESIGN.md's comparison of the row blocking is measured)
#endif
#ifndef CRH_DISPLACE_EDGE_TEMPLATE
#define CRH_DISPLACE_EDGE_TEMPLATE 0 // (a build with -DCRH_DISPLACE_EDGE_TEMPLATE=1 instantiates the kernel per wrapping edge: DESIGN.md's comparison)
#endif
typedef Tile<CRH_DISPLACE_ROWS> DisplaceTile; // adjacent output rows per lane: their fetches are in flight together
constexpr int kDisplaceRows = DisplaceTile::Rows;
constexpr uint32_t kDisplaceRuntimeEdge = 4; // EDGE of the kernel that takes its wrapping edge (1..3) from the constants

// One index of a tap against its axis of n texels -> an index the lane may read, and whether the tap is the source's texel there: always
// under a wrapping edge; under TRANSPARENT the index is clamped and the test says whether the value counts.
template <bool WRAPPED>
__device__ __forceinline__ uint32_t displace_index(int i, int n, uint32_t edge, bool* inside) {
    if (WRAPPED) {
        *inside = true;
        return (uint32_t)edge_wrap_branching(i, n, edge);
    }
    *inside = (uint32_t)i < (uint32_t)n;
    return (uint32_t)(i < 0 ? 0 : i >= n ? n - 1 : i);
}
} // namespace

// crh_image_displace: a data-dependent gather, bound by the latency of its fetches, on a tile of 64 x 16 texels (image_geometry.hpp: Tile):
// a wave's map load and its store are 256 contiguous bytes per instruction and only the source read is a gather. No halo can be staged:
// an offset reaches 512 texels either way. A lane works in four steps so that its loads are in flight together: (1) the map texels of
// its rows; (2) per row the offsets by displace.hpp's rule (the unpremultiply's 256 reciprocals are in LDS, one word staged per lane),
// the taps, and for each tap a texel index formed ONLY from wrapped (edge_wrap_branching) or clamped indices, with under TRANSPARENT a bit that
// says whether the tap lies inside; (3) all fetches, 4 per row under LINEAR and 1 under NEAREST — 16 or 4 loads issued before the first
// is consumed; (4) the taps outside zeroed, the blend, the store. A lane outside the image reads the map's last column or row, computes
// like any other and does not store. Every index is below w h <= 2^28. EDGE = 0 is TRANSPARENT, 1..3 a wrapping edge as a constant,
// kDisplaceRuntimeEdge the wrapping edge of the constants (wave-uniform: the wrap branches on an SGPR).
template <uint32_t FILTER, uint32_t EDGE>
__global__ __launch_bounds__(DisplaceTile::Lanes) void k_image_displace(const uint32_t* __restrict__ src, const uint32_t* __restrict__ map, uint32_t w, uint32_t h, DisplaceConstants f,
                                                                                    uint32_t* __restrict__ out) {
    constexpr int TAPS = FILTER == kDisplaceLinear ? 4 : 1;
    constexpr bool WRAPPED = EDGE != kDisplaceTransparent;
    __shared__ uint32_t recip[256];
    recip[threadIdx.x] = k_unpremultiply.r[threadIdx.x];
    __syncthreads();
    const uint32_t edge = EDGE == kDisplaceRuntimeEdge ? f.edge : EDGE;
    const DisplaceTile tile;
    const uint32_t i = tile.column(), j0 = tile.row();
    const uint32_t column = i < w ? i : w - 1u;
    uint32_t m[kDisplaceRows];
#pragma unroll
    for (int b = 0; b < kDisplaceRows; ++b) {
        const uint32_t j = j0 + (uint32_t)b;
        m[b] = map[(j < h ? j : h - 1u) * w + column];
    }
    DisplaceTaps taps[kDisplaceRows];
    uint32_t at[kDisplaceRows][TAPS], inside[kDisplaceRows];
#pragma unroll
    for (int b = 0; b < kDisplaceRows; ++b) {
        int32_t q[2];
        displace_offsets(m[b], f, recip, q);
        taps[b] = displace_taps<FILTER>(displace_position(i, q[0]), displace_position(j0 + (uint32_t)b, q[1]));
        bool in_x0, in_y0;
        const uint32_t x0 = displace_index<WRAPPED>(taps[b].i0, (int)w, edge, &in_x0), y0 = displace_index<WRAPPED>(taps[b].j0, (int)h, edge, &in_y0) * w;
        at[b][0] = y0 + x0, inside[b] = in_x0 && in_y0 ? 1u : 0u;
        if constexpr (FILTER == kDisplaceLinear) {
            bool in_x1, in_y1;
            const uint32_t x1 = displace_index<WRAPPED>(taps[b].i0 + 1, (int)w, edge, &in_x1), y1 = displace_index<WRAPPED>(taps[b].j0 + 1, (int)h, edge, &in_y1) * w;
            at[b][1] = y0 + x1, at[b][2] = y1 + x0, at[b][3] = y1 + x1;
            inside[b] |= (in_x1 && in_y0 ? 2u : 0u) | (in_x0 && in_y1 ? 4u : 0u) | (in_x1 && in_y1 ? 8u : 0u);
        }
    }
    uint32_t s[kDisplaceRows][TAPS];
#pragma unroll
    for (int b = 0; b < kDisplaceRows; ++b)
#pragma unroll
        for (int t = 0; t < TAPS; ++t) s[b][t] = src[at[b][t]];
    if (i >= w) return;
#pragma unroll
    for (int b = 0; b < kDisplaceRows; ++b) {
        const uint32_t j = j0 + (uint32_t)b;
        if (!WRAPPED) {
#pragma unroll
            for (int t = 0; t < TAPS; ++t) s[b][t] = (inside[b] >> t) & 1u ? s[b][t] : 0u;
        }
        if (j < h) out[j * w + i] = displace_blend<FILTER>(s[b], taps[b]);
    }
}

void launch_image_displace(const uint32_t* src, const uint32_t* map, uint32_t w, uint32_t h, const DisplaceConstants& f, uint32_t* out, hipStream_t stream) {
    const dim3 grid = DisplaceTile::grid(w, h), block(DisplaceTile::Lanes);
#define CRH_DISPLACE_LAUNCH(EDGE)                                                                                                              \
    do {                                                                                                                                       \
        if (f.filter == kDisplaceLinear) hipLaunchKernelGGL((k_image_displace<kDisplaceLinear, EDGE>), grid, block, 0, stream, src, map, w, h, f, out); \
        else hipLaunchKernelGGL((k_image_displace<kDisplaceNearest, EDGE>), grid, block, 0, stream, src, map, w, h, f, out);                    \
    } while (0)
    if (f.edge == kDisplaceTransparent) CRH_DISPLACE_LAUNCH(kDisplaceTransparent);
#if CRH_DISPLACE_EDGE_TEMPLATE
    else if (f.edge == 1u) CRH_DISPLACE_LAUNCH(1u);
    else if (f.edge == 2u) CRH_DISPLACE_LAUNCH(2u);
    else CRH_DISPLACE_LAUNCH(3u);
#else
    else CRH_DISPLACE_LAUNCH(kDisplaceRuntimeEdge);
#endif
#undef CRH_DISPLACE_LAUNCH
}

namespace {
#ifndef CRH_TRANSFORM_BLOCK
#define CRH_TRANSFORM_BLOCK 8 // texels of one output row per wave instruction: 64 (the displace tile), 16 or 8 (a build with -DCRH_TRANSFORM_BLOCK=64 or 16 is how DESIGN.md's comparison of the lane mappings is measured)
#endif
#ifndef CRH_TRANSFORM_ROWS
#define CRH_TRANSFORM_ROWS 4 // outputs per lane, BH rows apart: their fetches are in flight together under NEAREST and LINEAR
#endif
// Block tile. 256 lanes, four waves; a wave instruction covers BW x BH texels, BW BH = 64: lane l the texel (l % BW, l / BW) of the block, so
// that the source footprint of a wave's fetch is compact under any angle: under a quarter turn 64 lanes of one output row read 64 source
// rows, BW x BH lanes read BH segments of BW texels in BW rows. A lane produces ROWS outputs of one column, BH rows apart: a wave BW x BH ROWS
// texels. The waves lie side by side while the tile is narrower than 64 texels and one below the other from there: BW = 64 is
// image_geometry.hpp's Tile<ROWS> lane for lane, BW = 16 a tile of 64 x 4 ROWS, BW = 8 one of 32 x 8 ROWS. A wave's store is BH segments
// of 4 BW bytes. The wave is in an SGPR.
template <int BW, int ROWS>
struct BlockTile {
    static constexpr int BH = 64 / BW, WavesX = BW >= 64 ? 1 : 4, WavesY = 4 / WavesX, Rows = ROWS, W = BW * WavesX, H = BH * ROWS * WavesY, Lanes = 256;
    static_assert(BW * BH == 64 && WavesX * WavesY == 4, "a wave instruction is one block; four waves");
    uint32_t i, j0;
    __device__ __forceinline__ BlockTile() {
        const uint32_t lane = threadIdx.x & 63u, wave = wave_of_workgroup();
        i = blockIdx.x * (uint32_t)W + (wave % (uint32_t)WavesX) * (uint32_t)BW + lane % (uint32_t)BW;
        j0 = blockIdx.y * (uint32_t)H + (wave / (uint32_t)WavesX) * (uint32_t)(BH * ROWS) + lane / (uint32_t)BW;
    }
    __device__ __forceinline__ uint32_t column() const { return i; }                           // the lane's output column
    __device__ __forceinline__ uint32_t row(int b) const { return j0 + (uint32_t)(b * BH); }   // its b-th output row
    static dim3 grid(uint32_t w, uint32_t h) { return dim3((w + (uint32_t)W - 1u) / (uint32_t)W, (h + (uint32_t)H - 1u) / (uint32_t)H); } // <= 512 x 1024
};
typedef BlockTile<CRH_TRANSFORM_BLOCK, CRH_TRANSFORM_ROWS> TransformTile;
constexpr int kTransformRows = TransformTile::Rows;
__device__ const TransformCubicTable k_transform_cubic{}; // transform.hpp's weights, staged in LDS by every workgroup of the CUBIC kernel
} // namespace

// crh_image_transform: a gather bound by the latency of its fetches, like k_image_displace and in its four steps, on a block tile
// (BlockTile above). No map is read: (1) a lane's positions, each computed from (i, j) alone by transform.hpp's rule — six binary64
// multiply-adds, under PROJECTIVE three more and two divisions; no stepping from a neighbour, so every texel has the rule's bits; (2) the
// taps, and for each tap a texel index formed ONLY from wrapped (edge_wrap_branching) or clamped indices of the SOURCE's axes, with under
// TRANSPARENT a bit that says whether the tap lies inside; (3) all fetches — under NEAREST and LINEAR those of all the lane's rows, 4 or 16
// loads, under CUBIC the 16 of one row at a time — issued before the first is consumed; (4) the taps outside zeroed, the blend
// (displace_blend, or transform_cubic_blend with the weights of the two phases from the table in LDS, one 8-byte entry staged per lane),
// zero for a texel behind the horizon, the store. A lane outside the result computes like any other (its position clamps, its indices are
// wrapped or clamped) and does not store. Every index is below src_w src_h <= 2^28. EDGE as in k_image_displace.
template <uint32_t FILTER, uint32_t EDGE, bool PROJECTIVE>
__global__ __launch_bounds__(TransformTile::Lanes) void k_image_transform(const uint32_t* __restrict__ src, uint32_t sw, uint32_t sh, TransformConstants f, uint32_t* __restrict__ out, uint32_t w,
                                                                                     uint32_t h) {
    constexpr bool WRAPPED = EDGE != kTransformTransparent;
    const uint32_t edge = EDGE == kDisplaceRuntimeEdge ? f.edge : EDGE;
    const TransformTile tile;
    const uint32_t i = tile.column();
    if constexpr (FILTER == kTransformCubic) {
        __shared__ uint2 cubic[256];
        cubic[threadIdx.x] = reinterpret_cast<const uint2*>(k_transform_cubic.c)[threadIdx.x];
        __syncthreads();
#pragma unroll
        for (int b = 0; b < kTransformRows; ++b) {
            const uint32_t j = tile.row(b);
            int32_t X, Y;
            const bool visible = transform_position<PROJECTIVE>(f.m, i, j, &X, &Y);
            const TransformCubicTaps t = transform_cubic_taps(X, Y);
            uint32_t x[4], y[4], inside = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool in_x, in_y;
                x[k] = displace_index<WRAPPED>(t.i0 - 1 + k, (int)sw, edge, &in_x), y[k] = displace_index<WRAPPED>(t.j0 - 1 + k, (int)sh, edge, &in_y) * sw;
                inside |= (in_x ? 1u : 0u) << k | (in_y ? 16u : 0u) << k;
            }
            uint32_t s[16];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) s[4 * r + k] = src[y[r] + x[k]];
            if (!WRAPPED) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[4 * r + k] = (inside >> k) & (inside >> (4 + r)) & 1u ? s[4 * r + k] : 0u;
            }
            const uint2 px = cubic[t.fx], py = cubic[t.fy];
            const int16_t cx[4] = {(int16_t)px.x, (int16_t)(px.x >> 16), (int16_t)px.y, (int16_t)(px.y >> 16)}, cy[4] = {(int16_t)py.x, (int16_t)(py.x >> 16), (int16_t)py.y, (int16_t)(py.y >> 16)};
            const uint32_t value = transform_cubic_blend(s, cx, cy);
            if (i < w && j < h) out[j * w + i] = visible ? value : 0u;
        }
    } else {
        constexpr int TAPS = FILTER == kTransformLinear ? 4 : 1;
        DisplaceTaps taps[kTransformRows];
        uint32_t at[kTransformRows][TAPS], inside[kTransformRows];
        bool visible[kTransformRows];
#pragma unroll
        for (int b = 0; b < kTransformRows; ++b) {
            int32_t X, Y;
            visible[b] = transform_position<PROJECTIVE>(f.m, i, tile.row(b), &X, &Y);
            taps[b] = displace_taps<FILTER>(X, Y);
            bool in_x0, in_y0;
            const uint32_t x0 = displace_index<WRAPPED>(taps[b].i0, (int)sw, edge, &in_x0), y0 = displace_index<WRAPPED>(taps[b].j0, (int)sh, edge, &in_y0) * sw;
            at[b][0] = y0 + x0, inside[b] = in_x0 && in_y0 ? 1u : 0u;
            if constexpr (FILTER == kTransformLinear) {
                bool in_x1, in_y1;
                const uint32_t x1 = displace_index<WRAPPED>(taps[b].i0 + 1, (int)sw, edge, &in_x1), y1 = displace_index<WRAPPED>(taps[b].j0 + 1, (int)sh, edge, &in_y1) * sw;
                at[b][1] = y0 + x1, at[b][2] = y1 + x0, at[b][3] = y1 + x1;
                inside[b] |= (in_x1 && in_y0 ? 2u : 0u) | (in_x0 && in_y1 ? 4u : 0u) | (in_x1 && in_y1 ? 8u : 0u);
            }
        }
        uint32_t s[kTransformRows][TAPS];
#pragma unroll
        for (int b = 0; b < kTransformRows; ++b)
#pragma unroll
            for (int t = 0; t < TAPS; ++t) s[b][t] = src[at[b][t]];
        if (i >= w) return;
#pragma unroll
        for (int b = 0; b < kTransformRows; ++b) {
            const uint32_t j = tile.row(b);
            if (!WRAPPED) {
#pragma unroll
                for (int t = 0; t < TAPS; ++t) s[b][t] = (inside[b] >> t) & 1u ? s[b][t] : 0u;
            }
            if (j < h) out[j * w + i] = visible[b] ? displace_blend<FILTER>(s[b], taps[b]) : 0u;
        }
    }
}

void launch_image_transform(const uint32_t* src, uint32_t src_w, uint32_t src_h, const TransformConstants& f, uint32_t* out, uint32_t w, uint32_t h, hipStream_t stream) {
    const dim3 grid = TransformTile::grid(w, h), block(TransformTile::Lanes);
#define CRH_TRANSFORM_LAUNCH(FILTER, EDGE)                                                                                                             \
    do {                                                                                                                                               \
        if (f.projective) hipLaunchKernelGGL((k_image_transform<FILTER, EDGE, true>), grid, block, 0, stream, src, src_w, src_h, f, out, w, h);        \
        else hipLaunchKernelGGL((k_image_transform<FILTER, EDGE, false>), grid, block, 0, stream, src, src_w, src_h, f, out, w, h);                    \
    } while (0)
#define CRH_TRANSFORM_LAUNCH_EDGE(FILTER)                                                      \
    do {                                                                                       \
        if (f.edge == kTransformTransparent) CRH_TRANSFORM_LAUNCH(FILTER, kTransformTransparent); \
        else CRH_TRANSFORM_LAUNCH(FILTER, kDisplaceRuntimeEdge);                               \
    } while (0)
    if (f.filter == kTransformCubic) CRH_TRANSFORM_LAUNCH_EDGE(kTransformCubic);
    else if (f.filter == kTransformLinear) CRH_TRANSFORM_LAUNCH_EDGE(kTransformLinear);
    else CRH_TRANSFORM_LAUNCH_EDGE(kTransformNearest);
#undef CRH_TRANSFORM_LAUNCH_EDGE
#undef CRH_TRANSFORM_LAUNCH
}

namespace {
constexpr int kDistanceColumns = 64;   // vertical: columns per workgroup, one per lane of its single wave
constexpr int kDistanceSegment = 256;  // horizontal: output texels of one row per workgroup, one per lane (k_image_morph_h's segment)
constexpr int kDistanceApron = 255;    // CRH_MAX_DISTANCE_SPREAD: column distances staged beyond the segment on either side
constexpr int kDistanceOwned = (kDistanceSegment + 2 * kDistanceApron + kDistanceSegment - 1) / kDistanceSegment; // 3: staged bytes per lane
static_assert(kDistanceApron == (int)kDistanceMaxSpread, "the apron holds the largest spread");
} // namespace

// Vertical pass: the source to g, one byte per texel of the result: the distance along the column to the nearest target (distance.hpp:
// a texel inside the shape for OUTSIDE, one that is not for INSIDE), 0 .. spread - 1, or 255 where there is none within reach. Grid
// (ceil(out_w / 64), ceil(out_h / ROWS)), one wave: lanes run along x, so every global and LDS access of the wave is 64 consecutive
// words or bytes. The workgroup owns the output rows j0 .. j0 + ROWS - 1 of 64 columns. A lane first walks its column UP, from
// spread - 1 rows below its last row to its first, counting the rows since the last target, and stores the count of each of its own rows
// in LDS (its own byte: no lane reads another's, so no barrier; a count of 0 is a target); then DOWN from spread - 1 rows above its
// first row, counting again, over its own rows from the LDS bytes alone: g is the smaller of the two counts. ROWS + 2 (spread - 1) rows
// read for ROWS outputs, at any ROWS; the launcher takes 32 rows for spreads up to 16 and 128 above. `origin`: the source texel
// under result texel (0, 0) is (-origin, -origin) (the spread for a growing result, else 0). The row index is wave-uniform: the wrap is
// scalar arithmetic, its one remainder per walk is taken at the walk's first row (edge.hpp's phase), and the address always comes
// from a wrapped or clamped row and column, so the loads of an unrolled stretch are unconditional and in flight together.
template <bool INSIDE, int ROWS>
__global__ __launch_bounds__(kDistanceColumns) void k_image_distance_v(const uint32_t* __restrict__ src, uint32_t src_w, uint32_t src_h, uint8_t* __restrict__ g, uint32_t out_w, uint32_t out_h,
                                                                        uint32_t origin, DistanceConstants f) {
    __shared__ uint8_t below[ROWS][kDistanceColumns];
    constexpr uint32_t MODE = INSIDE ? kDistanceInside : kDistanceOutside;
    const uint32_t lane = threadIdx.x, x = blockIdx.x * (uint32_t)kDistanceColumns + lane;
    if (x >= out_w) return; // (no barrier below: a lane shares nothing with its neighbours)
    const uint32_t j0 = blockIdx.y * (uint32_t)ROWS;
    const uint32_t rows = out_h - j0 < (uint32_t)ROWS ? out_h - j0 : (uint32_t)ROWS; // (j0 < out_h by the grid): every LDS index is below ROWS
    const uint32_t reach = (f.spread < kDistanceMaxSpread ? f.spread : kDistanceMaxSpread) - 1u;
    const int n = (int)src_h, period = edge_period(n, f.edge);
    const int xs = (int)x - (int)origin;
    const bool in_x = f.edge != kDistanceTransparent || (uint32_t)xs < src_w;
    const uint32_t* column = src + edge_wrap(xs, (int)src_w, f.edge); // (TRANSPARENT clamps: an address the lane may read)
    auto target_of = [&](int i, int phase) {
        const uint32_t texel = column[(size_t)edge_wrap_at(i, phase, n, f.edge) * src_w];
        const bool inside = distance_inside(texel, f) && (f.edge != kDistanceTransparent || ((uint32_t)i < src_h && in_x));
        return distance_target(inside, MODE);
    };
    const int first = (int)j0 - (int)origin, last = first + (int)rows - 1; // the source rows under the workgroup's first and last row
    uint32_t d = kDistanceNone;
    int i = last + (int)reach, phase = edge_phase(i, n, f.edge);
#pragma unroll 8
    for (uint32_t k = 0u; k < reach; ++k, --i) {
        d = distance_step(d, target_of(i, phase));
        phase = edge_phase_before(phase, period);
    }
#pragma unroll 8
    for (uint32_t m = rows; m-- > 0u; --i) {
        d = distance_step(d, target_of(i, phase));
        phase = edge_phase_before(phase, period);
        below[m][lane] = (uint8_t)d;
    }
    d = kDistanceNone;
    i = first - (int)reach, phase = edge_phase(i, n, f.edge);
#pragma unroll 8
    for (uint32_t k = 0u; k < reach; ++k, ++i) {
        d = distance_step(d, target_of(i, phase));
        phase = edge_phase_next(phase, period);
    }
    for (uint32_t m = 0u; m < rows; ++m) {
        const uint32_t b = below[m][lane];
        d = distance_step(d, b == 0u);
        g[(size_t)(j0 + m) * out_w + x] = (uint8_t)distance_column(d < b ? d : b, f.spread);
    }
}

// Horizontal pass: g to the result, D2(x, y) = min over dx of dx^2 + g(x + dx, y)^2. Grid (ceil(out_w / 256), out_h), 256 lanes: the
// workgroup stages the 256 + 2 spread bytes of g its segment of one row reads (at most 766, lane l the bytes l, l + 256 and l + 512) and
// the 255 thresholds of the spread (distance.hpp; made on the host, one word per lane). Under a same-size edge a column outside the
// row is read through the wrap; under TRANSPARENT it is "none" (OUTSIDE: nothing out there) or 0 (INSIDE: off the image is off the
// shape). A segment whose staged bytes are all "none" writes its bytes without scanning (the barrier that publishes the bytes also
// votes). Otherwise a lane scans dx = 0, 1, .. and stops as soon as dx^2 reaches the best value found (distance_scan): two LDS bytes at
// lane +- dx per step, consecutive lanes consecutive bytes; neighbouring texels' distances differ by at most one, so a wave's lanes
// stop within a few steps of each other. Then c(D2) by eight halvings over the thresholds in LDS: no square root. Every LDS index is
// lane + spread +- dx with dx < spread, inside the staged bytes; every address of g comes from a wrapped or range-checked column.
template <bool INSIDE>
__global__ __launch_bounds__(kDistanceSegment) void k_image_distance_h(const uint8_t* __restrict__ g, uint32_t out_w, const uint32_t* __restrict__ thresholds, DistanceConstants f,
                                                                        uint32_t* __restrict__ out) {
    __shared__ uint8_t staged[kDistanceOwned * kDistanceSegment];
    __shared__ uint32_t codes[256];
    constexpr uint32_t MODE = INSIDE ? kDistanceInside : kDistanceOutside;
    const uint32_t j = blockIdx.y, o0 = blockIdx.x * (uint32_t)kDistanceSegment, lane = threadIdx.x;
    const uint32_t spread = f.spread < kDistanceMaxSpread ? f.spread : kDistanceMaxSpread; // (the host refuses more: the bound keeps every LDS index staged)
    const uint8_t* row = g + (size_t)j * out_w;
    const uint32_t n_staged = (uint32_t)kDistanceSegment + 2u * spread;
    const int first = (int)o0 - (int)spread; // the column of staged byte 0
    codes[lane] = thresholds[lane];
    int any = 0;
#pragma unroll
    for (int t = 0; t < kDistanceOwned; ++t) {
        const uint32_t at = lane + (uint32_t)(t * kDistanceSegment);
        if (at < n_staged) {
            const int i = first + (int)at;
            uint32_t v = INSIDE ? 0u : kDistanceNone;
            if (f.edge != kDistanceTransparent) v = row[edge_wrap(i, (int)out_w, f.edge)];
            else if ((uint32_t)i < out_w) v = row[i];
            staged[at] = (uint8_t)v;
            any |= v != kDistanceNone;
        }
    }
    const bool scan = __syncthreads_or(any) != 0;
    const uint32_t o = o0 + lane;
    if (o >= out_w) return;
    uint32_t c = 255u; // nothing within the spread
    if (scan) {
        const uint8_t* centre = staged + lane + spread;
        c = distance_code(codes, distance_scan(spread, [&](int dx) -> uint32_t { return centre[dx]; }));
    }
    out[(size_t)j * out_w + o] = distance_texel(c, MODE);
}

void launch_image_distance_v(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint8_t* g, uint32_t out_w, uint32_t out_h, uint32_t origin, const DistanceConstants& f, hipStream_t stream) {
    const uint32_t columns = (out_w + (uint32_t)kDistanceColumns - 1u) / (uint32_t)kDistanceColumns;
#define CRH_DISTANCE_V_LAUNCH(ROWS)                                                                                                                                                  \
    do {                                                                                                                                                                             \
        const dim3 grid(columns, (out_h + (ROWS) - 1u) / (ROWS)); /* <= 256 x 512 */                                                                                                 \
        if (f.mode == kDistanceInside) hipLaunchKernelGGL((k_image_distance_v<true, ROWS>), grid, dim3(kDistanceColumns), 0, stream, src, src_w, src_h, g, out_w, out_h, origin, f); \
        else hipLaunchKernelGGL((k_image_distance_v<false, ROWS>), grid, dim3(kDistanceColumns), 0, stream, src, src_w, src_h, g, out_w, out_h, origin, f);                          \
    } while (0)
    if (f.spread <= 16u) CRH_DISTANCE_V_LAUNCH(32);
    else CRH_DISTANCE_V_LAUNCH(128); // (more workgroups beat fewer rows read: 256 and 512 rows were measured at spread 255 and dropped)
#undef CRH_DISTANCE_V_LAUNCH
}

void launch_image_distance_h(const uint8_t* g, uint32_t out_w, uint32_t out_h, const uint32_t* thresholds, const DistanceConstants& f, uint32_t* out, hipStream_t stream) {
    const dim3 grid((out_w + (uint32_t)kDistanceSegment - 1u) / (uint32_t)kDistanceSegment, out_h); // out_h <= 16384 rows: below the grid's limit of 65535
    if (f.mode == kDistanceInside) hipLaunchKernelGGL(k_image_distance_h<true>, grid, dim3(kDistanceSegment), 0, stream, g, out_w, thresholds, f, out);
    else hipLaunchKernelGGL(k_image_distance_h<false>, grid, dim3(kDistanceSegment), 0, stream, g, out_w, thresholds, f, out);
}

namespace {
constexpr int kResizeRows = 64;     // horizontal: source rows per workgroup, one per lane of a wave
constexpr int kResizeWaves = 4;     // waves per workgroup, both passes
constexpr int kResizeGroup = 32;    // horizontal: output columns per workgroup
constexpr int kResizePerWave = kResizeGroup / kResizeWaves; // horizontal: output columns per wave, each four accumulators per lane
constexpr int kResizeChunk = 64;    // horizontal: source columns staged in LDS at a time; even, so a tap pair never straddles two chunks
constexpr int kResizeColumns = 64;  // vertical: columns per workgroup, one per lane of a wave
constexpr int kResizeBlockRows = 32; // vertical: output rows per workgroup, eight per wave
static_assert(kResizeChunk == kResizeColumns && kResizeRows == kResizeColumns && kResizeChunk % 2 == 0 && kResizeGroup % kResizeWaves == 0 && kResizeBlockRows % kResizeWaves == 0, "resize tiles");

typedef short i16x2 __attribute__((ext_vector_type(2)));
// acc + v.i16[0] * q.i16[0] + v.i16[1] * q.i16[1] in signed 32 bits (v_dot2_i32_i16): two taps of one channel per instruction
__device__ __forceinline__ int32_t sdot2(uint32_t v, uint32_t q, int32_t acc) { return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, v), __builtin_bit_cast(i16x2, q), acc, false); }
// byte k of two texels as two 16-bit fields, (a.u8[k], b.u8[k]): one v_perm_b32 (selector 0x0C = a zero byte)
template <int K> __device__ __forceinline__ uint32_t channel_pair(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x0C040C00u + (uint32_t)K * 0x00010001u); }
} // namespace

// crh_image_resize, horizontal pass: the source to the intermediate, four 16-bit values per texel, the result's width and the source's
// height (resize.hpp: the rule, and the layout of `table`, whose windows start on an even column and hold an even number of taps).
// The taps differ per output COLUMN, so lanes run along y: grid (ceil(out_w / 32), ceil(src_h / 64)), 4 waves. A workgroup owns 32 output
// columns of 64 rows; wave w owns columns 8 w .. 8 w + 7 of them, lane l row l: an output column's first index, count and taps are
// wave-uniform and come through the scalar cache. The source columns the 32 outputs read — from the first window's start to the last
// window's end; both rise with the output — are staged 64 at a time, TRANSPOSED: wave w loads rows w, w + 4, .. with lanes along x (64
// consecutive words) and writes tile[column][row], 65 words per column, so the stores and the reads tile[column][lane] are both
// conflict-free. A column beyond the source (only the one under a padding zero tap) and the columns beyond the span are staged as
// zeros, a row beyond the source repeats the last row and is never stored. Per chunk a wave adds, for each of its 8 outputs, the part of
// the window inside the chunk: a tap pair is one scalar word, two LDS words, four v_perm_b32 that regroup the two texels by channel and
// four v_dot2_i32_i16. The 32 accumulators live across chunks (an output's window may span up to nine of them). The results go back
// through LDS, so a row's 32 outputs leave as 256 consecutive bytes. Every global address is (a row clamped to src_h - 1) * src_w + (a
// column tested against src_w); every LDS column index is below 64: chunk + 64 bounds the inner loop, and pairs are even-aligned.
__global__ __launch_bounds__(kResizeColumns * kResizeWaves) void k_image_resize_h(const uint32_t* __restrict__ src, uint32_t src_w, uint32_t src_h, uint2* __restrict__ tmp, uint32_t out_w,
                                                                                  const uint32_t* __restrict__ table, uint32_t pairs) {
    __shared__ uint32_t tile[kResizeChunk][kResizeRows + 1];
    __shared__ uint2 done[kResizeRows][kResizeGroup + 1];
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t o0 = blockIdx.x * (uint32_t)kResizeGroup, j0 = blockIdx.y * (uint32_t)kResizeRows;
    const uint32_t o_last = min(o0 + (uint32_t)kResizeGroup, out_w) - 1u; // (o0 < out_w by the grid)
    const uint32_t* first = table;
    const uint32_t* count = table + out_w;
    const uint32_t* taps = table + 2u * (size_t)out_w;
    const uint32_t span_lo = first[o0], span_hi = first[o_last] + count[o_last]; // both even; span_hi <= src_w + 1
    int32_t acc[kResizePerWave][4];
#pragma unroll
    for (int k = 0; k < kResizePerWave; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
    for (uint32_t chunk = span_lo; chunk < span_hi; chunk += (uint32_t)kResizeChunk) {
        const uint32_t chunk_hi = min(chunk + (uint32_t)kResizeChunk, span_hi); // even
        __syncthreads(); // (the columns of the chunk before have been read)
        for (uint32_t r = wave; r < (uint32_t)kResizeRows; r += (uint32_t)kResizeWaves) {
            const uint32_t row = min(j0 + r, src_h - 1u), column = chunk + lane;
            uint32_t texel = 0u;
            if (column < chunk_hi && column < src_w) texel = src[(size_t)row * src_w + column];
            tile[lane][r] = texel;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kResizePerWave; ++k) {
            const uint32_t o = o0 + wave * (uint32_t)kResizePerWave + (uint32_t)k; // wave-uniform
            if (o > o_last) break;
            const uint32_t f = first[o], from = max(f, chunk), to = min(f + count[o], chunk_hi); // all even
            const uint32_t* q = taps + (size_t)o * pairs;
            for (uint32_t i = from; i < to; i += 2u) {
                const uint32_t qq = q[(i - f) >> 1];
                const uint32_t a = tile[i - chunk][lane], b = tile[i - chunk + 1u][lane];
                acc[k][0] = sdot2(channel_pair<0>(a, b), qq, acc[k][0]), acc[k][1] = sdot2(channel_pair<1>(a, b), qq, acc[k][1]);
                acc[k][2] = sdot2(channel_pair<2>(a, b), qq, acc[k][2]), acc[k][3] = sdot2(channel_pair<3>(a, b), qq, acc[k][3]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kResizePerWave; ++k)
        done[lane][wave * (uint32_t)kResizePerWave + (uint32_t)k] =
            make_uint2(resize_intermediate(acc[k][0]) | resize_intermediate(acc[k][1]) << 16, resize_intermediate(acc[k][2]) | resize_intermediate(acc[k][3]) << 16);
    __syncthreads();
    const uint32_t column = threadIdx.x % (uint32_t)kResizeGroup, o = o0 + column;
    for (uint32_t r = threadIdx.x / (uint32_t)kResizeGroup; r < (uint32_t)kResizeRows; r += (uint32_t)(kResizeColumns * kResizeWaves / kResizeGroup))
        if (o < out_w && j0 + r < src_h) tmp[(size_t)(j0 + r) * out_w + o] = done[r][column];
}

// crh_image_resize, vertical pass: the intermediate to the result. Grid (ceil(out_w / 64), ceil(out_h / 32)), 4 waves: lanes run along x, so
// every global access of a wave is 64 consecutive 8- or 4-byte words, and an output row's first index, count and taps are wave-uniform
// and come through the scalar cache. Wave w owns the output rows w, w + 4, .. w + 28 of the workgroup's 32, so the four waves walk through
// the intermediate together: neighbouring output rows' windows overlap by the factor 2 r when minifying and coincide when magnifying, and
// the overlap is served by the CU's vector cache, not staged. The rows of a window are taken in pairs: the 16-bit values are biased to
// signed (t - 32768: one v_xor_b32 per word), the two rows regrouped by channel (four v_perm_b32) and each channel takes both taps in one
// v_dot2_i32_i16. The taps sum to 16384, so the biased sum is the true one minus 2^29, |.| <= 32768 * 32768; 2^29 goes back on before
// the rounding. The second row of a pair is clamped to tmp_h - 1: it is one past the source only under a padding zero tap. Every address
// is (a row below tmp_h) * out_w + (a column clamped to out_w - 1); the store is behind the column's test.
__global__ __launch_bounds__(kResizeColumns * kResizeWaves) void k_image_resize_v(const uint2* __restrict__ tmp, uint32_t tmp_h, uint32_t* __restrict__ out, uint32_t out_w, uint32_t out_h,
                                                                                  const uint32_t* __restrict__ table, uint32_t pairs) {
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t x = blockIdx.x * (uint32_t)kResizeColumns + lane, xc = min(x, out_w - 1u);
    const uint32_t* first = table;
    const uint32_t* count = table + out_h;
    const uint32_t* taps = table + 2u * (size_t)out_h;
    for (uint32_t i = blockIdx.y * (uint32_t)kResizeBlockRows + wave; i < min((blockIdx.y + 1u) * (uint32_t)kResizeBlockRows, out_h); i += (uint32_t)kResizeWaves) {
        const uint32_t f = first[i], n = count[i] >> 1;
        const uint32_t* q = taps + (size_t)i * pairs;
        int32_t r = 0, g = 0, b = 0, a = 0;
#pragma unroll 2
        for (uint32_t p = 0; p < n; ++p) {
            const uint32_t row0 = f + 2u * p, row1 = min(row0 + 1u, tmp_h - 1u); // row0 <= tmp_h - 1: a window's first tap of a pair is inside the source
            const uint2 t0 = tmp[(size_t)row0 * out_w + xc], t1 = tmp[(size_t)row1 * out_w + xc];
            const uint32_t rg0 = t0.x ^ 0x80008000u, ba0 = t0.y ^ 0x80008000u, rg1 = t1.x ^ 0x80008000u, ba1 = t1.y ^ 0x80008000u;
            const uint32_t qq = q[p];
            r = sdot2(low_halves(rg0, rg1), qq, r), g = sdot2(high_halves(rg0, rg1), qq, g);
            b = sdot2(low_halves(ba0, ba1), qq, b), a = sdot2(high_halves(ba0, ba1), qq, a);
        }
        const int32_t bias = 1 << 29;
        if (x < out_w) out[(size_t)i * out_w + x] = resize_texel(resize_code(r + bias), resize_code(g + bias), resize_code(b + bias), resize_code(a + bias));
    }
}

void launch_image_resize_h(const uint32_t* src, uint32_t src_w, uint32_t src_h, void* tmp, uint32_t out_w, const uint32_t* table, uint32_t pairs, hipStream_t stream) {
    const dim3 grid((out_w + (uint32_t)kResizeGroup - 1u) / (uint32_t)kResizeGroup, (src_h + (uint32_t)kResizeRows - 1u) / (uint32_t)kResizeRows); // <= 512 x 256
    hipLaunchKernelGGL(k_image_resize_h, grid, dim3(kResizeColumns * kResizeWaves), 0, stream, src, src_w, src_h, static_cast<uint2*>(tmp), out_w, table, pairs);
}

void launch_image_resize_v(const void* tmp, uint32_t tmp_h, uint32_t* out, uint32_t out_w, uint32_t out_h, const uint32_t* table, uint32_t pairs, hipStream_t stream) {
    const dim3 grid((out_w + (uint32_t)kResizeColumns - 1u) / (uint32_t)kResizeColumns, (out_h + (uint32_t)kResizeBlockRows - 1u) / (uint32_t)kResizeBlockRows); // <= 256 x 512
    hipLaunchKernelGGL(k_image_resize_v, grid, dim3(kResizeColumns * kResizeWaves), 0, stream, static_cast<const uint2*>(tmp), tmp_h, out, out_w, out_h, table, pairs);
}

// crh_image_crop and crh_image_create_from_frame_region. A copy: 4 bytes read (inside the source) and 4 written per texel, streaming
// (image_geometry.hpp) over the RESULT, one aligned store per group. The source's group is one load of 4 V bytes only where `source_wide`
// says so (stream_wide); otherwise V loads of 4 bytes. Every source address is formed behind region_source's range check (regions.hpp: the
// wrapped sum is below the source's size exactly when the true one is in range, for any int32 x and y), and every texel of the result is
// written exactly once, the zeros outside the source included: nothing clears the result first.
template <int V>
__global__ __launch_bounds__(kStreamLanes) void k_image_crop(const uint32_t* __restrict__ source, uint32_t source_w, uint32_t source_h, uint32_t x, uint32_t y, uint32_t source_wide,
                                                                 uint32_t* __restrict__ out, uint32_t w, uint32_t h) {
    typedef typename TexelGroup<V>::type Group;
    const uint32_t i = stream_column<V>();
    if (i >= w) return; // (the whole group is outside)
    for (uint32_t j = blockIdx.y; j < h; j += gridDim.y) {
        Group r = 0u;
        uint32_t sj = 0u, si = 0u;
        if (region_source(j, y, source_h, &sj)) {
            const uint32_t* line = source + (size_t)sj * source_w;
            if (source_wide) {
                if (region_source(i, x, source_w, &si)) r = *reinterpret_cast<const Group*>(line + si); // (si % V == 0 and source_w % V == 0: si + V - 1 < source_w)
            } else {
#pragma unroll
                for (int t = 0; t < V; ++t)
                    if (region_source(i + (uint32_t)t, x, source_w, &si)) r[t] = line[si];
            }
        }
        *reinterpret_cast<Group*>(out + (size_t)j * w + i) = r;
    }
}

void launch_image_crop(const uint32_t* source, uint32_t source_w, uint32_t source_h, int32_t x, int32_t y, uint32_t* out, uint32_t w, uint32_t h, hipStream_t stream) {
    const StreamGrid g = stream_grid(w, h, kStreamBlocks);
    const uint32_t wide = stream_wide(g.v, source_w, x);
#define CRH_CROP_LAUNCH(V) hipLaunchKernelGGL(k_image_crop<V>, g.grid, dim3(kStreamLanes), 0, stream, source, source_w, source_h, (uint32_t)x, (uint32_t)y, wide, out, w, h)
    CRH_STREAM_DISPATCH(g.v, CRH_CROP_LAUNCH);
#undef CRH_CROP_LAUNCH
}

namespace {
// crh_image_statistics' grid cap, chosen for it: every workgroup leaves a partial result of kStatsWords words (4116 bytes), so kStreamBlocks
// of them would write half of what a 4096^2 image holds. 512 = 256 CUs x 2 workgroups of eight waves, 256 lanes along the row by two rows;
// a lane takes its rows two at a time, so that it has two loads in flight where k_image_color_filter has two workgroups on the SIMD. The
// partials of a 4096^2 image are 2 MB written and read once: 3 % of its bytes.
constexpr uint32_t kStatsBlocks = 512;
constexpr int kStatsRows = 2;                                  // rows of lanes in a workgroup (threadIdx.y)
constexpr int kStatsWaves = kStatsRows * kStreamLanes / 64; // a histogram each: 32 KB of LDS
constexpr int kStatsMergeWords = 64, kStatsMergeSlices = 16; // k_image_stats_merge: words per workgroup, one per lane of a wave; partials in flight per word
enum { kStatsPlain = 0, kStatsZeros = 1, kStatsRuns = 2 }; // what k_image_stats does about contention: DESIGN.md §7 "Regions and statistics" has the measurement
} // namespace

// crh_image_statistics, the pass over the texels. Streaming (image_geometry.hpp), 4 bytes read per texel, with two rows of lanes: the lanes
// of threadIdx.y = s stride over the rows 2 blockIdx.y + s, + 2 gridDim.y, ..., two per turn. Histograms accumulate
// in LDS, one of 4 x 256 words per wave (no wave contends with another; 32 KB per workgroup), by ds_add_u32 without return. A lane's columns are fixed, so the
// bounds are kept per lane as a mask of its V columns that were hit, the first and last row with a hit, and the number of hits, joined
// across the wave by shuffles at the end. What this does about the input the call is for — a layer that is almost all (0, 0, 0, 0), where
// a plain histogram sends 64 lanes to one LDS address four times per texel:
//   M >= kStatsZeros  a texel that is 0 costs one register increment per lane; the wave adds them to bin 0 of each channel once, at the end.
//   M == kStatsRuns   a row's groups that are ONE texel value across the whole wave (one readfirstlane, V compares, one ballot) are counted
//                     in a wave-uniform run (value, length) that goes to LDS only when the value changes: a constant layer, opaque or
//                     transparent, issues four LDS adds per wave per run.
// Workgroups never wait for one another: each writes its partial result (regions.hpp's words, the bounds still in their "empty" form) to
// its own slab; k_image_stats_merge below sums the slabs.
template <int V, int M>
__global__ __launch_bounds__(kStreamLanes * kStatsRows) void k_image_stats(const uint32_t* __restrict__ src, uint32_t w, uint32_t h, StatsConstants f, uint32_t* __restrict__ partial) {
    typedef typename TexelGroup<V>::type Group;
    __shared__ uint32_t hist[kStatsWaves][kStatsHistogramWords];
    __shared__ uint32_t edge[kStatsWaves][5];
    const uint32_t lane = threadIdx.y * (uint32_t)kStreamLanes + threadIdx.x; // of the workgroup
    for (uint32_t k = lane; k < (uint32_t)kStatsWaves * kStatsHistogramWords; k += (uint32_t)(kStreamLanes * kStatsRows)) (&hist[0][0])[k] = 0u;
    __syncthreads();
    const uint32_t wave = lane >> 6;
    uint32_t* mine = hist[wave];
    const uint32_t i = stream_column<V>();
    const bool live = i < w; // (the whole group is inside or outside)
    const uint64_t live_lanes = __ballot(live);
    uint32_t columns = 0u, row0 = 0xFFFFFFFFu, row1 = 0u, hits = 0u, zeros = 0u;
    uint32_t run_texel = 0u, run_length = 0u; // wave-uniform
    if (live_lanes != 0ull) { // (a wave's lanes are consecutive columns: lane 0 of a wave with a live lane is live)
        const uint32_t stride = (uint32_t)kStatsRows * gridDim.y;
        for (uint32_t j0 = (uint32_t)kStatsRows * blockIdx.y + threadIdx.y; j0 < h; j0 += 2u * stride) {
            const uint32_t j1 = j0 + stride;
            Group g[2];
            g[0] = 0u, g[1] = 0u;
            if (live) {
                g[0] = *reinterpret_cast<const Group*>(src + (size_t)j0 * w + i);
                if (j1 < h) g[1] = *reinterpret_cast<const Group*>(src + (size_t)j1 * w + i);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t j = u ? j1 : j0;
                if (j >= h) break; // (the same for the whole wave)
                const Group t = g[u];
                uint32_t hit = 0u;
#pragma unroll
                for (int k = 0; k < V; ++k) hit |= stats_inside(t[k], f) ? 1u << k : 0u;
                if (live && hit != 0u) columns |= hit, hits += (uint32_t)__popc(hit), row0 = stats_min(row0, j), row1 = stats_max(row1, j + 1u);
                bool counted = false;
                if (M == kStatsRuns) {
                    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)t[0]);
                    bool same = true;
#pragma unroll
                    for (int k = 0; k < V; ++k) same = same && t[k] == first;
                    if (__ballot(live && same) == live_lanes) { // the row's part in this wave is one value
                        const uint32_t n = (uint32_t)__popcll(live_lanes) * (uint32_t)V;
                        if (first != run_texel && run_length != 0u) {
                            if ((threadIdx.x & 63u) == 0u)
                                for (uint32_t c = 0; c < 4u; ++c) atomicAdd(&mine[256u * c + stats_code(run_texel, c)], run_length);
                            run_length = 0u;
                        }
                        run_texel = first, run_length += n;
                        counted = true;
                    }
                }
                if (!counted && live) {
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        if (M >= kStatsZeros && t[k] == 0u) {
                            zeros += 1u;
                        } else {
#pragma unroll
                            for (uint32_t c = 0; c < 4u; ++c) atomicAdd(&mine[256u * c + stats_code(t[k], c)], 1u);
                        }
                    }
                }
            }
        }
        if (run_length != 0u && (threadIdx.x & 63u) == 0u)
            for (uint32_t c = 0; c < 4u; ++c) atomicAdd(&mine[256u * c + stats_code(run_texel, c)], run_length);
        if (zeros != 0u)
            for (uint32_t c = 0; c < 4u; ++c) atomicAdd(&mine[256u * c], zeros);
    }
    // the lane's bounds, joined across the wave, then across the workgroup's waves
    StatsBounds b;
    if (hits != 0u) b.x0 = i + (uint32_t)__builtin_ctz(columns), b.x1 = i + 32u - (uint32_t)__builtin_clz(columns), b.y0 = row0, b.y1 = row1, b.count = hits;
#pragma unroll
    for (int d = 32; d != 0; d >>= 1) {
        StatsBounds o;
        o.x0 = __shfl_xor(b.x0, d), o.y0 = __shfl_xor(b.y0, d), o.x1 = __shfl_xor(b.x1, d), o.y1 = __shfl_xor(b.y1, d), o.count = __shfl_xor(b.count, d);
        stats_join(b, o);
    }
    if ((threadIdx.x & 63u) == 0u) edge[wave][0] = b.x0, edge[wave][1] = b.y0, edge[wave][2] = b.x1, edge[wave][3] = b.y1, edge[wave][4] = b.count;
    __syncthreads();
    uint32_t* slab = partial + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * kStatsWords;
    for (uint32_t at = lane; at < kStatsHistogramWords; at += (uint32_t)(kStreamLanes * kStatsRows)) {
        uint32_t sum = 0u;
#pragma unroll
        for (int v = 0; v < kStatsWaves; ++v) sum += hist[v][at];
        slab[at] = sum;
    }
    if (lane == 0u) {
        StatsBounds all;
        for (int v = 0; v < kStatsWaves; ++v) {
            StatsBounds o;
            o.x0 = edge[v][0], o.y0 = edge[v][1], o.x1 = edge[v][2], o.y1 = edge[v][3], o.count = edge[v][4];
            stats_join(all, o);
        }
        slab[kStatsX0] = all.x0, slab[kStatsY0] = all.y0, slab[kStatsX1] = all.x1, slab[kStatsY1] = all.y1, slab[kStatsCount] = all.count;
    }
}

// crh_image_statistics, the sum of the n partial results: word `at` of the result is the sum (the histogram, the count), the minimum
// (x0, y0) or the maximum (x1, y1) of word `at` of every slab; a minimum that is still "empty" is the header's 0. A workgroup owns 64
// consecutive words, a lane of threadIdx.y = s the slabs s, s + 16, ...: 64 consecutive words of a slab are one 256-byte load of a wave.
__global__ __launch_bounds__(kStatsMergeWords * kStatsMergeSlices) void k_image_stats_merge(const uint32_t* __restrict__ partial, uint32_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t part[kStatsMergeSlices][kStatsMergeWords];
    const uint32_t at = blockIdx.x * (uint32_t)kStatsMergeWords + threadIdx.x;
    const bool lowest = at == kStatsX0 || at == kStatsY0, highest = at == kStatsX1 || at == kStatsY1;
    uint32_t v = lowest ? 0xFFFFFFFFu : 0u;
    if (at < kStatsWords) {
        // eight slabs' words at a time: the loads are independent, and taken one by one each would wait out the last one's latency
        for (uint32_t p = threadIdx.y; p < n; p += 8u * (uint32_t)kStatsMergeSlices) {
            uint32_t o[8];
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                const uint32_t q = p + k * (uint32_t)kStatsMergeSlices;
                const uint32_t word = partial[(size_t)stats_min(q, n - 1u) * kStatsWords + at]; // (every load is issued: a slab beyond the last reads the last and is not counted)
                o[k] = q < n ? word : lowest ? 0xFFFFFFFFu : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) v = lowest ? stats_min(v, o[k]) : highest ? stats_max(v, o[k]) : v + o[k];
        }
    }
    part[threadIdx.y][threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.y != 0u || at >= kStatsWords) return;
    for (int s = 1; s < kStatsMergeSlices; ++s) {
        const uint32_t o = part[s][threadIdx.x];
        v = lowest ? stats_min(v, o) : highest ? stats_max(v, o) : v + o;
    }
    out[at] = lowest && v == 0xFFFFFFFFu ? 0u : v;
}

namespace {
StreamGrid stats_grid(uint32_t w, uint32_t h) { return stream_grid(w, (h + (uint32_t)kStatsRows - 1u) / (uint32_t)kStatsRows, kStatsBlocks); }
} // namespace

uint32_t image_stats_partials(uint32_t w, uint32_t h) {
    const StreamGrid g = stats_grid(w, h);
    return g.grid.x * g.grid.y;
}

void launch_image_stats(const uint32_t* src, uint32_t w, uint32_t h, const StatsConstants& f, uint32_t* partial, hipStream_t stream) {
    const StreamGrid g = stats_grid(w, h);
    // CRH_STATS_VARIANT = 0 (a plain LDS histogram) or 1 (+ the zero texels in a register) builds the measurement's other arms; anything else is the default
    static const int variant = [] {
        const char* e = std::getenv("CRH_STATS_VARIANT");
        return e && (e[0] == '0' || e[0] == '1') && e[1] == 0 ? e[0] - '0' : (int)kStatsRuns;
    }();
#define CRH_STATS_LAUNCH(V, M) hipLaunchKernelGGL((k_image_stats<V, M>), g.grid, dim3(kStreamLanes, kStatsRows), 0, stream, src, w, h, f, partial)
    if (variant == kStatsPlain) CRH_STREAM_DISPATCH(g.v, CRH_STATS_LAUNCH, kStatsPlain);
    else if (variant == kStatsZeros) CRH_STREAM_DISPATCH(g.v, CRH_STATS_LAUNCH, kStatsZeros);
    else CRH_STREAM_DISPATCH(g.v, CRH_STATS_LAUNCH, kStatsRuns);
#undef CRH_STATS_LAUNCH
}

void launch_image_stats_merge(const uint32_t* partial, uint32_t n, uint32_t* out, hipStream_t stream) {
    const uint32_t blocks = (kStatsWords + (uint32_t)kStatsMergeWords - 1u) / (uint32_t)kStatsMergeWords;
    hipLaunchKernelGGL(k_image_stats_merge, dim3(blocks), dim3(kStatsMergeWords, kStatsMergeSlices), 0, stream, partial, n, out);
}

} // namespace crh
