// csrc/edge.hpp — the edge rule of the image filters (include/contrast_hip.h: CRH_BLUR_EDGE_*), written once: what an index outside an axis
// of n texels reads. Edge 0 is TRANSPARENT (zero out there), 1..3 are PAD, REPEAT and REFLECT, the image-paint block's wrap(i, n): any int32
// i, 1 <= n <= 16384 -> [0, n). |i| may be many times n (a radius of 192 on a one-texel axis), so REPEAT and REFLECT reduce with a
// remainder, not a single fold. The kernels of image_filter.hip and the host models of the filters' headers all call these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crh {

// The phase form, in two parts, so that a walk along an axis pays the remainder once: the phase of i is i mod the period (n for REPEAT,
// 2 n for REFLECT; 0 for the edges without a period).
__host__ __device__ __forceinline__ int edge_period(int n, uint32_t edge) { return edge == 2u ? n : edge == 3u ? 2 * n : 1; }
__host__ __device__ __forceinline__ int edge_phase(int i, int n, uint32_t edge) {
    if (edge < 2u) return 0;
    const int p = edge_period(n, edge);
    const int k = i % p;
    return k < 0 ? k + p : k;
}
// the phase of i + 1 and of i - 1 from the phase of i: no division
__host__ __device__ __forceinline__ int edge_phase_next(int k, int period) { return k + 1 == period ? 0 : k + 1; }
__host__ __device__ __forceinline__ int edge_phase_before(int k, int period) { return k == 0 ? period - 1 : k - 1; }
// wrap(i, n) from i and its phase k, without a branch or a division. PAD clamps i; REPEAT is the phase; REFLECT folds the phase's second half
// back. Under TRANSPARENT (edge 0) it clamps as PAD does, which gives a caller that selects zero outside [0, n) an address it may still read.
__host__ __device__ __forceinline__ int edge_wrap_at(int i, int k, int n, uint32_t edge) {
    const int clamped = i < 0 ? 0 : i >= n ? n - 1 : i;
    const int folded = k < n ? k : 2 * n - 1 - k;
    return edge < 2u ? clamped : folded;
}
__host__ __device__ __forceinline__ int edge_wrap(int i, int n, uint32_t edge) { return edge_wrap_at(i, edge_phase(i, n, edge), n, edge); }

// The branching form, edges 1..3 only: an index inside returns at once, and the remainder runs only in the waves that leave the image.
// The two forms give the same index and compile differently; a kernel keeps the one it was measured with.
__host__ __device__ __forceinline__ int edge_wrap_branching(int i, int n, uint32_t edge) {
    if ((uint32_t)i < (uint32_t)n) return i; // (inside: every edge agrees)
    if (edge == 1u) return i < 0 ? 0 : n - 1;
    const int p = edge == 2u ? n : 2 * n;
    int k = i % p;
    if (k < 0) k += p;
    return k < n ? k : p - 1 - k;
}

// Element i of a line of n elements, line[i * stride + offset] (a row: stride 1; a column of a w-wide image: stride w, offset x), by the edge:
// the two ways the kernels read one. Both form every address from a wrapped, clamped or range-checked index, so none lies outside the line.
// "Wrapped load, or zero": under TRANSPARENT an index outside is not loaded at all.
template <bool BRANCHING = false, typename T>
__host__ __device__ __forceinline__ T edge_load(const T* line, int i, int n, uint32_t edge, size_t stride = 1, size_t offset = 0) {
    T value = T{};
    if (edge != 0u) value = line[(size_t)(BRANCHING ? edge_wrap_branching(i, n, edge) : edge_wrap(i, n, edge)) * stride + offset];
    else if ((uint32_t)i < (uint32_t)n) value = line[(size_t)i * stride + offset];
    return value;
}
// "Clamped address, unconditional load, select zero", i with its phase k: the loads of an unrolled stretch are in flight together.
template <typename T>
__host__ __device__ __forceinline__ T edge_load_select(const T* line, int i, int k, int n, uint32_t edge, size_t stride = 1) {
    const T value = line[(size_t)edge_wrap_at(i, k, n, edge) * stride];
    return edge == 0u && (uint32_t)i >= (uint32_t)n ? T{} : value;
}

} // namespace crh
