// csrc/raster.hip — tile-binned compute rasterizer that replaces the reference's stencil-then-cover passes
// (Shape::render renderer.rs:267-355, stencil states renderer.rs:565-582,692-754,761-861, fragment stages shaders.wgsl:155-355).
//
// The frame is cut into 16x16-pixel tiles; one wavefront owns one tile (msaa 1: lane = column x row group, four pixels per lane; msaa 4:
// four wavefronts per tile, one pixel x four samples per lane), so the stencil byte of the reference (winding counter, clip nesting
// counter), the saved alpha layers and the colour of a sample never leave the owning lane's registers, and no workgroup barrier is
// needed anywhere in the raster kernel (except in the rare tile whose list is too long for LDS and is sorted in global memory).
//
//   k_scan_*           two-kernel exclusive scan (primitive ranges per Shape / draw item, tile list offsets per frame)
//   k_prim_setup<S,P>  one wavefront per draw item (= Shape in the plain pass), one lane per triangle: vertex stage (shaders.wgsl:13-27,
//                      66-151), edge functions in canonical orientation, clamped pixel box, attribute planes -> a 128-byte record, once
//                      per frame. Primitive ids are contiguous per item and ascend in draw order (item, then line / joint / solid / IQ /
//                      IC / RQ / RC / cover = renderer.rs:275-354).
//   k_tile_walk<S,F>   count pass (F = false) and fill pass (F = true) of the per-tile lists: kWalkWaves wavefronts per item, lane =
//                      triangle, exact tile test (an edge function is monotone in x and y under fmaf, so the best tile corner
//                      decides), ballot + popcount -> ONE atomic per (64-triangle chunk, tile); the fill pass writes prim ids.
//   k_raster_tile<..>  sorts the tile's list by prim id (= draw order) in registers / LDS / global memory and walks it; see the kernel's
//                      comment. Workgroup b runs on XCD b % 8: tiles are dealt to the XCDs in 8x8 blocks (L2 locality of the records).
//   Coverage and attribute arithmetic follow oracle/raster.hpp operation by operation (tile-relative constants, explicit fmaf), so
//   pixels are bit-identical to the CPU spec.
//
// Roofline note: algorithmic traffic = emitted vertices read once + W*H*4 bytes written once; the raster kernel is VALU-issue bound
// (edge functions per sample), the others latency bound; there is no GEMM shape for MFMA anywhere.
#include <type_traits>

#include "launch.hpp"
#include "paint_angle.hpp"
#include "raster_tile_list.hpp"

namespace crh {

// ---------------------------------------------------------------------------------------------- scans
// Two-kernel exclusive scan over a u32 array (1024 items per block): out[i] = sum of in[0..i), out[n] = total.
struct ScanJob {
    const uint32_t* in;
    uint32_t* out;
    uint32_t* block_sum;
    uint32_t n, blocks;
    uint32_t* max_out; // optional: atomicMax of the items (the longest tile list)
};
// candidate counts are transform independent: one lane per Shape (runs at the end of tessellation, before the scan)
__global__ __launch_bounds__(256) void k_shape_ncand(SceneDev s, uint32_t* shape_ncand) {
    const uint32_t shape = blockIdx.x * 256u + threadIdx.x;
    if (shape >= s.n_shapes) return;
    uint32_t c[8];
    shape_ncand[shape] = shape_candidates(s, shape, c);
}
// the same per draw item of a recorded pass (per frame)
__global__ __launch_bounds__(256) void k_item_ncand(SceneDev s, RasterParams r, uint32_t* item_ncand) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n_items) return;
    uint32_t cb[8], first, last;
    item_candidates(s, r.items[i], cb, first, last);
    item_ncand[i] = last - first;
}
CRH_D void scan_local_body(const ScanJob& j) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t i0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < j.n ? j.in[i0 + k] : 0u;
    const uint32_t mine = v[0] + v[1] + v[2] + v[3];
    uint32_t incl = mine;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (j.max_out) {
        uint32_t longest = max(max(v[0], v[1]), max(v[2], v[3]));
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d, 64));
        if (lane == 0 && longest > 0u) atomicMax(j.max_out, longest);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; ++w) base += wave_sum[w];
    uint32_t run = base + incl - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < j.n) j.out[i0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 255) j.block_sum[blockIdx.x] = run;
}
__global__ __launch_bounds__(256) void k_scan_local(ScanJob j) { scan_local_body(j); }
// two scans of equally many items in one launch (blockIdx.y picks the job): the primitive ids and the slot ranges per Shape
__global__ __launch_bounds__(256) void k_scan_local2(ScanJob a, ScanJob b) { scan_local_body(blockIdx.y ? b : a); }
// mode 0: primitive ranges; mode 1: tile list offsets (also publishes the pair count and the overflow flag)
CRH_D void scan_add_body(const ScanJob& j, const RasterParams& r, int mode) {
    __shared__ uint32_t partial[256];
    uint32_t sum = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256u) sum += j.block_sum[k];
    partial[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < (uint32_t)d) partial[threadIdx.x] += partial[threadIdx.x + d];
        __syncthreads();
    }
    const uint32_t base = partial[0];
    const uint32_t i0 = blockIdx.x * 1024u + threadIdx.x * 4u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < j.n) j.out[i0 + k] += base;
    if (blockIdx.x + 1u == j.blocks && threadIdx.x == 0) {
        const uint32_t total = base + j.block_sum[blockIdx.x];
        j.out[j.n] = total;
        if (mode == 1) {
            r.overflow[1] = total;
            r.overflow[0] = total > r.pair_capacity ? 1u : 0u;
        }
    }
}
__global__ __launch_bounds__(256) void k_scan_add(ScanJob j, RasterParams r, int mode) { scan_add_body(j, r, mode); }
__global__ __launch_bounds__(256) void k_scan_add2(ScanJob a, ScanJob b) {
    RasterParams unused = {};
    scan_add_body(blockIdx.y ? b : a, unused, 0);
}

// ---------------------------------------------------------------------------------------------- exact tile test
// An edge function E = fma(ry, bx, fma(rx, nay, c)) is monotone in rx and in ry (fmaf rounds monotonically), so its extremes over a
// box of sample positions sit at the corners. Sample positions inside a tile span [s_lo, 15 + s_hi] in x and in y. A tile is a hit of
// a triangle when the triangle's pixel box overlaps it and no edge rejects its best tile corner — a conservative superset of "some
// sample of the tile is covered" (three half planes each touching the tile do not imply a common point); the raster kernel decides per
// sample. The test itself is written out in k_tile_walk, with the tile-invariant parts hoisted.

// tile rectangle that bounds the pixel boxes of the wave's (up to 64) triangles; false when no lane draws anything
CRH_D bool wave_tile_rect(bool valid, const PrimCoverage& cov, uint32_t& tx0, uint32_t& tx1, uint32_t& ty0, uint32_t& ty1) {
    uint32_t x0 = valid ? cov.box.x : 0xFFFFu, x1 = valid ? cov.box.y : 0u, y0 = valid ? cov.box.z : 0xFFFFu, y1 = valid ? cov.box.w : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        x0 = min(x0, (uint32_t)__shfl_xor((int)x0, d, 64));
        y0 = min(y0, (uint32_t)__shfl_xor((int)y0, d, 64));
        x1 = max(x1, (uint32_t)__shfl_xor((int)x1, d, 64));
        y1 = max(y1, (uint32_t)__shfl_xor((int)y1, d, 64));
    }
    tx0 = x0 / kTile;
    tx1 = x1 / kTile;
    ty0 = y0 / kTile;
    ty1 = y1 / kTile;
    return x0 != 0xFFFFu;
}

// ---------------------------------------------------------------------------------------------- k_prim_setup
// PROJ == false: every instance is plain (the host checked), the projective setup is compiled out
template <int S, bool PROJ>
__global__ __launch_bounds__(64) void k_prim_setup(SceneDev s, RasterParams r) {
    const uint32_t item = blockIdx.x, lane = threadIdx.x;
    const DrawItem it = item_of(r, item);
    const uint32_t shape = it.shape;
    const float* m = r.transforms + 16u * it.instance;
    // oracle/raster.hpp is_plain_instance: clip.w == 1 and clip.z a constant in [0, 1]; every other matrix takes the projective setup
    const bool plain = !PROJ || (m[3] == 0.0f && m[7] == 0.0f && m[15] == 1.0f && m[2] == 0.0f && m[6] == 0.0f && m[14] >= 0.0f && m[14] <= 1.0f);
    uint32_t cb[8], first_candidate, last_candidate;
    item_candidates(s, it, cb, first_candidate, last_candidate);
    const uint32_t n_candidates = last_candidate - first_candidate;
    const uint32_t prim0 = r.shape_prim_begin[item];
    const uint32_t cover_op = (it.ops >> 4) ? (it.ops >> 4) - 1u : (uint32_t)CRH_OP_COLOR;
    if (prim0 + n_candidates > r.prim_capacity) return; // cannot happen: the capacity is an upper bound derived from the totals
    const uint32_t* b0 = s.shape_base + shape * kShapeRow;
    const uint32_t lv0 = b0[CH_LINE_V], j0 = b0[CH_JOINT], sv0 = b0[CH_SOLID_V], iq0 = b0[CH_IQ], ic0 = b0[CH_IC_V], rq0 = b0[CH_RQ], rc0 = b0[CH_RC_V],
                   hull0 = b0[CH_HULL];
    const uint32_t dyn0 = s.shape_dyn_begin[shape];
    const float W = (float)r.width, H = (float)r.height;
    for (uint32_t c0 = 0; c0 < n_candidates; c0 += 64u) { // all 64 lanes stay in the loop: the tile walk below is wave-wide
        const uint32_t c = first_candidate + c0 + lane; // in the Shape's candidate numbering
        const bool in_range_c = c0 + lane < n_candidates;
        float2 p[3] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
        float attr[3][4] = {};
        uint32_t kind = KIND_SOLID, flat_u = 0, desc = 0;
        float end_y = 0.0f;
        int n_attr = 0;
        bool valid = true;
        uint32_t i0 = 0, i1 = 0, i2 = 0;
        auto strip = [&](uint32_t k, uint32_t base) { // strip triangle k: even (k, k+1, k+2), odd (k, k+2, k+1); provoking vertex k
            i0 = base + k;
            i1 = base + ((k & 1u) ? k + 2u : k + 1u);
            i2 = base + ((k & 1u) ? k + 1u : k + 2u);
        };
        if (!in_range_c) {
            valid = false;
        } else if (c < cb[0]) { // stroke line strips (vertex2f1u / stencil_stroke_line)
            const uint32_t k = c;
            valid = s.line_pair_cut[(lv0 + k) >> 1] == 0;
            strip(k, lv0);
            const Vertex2f1i a = s.line_v[i0], b = s.line_v[i1], d = s.line_v[i2];
            p[0] = make_float2(a.x, a.y);
            p[1] = make_float2(b.x, b.y);
            p[2] = make_float2(d.x, d.y);
            attr[0][0] = a.u, attr[0][1] = a.v;
            attr[1][0] = b.u, attr[1][1] = b.v;
            attr[2][0] = d.u, attr[2][1] = d.v;
            flat_u = a.i; // i0 is the provoking vertex
            end_y = a.v;
            desc = dyn0 + (a.i & 65535u);
            kind = KIND_LINE;
            n_attr = 2;
        } else if (c < cb[1]) { // stroke joint strips: 5 vertices, 3 triangles per join
            const uint32_t q = c - cb[0], jn = q / 3u, k = q - 3u * jn;
            strip(k, 5u * (j0 + jn));
            const Vertex3f1i a = s.joint_v[i0], b = s.joint_v[i1], d = s.joint_v[i2];
            p[0] = make_float2(a.x, a.y);
            p[1] = make_float2(b.x, b.y);
            p[2] = make_float2(d.x, d.y);
            attr[0][0] = a.u, attr[0][1] = a.v, attr[0][2] = a.w;
            attr[1][0] = b.u, attr[1][1] = b.v, attr[1][2] = b.w;
            attr[2][0] = d.u, attr[2][1] = d.v, attr[2][2] = d.w;
            flat_u = a.i;
            desc = dyn0 + (flat_u & 65535u);
            kind = KIND_JOINT;
            n_attr = 3;
        } else if (c < cb[2]) { // solid strips (vertex0 / stencil_solid)
            const uint32_t k = c - cb[1];
            const uint8_t f0 = s.solid_flag[sv0 + k], f1 = s.solid_flag[sv0 + k + 1u];
            valid = ((f0 | f1) & 2u) == 0;
            const uint32_t parity = f0 & 1u;
            i0 = sv0 + k;
            i1 = sv0 + (parity ? k + 2u : k + 1u);
            i2 = sv0 + (parity ? k + 1u : k + 2u);
            const Vertex0 a = s.solid_v[i0], b = s.solid_v[i1], d = s.solid_v[i2];
            p[0] = make_float2(a.x, a.y);
            p[1] = make_float2(b.x, b.y);
            p[2] = make_float2(d.x, d.y);
        } else if (c < cb[3]) {
            const uint32_t at = 3u * (iq0 + (c - cb[2]));
            for (int v = 0; v < 3; ++v) {
                const Vertex2f a = s.iq_v[at + v];
                p[v] = make_float2(a.x, a.y);
                attr[v][0] = a.u, attr[v][1] = a.v;
            }
            kind = KIND_IQ;
            n_attr = 2;
        } else if (c < cb[4]) {
            const uint32_t at = ic0 + 3u * (c - cb[3]);
            for (int v = 0; v < 3; ++v) {
                const Vertex3f a = s.ic_v[at + v];
                p[v] = make_float2(a.x, a.y);
                attr[v][0] = a.u, attr[v][1] = a.v, attr[v][2] = a.w;
            }
            kind = KIND_IC;
            n_attr = 3;
        } else if (c < cb[5]) {
            const uint32_t at = 3u * (rq0 + (c - cb[4]));
            for (int v = 0; v < 3; ++v) {
                const Vertex3f a = s.rq_v[at + v];
                p[v] = make_float2(a.x, a.y);
                attr[v][0] = a.u, attr[v][1] = a.v, attr[v][2] = a.w;
            }
            kind = KIND_RQ;
            n_attr = 3;
        } else if (c < cb[6]) {
            const uint32_t at = rc0 + 3u * (c - cb[5]);
            for (int v = 0; v < 3; ++v) {
                const Vertex4f a = s.rc_v[at + v];
                p[v] = make_float2(a.x, a.y);
                attr[v][0] = a.k, attr[v][1] = a.l, attr[v][2] = a.m, attr[v][3] = a.n;
            }
            kind = KIND_RC;
            n_attr = 4;
        } else { // cover: hull strip (vertex_color / color_cover)
            strip(c - cb[6], hull0);
            const Vertex0 a = s.hull_v[i0], b = s.hull_v[i1], d = s.hull_v[i2];
            p[0] = make_float2(a.x, a.y);
            p[1] = make_float2(b.x, b.y);
            p[2] = make_float2(d.x, d.y);
            kind = KIND_COVER;
        }
        // ---- oracle/raster.hpp setup_triangle + setup_attribute
        PrimRec rec;
        PrimProj proj = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        rec.cov.box = make_ushort4(0xFFFFu, 0, 0, 0);
        bool drawn = false;
        const uint32_t clip_ref = kind == KIND_COVER ? (it.refs >> 8) & 255u : it.refs & 255u;
        // bits 0-2 top-left, 3 front, 4-6 kind, 7-9 cover operation, 16-23 stencil reference (clip depth), 24-27 alpha layer, 28 projective
        const uint32_t flags_common = (kind << 4) | (cover_op << 7) | (clip_ref << 16) | (((it.refs >> 16) & 15u) << 24);
        const bool culled_kind = kind == KIND_COVER && cover_op == CRH_OP_COLOR && r.cull_mode != 0u; // Configuration::cull_mode: the colour cover only
        if (!PROJ || plain) {
#pragma unroll
        for (int v = 0; v < 3; ++v) p[v] = to_framebuffer(m, W, H, p[v].x, p[v].y);
        const float d1x = p[1].x - p[0].x, d1y = p[1].y - p[0].y;
        const float d2x = p[2].x - p[0].x, d2y = p[2].y - p[0].y;
        const float det = d1x * d2y - d2x * d1y;
        if (in_range_c && valid && det != 0.0f && det == det && is_finite(det)) {
            float minx = fminf(p[0].x, fminf(p[1].x, p[2].x)), maxx = fmaxf(p[0].x, fmaxf(p[1].x, p[2].x));
            float miny = fminf(p[0].y, fminf(p[1].y, p[2].y)), maxy = fmaxf(p[0].y, fmaxf(p[1].y, p[2].y));
            const bool nan_free = minx == minx && maxx == maxx && miny == miny && maxy == maxy;
            // inclusive pixel range: clamp, floor, THEN compare (oracle/raster.hpp setup_triangle)
            const int x0 = (int)floorf(fminf(fmaxf(minx, 0.0f), W)), x1 = (int)floorf(fmaxf(fminf(maxx, W - 1.0f), -1.0f));
            const int y0 = (int)floorf(fminf(fmaxf(miny, 0.0f), H)), y1 = (int)floorf(fmaxf(fminf(maxy, H - 1.0f), -1.0f));
            if (nan_free && x0 <= x1 && y0 <= y1 && !(culled_kind && (r.cull_mode == CRH_CULL_FRONT) == (det < 0.0f))) {
                drawn = true;
                rec.cov.box = make_ushort4((unsigned short)x0, (unsigned short)x1, (unsigned short)y0, (unsigned short)y1);
                const float inv_det = 1.0f / det;
                const bool front = det < 0.0f; // y-down cross < 0 == counter-clockwise on screen (FrontFace::Ccw, renderer.rs:477)
                const float2 nv[3] = {p[0], det < 0.0f ? p[2] : p[1], det < 0.0f ? p[1] : p[2]}; // clockwise-in-y-down edge walk
                uint32_t flags = (front ? 8u : 0u) | flags_common;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float2 a = nv[i], b = nv[(i + 1) % 3];
                    const float dx = b.x - a.x, dy = b.y - a.y;
                    if (dy < 0.0f || (dy == 0.0f && dx > 0.0f)) flags |= 1u << i; // top-left rule
                    const bool flip = !(a.x < b.x || (a.x == b.x && a.y < b.y));   // canonical (lexicographic) endpoint order
                    const float2 el = flip ? b : a, eh = flip ? a : b;
                    const float sg = flip ? -1.0f : 1.0f;
                    rec.cov.lo_x[i] = el.x;
                    rec.cov.lo_y[i] = el.y;
                    rec.cov.bx[i] = (eh.x - el.x) * sg;
                    rec.cov.nay[i] = -(eh.y - el.y) * sg;
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if (a < n_attr) {
                        const float da1 = attr[1][a] - attr[0][a], da2 = attr[2][a] - attr[0][a];
                        rec.frag.a0[a] = attr[0][a];
                        rec.frag.gx[a] = (da1 * d2y - da2 * d1y) * inv_det;
                        rec.frag.gy[a] = (da2 * d1x - da1 * d2x) * inv_det;
                    } else {
                        rec.frag.a0[a] = rec.frag.gx[a] = rec.frag.gy[a] = 0.0f;
                    }
                }
                if (kind == KIND_COVER) { // color_cover: (rgb * a, a), shaders.wgsl:304-309
                    const float* color = r.colors + 4u * it.instance;
                    rec.frag.a0[0] = color[0] * color[3];
                    rec.frag.a0[1] = color[1] * color[3];
                    rec.frag.a0[2] = color[2] * color[3];
                    rec.frag.a0[3] = color[3];
                    rec.frag.gx[0] = m[14]; // the fragment depth of a plain instance
                }
                rec.frag.v0x = p[0].x;
                rec.frag.v0y = p[0].y;
                rec.frag.flat_u = flat_u;
                rec.frag.end_y = end_y;
                rec.cov.flags = flags;
                rec.cov.desc = desc;
            }
        }
        } else if (PROJ) {
        // ---- oracle/raster.hpp setup_projective + setup_projective_plane, operation by operation
        float PX[3], PY[3], PZ[3], PW[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const float cx = (m[0] * p[v].x + m[4] * p[v].y) + m[12];
            const float cy = (m[1] * p[v].x + m[5] * p[v].y) + m[13];
            const float cz = (m[2] * p[v].x + m[6] * p[v].y) + m[14];
            const float cw = (m[3] * p[v].x + m[7] * p[v].y) + m[15];
            PX[v] = (cx * 0.5f + cw * 0.5f) * W;
            PY[v] = (cw * 0.5f - cy * 0.5f) * H;
            PZ[v] = cz;
            PW[v] = cw;
        }
        const int k = PW[0] > 0.0f ? 0 : (PW[1] > 0.0f ? 1 : (PW[2] > 0.0f ? 2 : -1)); // the first vertex in front of the eye
        bool ok = in_range_c && valid && k >= 0;
#pragma unroll
        for (int v = 0; v < 3; ++v) ok = ok && is_finite(PX[v]) && is_finite(PY[v]) && is_finite(PZ[v]) && is_finite(PW[v]);
        const float c0 = PX[1] * PY[2] - PY[1] * PX[2], a0 = PY[1] * PW[2] - PW[1] * PY[2], b0 = PW[1] * PX[2] - PX[1] * PW[2];
        const float det = (PX[0] * a0 + PY[0] * b0) + PW[0] * c0;
        ok = ok && det != 0.0f && is_finite(det);
        const bool front = det < 0.0f;
        uint32_t flags = (front ? 8u : 0u) | flags_common | kFlagProjective;
        const int order[3] = {0, det < 0.0f ? 2 : 1, det < 0.0f ? 1 : 2};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int ia = order[i], ib = order[(i + 1) % 3];
            const float aX = PX[ia], aY = PY[ia], aW = PW[ia], bX = PX[ib], bY = PY[ib], bW = PW[ib];
            const bool flip = !(aX < bX || (aX == bX && (aY < bY || (aY == bY && aW < bW)))); // canonical (lexicographic) endpoint order
            const float lX = flip ? bX : aX, lY = flip ? bY : aY, lW = flip ? bW : aW, hX = flip ? aX : bX, hY = flip ? aY : bY, hW = flip ? aW : bW;
            const float nay = lY * hW - lW * hY, bx = lW * hX - lX * hW;
            const float sg = flip ? -1.0f : 1.0f;
            const float A = nay * sg, B = bx * sg; // exact: the oracle negates
            if (A > 0.0f || (A == 0.0f && B > 0.0f)) flags |= 1u << i;
            const bool use_lo = lW > 0.0f || (!(hW > 0.0f) && lW != 0.0f);
            const float nX = use_lo ? lX : hX, nY = use_lo ? lY : hY, nW = use_lo ? lW : hW;
            ok = ok && nW != 0.0f;
            const float ax = nX / nW, ay = nY / nW;
            ok = ok && is_finite(ax) && is_finite(ay);
            rec.cov.lo_x[i] = ax;
            rec.cov.lo_y[i] = ay;
            rec.cov.bx[i] = B;
            rec.cov.nay[i] = A;
        }
        int x0 = 0, y0 = 0, x1 = (int)r.width - 1, y1 = (int)r.height - 1; // crossing the eye plane: every pixel is a candidate
        if (PW[0] > 0.0f && PW[1] > 0.0f && PW[2] > 0.0f) {
            const float q0x = PX[0] / PW[0], q1x = PX[1] / PW[1], q2x = PX[2] / PW[2], q0y = PY[0] / PW[0], q1y = PY[1] / PW[1], q2y = PY[2] / PW[2];
            const float minx = fminf(q0x, fminf(q1x, q2x)), maxx = fmaxf(q0x, fmaxf(q1x, q2x));
            const float miny = fminf(q0y, fminf(q1y, q2y)), maxy = fmaxf(q0y, fmaxf(q1y, q2y));
            ok = ok && minx == minx && maxx == maxx && miny == miny && maxy == maxy;
            x0 = (int)floorf(fminf(fmaxf(minx, 0.0f), W));
            x1 = (int)floorf(fmaxf(fminf(maxx, W - 1.0f), -1.0f));
            y0 = (int)floorf(fminf(fmaxf(miny, 0.0f), H));
            y1 = (int)floorf(fmaxf(fminf(maxy, H - 1.0f), -1.0f));
            ok = ok && x0 <= x1 && y0 <= y1;
        }
        // planes relative to the anchor = the projection of vertex k (index 0 = k, then cyclic)
        const int kk = k < 0 ? 0 : k, ku = (kk + 1) % 3, kv = (kk + 2) % 3;
        float KX = 0.0f, KY = 0.0f, KZ = 0.0f, KW = 1.0f, UX = 0.0f, UY = 0.0f, UZ = 0.0f, UW = 1.0f, VX = 0.0f, VY = 0.0f, VZ = 0.0f, VW = 1.0f;
        float fk[4], fu[4], fv[4];
#pragma unroll
        for (int v = 0; v < 3; ++v) { // register-only selection (no dynamic indexing)
            if (v == kk) KX = PX[v], KY = PY[v], KZ = PZ[v], KW = PW[v];
            if (v == ku) UX = PX[v], UY = PY[v], UZ = PZ[v], UW = PW[v];
            if (v == kv) VX = PX[v], VY = PY[v], VZ = PZ[v], VW = PW[v];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (v == kk) fk[a] = attr[v][a];
                if (v == ku) fu[a] = attr[v][a];
                if (v == kv) fv[a] = attr[v][a];
            }
        }
        const float ancx = KX / KW, ancy = KY / KW;
        const float lx0 = UX - ancx * UW, ly0 = UY - ancy * UW, lx1 = VX - ancx * VW, ly1 = VY - ancy * VW;
        const float local_det = KW * (lx0 * ly1 - ly0 * lx1);
        ok = ok && local_det != 0.0f && is_finite(local_det);
        ok = ok && !(culled_kind && (r.cull_mode == CRH_CULL_FRONT) == front);
        if (ok) {
            drawn = true;
            rec.cov.box = make_ushort4((unsigned short)x0, (unsigned short)x1, (unsigned short)y0, (unsigned short)y1);
            const float inv_det = 1.0f / local_det;
            const float ak = ly0 * VW - UW * ly1, bk = UW * lx1 - lx0 * VW; // P'_u x P'_v
            const float au = ly1 * KW, bu = -(lx1 * KW);                    // P'_v x P'_k
            const float av = -(KW * ly0), bv = KW * lx0;                    // P'_k x P'_u
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (a < n_attr) {
                    rec.frag.a0[a] = fk[a] / KW;
                    rec.frag.gx[a] = ((fk[a] * ak + fu[a] * au) + fv[a] * av) * inv_det;
                    rec.frag.gy[a] = ((fk[a] * bk + fu[a] * bu) + fv[a] * bv) * inv_det;
                } else {
                    rec.frag.a0[a] = rec.frag.gx[a] = rec.frag.gy[a] = 0.0f;
                }
            }
            proj.ax = ancx;
            proj.ay = ancy;
            proj.q0 = 1.0f / KW;
            proj.qgx = ((1.0f * ak + 1.0f * au) + 1.0f * av) * inv_det;
            proj.qgy = ((1.0f * bk + 1.0f * bu) + 1.0f * bv) * inv_det;
            proj.z0 = KZ / KW;
            proj.zgx = ((KZ * ak + UZ * au) + VZ * av) * inv_det;
            proj.zgy = ((KZ * bk + UZ * bu) + VZ * bv) * inv_det;
            if (kind == KIND_COVER) {
                const float* color = r.colors + 4u * it.instance;
                rec.frag.a0[0] = color[0] * color[3];
                rec.frag.a0[1] = color[1] * color[3];
                rec.frag.a0[2] = color[2] * color[3];
                rec.frag.a0[3] = color[3];
            }
            rec.frag.v0x = ancx;
            rec.frag.v0y = ancy;
            rec.frag.flat_u = flat_u;
            rec.frag.end_y = end_y;
            rec.cov.flags = flags;
            rec.cov.desc = desc;
        }
        } // projective
        if (in_range_c) {
            if (drawn) {
                r.prim_rec[prim0 + c0 + lane] = rec;
                if (PROJ && !plain) r.prim_proj[prim0 + c0 + lane] = proj; // the host allocates the side array whenever an instance is not plain
            } else {
                r.prim_rec[prim0 + c0 + lane].cov.box = rec.cov.box;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- k_tile_walk
// Count pass (FILL = false) and fill pass (FILL = true) of the tile lists. One workgroup of kWalkWaves wavefronts per draw item; its
// triangles are taken 64 at a time (lane = triangle) and wavefront w walks every kWalkWaves-th tile ROW of the chunk's tile rectangle,
// so the largest Shapes (hundreds of tiles) do not leave one long serial tail. Stand-alone four wavefronts per item are fastest
// (1: 0.92 ms tail; 16: idle waves dominate); with frames overlapping two are, because the walks then share the CUs
// with the raster kernel and total work counts, not the tail.
//   count: ballot of the lanes whose triangle can touch the tile -> ONE atomic per (chunk, tile)
//   fill : lane 0 reserves popcount(ballot) slots of the tile's list with one returning atomic (consumed one iteration later, after
//          the next tile's test has been computed, so its latency is hidden); every hit lane writes
//          prim id at its rank.
constexpr uint32_t kWalkWaves = CRH_WALK_WAVES;
template <int S, bool FILL>
__global__ __launch_bounds__(64 * kWalkWaves) void k_tile_walk(SceneDev s, RasterParams r) {
    const uint32_t shape = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (FILL && r.overflow[0]) return;
    const uint32_t prim0 = r.shape_prim_begin[shape], n_candidates = r.shape_prim_begin[shape + 1] - prim0;
    if (prim0 + n_candidates > r.prim_capacity) return;
    for (uint32_t c0 = 0; c0 < n_candidates; c0 += 64u) {
        const uint32_t c = c0 + lane;
        ushort4 box = make_ushort4(0xFFFFu, 0, 0, 0);
        if (c < n_candidates) box = r.prim_rec[prim0 + c].cov.box;
        PrimCoverage cov;
        cov.box = box;
        const bool drawn = box.x != 0xFFFFu;
        uint32_t tx_a, tx_b, ty_a, ty_b;
        if (!wave_tile_rect(drawn, cov, tx_a, tx_b, ty_a, ty_b)) continue;
        if (ty_a + wave > ty_b) continue; // this wavefront has no row in the chunk's rectangle
        if (drawn) cov = r.prim_rec[prim0 + c].cov;
        unsigned long long pending_ballot = 0;
        uint32_t pending_entry = 0, pending_base = 0;
        auto flush = [&]() {
            if (!pending_ballot) return;
            const uint32_t base = __shfl(pending_base, 0, 64);
            if ((pending_ballot >> lane) & 1ull) r.tile_list[base + (uint32_t)__popcll(pending_ballot & ((1ull << lane) - 1ull))] = pending_entry;
        };
        // TileTest with everything that does not depend on the tile hoisted out of the loops (the same operations in the same order: the
        // result is bit-identical): the best corner of every edge, the row term of the edge constants, the row half of the box test
        float best_x[3], best_y[3];
        {
            const float lo = sample_lo(S), hi = (float)(kTile - 1) + sample_hi(S); // the extreme sample offsets of the pattern
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                best_x[i] = cov.nay[i] > 0.0f ? hi : lo;
                best_y[i] = cov.bx[i] > 0.0f ? hi : lo;
            }
        }
        const int tl0 = (int)(cov.flags & 1u), tl1 = (int)((cov.flags >> 1) & 1u), tl2 = (int)((cov.flags >> 2) & 1u);
        for (uint32_t ty = ty_a + wave; ty <= ty_b; ty += kWalkWaves) {
            const int tpy = (int)(ty * kTile);
            const bool row_overlap = drawn && (int)cov.box.z <= tpy + kTile - 1 && (int)cov.box.w >= tpy;
            const float ty0 = (float)tpy;
            float row_term[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) row_term[i] = cov.bx[i] * (ty0 - cov.lo_y[i]);
            for (uint32_t tx = tx_a; tx <= tx_b; ++tx) {
                const int tpx = (int)(tx * kTile);
                const float tx0 = (float)tpx;
                bool hit = row_overlap && (int)cov.box.x <= tpx + kTile - 1 && (int)cov.box.y >= tpx;
                const float e0 = fmaf(best_y[0], cov.bx[0], fmaf(best_x[0], cov.nay[0], row_term[0] + cov.nay[0] * (tx0 - cov.lo_x[0])));
                const float e1 = fmaf(best_y[1], cov.bx[1], fmaf(best_x[1], cov.nay[1], row_term[1] + cov.nay[1] * (tx0 - cov.lo_x[1])));
                const float e2 = fmaf(best_y[2], cov.bx[2], fmaf(best_x[2], cov.nay[2], row_term[2] + cov.nay[2] * (tx0 - cov.lo_x[2])));
                hit = hit && (e0 > 0.0f || (e0 == 0.0f && tl0)) && (e1 > 0.0f || (e1 == 0.0f && tl1)) && (e2 > 0.0f || (e2 == 0.0f && tl2));
                const unsigned long long ballot = __ballot(hit);
                if (!ballot) continue;
                const uint32_t tile = ty * r.tiles_x + tx;
                if (!FILL) {
                    if (lane == 0) atomicAdd(&r.tile_count[tile], (uint32_t)__popcll(ballot));
                } else {
                    uint32_t base = 0;
                    if (lane == 0) base = r.tile_offset[tile] + atomicAdd(&r.tile_cursor[tile], (uint32_t)__popcll(ballot));
                    flush(); // the previous tile's atomic has had a whole iteration to return
                    pending_ballot = ballot;
                    pending_entry = prim0 + c;
                    pending_base = base;
                }
            }
        }
        if (FILL) flush();
    }
}

// ---------------------------------------------------------------------------------------------- k_raster_tile

// One workgroup per 16x16 tile, lane = (column px, row group rq), ROWS = tile_rows(S) pixel rows per lane:
//   ROWS == 4 (msaa 1): ONE wavefront per tile; the lane owns the pixels (px, 4b + rq), b = 0..3, so a primitive's entry setup, tile
//                       constants and kind dispatch are paid once per (tile, primitive) and only the per-sample arithmetic repeats;
//   ROWS == 2 (msaa 2): two wavefronts per tile, wavefront w owns rows 8w..8w+7 — 2 samples x 2 rows per lane, the same four sample
//                       states per lane as msaa 1 and 4;
//   ROWS == 1 (msaa 4): four wavefronts per tile, wavefront w owns rows 4w..4w+3 — 4 samples x 1 row per lane keeps the per-lane state
//                       (winding + colour of every sample) at the same 20 registers instead of 80;
//   ROWS == 1 (msaa 8): the msaa 4 layout with eight samples per lane (twice the per-lane state; DESIGN.md §7 has its registers).
//   OPS == true: the full RenderOperation set — every sample also carries the clip nesting counter and up to kMaxAlphaLayers saved
//                alphas; OPS == false is the plain Stencil + Color pass at clip depth 0 (what the benchmark runs).
constexpr int kMaxAlphaLayers = 4;
//   STROKES == false: the scene has no stroked path, so the stroke fragment stages (and the registers their out-of-line dashed pattern
//                walk reserves) are compiled out: fewer VGPRs, more waves per SIMD.
//   BLEND == true (with OPS only): the colour cover blends with the renderer's Configuration::blending (`bf`) instead of premultiplied
//                "over": the kernel k_raster_blend. Both kernels include the one body, csrc/raster_tile_body.inc.
// the image block of the body (IMAGES: k_raster_image below, compiled out of the other kernels)
CRH_D float image_coord(float u) { // NaN -> 0, then clamped to +-2^24: the floor that follows is an exact int
    const float x = u == u ? u : 0.0f;
    return fminf(fmaxf(x, -16777216.0f), 16777216.0f);
}
CRH_D int image_wrap(int i, int n, uint32_t spread) { // -> [0, n): n >= 1 (crh_image_create), |i| <= 2^24 + 1; spread is wave uniform
    if (spread == CRH_SPREAD_REPEAT) {
        const int k = i % n;
        return k < 0 ? k + n : k;
    }
    if (spread == CRH_SPREAD_REFLECT) {
        const int n2 = 2 * n;
        int k = i % n2;
        k = k < 0 ? k + n2 : k;
        return k < n ? k : n2 - 1 - k;
    }
    return min(max(i, 0), n - 1);
}
CRH_D float texel_channel(uint32_t texel, int ch) { return (float)((texel >> (8 * ch)) & 255u) / 255.0f; }
// how many of a turn's four samples fetch their texels together (msaa 8 holds eight samples' state per lane: DESIGN.md §7 "Image paints")
#define CRH_IMAGE_FETCH_TOGETHER(S_) ((S_) == 8 ? 1 : 4)
// ---- the mipmap block of the body (MIPS: k_raster_mip below, compiled out of the other kernels; include/contrast_hip.h crh_image_generate_mipmaps states the model)
// how many of a sample's two levels are fetched in one go: both where the registers allow it, one after the other where eight samples' state is held
#define CRH_MIP_LEVELS_TOGETHER(S_) ((S_) == 8 ? 1 : 2)
// lod = clamp(log2(rho), 0, L - 1) from rho^2 (half the logarithm: no square root); NaN and rho == 0 give 0
CRH_D float mip_lod(float rho2, uint32_t levels) { return fminf(fmaxf(0.5f * __log2f(rho2), 0.0f), (float)(levels - 1u)); }
// rho^2 = the longer column of J = d(u, v) / d(frame position), squared: jx = (dX/dsx, dY/dsx), jy = (dX/dsy, dY/dsy) of the path position,
// taken through the path -> texel map m. A NaN column wins (lod 0).
CRH_D float mip_rho2(const float (&m)[6], float dXx, float dYx, float dXy, float dYy) {
    const float ux = m[0] * dXx + m[1] * dYx, vx = m[3] * dXx + m[4] * dYx;
    const float uy = m[0] * dXy + m[1] * dYy, vy = m[3] * dXy + m[4] * dYy;
    const float cx = ux * ux + vx * vx, cy = uy * uy + vy * vy;
    return (cx > cy || cx != cx) ? cx : cy;
}
// The texels a sample reads at one level — one for NEAREST, four for LINEAR — every address from indices wrapped with the level's own size,
// and the fractions of the LINEAR filter: the image block's rule at texel coordinates (u, v) of that level. Loads only; image_filter unpacks.
CRH_D void image_fetch(const uint32_t* texels, uint32_t width, uint32_t height, float u, float v, bool linear, uint32_t spread_x, uint32_t spread_y, uint32_t (&tex)[4], float (&frac)[2]) {
    const int iw = (int)width, ih = (int)height;
    if (linear) {
        const float au = u - 0.5f, av = v - 0.5f;
        const float fu = floorf(au), fv = floorf(av);
        frac[0] = au - fu, frac[1] = av - fv;
        const int i0 = image_wrap((int)fu, iw, spread_x), i1 = image_wrap((int)fu + 1, iw, spread_x);
        const int j0 = image_wrap((int)fv, ih, spread_y), j1 = image_wrap((int)fv + 1, ih, spread_y);
        tex[0] = texels[(uint32_t)j0 * width + (uint32_t)i0];
        tex[1] = texels[(uint32_t)j0 * width + (uint32_t)i1];
        tex[2] = texels[(uint32_t)j1 * width + (uint32_t)i0];
        tex[3] = texels[(uint32_t)j1 * width + (uint32_t)i1];
    } else {
        const int i0 = image_wrap((int)floorf(u), iw, spread_x), j0 = image_wrap((int)floorf(v), ih, spread_y);
        tex[0] = texels[(uint32_t)j0 * width + (uint32_t)i0];
    }
}
CRH_D float image_filter(const uint32_t (&tex)[4], const float (&frac)[2], bool linear, int ch) {
    const float t00 = texel_channel(tex[0], ch);
    if (!linear) return t00;
    const float t01 = texel_channel(tex[1], ch), t10 = texel_channel(tex[2], ch), t11 = texel_channel(tex[3], ch);
    const float top = t00 + frac[0] * (t01 - t00), bottom = t10 + frac[0] * (t11 - t10);
    return top + frac[1] * (bottom - top);
}
// What an affine item's mipmapped cover needs, wave uniform (one Jacobian for every sample): the two level records and the fraction between them
struct MipUniform {
    ImageLevel level[2];
    float f;
};
CRH_D MipUniform mip_uniform(const PaintItem& pi, const ImagePaintRec& im) {
    MipUniform out;
    const float lod = mip_lod(mip_rho2(im.m, pi.h[0], pi.h[3], pi.h[1], pi.h[4]), im.levels);
    const uint32_t l0 = __builtin_amdgcn_readfirstlane((uint32_t)lod), l1 = min(l0 + 1u, im.levels - 1u);
    out.f = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(lod - (float)l0)));
    out.level[0] = load_uniform(&im.chain[l0]);
    out.level[1] = load_uniform(&im.chain[l1]);
    return out;
}
// N samples of a mipmapped image paint at the frame positions (fx, fy) -> the premultiplied value s(l0) + f (s(l1) - s(l0)) of each.
// UNIFORM (an affine item): the levels and f of `uni`, and no fetch at the second level when f == 0 — a magnified placement costs what its base
// filter costs. Otherwise (a projective item) lod per sample from the sample's own (X, Y, W), and the level records by per-lane loads from the
// table. All loads of a step — N samples x CRH_MIP_LEVELS_TOGETHER levels — are issued before the first unpack.
template <int N, int TOGETHER, bool UNIFORM>
CRH_D void mip_samples(const PaintItem& pi, const ImagePaintRec& im, const MipUniform& uni, const float (&fx)[N], const float (&fy)[N], float (&out)[N][4]) {
    const bool linear = (im.filter & 1u) == CRH_FILTER_LINEAR;
    const uint32_t* chain = reinterpret_cast<const uint32_t*>(im.chain);
    float u[N], v[N], f[N];
    uint32_t level[N][2];
    int second = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        float X = fmaf(fy[c], pi.h[1], fmaf(fx[c], pi.h[0], pi.h[2])), Y = fmaf(fy[c], pi.h[4], fmaf(fx[c], pi.h[3], pi.h[5]));
        if (UNIFORM) {
            f[c] = uni.f;
            level[c][0] = level[c][1] = 0u; // (not read)
        } else {
            const float W = fmaf(fy[c], pi.h[7], fmaf(fx[c], pi.h[6], pi.h[8]));
            X = X / W;
            Y = Y / W;
            // d(X, Y) / d(sx, sy) = (h0 - X h6, h3 - Y h6; h1 - X h7, h4 - Y h7) / W: the division once, on rho^2
            const float rho2 = mip_rho2(im.m, pi.h[0] - X * pi.h[6], pi.h[3] - Y * pi.h[6], pi.h[1] - X * pi.h[7], pi.h[4] - Y * pi.h[7]) / (W * W);
            const float lod = mip_lod(rho2, im.levels);
            level[c][0] = (uint32_t)lod;
            level[c][1] = min(level[c][0] + 1u, im.levels - 1u);
            f[c] = lod - (float)level[c][0];
        }
        second |= (int)(f[c] != 0.0f);
        u[c] = image_coord(fmaf(Y, im.m[1], fmaf(X, im.m[0], im.m[2])));
        v[c] = image_coord(fmaf(Y, im.m[4], fmaf(X, im.m[3], im.m[5])));
    }
    const bool both = UNIFORM ? uni.f != 0.0f : __any(second) != 0; // wave uniform
    auto step = [&](auto first) __attribute__((always_inline)) { // the levels [p0, p0 + TOGETHER) of every sample; p0 a compile-time constant, so that no array is indexed at run time
        constexpr int p0 = decltype(first)::value;
        uint32_t tex[N][TOGETHER][4];
        float frac[N][TOGETHER][2];
        ImageLevel lr[UNIFORM ? 1 : N][TOGETHER]; // a projective item: the records of this step's levels, all loaded before the first texel address
        if (!UNIFORM) {
#pragma unroll
            for (int c = 0; c < N; ++c)
#pragma unroll
                for (int p = p0; p < p0 + TOGETHER; ++p) {
                    if (p == 1 && !both) continue;
                    const ImageLevel* at = &im.chain[level[c][p]]; // level < im.levels <= kMaxImageLevels: inside the table
                    lr[c][p - p0].offset = at->offset, lr[c][p - p0].width = at->width, lr[c][p - p0].height = at->height;
                    lr[c][p - p0].sx = at->sx, lr[c][p - p0].sy = at->sy;
                }
        }
#pragma unroll
        for (int c = 0; c < N; ++c)
#pragma unroll
            for (int p = p0; p < p0 + TOGETHER; ++p) {
                if (p == 1 && !both) continue;
                if (UNIFORM) {
                    const ImageLevel& l = uni.level[p];
                    const uint32_t* texels = l.offset == 0u ? im.texels : chain + l.offset; // wave uniform: level 0 is the image's own allocation
                    image_fetch(texels, l.width, l.height, u[c] * l.sx, v[c] * l.sy, linear, im.spread_x, im.spread_y, tex[c][p - p0], frac[c][p - p0]);
                } else {
                    const ImageLevel& l = lr[c][p - p0];
                    const uint32_t* texels = level[c][p] == 0u ? im.texels : chain + l.offset;
                    image_fetch(texels, l.width, l.height, u[c] * l.sx, v[c] * l.sy, linear, im.spread_x, im.spread_y, tex[c][p - p0], frac[c][p - p0]);
                }
            }
#pragma unroll
        for (int c = 0; c < N; ++c)
#pragma unroll
            for (int p = p0; p < p0 + TOGETHER; ++p) {
                if (p == 1 && !both) continue;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const float value = image_filter(tex[c][p - p0], frac[c][p - p0], linear, ch);
                    out[c][ch] = p == 0 ? value : out[c][ch] + f[c] * (value - out[c][ch]);
                }
            }
    };
    step(std::integral_constant<int, 0>());
    if (TOGETHER == 1 && both) step(std::integral_constant<int, 1>());
}
template <int S, int ROWS, bool OPS, bool STROKES, bool XFMT = false> // XFMT: the frame formats 3-8 (raster_common.hpp store_px)
__global__ __launch_bounds__(64 * (4 / ROWS)) __attribute__((amdgpu_waves_per_eu((OPS || STROKES || S >= 4) ? 1 : CRH_TILE_WAVES))) void k_raster_tile(SceneDev s, RasterParams r) {
    constexpr bool BLEND = false, PAINT = false, IMAGES = false, MIPS = false;
    const BlendForm bf = {}; // (not read: the blend block is compiled out)
    const PaintArgs pa = {}; // (nor this: the paint block is)
    const ImageArgs ia = {};
#include "raster_tile_body.inc"
}
// The general variant with the renderer's blend state in place of "over" (Configuration::blending; ROWS = tile_rows(S) as above)
template <int S, bool STROKES, bool XFMT = false>
__global__ __launch_bounds__(64 * tile_waves(S)) __attribute__((amdgpu_waves_per_eu(1))) void k_raster_blend(SceneDev s, RasterParams r, BlendForm bf) {
    constexpr int ROWS = tile_rows(S);
    constexpr bool OPS = true, BLEND = true, PAINT = false, IMAGES = false, MIPS = false;
    const PaintArgs pa = {};
    const ImageArgs ia = {};
#include "raster_tile_body.inc"
}
// k_raster_blend with gradient paints (crh_scene_set_paints): the colour cover of a painted item takes its source per sample from the paint
// tables `pa`; every other primitive, an unpainted item's cover included, is drawn as k_raster_blend draws it. The pass of a Scene that draws a
// painted instance runs this kernel whatever the blend state — under "over" with the blend form of "over".
template <int S, bool STROKES, bool XFMT = false>
__global__ __launch_bounds__(64 * tile_waves(S)) __attribute__((amdgpu_waves_per_eu(1))) void k_raster_paint(SceneDev s, RasterParams r, BlendForm bf, PaintArgs pa) {
    constexpr int ROWS = tile_rows(S);
    constexpr bool OPS = true, BLEND = true, PAINT = true, IMAGES = false, MIPS = false;
    const ImageArgs ia = {}; // (not read: the image block is compiled out)
#include "raster_tile_body.inc"
}
// k_raster_paint with image paints (crh_scene_set_paints_with_images): the colour cover of an image-painted item takes its source per sample from
// the texels of an RGBA8 image in HBM — CDNA has no sampler, so the wrap, the fetch (one texel for NEAREST, four for LINEAR) and the filter are
// plain code in the body's image block (IMAGES, compiled out of the three kernels above). Gradient-painted and unpainted items are drawn as
// k_raster_paint draws them. Only the pass that draws an image-painted instance through a Color cover runs this kernel.
template <int S, bool STROKES, bool XFMT = false>
__global__ __launch_bounds__(64 * tile_waves(S)) __attribute__((amdgpu_waves_per_eu(1))) void k_raster_image(SceneDev s, RasterParams r, BlendForm bf, PaintArgs pa, ImageArgs ia) {
    constexpr int ROWS = tile_rows(S);
    constexpr bool OPS = true, BLEND = true, PAINT = true, IMAGES = true, MIPS = false;
#include "raster_tile_body.inc"
}
// k_raster_image with mipmaps (CRH_FILTER_MIPMAP on an image with a level chain, crh_image_generate_mipmaps): an image paint that carries the flag takes
// its source from two levels of the chain, chosen per item (affine) or per sample (projective) by the size of a pixel in texels — the body's mipmap
// block (MIPS, compiled out of the four kernels above). Every other item, an unflagged image paint's included, is drawn as k_raster_image draws it.
// Only the pass that draws a flagged image paint through a Color cover runs this kernel.
template <int S, bool STROKES, bool XFMT = false>
__global__ __launch_bounds__(64 * tile_waves(S)) __attribute__((amdgpu_waves_per_eu(1))) void k_raster_mip(SceneDev s, RasterParams r, BlendForm bf, PaintArgs pa, ImageArgs ia) {
    constexpr int ROWS = tile_rows(S);
    constexpr bool OPS = true, BLEND = true, PAINT = true, IMAGES = true, MIPS = true;
#include "raster_tile_body.inc"
}
// crh_image_generate_mipmaps, one launch per level, one thread per texel of the level written: the rounded mean of the 2 x 2 block of the level
// above per channel, (a + b + c + d + 2) >> 2 on the codes, the block's columns and rows clamped to that level (a level one texel wide or high).
__global__ __launch_bounds__(256) void k_image_downsample(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint32_t* dst, uint32_t dst_w, uint32_t dst_h) {
    const uint32_t at = blockIdx.x * 256u + threadIdx.x; // < 2^26: a level >= 1 has at most 8192^2 texels
    if (at >= dst_w * dst_h) return;
    const uint32_t j = at / dst_w, i = at - j * dst_w;
    const uint32_t i0 = min(2u * i, src_w - 1u), i1 = min(2u * i + 1u, src_w - 1u), j0 = min(2u * j, src_h - 1u), j1 = min(2u * j + 1u, src_h - 1u);
    const uint32_t a = src[j0 * src_w + i0], b = src[j0 * src_w + i1], c = src[j1 * src_w + i0], d = src[j1 * src_w + i1];
    uint32_t out = 0u;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int sh = 8 * ch;
        out |= ((((a >> sh) & 255u) + ((b >> sh) & 255u) + ((c >> sh) & 255u) + ((d >> sh) & 255u) + 2u) >> 2) << sh;
    }
    dst[at] = out;
}
// Behind k_paint_items in an image-painted pass, one thread per draw item: the record of an item whose instance names an image paint (an
// association index at or beyond the gradients') gets paint = 0, pad = image paint + 1. The condition is k_paint_items' own, so only records
// it wrote are touched.
__global__ __launch_bounds__(64) void k_paint_items_images(RasterParams r, PaintTable t, uint32_t n_gradients) {
    const uint32_t item = blockIdx.x * 64u + threadIdx.x;
    if (item >= r.n_items) return;
    const DrawItem it = item_of(r, item);
    const int32_t paint = it.instance < t.n_instances ? t.instance_paint[it.instance] : -1;
    if (paint < (int32_t)n_gradients || (it.ops >> 4) != (uint32_t)CRH_OP_COLOR + 1u) return;
    if (r.shape_prim_begin[item + 1] > r.prim_capacity) return;
    t.items[item].paint = 0u;
    t.items[item].pad = (uint32_t)paint - n_gradients + 1u;
}

// One wavefront per draw item of a painted pass, behind k_prim_setup: an item whose instance has a paint and whose cover is Color gets its
// PaintItem record and its cover primitives the tag item + 1 (frag.flat_u, which k_prim_setup leaves 0 on every cover).
// The record holds the inverse of the item's path -> pixel homography. A Shape lies in z = 0, so clip = M (x, y, 0, 1) takes columns 0, 1, 3 and
// rows x, y, w of the instance transform; the clip -> pixel map of to_framebuffer follows, and the product is inverted in float64 (adjugate / scale).
// Evaluated here rather than on the host: the instance data is double buffered on the device and a pass that is drawn again reads the older set,
// so the record follows the very buffer k_prim_setup read.
__global__ __launch_bounds__(64) void k_paint_items(RasterParams r, PaintTable t) {
    const uint32_t item = blockIdx.x, lane = threadIdx.x;
    const DrawItem it = item_of(r, item);
    const int32_t paint = it.instance < t.n_instances ? t.instance_paint[it.instance] : -1;
    if (paint < 0 || (it.ops >> 4) != (uint32_t)CRH_OP_COLOR + 1u) return;
    const uint32_t prim0 = r.shape_prim_begin[item], prim1 = r.shape_prim_begin[item + 1];
    if (prim1 > r.prim_capacity) return; // (as k_prim_setup: cannot happen)
    if (lane == 0) {
        const float* m = r.transforms + 16u * it.instance;
        const double W = (double)r.width, H = (double)r.height;
        const double a[3][3] = {{0.5 * W * ((double)m[0] + (double)m[3]), 0.5 * W * ((double)m[4] + (double)m[7]), 0.5 * W * ((double)m[12] + (double)m[15])},
                                {0.5 * H * ((double)m[3] - (double)m[1]), 0.5 * H * ((double)m[7] - (double)m[5]), 0.5 * H * ((double)m[15] - (double)m[13])},
                                {(double)m[3], (double)m[7], (double)m[15]}};
        double inv[9] = {a[1][1] * a[2][2] - a[1][2] * a[2][1], a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1],
                         a[1][2] * a[2][0] - a[1][0] * a[2][2], a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2],
                         a[1][0] * a[2][1] - a[1][1] * a[2][0], a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]};
        const bool affine = m[3] == 0.0f && m[7] == 0.0f;
        // a homography is defined up to scale: an affine one is scaled to W == 1 (the kernel skips the division), any other to a largest entry of 1
        double scale = inv[8];
        if (!affine) {
            scale = 0.0;
            for (int i = 0; i < 9; ++i) scale = fmax(scale, fabs(inv[i]));
        }
        PaintItem out;
        bool finite = scale != 0.0;
        for (int i = 0; i < 9; ++i) {
            out.h[i] = (float)(inv[i] / scale);
            finite = finite && is_finite(out.h[i]);
        }
        if (affine) out.h[6] = 0.0f, out.h[7] = 0.0f, out.h[8] = 1.0f;
        if (!finite) // a singular transform draws nothing; the record stays harmless
            for (int i = 0; i < 9; ++i) out.h[i] = 0.0f;
        out.affine = (affine || !finite) ? 1u : 0u;
        out.paint = (uint32_t)paint;
        out.pad = 0u;
        for (int ch = 0; ch < 4; ++ch) out.tint[ch] = r.colors[4u * it.instance + ch];
        t.items[item] = out;
    }
    for (uint32_t p = prim0 + lane; p < prim1; p += 64u) {
        const PrimCoverage& cov = r.prim_rec[p].cov;
        if (cov.box.x != 0xFFFFu && ((cov.flags >> 4) & 7u) == KIND_COVER) r.prim_rec[p].frag.flat_u = item + 1u;
    }
}

// ordered premultiplied "over" of n RGBA8 layers: dst = L0 under L1 under ...
__global__ __launch_bounds__(256) void k_composite(const uint8_t* const* layers, uint32_t n_layers, uint64_t n_pixels, uint8_t* dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pixels) return;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t l = 0; l < n_layers; ++l) {
        const uchar4 p = reinterpret_cast<const uchar4*>(layers[l])[i];
        const float sr[4] = {(float)p.x * (1.0f / 255.0f), (float)p.y * (1.0f / 255.0f), (float)p.z * (1.0f / 255.0f), (float)p.w * (1.0f / 255.0f)};
        const float k = 1.0f - sr[3];
        for (int c = 0; c < 4; ++c) acc[c] = sr[c] + acc[c] * k;
    }
    uint32_t packed = 0;
    for (int c = 0; c < 4; ++c) {
        float x = acc[c] < 0.0f ? 0.0f : (acc[c] > 1.0f ? 1.0f : acc[c]);
        packed |= (uint32_t)(int)(x * 255.0f + 0.5f) << (8 * c);
    }
    reinterpret_cast<uint32_t*>(dst)[i] = packed;
}

__global__ __launch_bounds__(256) void k_state_colors_from_image(RasterParams r, uint32_t samples) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)r.width * r.height) return;
    const uint32_t gy = (uint32_t)(i / r.width), gx = (uint32_t)(i - (uint64_t)gy * r.width);
    const float4 c = r.format > CRH_FORMAT_RGBA8_ATTACHMENT ? load_px<true>(r, gx, gy) : load_pixel(r, gx, gy);
    for (uint32_t k = 0; k < samples; ++k) reinterpret_cast<float4*>(r.state_color)[i * samples + k] = c;
}

// crh_selftest_srgb: the kernels' encode on x[0, n), their decode on the 256 codes
__global__ __launch_bounds__(256) void k_selftest_srgb(const float* x, uint8_t* codes, uint64_t n, float* decoded) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) codes[i] = (uint8_t)srgb_encode(x[i]);
    if (i < 256u) decoded[i] = srgb_decode((uint32_t)i);
}

// ---------------------------------------------------------------------------------------------- launchers
static ScanJob scan_job(const uint32_t* in, uint32_t* out, uint32_t* block_sum, uint32_t n, uint32_t* max_out = nullptr) {
    return ScanJob{in, out, block_sum, n, (n + 1023u) / 1024u, max_out};
}

// transform independent: contiguous primitive ids per Shape (runs at the end of tessellation)
void launch_prim_ranges(const SceneDev& s, uint32_t* shape_ncand, uint32_t* shape_prim_begin, uint32_t* scratch, hipStream_t stream) {
    if (s.n_shapes == 0) {
        (void)hipMemsetAsync(shape_prim_begin, 0, 4, stream);
        return;
    }
    hipLaunchKernelGGL(k_shape_ncand, dim3((s.n_shapes + 255u) / 256u), dim3(256), 0, stream, s, shape_ncand);
    const ScanJob j = scan_job(shape_ncand, shape_prim_begin, scratch, s.n_shapes);
    RasterParams unused = {};
    hipLaunchKernelGGL(k_scan_local, dim3(j.blocks), dim3(256), 0, stream, j);
    hipLaunchKernelGGL(k_scan_add, dim3(j.blocks), dim3(256), 0, stream, j, unused, 0);
}
// per frame, for a recorded pass: candidate counts and contiguous primitive ids per draw item
void launch_item_ranges(const SceneDev& s, const RasterParams& r, uint32_t* item_ncand, uint32_t* item_prim_begin, uint32_t* scratch, hipStream_t stream) {
    hipLaunchKernelGGL(k_item_ncand, dim3((r.n_items + 255u) / 256u), dim3(256), 0, stream, s, r, item_ncand);
    const ScanJob j = scan_job(item_ncand, item_prim_begin, scratch, r.n_items);
    RasterParams unused = {};
    hipLaunchKernelGGL(k_scan_local, dim3(j.blocks), dim3(256), 0, stream, j);
    hipLaunchKernelGGL(k_scan_add, dim3(j.blocks), dim3(256), 0, stream, j, unused, 0);
}
template <int S>
static void launch_prim_setup_walk(const SceneDev& s, const RasterParams& r, hipStream_t stream, MarkFn mark, void* ctx, hipEvent_t after_setup) {
    if (r.n_items) {
        if (r.prim_proj)
            hipLaunchKernelGGL((k_prim_setup<S, true>), dim3(r.n_items), dim3(64), 0, stream, s, r);
        else
            hipLaunchKernelGGL((k_prim_setup<S, false>), dim3(r.n_items), dim3(64), 0, stream, s, r);
    }
    if (after_setup) (void)hipEventRecord(after_setup, stream);
    if (mark) mark(ctx, "raster_prim_setup", 0);
    if (r.n_items) hipLaunchKernelGGL((k_tile_walk<S, false>), dim3(r.n_items), dim3(64 * kWalkWaves), 0, stream, s, r);
}
// `after_setup` (optional) is recorded when k_prim_setup, the last reader of the tessellated vertex streams, has been enqueued. The three
// launchers of the triangle pass launch nothing for a sample count it does not draw (api.hip render_impl refuses such a pass up front).
void launch_bin(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, hipEvent_t after_setup) {
    if (!triangle_pass_samples(samples)) return;
    // tile_cursor, tile_count and the overflow words are adjacent: one clear ([5] belongs to the edge pass (bin_edges.hip); cleared so that the host never sees a stale flag)
    launch_clear_words(r.tile_cursor, 2u * (size_t)r.n_tiles + 8u, stream); // (single-wave workgroups: bin_edges.hip)
    switch (samples) {
        case 1: launch_prim_setup_walk<1>(s, r, stream, mark, ctx, after_setup); break;
        case 2: launch_prim_setup_walk<2>(s, r, stream, mark, ctx, after_setup); break;
        case 4: launch_prim_setup_walk<4>(s, r, stream, mark, ctx, after_setup); break;
        case 8: launch_prim_setup_walk<8>(s, r, stream, mark, ctx, after_setup); break;
    }
    if (mark) mark(ctx, "raster_tile_count", 0);
    const ScanJob j = scan_job(r.tile_count, r.tile_offset, r.scan_scratch, r.n_tiles, r.overflow + 3); // overflow[3] = longest tile list
    hipLaunchKernelGGL(k_scan_local, dim3(j.blocks), dim3(256), 0, stream, j);
    hipLaunchKernelGGL(k_scan_add, dim3(j.blocks), dim3(256), 0, stream, j, r, 1);
    if (mark) mark(ctx, "raster_tile_scan", 0);
}
// `after_fill` (optional) is recorded when the fill pass, the last reader of the per-item primitive ranges, has been enqueued
void launch_fill(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx,
                 hipEvent_t after_fill) {
    if (r.n_items) {
        switch (samples) {
            case 1: hipLaunchKernelGGL((k_tile_walk<1, true>), dim3(r.n_items), dim3(64 * kWalkWaves), 0, stream, s, r); break;
            case 2: hipLaunchKernelGGL((k_tile_walk<2, true>), dim3(r.n_items), dim3(64 * kWalkWaves), 0, stream, s, r); break;
            case 4: hipLaunchKernelGGL((k_tile_walk<4, true>), dim3(r.n_items), dim3(64 * kWalkWaves), 0, stream, s, r); break;
            case 8: hipLaunchKernelGGL((k_tile_walk<8, true>), dim3(r.n_items), dim3(64 * kWalkWaves), 0, stream, s, r); break;
        }
    }
    if (after_fill) (void)hipEventRecord(after_fill, stream);
    if (mark) mark(ctx, "raster_tile_fill", 0);
}
// The raster kernel of msaa S: k_raster_mip for a pass that draws an image paint with CRH_FILTER_MIPMAP, k_raster_image for a pass that draws an image-painted instance, k_raster_paint for a pass that draws a (gradient-)painted one, k_raster_blend for a blend state other than "over"
// (r.general is set with both), else k_raster_tile, OPS for
// clip nesting / alpha contexts / depth / projective instances
template <int S>
static void launch_raster_s(const SceneDev& s, const RasterParams& r, hipStream_t stream, dim3 grid, bool has_stroke, const BlendForm* blend, const PaintArgs* paint, const ImageArgs* images, bool mips) {
    constexpr int ROWS = tile_rows(S);
    const dim3 block(64u * tile_waves(S));
    const uint32_t lds = tile_waves(S) * r.sort_capacity * 4u;
    const bool xfmt = r.format > CRH_FORMAT_RGBA8_ATTACHMENT; // BGRA / sRGB targets: the XFMT instantiations
#define CRH_LAUNCH_TILE(OPS_, STROKES_)                                                                                   \
    do {                                                                                                                \
        if (xfmt)                                                                                                       \
            hipLaunchKernelGGL((k_raster_tile<S, ROWS, OPS_, STROKES_, true>), grid, block, lds, stream, s, r);        \
        else                                                                                                            \
            hipLaunchKernelGGL((k_raster_tile<S, ROWS, OPS_, STROKES_>), grid, block, lds, stream, s, r);              \
    } while (0)
#define CRH_LAUNCH_BLEND(STROKES_)                                                                                        \
    do {                                                                                                                \
        if (xfmt)                                                                                                       \
            hipLaunchKernelGGL((k_raster_blend<S, STROKES_, true>), grid, block, lds, stream, s, r, *blend);           \
        else                                                                                                            \
            hipLaunchKernelGGL((k_raster_blend<S, STROKES_>), grid, block, lds, stream, s, r, *blend);                 \
    } while (0)
#define CRH_LAUNCH_PAINT(STROKES_)                                                                                        \
    do {                                                                                                                \
        if (xfmt)                                                                                                       \
            hipLaunchKernelGGL((k_raster_paint<S, STROKES_, true>), grid, block, lds, stream, s, r, *blend, *paint);   \
        else                                                                                                            \
            hipLaunchKernelGGL((k_raster_paint<S, STROKES_>), grid, block, lds, stream, s, r, *blend, *paint);         \
    } while (0)
#define CRH_LAUNCH_IMAGE(STROKES_)                                                                                                 \
    do {                                                                                                                         \
        if (xfmt)                                                                                                                \
            hipLaunchKernelGGL((k_raster_image<S, STROKES_, true>), grid, block, lds, stream, s, r, *blend, *paint, *images);   \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_raster_image<S, STROKES_>), grid, block, lds, stream, s, r, *blend, *paint, *images);         \
    } while (0)
#define CRH_LAUNCH_MIP(STROKES_)                                                                                                   \
    do {                                                                                                                         \
        if (xfmt)                                                                                                                \
            hipLaunchKernelGGL((k_raster_mip<S, STROKES_, true>), grid, block, lds, stream, s, r, *blend, *paint, *images);     \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_raster_mip<S, STROKES_>), grid, block, lds, stream, s, r, *blend, *paint, *images);           \
    } while (0)
    if (blend && paint && images && mips) {
        if (has_stroke) CRH_LAUNCH_MIP(true); else CRH_LAUNCH_MIP(false);
    } else if (blend && paint && images) {
        if (has_stroke) CRH_LAUNCH_IMAGE(true); else CRH_LAUNCH_IMAGE(false);
    } else if (blend && paint) {
        if (has_stroke) CRH_LAUNCH_PAINT(true); else CRH_LAUNCH_PAINT(false);
    } else if (blend) {
        if (has_stroke) CRH_LAUNCH_BLEND(true); else CRH_LAUNCH_BLEND(false);
    } else if (r.general) {
        if (has_stroke) CRH_LAUNCH_TILE(true, true); else CRH_LAUNCH_TILE(true, false);
    } else {
        if (has_stroke) CRH_LAUNCH_TILE(false, true); else CRH_LAUNCH_TILE(false, false);
    }
#undef CRH_LAUNCH_TILE
#undef CRH_LAUNCH_BLEND
#undef CRH_LAUNCH_PAINT
#undef CRH_LAUNCH_IMAGE
#undef CRH_LAUNCH_MIP
}
void launch_paint_items(const RasterParams& r, const PaintTable& t, hipStream_t stream) {
    if (r.n_items) hipLaunchKernelGGL(k_paint_items, dim3(r.n_items), dim3(64), 0, stream, r, t);
}
void launch_paint_items_images(const RasterParams& r, const PaintTable& t, uint32_t n_gradients, hipStream_t stream) {
    if (r.n_items) hipLaunchKernelGGL(k_paint_items_images, dim3((r.n_items + 63u) / 64u), dim3(64), 0, stream, r, t, n_gradients);
}
// One level of an image's chain from the level above it (crh_image_generate_mipmaps)
void launch_image_downsample(const uint32_t* src, uint32_t src_w, uint32_t src_h, uint32_t* dst, uint32_t dst_w, uint32_t dst_h, hipStream_t stream) {
    hipLaunchKernelGGL(k_image_downsample, dim3((dst_w * dst_h + 255u) / 256u), dim3(256), 0, stream, src, src_w, src_h, dst, dst_w, dst_h);
}
// -> RasterVariant (0: nothing launched)
uint32_t launch_raster(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx,
                   uint64_t raster_bytes, bool has_stroke, const BlendForm* blend, const PaintArgs* paint, const ImageArgs* images, bool mips) {
    // 8x8-tile blocks, an equal number per XCD (k_raster_tile's tile order)
    constexpr uint32_t kBlock = 1u << CRH_XCD_BLOCK_LOG2;
    const uint32_t blocks = ((r.tiles_x + kBlock - 1u) / kBlock) * ((r.tiles_y + kBlock - 1u) / kBlock);
    const dim3 grid((r.tile_order && r.order_places) ? r.order_places : ((blocks + 7u) / 8u) * kBlock * kBlock * 8u);
    switch (samples) {
        case 1: launch_raster_s<1>(s, r, stream, grid, has_stroke, blend, paint, images, mips); break;
        case 2: launch_raster_s<2>(s, r, stream, grid, has_stroke, blend, paint, images, mips); break;
        case 4: launch_raster_s<4>(s, r, stream, grid, has_stroke, blend, paint, images, mips); break;
        case 8: launch_raster_s<8>(s, r, stream, grid, has_stroke, blend, paint, images, mips); break;
        default: return 0u;
    }
    if (mark) mark(ctx, "raster_tiles", raster_bytes);
    return (r.general || blend) ? kRasterOps : kRasterTile;
}
// exported to bin_edges.hip
void launch_scan_u32(const uint32_t* in, uint32_t* out, uint32_t* block_sum, uint32_t n, hipStream_t stream) {
    const ScanJob j = scan_job(in, out, block_sum, n);
    RasterParams unused = {};
    hipLaunchKernelGGL(k_scan_local, dim3(j.blocks), dim3(256), 0, stream, j);
    hipLaunchKernelGGL(k_scan_add, dim3(j.blocks), dim3(256), 0, stream, j, unused, 0);
}
void launch_scan_u32_pair(const uint32_t* in0, uint32_t* out0, uint32_t* block_sum0, const uint32_t* in1, uint32_t* out1, uint32_t* block_sum1, uint32_t n, hipStream_t stream) {
    const ScanJob a = scan_job(in0, out0, block_sum0, n), b = scan_job(in1, out1, block_sum1, n);
    hipLaunchKernelGGL(k_scan_local2, dim3(a.blocks, 2), dim3(256), 0, stream, a, b);
    hipLaunchKernelGGL(k_scan_add2, dim3(a.blocks, 2), dim3(256), 0, stream, a, b);
}
void launch_scan_tiles(const RasterParams& r, hipStream_t stream) { // tile_count -> tile_offset; publishes the pair total and the longest list
    const ScanJob j = scan_job(r.tile_count, r.tile_offset, r.scan_scratch, r.n_tiles, r.overflow + 3);
    hipLaunchKernelGGL(k_scan_local, dim3(j.blocks), dim3(256), 0, stream, j);
    hipLaunchKernelGGL(k_scan_add, dim3(j.blocks), dim3(256), 0, stream, j, r, 1);
}
// A frame that starts keeping its pass state while it already shows an image: every sample of a pixel starts from the pixel's resolved colour
// (what a pass over existing content has always read, load_pixel).
void launch_state_colors_from_image(const RasterParams& r, uint32_t samples, hipStream_t stream) {
    const uint64_t n = (uint64_t)r.width * r.height;
    hipLaunchKernelGGL(k_state_colors_from_image, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, r, samples);
}
void launch_selftest_srgb(const float* x, uint8_t* codes, uint64_t n, float* decoded, hipStream_t stream) {
    const uint64_t threads = n > 256u ? n : 256u;
    hipLaunchKernelGGL(k_selftest_srgb, dim3((uint32_t)((threads + 255u) / 256u)), dim3(256), 0, stream, x, codes, n, decoded);
}
void launch_composite(const uint8_t* const* layers_dev, uint32_t n_layers, uint64_t n_pixels, uint8_t* dst, hipStream_t stream) {
    hipLaunchKernelGGL(k_composite, dim3((uint32_t)((n_pixels + 255) / 256)), dim3(256), 0, stream, layers_dev, n_layers, n_pixels, dst);
}

} // namespace crh
