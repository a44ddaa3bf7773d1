// csrc/bin_edges.hip — the binning half of the edge pass (formulation and slot layout: edge_slots.hpp): per draw item the slots are set up
// and their keys binned into the tiles' lists in ONE traversal, and the ranges and scans around it.
//
//   k_bin_edges<S, Q>  ONE traversal per draw item: waves 0-1 set up and walk the triangles, waves 2-3 the boundary edges (fill chain +
//                      hull chain) over the item's tile rectangle; per tile they count entries (one atomic), sum the backdrop (one lane per
//                      edge, ballots) and append (tile, key) pairs to a wave-private LDS stage that is flushed to the pair stream in blocks
//                      (one atomic per block). Q: the items k_bin_flat queued.
//   k_bin_flat<S, T, R> the same binning with the lanes packed ACROSS draw items: a batch of consecutive items per workgroup of T threads;
//                      the host cuts a pass into batches (flat_batches, flat_batch_limits, flat_threads_for) or sends it item by item (bin_itemwise).
//                      R: the entries' places are taken from records of the first walk's hits instead of from a second walk (CRH_BIN_REPLAY).
//   k_scatter          pair -> its slot in the tile's list (offsets from the scan of the counts).
//   the ranges         k_item_nslots / k_shape_counts and the single-wave scans: slots per item or Shape and their prefixes (launch_slot_ranges,
//                      launch_plain_ranges); k_tile_caps: the places of the next frames' lists (launch_tile_bases); k_shape_bounds, k_slab_items:
//                      which items miss the slab of a multi-GPU pass.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "edge_slots.hpp"
#include "launch.hpp"

namespace crh {

// What the primitives of one draw item are set up from: gathered once per item (a wavefront's scalar registers in k_bin_edges, an LDS
// record in k_bin_flat) instead of through the Shape's rows of shape_base per primitive.
struct ItemCtx {
    uint32_t shape, instance, dyn0;
    uint32_t lv0, jn0, iq0, ic0, rq0, rc0, hull0, sv0; // the Shape's first record in every stream
    uint32_t cb[8];                                    // shape_candidates()
    float m0, m4, m12, m1, m5, m13;                    // the rows of the instance matrix to_framebuffer() uses
    float col[4];                                      // straight-alpha colour of the instance
};
CRH_D ItemCtx item_ctx(const SceneDev& s, const RasterParams& r, const DrawItem& it, const uint32_t cb[8]) {
    ItemCtx c;
    const uint32_t* b0 = s.shape_base + it.shape * kShapeRow;
    c.shape = it.shape, c.instance = it.instance, c.dyn0 = s.shape_dyn_begin[it.shape];
    c.lv0 = b0[CH_LINE_V], c.jn0 = b0[CH_JOINT], c.iq0 = b0[CH_IQ], c.ic0 = b0[CH_IC_V], c.rq0 = b0[CH_RQ], c.rc0 = b0[CH_RC_V], c.hull0 = b0[CH_HULL], c.sv0 = b0[CH_SOLID_V];
#pragma unroll
    for (int i = 0; i < 8; ++i) c.cb[i] = cb[i];
    const float* m = r.transforms + 16u * it.instance;
    c.m0 = m[0], c.m4 = m[4], c.m12 = m[12], c.m1 = m[1], c.m5 = m[5], c.m13 = m[13];
    const float* color = r.colors + 4u * it.instance;
    c.col[0] = color[0], c.col[1] = color[1], c.col[2] = color[2], c.col[3] = color[3];
    return c;
}
CRH_D float2 to_framebuffer(const ItemCtx& c, float w, float h, float x, float y) { // raster_common.hpp to_framebuffer, operation for operation
    const float cx = (c.m0 * x + c.m4 * y) + c.m12;
    const float cy = (c.m1 * x + c.m5 * y) + c.m13;
    return make_float2((cx * 0.5f + 0.5f) * w, (0.5f - cy * 0.5f) * h);
}
// The tile split of the multi-GPU path: does the item's Shape, as this instance places it, miss the rows of the pass' slab altogether? Then the
// binning kernels need not set its primitives up (one rank of eight used to set all 100 000 items of config 4 up to find that 7 in 8 have no row
// in its slab). The box is the Shape's own (k_shape_bounds), its four corners go through the instance's affine map — the extremes of y are at
// corners —, a tile row of margin absorbs the rounding of that map against the vertices' own. Unbounded boxes (stroked Shapes, degenerate hulls)
// and anything not finite never pass the test.
CRH_D bool item_misses_slab(const RasterParams& r, const DrawItem& it) {
    if (!r.shape_bounds) return false;
    const float* bb = r.shape_bounds + 4u * it.shape;
    const float* m = r.transforms + 16u * it.instance;
    const float m1 = m[1], m5 = m[5], m13 = m[13]; // (the row of the instance matrix to_framebuffer() takes y from)
    const float y00 = (m1 * bb[0] + m5 * bb[1]) + m13, y10 = (m1 * bb[2] + m5 * bb[1]) + m13, y01 = (m1 * bb[0] + m5 * bb[3]) + m13, y11 = (m1 * bb[2] + m5 * bb[3]) + m13;
    const float h = (float)r.height;
    const float cy_hi = fmaxf(fmaxf(y00, y10), fmaxf(y01, y11)), cy_lo = fminf(fminf(y00, y10), fminf(y01, y11));
    const float top = (0.5f - cy_hi * 0.5f) * h, bottom = (0.5f - cy_lo * 0.5f) * h; // (to_framebuffer: y grows downwards)
    const float slab_top = (float)(r.slab_ty0 * kTile), slab_bottom = (float)(min(r.slab_ty1, r.tiles_y) * kTile);
    const bool finite = is_finite(y00) && is_finite(y10) && is_finite(y01) && is_finite(y11);
    return finite && (bottom + (float)kTile < slab_top || top - (float)kTile >= slab_bottom);
}
__global__ __launch_bounds__(256) void k_shape_bounds(SceneDev s, float* bounds) {
    const uint32_t shape = blockIdx.x * 256u + threadIdx.x;
    if (shape >= s.n_shapes) return;
    const uint32_t* b0 = s.shape_base + shape * kShapeRow;
    const uint32_t* b1 = b0 + NCH;
    const uint32_t hn = s.hull_count[shape];
    const float inf = __uint_as_float(0x7f800000u);
    float4 box = make_float4(-inf, -inf, inf, inf); // unbounded: never left out
    // a filled Shape draws polygon vertices and curve control points — all of them hull candidates (fill.rs:263-367), so the hull's box holds
    // them; a stroked one also draws join triangles around the path's own control points (stroke.rs:53-121), which an offset stroke leaves outside
    const bool stroked = (b1[CH_LINE_V] - b0[CH_LINE_V]) + (b1[CH_JOINT] - b0[CH_JOINT]) != 0u;
    if (!stroked && hn >= 3u) {
        box = make_float4(inf, inf, -inf, -inf);
        const Vertex0* v = s.hull_v + b0[CH_HULL];
        for (uint32_t i = 0; i < hn; ++i) box.x = fminf(box.x, v[i].x), box.y = fminf(box.y, v[i].y), box.z = fmaxf(box.z, v[i].x), box.w = fmaxf(box.w, v[i].y);
    }
    reinterpret_cast<float4*>(bounds)[shape] = box;
}
void launch_shape_bounds(const SceneDev& s, float* bounds, hipStream_t stream) {
    if (s.n_shapes) hipLaunchKernelGGL(k_shape_bounds, dim3((s.n_shapes + 255u) / 256u), dim3(256), 0, stream, s, bounds);
}
// one lane per item of a pass with a slab: r.item_elsewhere[item] = the item misses the slab. (A kernel of its own in front of the binning kernels:
// the test inside k_bin_flat's first phase cost that kernel its last free registers — 12 B of scratch, whose accesses wait with the record stores.)
__global__ __launch_bounds__(256) void k_slab_items(RasterParams r, uint8_t* elsewhere) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item < r.n_items) elsewhere[item] = item_misses_slab(r, item_of(r, item)) ? 1u : 0u;
}
void launch_slab_items(const RasterParams& r, uint8_t* elsewhere, hipStream_t stream) {
    if (r.n_items) hipLaunchKernelGGL(k_slab_items, dim3((r.n_items + 255u) / 256u), dim3(256), 0, stream, r, elsewhere);
}
__global__ __launch_bounds__(256) void k_item_nslots(SceneDev s, RasterParams r, uint32_t n_items, uint32_t* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    out[i] = item_slots(s, item_of(r, i)).total;
}

// ---------------------------------------------------------------------------------------------- triangle setup (plain instances)
// oracle/raster.hpp setup_triangle + setup_attribute for candidate c of the Shape (lines, joints, curve lists); false: nothing to draw
// In four steps, so that k_bin_flat can keep its global loads in front of its record stores and hold no more of a triangle than the step at hand
// needs: the loads; the vertices on the frame (false: nothing to draw); the coverage half; the fragment half. setup_plain_triangle is all four.
struct PlainTri {
    float2 p[3];
    float attr[3][4];
    uint32_t kind, flat_u, desc;
    float end_y;
    int n_attr;
    bool valid;
};
#ifndef CRH_BIN_LOADS_TRIS
#define CRH_BIN_LOADS_TRIS 1 // 0: a branch per kind with its own loads and its own wait (A/B runs)
#endif
// The values the compiler is told nothing about any more: they are in their registers HERE. Behind the last of a group of global loads this keeps
// the loads in front of it and together — left alone the compiler sinks every load to its first use, into whatever branch consumes it, and a
// wavefront then waits for memory once per branch instead of once per group.
template <class T>
CRH_D void held(T& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(T) == 4, "one vector register");
    asm volatile("" : "+v"(v));
#endif
}
#if CRH_BIN_LOADS_TRIS
// A triangle's three vertices as they lie in memory, whatever its kind: the seven vertex streams differ in base and stride only (2, 4, 5 or 6 words
// a vertex), and a triangle is three consecutive vertices of one of them. Every lane issues the same nine 8-byte loads — words 0-1 of each vertex, the
// pair that holds words 2-3, the pair that ends with the vertex' last word — at addresses chosen with selects, so a wavefront of mixed kinds waits
// once, and no pair reaches beyond its own vertex (the last vertex of a stream is the last thing allocated).
struct __attribute__((may_alias)) WordPair {
    float a, b;
};
struct TriRaw {
    WordPair xy[3], mid[3], end[3];
    uint32_t cut, which; // line_pair_cut of a stroke line's pair; which: 0 line, 1 joint, 2 IQ, 3 IC, 4 RQ, 5 RC, 6 hull strip
};
CRH_D uint32_t tri_stride(uint32_t which) { // words per vertex: Vertex2f1i, Vertex3f1i, Vertex2f, Vertex3f, Vertex3f, Vertex4f, Vertex0
    return which == 6u ? 2u : (which == 2u ? 4u : ((which == 1u || which == 5u) ? 6u : 5u));
}
CRH_D void issue_plain_triangle(const SceneDev& s, const ItemCtx& ctx, uint32_t c, TriRaw& raw) {
    const uint32_t* cb = ctx.cb;
    const uint32_t which = (c >= cb[0] ? 1u : 0u) + (c >= cb[1] ? 1u : 0u) + (c >= cb[3] ? 1u : 0u) + (c >= cb[4] ? 1u : 0u) + (c >= cb[5] ? 1u : 0u) + (c >= cb[6] ? 1u : 0u);
    const uint32_t q = c - cb[0], jn = q / 3u, jk = q - 3u * jn;
    // the first vertex and the strip position's parity (strips: odd positions take their last two vertices swapped)
    const uint32_t first = which == 0u ? ctx.lv0 + c
                         : which == 1u ? 5u * (ctx.jn0 + jn) + jk
                         : which == 2u ? 3u * (ctx.iq0 + (c - cb[2]))
                         : which == 3u ? ctx.ic0 + 3u * (c - cb[3])
                         : which == 4u ? 3u * (ctx.rq0 + (c - cb[4]))
                         : which == 5u ? ctx.rc0 + 3u * (c - cb[5])
                                       : ctx.hull0 + (c - cb[6]);
    const uint32_t odd = which == 0u ? (c & 1u) : (which == 1u ? (jk & 1u) : (which == 6u ? ((c - cb[6]) & 1u) : 0u));
    const float* base = which == 0u ? reinterpret_cast<const float*>(s.line_v)
                      : which == 1u ? reinterpret_cast<const float*>(s.joint_v)
                      : which == 2u ? reinterpret_cast<const float*>(s.iq_v)
                      : which == 3u ? reinterpret_cast<const float*>(s.ic_v)
                      : which == 4u ? reinterpret_cast<const float*>(s.rq_v)
                      : which == 5u ? reinterpret_cast<const float*>(s.rc_v)
                                    : reinterpret_cast<const float*>(s.hull_v);
    const uint32_t stride = tri_stride(which), mid = min(2u, stride - 2u), end = min(4u, stride - 2u);
    const uint32_t at[3] = {first, first + 1u + odd, first + 2u - odd};
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const float* pv = base + (size_t)at[v] * stride;
        raw.xy[v] = *reinterpret_cast<const WordPair*>(pv);
        raw.mid[v] = *reinterpret_cast<const WordPair*>(pv + mid);
        raw.end[v] = *reinterpret_cast<const WordPair*>(pv + end);
    }
    raw.cut = 0u;
    if (which == 0u) raw.cut = s.line_pair_cut[(ctx.lv0 + c) >> 1];
    raw.which = which;
}
CRH_D void hold_plain_triangle(TriRaw& raw) {
#pragma unroll
    for (int v = 0; v < 3; ++v) held(raw.xy[v].a), held(raw.xy[v].b), held(raw.mid[v].a), held(raw.mid[v].b), held(raw.end[v].a), held(raw.end[v].b);
    held(raw.cut);
}
// the fields by kind (the words themselves: a record keeps its bits)
CRH_D void finish_plain_triangle(const ItemCtx& ctx, const TriRaw& raw, PlainTri& out) {
    const uint32_t which = raw.which, stride = tri_stride(which);
    const int n_attr = which == 6u ? 0 : (which == 5u ? 4 : ((which == 0u || which == 2u) ? 2 : 3));
    const bool stroke = which <= 1u;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        out.p[v] = make_float2(raw.xy[v].a, raw.xy[v].b);
        out.attr[v][0] = n_attr > 0 ? raw.mid[v].a : 0.0f;
        out.attr[v][1] = n_attr > 1 ? raw.mid[v].b : 0.0f;
        out.attr[v][2] = n_attr > 2 ? (stride == 6u ? raw.end[v].a : raw.end[v].b) : 0.0f;
        out.attr[v][3] = n_attr > 3 ? raw.end[v].b : 0.0f;
    }
    out.flat_u = stroke ? __float_as_uint(raw.end[0].b) : 0u; // (the provoking vertex' integer is its last word)
    out.end_y = which == 0u ? raw.mid[0].b : 0.0f;
    out.desc = stroke ? ctx.dyn0 + (out.flat_u & 65535u) : 0u;
    out.kind = which == 0u ? (uint32_t)KIND_LINE : which == 1u ? (uint32_t)KIND_JOINT : which == 2u ? (uint32_t)KIND_IQ : which == 3u ? (uint32_t)KIND_IC : which == 4u ? (uint32_t)KIND_RQ : which == 5u ? (uint32_t)KIND_RC : EK_COVER_TRI;
    out.n_attr = n_attr;
    out.valid = raw.cut == 0u;
}
CRH_D void load_plain_triangle(const SceneDev& s, const ItemCtx& ctx, uint32_t c, PlainTri& out) {
    TriRaw raw;
    issue_plain_triangle(s, ctx, c, raw);
    hold_plain_triangle(raw);
    finish_plain_triangle(ctx, raw, out);
}
#else
CRH_D void load_plain_triangle(const SceneDev& s, const ItemCtx& ctx, uint32_t c, PlainTri& out) {
    const uint32_t* cb = ctx.cb;
    const uint32_t dyn0 = ctx.dyn0;
    float2 p[3];
    float attr[3][4] = {};
    uint32_t kind, flat_u = 0, desc = 0;
    float end_y = 0.0f;
    int n_attr;
    bool valid = true;
    if (c < cb[0]) { // stroke line strips
        const uint32_t lv0 = ctx.lv0, k = c;
        valid = s.line_pair_cut[(lv0 + k) >> 1] == 0;
        const uint32_t i0 = lv0 + k, i1 = lv0 + ((k & 1u) ? k + 2u : k + 1u), i2 = lv0 + ((k & 1u) ? k + 1u : k + 2u);
        const Vertex2f1i a = s.line_v[i0], b = s.line_v[i1], d = s.line_v[i2];
        p[0] = make_float2(a.x, a.y), p[1] = make_float2(b.x, b.y), p[2] = make_float2(d.x, d.y);
        attr[0][0] = a.u, attr[0][1] = a.v, attr[1][0] = b.u, attr[1][1] = b.v, attr[2][0] = d.u, attr[2][1] = d.v;
        flat_u = a.i;
        end_y = a.v;
        desc = dyn0 + (a.i & 65535u);
        kind = KIND_LINE;
        n_attr = 2;
    } else if (c < cb[1]) { // joint strips: 5 vertices, 3 triangles per join
        const uint32_t q = c - cb[0], jn = q / 3u, k = q - 3u * jn, base = 5u * (ctx.jn0 + jn);
        const uint32_t i0 = base + k, i1 = base + ((k & 1u) ? k + 2u : k + 1u), i2 = base + ((k & 1u) ? k + 1u : k + 2u);
        const Vertex3f1i a = s.joint_v[i0], b = s.joint_v[i1], d = s.joint_v[i2];
        p[0] = make_float2(a.x, a.y), p[1] = make_float2(b.x, b.y), p[2] = make_float2(d.x, d.y);
        attr[0][0] = a.u, attr[0][1] = a.v, attr[0][2] = a.w, attr[1][0] = b.u, attr[1][1] = b.v, attr[1][2] = b.w, attr[2][0] = d.u, attr[2][1] = d.v, attr[2][2] = d.w;
        flat_u = a.i;
        desc = dyn0 + (flat_u & 65535u);
        kind = KIND_JOINT;
        n_attr = 3;
    } else if (c < cb[3]) {
        const uint32_t at = 3u * (ctx.iq0 + (c - cb[2]));
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const Vertex2f a = s.iq_v[at + v];
            p[v] = make_float2(a.x, a.y);
            attr[v][0] = a.u, attr[v][1] = a.v;
        }
        kind = KIND_IQ;
        n_attr = 2;
    } else if (c < cb[4]) {
        const uint32_t at = ctx.ic0 + 3u * (c - cb[3]);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const Vertex3f a = s.ic_v[at + v];
            p[v] = make_float2(a.x, a.y);
            attr[v][0] = a.u, attr[v][1] = a.v, attr[v][2] = a.w;
        }
        kind = KIND_IC;
        n_attr = 3;
    } else if (c < cb[5]) {
        const uint32_t at = 3u * (ctx.rq0 + (c - cb[4]));
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const Vertex3f a = s.rq_v[at + v];
            p[v] = make_float2(a.x, a.y);
            attr[v][0] = a.u, attr[v][1] = a.v, attr[v][2] = a.w;
        }
        kind = KIND_RQ;
        n_attr = 3;
    } else if (c < cb[6]) {
        const uint32_t at = ctx.rc0 + 3u * (c - cb[5]);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const Vertex4f a = s.rc_v[at + v];
            p[v] = make_float2(a.x, a.y);
            attr[v][0] = a.k, attr[v][1] = a.l, attr[v][2] = a.m, attr[v][3] = a.n;
        }
        kind = KIND_RC;
        n_attr = 4;
    } else { // a triangle of the hull strip as a cover triangle (hull strips whose triangles face both ways)
        const uint32_t k = c - cb[6], hull0 = ctx.hull0;
        const Vertex0 a = s.hull_v[hull0 + k], b = s.hull_v[hull0 + ((k & 1u) ? k + 2u : k + 1u)], d = s.hull_v[hull0 + ((k & 1u) ? k + 1u : k + 2u)];
        p[0] = make_float2(a.x, a.y), p[1] = make_float2(b.x, b.y), p[2] = make_float2(d.x, d.y);
        kind = EK_COVER_TRI;
        n_attr = 0;
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        out.p[v] = p[v];
#pragma unroll
        for (int a = 0; a < 4; ++a) out.attr[v][a] = attr[v][a];
    }
    out.kind = kind, out.flat_u = flat_u, out.desc = desc, out.end_y = end_y, out.n_attr = n_attr, out.valid = valid;
}
#endif
// the vertices on the frame (t.p), the determinant and the pixel box; false: nothing to draw
CRH_D bool place_plain_triangle(const RasterParams& r, const ItemCtx& ctx, PlainTri& t, float& det_out, ushort4& box) {
    const float W = (float)r.width, H = (float)r.height;
    float2* p = t.p;
#pragma unroll
    for (int v = 0; v < 3; ++v) p[v] = to_framebuffer(ctx, W, H, p[v].x, p[v].y);
    const float d1x = p[1].x - p[0].x, d1y = p[1].y - p[0].y;
    const float d2x = p[2].x - p[0].x, d2y = p[2].y - p[0].y;
    const float det = d1x * d2y - d2x * d1y;
    det_out = det;
    if (!(t.valid && det != 0.0f && det == det && is_finite(det))) return false;
    const float minx = fminf(p[0].x, fminf(p[1].x, p[2].x)), maxx = fmaxf(p[0].x, fmaxf(p[1].x, p[2].x));
    const float miny = fminf(p[0].y, fminf(p[1].y, p[2].y)), maxy = fmaxf(p[0].y, fmaxf(p[1].y, p[2].y));
    const bool nan_free = minx == minx && maxx == maxx && miny == miny && maxy == maxy;
    const int x0 = (int)floorf(fminf(fmaxf(minx, 0.0f), W)), x1 = (int)floorf(fmaxf(fminf(maxx, W - 1.0f), -1.0f));
    const int y0 = (int)floorf(fminf(fmaxf(miny, 0.0f), H)), y1 = (int)floorf(fmaxf(fminf(maxy, H - 1.0f), -1.0f));
    if (!(nan_free && x0 <= x1 && y0 <= y1)) return false;
    box = make_ushort4((unsigned short)x0, (unsigned short)x1, (unsigned short)y0, (unsigned short)y1);
    return true;
}
// (cov.box is the caller's: place_plain_triangle's)
CRH_D void plain_triangle_coverage(const PlainTri& t, float det, PrimCoverage& cov) {
    const float2* p = t.p;
    const bool front = det < 0.0f;
    const float2 nv[3] = {p[0], det < 0.0f ? p[2] : p[1], det < 0.0f ? p[1] : p[2]};
    uint32_t flags = (front ? 8u : 0u) | (t.kind << 4);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float2 a = nv[i], b = nv[(i + 1) % 3];
        const float dx = b.x - a.x, dy = b.y - a.y;
        if (dy < 0.0f || (dy == 0.0f && dx > 0.0f)) flags |= 1u << i;
        const bool flip = !(a.x < b.x || (a.x == b.x && a.y < b.y));
        const float2 el = flip ? b : a, eh = flip ? a : b;
        const float sg = flip ? -1.0f : 1.0f;
        cov.lo_x[i] = el.x;
        cov.lo_y[i] = el.y;
        cov.bx[i] = (eh.x - el.x) * sg;
        cov.nay[i] = -(eh.y - el.y) * sg;
    }
    cov.flags = flags;
    cov.desc = t.desc;
}
CRH_D void plain_triangle_fragment(const ItemCtx& ctx, const PlainTri& t, float det, PrimFragment& frag) {
    const float2* p = t.p;
    const float d1x = p[1].x - p[0].x, d1y = p[1].y - p[0].y;
    const float d2x = p[2].x - p[0].x, d2y = p[2].y - p[0].y;
    const float inv_det = 1.0f / det;
    const int n_attr = t.n_attr;
#pragma unroll
    for (int a = 0; a < 4; ++a) { // selects, not branches on the run-time n_attr: those made the compiler index the record in scratch memory (40 B per lane,
        // and every scratch access is a vector-memory operation that waits for the record stores in flight)
        const float da1 = t.attr[1][a] - t.attr[0][a], da2 = t.attr[2][a] - t.attr[0][a];
        const bool on = a < n_attr;
        frag.a0[a] = on ? t.attr[0][a] : 0.0f;
        frag.gx[a] = on ? (da1 * d2y - da2 * d1y) * inv_det : 0.0f;
        frag.gy[a] = on ? (da2 * d1x - da1 * d2x) * inv_det : 0.0f;
    }
    if (t.kind == EK_COVER_TRI) { // color_cover: (rgb * a, a), shaders.wgsl:304-309
        const float* color = ctx.col;
        frag.a0[0] = color[0] * color[3], frag.a0[1] = color[1] * color[3], frag.a0[2] = color[2] * color[3], frag.a0[3] = color[3];
    }
    frag.v0x = p[0].x;
    frag.v0y = p[0].y;
    frag.flat_u = t.flat_u;
    frag.end_y = t.end_y;
}
CRH_D bool setup_plain_triangle(const SceneDev& s, const RasterParams& r, const ItemCtx& ctx, uint32_t c, PrimRec& rec) {
    PlainTri t;
    load_plain_triangle(s, ctx, c, t);
    float det;
    ushort4 box;
    if (!place_plain_triangle(r, ctx, t, det, box)) return false;
    rec.cov.box = box;
    plain_triangle_coverage(t, det, rec.cov);
    plain_triangle_fragment(ctx, t, det, rec.frag);
    return true;
}

// ---------------------------------------------------------------------------------------------- pair stage
// (tile, position in the tile's list, key) triples of one wavefront, staged in LDS and written out in blocks with coalesced stores. The
// position comes from the returning atomic on the tile's counter (addresses spread over the frame), so k_scatter needs no atomics. The
// pair stream is cut into kSubStreams regions with a cursor each — a wavefront's blocks go to the regions in turn: ONE cursor for
// the whole frame serialises ~10^4 same-address atomics in L2 and was measured to cost more than all the binning arithmetic.
constexpr uint32_t kStage = 512;
constexpr uint32_t kSubStreams = 64;
struct Stage {
    uint32_t* tile;
    uint32_t* pos;
    uint32_t* key;
    uint32_t used;
    uint32_t sub; // the sub-stream of the wavefront's next block
    uint32_t cap; // entries the wavefront's stage holds (flushed when fewer than 64 are free)
    uint32_t at;  // k_bin_flat: where the wavefront's next block goes in the pair stream — its share of the range the workgroup reserved (0xFFFFFFFF: dropped)
};
// direct tile lists (RasterParams::direct): the staged entries go where they belong
CRH_D void stage_flush_direct(Stage& st, const RasterParams& r, uint32_t lane) {
    for (uint32_t i = lane; i < st.used; i += 64u) {
        const uint32_t t = st.tile[i], p = st.pos[i], base = r.tile_base[t];
        if (p < r.tile_base[t + 1u] - base && base + p < r.pair_capacity) r.tile_list[base + p] = st.key[i]; // (places computed on the device may run beyond the buffer: seen here, drawn again)
        else r.overflow[0] = 1u; // the tile has outgrown the place the previous frame left it
    }
    __builtin_amdgcn_wave_barrier();
    st.used = 0u;
}
CRH_D void stage_flush(Stage& st, const RasterParams& r, uint32_t lane) {
    if (st.used == 0u) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (r.direct) return stage_flush_direct(st, r, lane);
    const uint32_t region = r.pair_capacity / kSubStreams;
    uint32_t base = 0;
    if (lane == 0u) {
#ifdef CRH_ABLATE
        if (r.debug & 262144u) base = (st.sub * 7919u) % (region / 2u); else
#endif
        base = atomicAdd(&r.pair_cursor[st.sub], st.used);
        if (base + st.used > region) r.overflow[5] = 1u; // this region is full: the host grows the stream and runs the pass again
    }
    base = __shfl(base, 0, 64);
    const uint32_t first = st.sub * region;
    for (uint32_t i = lane; i < st.used; i += 64u)
        if (base + i < region) {
            r.pair_tile[first + base + i] = st.tile[i];
            r.pair_pos[first + base + i] = st.pos[i];
            r.pair_key[first + base + i] = st.key[i];
        }
    __builtin_amdgcn_wave_barrier();
    st.used = 0u;
    st.sub = (st.sub + 7u) % kSubStreams; // the next block goes to another region: one huge Shape must not fill a single region
}
// k_bin_flat: the wavefront's block goes to the range reserved for it (no atomic, no wait: coalesced stores only)
CRH_D void stage_flush_reserved(Stage& st, const RasterParams& r, uint32_t lane) {
    if (st.used == 0u) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (r.direct) return stage_flush_direct(st, r, lane);
#ifdef CRH_ABLATE
    if (r.debug & 2097152u) st.at = 0xFFFFFFFFu; // tools/ablate_flat.sh: no pair stores
#endif
    if (st.at != 0xFFFFFFFFu) {
        for (uint32_t i = lane; i < st.used; i += 64u) {
            r.pair_tile[st.at + i] = st.tile[i];
            r.pair_pos[st.at + i] = st.pos[i];
            r.pair_key[st.at + i] = st.key[i];
        }
        st.at += st.used;
    }
    __builtin_amdgcn_wave_barrier();
    st.used = 0u;
}
CRH_D uint32_t lanes_below(unsigned long long ballot, uint32_t lane) { return (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull)); }
// the lanes of `ballot` append one entry each
template <bool RESERVED = false>
CRH_D void stage_append(Stage& st, const RasterParams& r, uint32_t lane, unsigned long long ballot, uint32_t tile, uint32_t pos, uint32_t key) {
#ifdef CRH_ABLATE
    if (r.debug & 512u) return;
#endif
    if ((ballot >> lane) & 1ull) {
        const uint32_t at = st.used + lanes_below(ballot, lane);
        st.tile[at] = tile;
        st.pos[at] = pos;
        st.key[at] = key;
    }
    st.used += (uint32_t)__popcll(ballot);
    if (st.used > st.cap - 64u) {
        if (RESERVED) stage_flush_reserved(st, r, lane); else stage_flush(st, r, lane);
    }
}

CRH_D bool accepts(float e, uint32_t tl) { return e > 0.0f || (e == 0.0f && tl != 0u); }

// ---------------------------------------------------------------------------------------------- k_bin_edges
struct BinEdge { // one boundary edge of the item, canonical orientation
    float lo_x, lo_y, hi_x, hi_y, bx, nay, ymin, ymax;
    uint32_t tl, hull;
    int sigma, down;
    bool valid;
    float strip_det; // hull chain: det of the strip triangle that starts at this position (0: none, degenerate or not finite)
};
// boundary chain of a zig-zag strip (vertex.rs:28-35): the edge owned by strip position `pos` runs to position `target`
//   pos 0 -> 1;  even pos >= 2 -> pos - 2;  odd pos -> pos + 2, or — at the end of the strip — to the other one of the last two positions
// Edge i of an item: i < n_fe the fill chain(s), then the hull chain (n_hull_chain edges: 0 when the hull is drawn as triangles).
// `n_fe` fill chain edges, then `n_hull_chain` hull chain edges. An endpoint that is not finite on the frame (finite vertices times a
// finite matrix can overflow) sets *broken: the chain is not closed any more, so its backdrops mean nothing — the frame is then drawn by
// the triangle pass, which skips exactly the strip triangles with a non-finite determinant as the reference's rasterizer would.
#ifndef CRH_BIN_LOADS_EDGES
#define CRH_BIN_LOADS_EDGES 1 // 0: the loads where the compiler puts them — in the branches that choose among them, five waits an edge (A/B runs)
#endif
#if CRH_BIN_LOADS_EDGES
// load_edge in four steps, so that a caller with several edges per lane (k_bin_flat: kFlatEdgeRounds) waits for memory twice whatever it holds: the
// flags of a fill edge and its neighbours; where the edge's vertices are — a fill edge's target follows from the three flags, a hull edge's from its
// position, both with selects —; the vertices (the end points and, for a hull edge, the other two of the strip triangle that starts at its position);
// the edge. Indices are clamped to the item's own vertices; what is selected always exists.
struct EdgeFlags {
    uint32_t f, f_prev, f_next;
};
CRH_D EdgeFlags load_edge_flags(const SceneDev& s, const ItemCtx& ctx, uint32_t n_fe, uint32_t i, bool fill) { // fill: the lane has a fill edge (i < n_fe)
    EdgeFlags o = {0u, 0u, 0u};
    if (fill) {
        const uint32_t g = ctx.sv0 + i, g_last = ctx.sv0 + n_fe - 1u;
        o.f = s.solid_flag[g], o.f_prev = s.solid_flag[i >= 1u ? g - 1u : g], o.f_next = s.solid_flag[min(g + 1u, g_last)];
    }
    return o;
}
CRH_D void hold_edge_flags(EdgeFlags& o) { held(o.f), held(o.f_prev), held(o.f_next); }
constexpr uint32_t kEwHull = 1u, kEwStrip = 2u, kEwNone = 4u; // a hull edge; ... with a strip triangle at its position; a strip of one vertex: no edge
struct EdgeWhere {
    const Vertex0* v;
    uint32_t a, b, c1, c2, bits;
};
CRH_D EdgeWhere edge_where(const SceneDev& s, const ItemCtx& ctx, uint32_t n_fe, uint32_t n_hull_chain, uint32_t i, const EdgeFlags& fl) {
    const bool fill = i < n_fe;
    const uint32_t g = ctx.sv0 + i, g_last = ctx.sv0 + n_fe - 1u;
    const uint32_t gm1 = i >= 1u ? g - 1u : g, gm2 = i >= 2u ? g - 2u : g, gp1 = min(g + 1u, g_last), gp2 = min(g + 2u, g_last);
    const bool odd = (fl.f & 1u) != 0u, last = (fl.f & 2u) != 0u;
    const bool first = !odd && (i == 0u || (fl.f_prev & 2u) != 0u);
    const uint32_t fill_b = first ? gp1 : (!odd ? gm2 : (last ? gm1 : ((fl.f_next & 2u) ? gp1 : gp2)));
    const uint32_t pos = i - n_fe, n = n_hull_chain, hull0 = ctx.hull0;
    const uint32_t target = pos == 0u ? 1u : ((pos & 1u) == 0u ? pos - 2u : (pos + 1u == n ? pos - 1u : (pos + 2u == n ? pos + 1u : pos + 2u)));
    const bool strip = !fill && pos + 2u < n; // strip triangle `pos` = (pos, pos + 1, pos + 2), odd ones with the last two swapped
    EdgeWhere w;
    w.v = fill ? s.solid_v : s.hull_v;
    w.a = fill ? g : hull0 + pos;
    w.b = fill ? fill_b : hull0 + target;
    w.c1 = strip ? hull0 + ((pos & 1u) ? pos + 2u : pos + 1u) : w.a;
    w.c2 = strip ? hull0 + ((pos & 1u) ? pos + 1u : pos + 2u) : w.a;
    w.bits = (fill ? 0u : kEwHull) | (strip ? kEwStrip : 0u) | ((fill && first && last) ? kEwNone : 0u);
    return w;
}
struct EdgeVerts {
    Vertex0 a, b, c1, c2;
};
CRH_D EdgeVerts load_edge_verts(const EdgeWhere& w, bool active) { // active: the lane has an edge
    EdgeVerts o = {};
    if (active) o.a = w.v[w.a], o.b = w.v[w.b], o.c1 = w.v[w.c1], o.c2 = w.v[w.c2];
    return o;
}
CRH_D void hold_edge_verts(EdgeVerts& o) { held(o.a.x), held(o.a.y), held(o.b.x), held(o.b.y), held(o.c1.x), held(o.c1.y), held(o.c2.x), held(o.c2.y); }
CRH_D BinEdge finish_edge(const RasterParams& r, const ItemCtx& ctx, uint32_t bits, const EdgeVerts& v) {
    BinEdge e = {};
    e.valid = false;
    if (bits & kEwNone) return e; // a strip of one vertex
    float2 a = make_float2(v.a.x, v.a.y), b = make_float2(v.b.x, v.b.y);
    const float W = (float)r.width, H = (float)r.height;
    if (bits & kEwHull) {
        e.hull = 1u;
        if (bits & kEwStrip) { // which way does the strip triangle face?
            const float2 p0 = to_framebuffer(ctx, W, H, v.a.x, v.a.y), p1 = to_framebuffer(ctx, W, H, v.c1.x, v.c1.y), p2 = to_framebuffer(ctx, W, H, v.c2.x, v.c2.y);
            const float d1x = p1.x - p0.x, d1y = p1.y - p0.y, d2x = p2.x - p0.x, d2y = p2.y - p0.y;
            const float det = d1x * d2y - d2x * d1y; // setup_plain_triangle's det
            e.strip_det = (det == det && is_finite(det)) ? det : 0.0f;
        }
    }
    a = to_framebuffer(ctx, W, H, a.x, a.y);
    b = to_framebuffer(ctx, W, H, b.x, b.y);
    if (!(is_finite(a.x) && is_finite(a.y) && is_finite(b.x) && is_finite(b.y))) {
        r.overflow[7] = 1u; // (see above; the host draws the frame again with the triangle pass)
        return e;
    }
    if (a.x == b.x && a.y == b.y) return e;
    const bool flip = !(a.x < b.x || (a.x == b.x && a.y < b.y)); // canonical (lexicographic) endpoint order
    const float2 lo = flip ? b : a, hi = flip ? a : b;
    e.lo_x = lo.x, e.lo_y = lo.y, e.hi_x = hi.x, e.hi_y = hi.y;
    e.bx = hi.x - lo.x;
    e.nay = -(hi.y - lo.y);
    const float dx = hi.x - lo.x, dy = hi.y - lo.y;
    e.tl = (dy < 0.0f || (dy == 0.0f && dx > 0.0f)) ? 1u : 0u;
    e.down = dy > 0.0f ? 1 : 0;
    e.sigma = flip ? 1 : -1; // -1: the chain runs in the canonical direction
    e.ymin = fminf(lo.y, hi.y), e.ymax = fmaxf(lo.y, hi.y);
    e.valid = true;
    return e;
}
CRH_D BinEdge load_edge(const SceneDev& s, const RasterParams& r, const ItemCtx& ctx, uint32_t n_fe, uint32_t n_hull_chain, uint32_t i) {
    const bool active = i < n_fe + n_hull_chain;
    EdgeFlags fl = load_edge_flags(s, ctx, n_fe, i, active && i < n_fe);
    hold_edge_flags(fl);
    const EdgeWhere w = edge_where(s, ctx, n_fe, n_hull_chain, i, fl);
    EdgeVerts v = load_edge_verts(w, active);
    hold_edge_verts(v);
    BinEdge e = {};
    e.valid = false;
    if (active) e = finish_edge(r, ctx, w.bits, v);
    return e;
}
#else
CRH_D BinEdge load_edge(const SceneDev& s, const RasterParams& r, const ItemCtx& ctx, uint32_t n_fe, uint32_t n_hull_chain, uint32_t i) {
    BinEdge e = {};
    e.valid = false;
    if (i >= n_fe + n_hull_chain) return e;
    float2 a, b;
    if (i < n_fe) {
        // Everything the edge may need is requested at once — the flags of the neighbours and the four vertices the chain can run to —
        // instead of flag -> neighbour's flag -> target vertex one after the other (the item's wavefront spent 40 % of its time in this
        // chain of dependent loads). Indices are clamped to the item's own vertices; what is selected always exists.
        const uint32_t sv0 = ctx.sv0, g = sv0 + i, g_last = sv0 + n_fe - 1u;
        const uint32_t gm1 = i >= 1u ? g - 1u : g, gm2 = i >= 2u ? g - 2u : g, gp1 = min(g + 1u, g_last), gp2 = min(g + 2u, g_last);
        const uint32_t f = s.solid_flag[g], f_prev = s.solid_flag[gm1], f_next = s.solid_flag[gp1];
        const Vertex0 va = s.solid_v[g], vm1 = s.solid_v[gm1], vm2 = s.solid_v[gm2], vp1 = s.solid_v[gp1], vp2 = s.solid_v[gp2];
        const bool odd = (f & 1u) != 0u, last = (f & 2u) != 0u;
        const bool first = !odd && (i == 0u || (f_prev & 2u) != 0u);
        Vertex0 vb;
        if (first) {
            if (last) return e; // a strip of one vertex
            vb = vp1;
        } else if (!odd) {
            vb = vm2;
        } else {
            vb = last ? vm1 : ((f_next & 2u) ? vp1 : vp2);
        }
        a = make_float2(va.x, va.y), b = make_float2(vb.x, vb.y);
    } else {
        const uint32_t pos = i - n_fe, n = n_hull_chain, hull0 = ctx.hull0;
        uint32_t target;
        if (pos == 0u)
            target = 1u;
        else if ((pos & 1u) == 0u)
            target = pos - 2u;
        else
            target = pos + 1u == n ? pos - 1u : (pos + 2u == n ? pos + 1u : pos + 2u);
        const Vertex0 va = s.hull_v[hull0 + pos], vb = s.hull_v[hull0 + target];
        a = make_float2(va.x, va.y), b = make_float2(vb.x, vb.y);
        e.hull = 1u;
        if (pos + 2u < n) { // strip triangle `pos` = (pos, pos + 1, pos + 2), odd ones with the last two swapped: which way does it face?
            const float W = (float)r.width, H = (float)r.height;
            const Vertex0 v1 = s.hull_v[hull0 + ((pos & 1u) ? pos + 2u : pos + 1u)], v2 = s.hull_v[hull0 + ((pos & 1u) ? pos + 1u : pos + 2u)];
            const float2 p0 = to_framebuffer(ctx, W, H, va.x, va.y), p1 = to_framebuffer(ctx, W, H, v1.x, v1.y), p2 = to_framebuffer(ctx, W, H, v2.x, v2.y);
            const float d1x = p1.x - p0.x, d1y = p1.y - p0.y, d2x = p2.x - p0.x, d2y = p2.y - p0.y;
            const float det = d1x * d2y - d2x * d1y; // setup_plain_triangle's det
            e.strip_det = (det == det && is_finite(det)) ? det : 0.0f;
        }
    }
    const float W = (float)r.width, H = (float)r.height;
    a = to_framebuffer(ctx, W, H, a.x, a.y);
    b = to_framebuffer(ctx, W, H, b.x, b.y);
    if (!(is_finite(a.x) && is_finite(a.y) && is_finite(b.x) && is_finite(b.y))) {
        r.overflow[7] = 1u; // (see above; the host draws the frame again with the triangle pass)
        return e;
    }
    if (a.x == b.x && a.y == b.y) return e;
    const bool flip = !(a.x < b.x || (a.x == b.x && a.y < b.y)); // canonical (lexicographic) endpoint order
    const float2 lo = flip ? b : a, hi = flip ? a : b;
    e.lo_x = lo.x, e.lo_y = lo.y, e.hi_x = hi.x, e.hi_y = hi.y;
    e.bx = hi.x - lo.x;
    e.nay = -(hi.y - lo.y);
    const float dx = hi.x - lo.x, dy = hi.y - lo.y;
    e.tl = (dy < 0.0f || (dy == 0.0f && dx > 0.0f)) ? 1u : 0u;
    e.down = dy > 0.0f ? 1 : 0;
    e.sigma = flip ? 1 : -1; // -1: the chain runs in the canonical direction
    e.ymin = fminf(lo.y, hi.y), e.ymax = fmaxf(lo.y, hi.y);
    e.valid = true;
    return e;
}
#endif
CRH_D float wave_min(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
CRH_D float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
CRH_D uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

// The exact tile test of a set-up triangle: its best tile corner per edge decides (an edge function is monotone in x and y under fmaf).
// A conservative superset of "some sample of the tile is covered"; the raster kernel decides per sample.
struct TileTest {
    float bx[3], nay[3], lo_x[3], lo_y[3];
    float s_lo, s_hi;  // extreme sample offsets inside a tile
    uint32_t tl;       // bits 0-2: top-left per edge
    CRH_D void set(const PrimCoverage& cov, float lo, float hi) {
#pragma unroll
        for (int i = 0; i < 3; ++i) bx[i] = cov.bx[i], nay[i] = cov.nay[i], lo_x[i] = cov.lo_x[i], lo_y[i] = cov.lo_y[i];
        s_lo = lo, s_hi = hi;
        tl = cov.flags & 7u;
    }
    CRH_D bool hit(uint32_t tx, uint32_t ty) const {
        const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) { // the best corner of the tile for this edge (selected here: two registers per edge less to carry)
            const float best_x = nay[i] > 0.0f ? s_hi : s_lo, best_y = bx[i] > 0.0f ? s_hi : s_lo;
            const float e = fmaf(best_y, bx[i], fmaf(best_x, nay[i], bx[i] * (ty0 - lo_y[i]) + nay[i] * (tx0 - lo_x[i])));
            ok = ok && accepts(e, (tl >> i) & 1u);
        }
        return ok;
    }
};
// Bins up to 64 set-up triangles (lane = triangle): every lane walks the tiles of ITS OWN pixel box — a few for a curve or stroke
// triangle; a triangle over more than kBigRect tiles is walked by the whole wavefront instead (lane = tile), one such triangle at a time.
#ifndef CRH_BIN_WAVES
#define CRH_BIN_WAVES 4 // measured 4, 5, 6: the same within noise (the kernel waits for memory, not for issue slots); 4 needs no spills
#endif
constexpr uint32_t kBigRect = 32;
constexpr uint32_t kRectLds = 256; // tiles of an item's rectangle whose backdrops fit the LDS table of the lane = edge path
CRH_D void bin_triangles(Stage& st, const RasterParams& r, uint32_t lane, bool drawn, const PrimCoverage& cov, uint32_t key, float s_lo, float s_hi) {
    TileTest test;
    test.set(cov, s_lo, s_hi);
    // (the tile rows of the pass' slab only, crh_frame_set_tile_rows: the raster kernels draw no others)
    const uint32_t bx0 = cov.box.x / kTile, bx1 = cov.box.y / kTile, by0 = max((uint32_t)cov.box.z / kTile, r.slab_ty0), by1 = min((uint32_t)cov.box.w / kTile + 1u, r.slab_ty1); // [by0, by1)
    const uint32_t nx = bx1 - bx0 + 1u, nt = (drawn && by0 < by1) ? nx * (by1 - by0) : 0u;
    const bool big = nt > kBigRect || (nt != 0u && (r.debug & 2u) != 0u); // debug bit 1 (tests): every triangle takes the wide path
    const uint32_t mine = big ? 0u : nt, longest = wave_max_u32(mine);
    uint32_t tx = bx0, ty = by0;
    for (uint32_t i = 0; i < longest; ++i) {
        const bool hit = i < mine && test.hit(tx, ty);
        const unsigned long long ballot = __ballot(hit);
        if (ballot) {
            const uint32_t tile = ty * r.tiles_x + tx;
            uint32_t pos = 0;
            if (hit) pos = atomicAdd(&r.tile_count[tile], 1u);
            stage_append(st, r, lane, ballot, tile, pos, key);
        }
        if (++tx > bx1) tx = bx0, ++ty;
    }
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        TileTest wide;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            wide.bx[i] = __shfl(test.bx[i], src, 64), wide.nay[i] = __shfl(test.nay[i], src, 64), wide.lo_x[i] = __shfl(test.lo_x[i], src, 64);
            wide.lo_y[i] = __shfl(test.lo_y[i], src, 64);
        }
        wide.s_lo = test.s_lo, wide.s_hi = test.s_hi;
        wide.tl = (uint32_t)__shfl((int)test.tl, src, 64);
        const uint32_t wx0 = (uint32_t)__shfl((int)bx0, src, 64), wy0 = (uint32_t)__shfl((int)by0, src, 64), wnx = (uint32_t)__shfl((int)nx, src, 64);
        const uint32_t wnt = (uint32_t)__shfl((int)nt, src, 64), wkey = (uint32_t)__shfl((int)key, src, 64);
        for (uint32_t base = 0; base < wnt; base += 64u) {
            const uint32_t q = base + lane, qy = q / wnx, qx = q - qy * wnx;
            const bool hit = q < wnt && wide.hit(wx0 + qx, wy0 + qy);
            const unsigned long long ballot = __ballot(hit);
            if (!ballot) continue;
            const uint32_t tile = (wy0 + qy) * r.tiles_x + (wx0 + qx);
            uint32_t pos = 0;
            if (hit) pos = atomicAdd(&r.tile_count[tile], 1u);
            stage_append(st, r, lane, ballot, tile, pos, wkey);
        }
    }
}

// The same for a chunk of triangles whose common tile rectangle fits an LDS table (the usual case): the lanes walk their boxes twice — once
// counting per tile (LDS), once emitting with positions from LDS cursors — and in between lane = tile reserves the positions with ONE
// returning atomic per tile. (bin_triangles pays a round trip to L2 per step of the walk: 60 % of that wavefront's time.)
CRH_D bool bin_triangles_counted(Stage& st, const RasterParams& r, uint32_t lane, bool drawn, const PrimCoverage& cov, uint32_t key, float s_lo, float s_hi,
                                 uint32_t* cursor) {
    const uint32_t bx0 = cov.box.x / kTile, bx1 = cov.box.y / kTile, by0 = cov.box.z / kTile, by1 = cov.box.w / kTile;
    // the chunk's rectangle
    uint32_t rx0 = drawn ? bx0 : 0xFFFFFFFFu, ry0 = drawn ? by0 : 0xFFFFFFFFu, rx1 = drawn ? bx1 : 0u, ry1 = drawn ? by1 : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        rx0 = min(rx0, (uint32_t)__shfl_xor((int)rx0, d, 64)), ry0 = min(ry0, (uint32_t)__shfl_xor((int)ry0, d, 64));
        rx1 = max(rx1, (uint32_t)__shfl_xor((int)rx1, d, 64)), ry1 = max(ry1, (uint32_t)__shfl_xor((int)ry1, d, 64));
    }
    if (rx0 == 0xFFFFFFFFu) return true; // nothing drawn
    const uint32_t nx = rx1 - rx0 + 1u, n_rect = nx * (ry1 - ry0 + 1u);
    if (n_rect > kRectLds || (r.debug & 2u) != 0u) return false; // the caller takes the walk with an atomic per step (debug bit 1: always)
    TileTest test;
    test.set(cov, s_lo, s_hi);
    const uint32_t bnx = bx1 - bx0 + 1u, nt = drawn ? bnx * (by1 - by0 + 1u) : 0u, longest = wave_max_u32(nt);
    for (uint32_t q = lane; q < n_rect; q += 64u) cursor[q] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint32_t tx = bx0, ty = by0;
    for (uint32_t i = 0; i < longest; ++i) { // count
        if (i < nt && test.hit(tx, ty)) atomicAdd(&cursor[(ty - ry0) * nx + (tx - rx0)], 1u);
        if (++tx > bx1) tx = bx0, ++ty;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < n_rect; base += 64u) { // reserve
        const uint32_t q = base + lane, qy = q / nx, qx = q - qy * nx;
        const uint32_t n = q < n_rect ? cursor[q] : 0u;
#ifdef CRH_ABLATE
        if (r.debug & 131072u) { if (n) cursor[q] = q & 7u; } else
#endif
        if (n) cursor[q] = atomicAdd(&r.tile_count[(ry0 + qy) * r.tiles_x + rx0 + qx], n);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    tx = bx0, ty = by0;
    for (uint32_t i = 0; i < longest; ++i) { // emit
        const bool hit = i < nt && test.hit(tx, ty);
        const unsigned long long ballot = __ballot(hit);
        if (ballot) {
            uint32_t pos = 0;
            if (hit) pos = atomicAdd(&cursor[(ty - ry0) * nx + (tx - rx0)], 1u);
            stage_append(st, r, lane, ballot, ty * r.tiles_x + tx, pos, key);
        }
        if (++tx > bx1) tx = bx0, ++ty;
    }
    return true;
}

#ifdef CRH_ABLATE // tools/bin_phases.py: where does a wavefront of k_bin_edges spend its time? (cycle counter deltas summed in overflow[80 ...])
#define CRH_PHASE(k)                                                                                                   \
    if (r.debug & 65536u) {                                                                                            \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                  \
        if (lane == 0u) atomicAdd(reinterpret_cast<unsigned long long*>(r.overflow + 80) + (k) + 8u * wave, now_ - phase_t); \
        phase_t = __builtin_amdgcn_s_memtime();                                                                        \
    }
#else
#define CRH_PHASE(k)
#endif
// One workgroup per draw item. Wavefront 0: the stroke and curve triangles (bin_triangles). Wavefront 1: the boundary edges, transposed —
// lane = tile of the item's rectangle (64 per pass), uniform loop over the edges (staged in LDS): every lane accumulates the backdrops of
// its tile and the bit mask of the edges that matter inside it, then emits its entries.
// QUEUED: the items are those k_bin_flat handed on (r.bin_queue, their number in r.overflow[6]) — the ones too large for its batches.
template <int S, bool QUEUED>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(CRH_BIN_WAVES))) void k_bin_edges(SceneDev s, RasterParams r) {
    __shared__ uint32_t stage_tile[2][kStage], stage_pos[2][kStage], stage_key[2][kStage];
    __shared__ float4 edge_a[64], edge_b[64];
    __shared__ int rect_bd[kRectLds], rect_hbd[kRectLds];    // lane = edge path: backdrops of the tiles of the item's rectangle ...
    __shared__ uint32_t rect_hull_touch[kRectLds / 32u];      // ... whether a hull edge matters inside the tile ...
    __shared__ uint32_t rect_cursor[kRectLds];                // ... and the count, then the next list position, of the edges that matter there
    __shared__ uint32_t rect_cursor_tri[kRectLds];            // the same for the triangle wavefront (its own rectangle, per chunk of 64 triangles)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Stage st = {stage_tile[wave], stage_pos[wave], stage_key[wave], 0u, ((2u * blockIdx.x + wave) * 2654435761u) >> 26, kStage, 0u}; // (a hash: consecutive wavefronts start in unrelated sub-streams)
    // a workgroup takes items blockIdx.x, blockIdx.x + gridDim.x, ...: the pair stage carries over from one item to the next (fewer, fuller
    // flushes), and the two wavefronts never synchronise with each other
    const uint32_t n_work = QUEUED ? min(r.overflow[6], r.n_items) : r.n_items;
    for (uint32_t work = blockIdx.x; work < n_work; work += gridDim.x) {
    __builtin_amdgcn_wave_barrier(); // (the previous item's readers of the LDS tables are through)
    const uint32_t item = QUEUED ? r.bin_queue[work] : work;
    const DrawItem it = item_of(r, item);
    const ItemSlots k = item_slots(s, it);
    const ItemCtx ctx = item_ctx(s, r, it, k.cb);
    const uint32_t slot0 = r.slot_begin[item];
    if (slot0 + k.total > r.slot_capacity) continue; // cannot happen: the capacity is the scan's total
    if (r.item_elsewhere && r.item_elsewhere[item] != 0u) continue; // (a pass with a slab: no tile row of the item's box is in it)
#ifdef CRH_ABLATE
    unsigned long long phase_t = __builtin_amdgcn_s_memtime();
#endif
    const float ry_first = S == 1 ? 0.5f : 0.125f, r_last = (float)(kTile - 1) + (S == 1 ? 0.5f : 0.875f); // extreme sample offsets inside a tile
#ifdef CRH_ABLATE
    if ((r.debug & 1024u) && wave == 0u) continue;
    if ((r.debug & 2048u) && wave == 1u) continue;
#endif
    if (wave == 0u) {
        // ---------------- triangles: 64 at a time, lane = triangle
        for (uint32_t t0 = 0; t0 < k.n_tri; t0 += 64u) {
            const uint32_t t = t0 + lane;
            PrimRec rec = {};
            bool drawn = false;
            CRH_PHASE(0) // item data
            if (t < k.n_tri) {
                const uint32_t c = t < k.cb[1] ? t : t - k.cb[1] + k.cb[2]; // the Shape's candidate numbering without the solid strips
                drawn = setup_plain_triangle(s, r, ctx, c, rec);
                if (drawn) *reinterpret_cast<PrimRec*>(r.slots + (size_t)(slot0 + 4u * t) * 32u) = rec;
            }
            CRH_PHASE(1) // triangle set-up
            if (!bin_triangles_counted(st, r, lane, drawn, rec.cov, slot0 + 4u * t, ry_first, r_last, rect_cursor_tri))
                bin_triangles(st, r, lane, drawn, rec.cov, slot0 + 4u * t, ry_first, r_last);
            CRH_PHASE(2) // walk
        }
    } else {
        // ---------------- boundary edges: fill chain(s) then hull chain
        const uint32_t fe_slot0 = slot0 + k.fe0, synth_a = slot0 + k.synth_a, hull_slot0 = slot0 + k.hull0, synth_b = slot0 + k.synth_b;
        const float* item_color = ctx.col;
        const bool opaque_item = item_color[3] == 1.0f && is_finite(item_color[0]) && is_finite(item_color[1]) && is_finite(item_color[2]) &&
                                 r.occlude != 0u && (r.debug & 32768u) == 0u; // debug bit 15 (tests, A/B runs): no tile is ever treated as replaced
        if (lane < 13u + kCoverOpaque) { // 4 backdrop + 27 COVER slots (the COVER ones carry the premultiplied source colour, shaders.wgsl:304-309)
            SynthRec sr = {};
            sr.flags = (EK_SYNTH << 4) | (lane << 8);
            sr.first_slot = slot0, sr.synth_a = synth_a;
            if (lane >= 4u) sr.r = item_color[0] * item_color[3], sr.g = item_color[1] * item_color[3], sr.b = item_color[2] * item_color[3], sr.a = item_color[3];
            *reinterpret_cast<SynthRec*>(r.slots + (size_t)(lane < 4u ? synth_a + lane : synth_b + lane - 4u) * 32u) = sr;
        }
        // Do all triangles of the hull strip face the same way? Then the cover — the UNION of those triangles (renderer.rs:340-354) — is
        // where the winding number of the strip's boundary chain is not zero, and the chain is binned. A strip that folds over itself
        // (andrew() decides turns with an absolute margin, convex_hull.rs:17-20: under f32 cancellation its output is not always convex)
        // is drawn as the reference draws it, triangle by triangle.
        uint32_t n_hull_chain = k.n_hull, n_edges = k.n_fe + n_hull_chain;
        unsigned long long faces_front = 0, faces_back = 0;
        // one chunk of (up to 64) edges -> LDS table (+ the heap records the first time)
        float minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
        BinEdge kept = {}; // the lane's edge of the first chunk (most items have no other)
        auto stage_chunk = [&](uint32_t i0, bool write_records) {
            const uint32_t i = i0 + lane;
            const BinEdge e = load_edge(s, r, ctx, k.n_fe, n_hull_chain, i);
            if (write_records && i0 == 0u) kept = e;
            const uint32_t flags = (EK_EDGE << 4) | (e.tl ? kEdgeTl : 0u) | (e.sigma > 0 ? kEdgeSigmaPos : 0u) | (e.hull ? kEdgeHull : 0u);
            if (e.valid && write_records) {
                EdgeRec er;
                er.flags = flags, er.pad0 = 0u;
                er.lo_x = e.lo_x, er.lo_y = e.lo_y, er.hi_x = e.hi_x, er.hi_y = e.hi_y, er.bx = e.bx, er.nay = e.nay;
                *reinterpret_cast<EdgeRec*>(r.slots + (size_t)(i < k.n_fe ? fe_slot0 + i : hull_slot0 + (i - k.n_fe)) * 32u) = er;
            }
            __builtin_amdgcn_wave_barrier(); // the previous chunk's readers are done
            edge_a[lane] = make_float4(e.lo_x, e.lo_y, e.bx, e.nay);
            edge_b[lane] = make_float4(e.ymin, e.ymax, e.hi_x, __uint_as_float(flags | (e.down ? 8u : 0u) | (e.valid ? 0x100u : 0u)));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (e.valid) {
                minx = fminf(minx, e.lo_x), maxx = fmaxf(maxx, e.hi_x);
                miny = fminf(miny, e.ymin), maxy = fmaxf(maxy, e.ymax);
            }
            if (write_records) { // (a strip triangle is judged at its first position whether or not that position's chain edge is valid)
                faces_front |= __ballot(e.strip_det < 0.0f);
                faces_back |= __ballot(e.strip_det > 0.0f);
            }
        };
        CRH_PHASE(0) // item data, synthetic slots
        for (uint32_t i0 = 0; i0 < n_edges; i0 += 64u) stage_chunk(i0, true); // records + the box of every vertex (one chunk: the table stays)
        CRH_PHASE(1) // edge records
        const bool hull_as_triangles = k.n_hull != 0u && ((faces_front != 0ull && faces_back != 0ull) || (r.debug & 4u) != 0u); // debug bit 2 (tests): always
        if (hull_as_triangles) { // the fill chain alone (rare: the staging is simply done again)
            n_hull_chain = 0u, n_edges = k.n_fe;
            minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
            for (uint32_t i0 = 0; i0 < n_edges; i0 += 64u) stage_chunk(i0, false);
        }
        const bool single = n_edges <= 64u && (r.debug & 1u) == 0u; // debug bit 0 (tests): the chunked path even for short chains
        minx = wave_min(minx), maxx = wave_max(maxx), miny = wave_min(miny), maxy = wave_max(maxy);
        const float W = (float)r.width, H = (float)r.height;
        const int px0 = (int)floorf(fminf(fmaxf(minx, 0.0f), W)), px1 = (int)floorf(fmaxf(fminf(maxx, W - 1.0f), -1.0f));
        const int py0 = (int)floorf(fminf(fmaxf(miny, 0.0f), H)), py1 = (int)floorf(fmaxf(fminf(maxy, H - 1.0f), -1.0f));
#ifdef CRH_ABLATE
        if (r.debug & 8192u) n_edges = 0u;
#endif
        // (... of the pass' slab of tile rows, crh_frame_set_tile_rows: every tile row's backdrops and entries are its own, so the others are simply left out)
        const uint32_t tx_a = (uint32_t)max(px0, 0) / kTile, tx_b = (uint32_t)max(px1, 0) / kTile, ty_a = max((uint32_t)max(py0, 0) / kTile, r.slab_ty0);
        const uint32_t ty_b_end = min((uint32_t)max(py1, 0) / kTile + 1u, r.slab_ty1), ty_b = ty_b_end - 1u; // (only used when ty_a < ty_b_end)
        const uint32_t nx = tx_b - tx_a + 1u, n_rect = ty_a < ty_b_end ? nx * (ty_b_end - ty_a) : 0u;
        const bool in_frame = n_edges != 0u && minx <= maxx && px0 <= px1 && py0 <= py1 && ty_a < ty_b_end;
        if (in_frame && n_rect <= kRectLds && (r.debug & 1u) == 0u) {
            // ---------------- lane = EDGE (the common case: the rectangle's backdrops fit the LDS table). The transposed loop below costs
            // edges x tiles of the rectangle; here every edge visits the tiles of its OWN box and the tile rows whose backdrop line it
            // crosses, the backdrops being summed in LDS.
            // Three passes: (1) every edge counts, per tile of its own box, whether it matters there (LDS counters) and adds its backdrop
            // terms; (2) lane = tile: ONE returning atomic on the tile's global counter reserves the positions of the item's entries in the
            // tile's list, the synthetic entries are emitted; (3) the edges walk their boxes again and take their positions from the LDS
            // cursors. (A returning global atomic per (edge, tile) visit made the wavefront wait for a round trip to L2 per step of the walk.)
            for (uint32_t q = lane; q < n_rect; q += 64u) rect_bd[q] = 0, rect_hbd[q] = 0, rect_cursor[q] = 0u;
            if (lane < kRectLds / 32u) rect_hull_touch[lane] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool one_chunk = k.n_fe + k.n_hull <= 64u;
            auto edge_of = [&](uint32_t i) {
                BinEdge e;
                if (one_chunk) { // still in registers (a hull chain that is drawn as triangles drops out: i >= n_edges)
                    e = kept;
                    e.valid = e.valid && i < n_edges;
                } else {
                    e = load_edge(s, r, ctx, k.n_fe, n_hull_chain, i);
                }
                return e;
            };
            // the tiles of the edge's own box (a conservative integer range; the exact test decides tile by tile), walked by all lanes together
            auto walk = [&](const BinEdge& e, auto&& visit) {
                uint32_t bx0 = tx_a, bx1 = tx_a, by0 = ty_a, nt = 0;
                if (e.valid) {
                    const int x_lo = (int)ceilf((e.lo_x - r_last) * (1.0f / (float)kTile) - 0.01f), x_hi = (int)floorf(e.hi_x * (1.0f / (float)kTile) + 0.01f);
                    const int y_lo = (int)ceilf((e.ymin - r_last) * (1.0f / (float)kTile) - 0.01f), y_hi = (int)floorf((e.ymax - ry_first) * (1.0f / (float)kTile) + 0.01f);
                    const int cx0 = max(x_lo, (int)tx_a), cx1 = min(x_hi, (int)tx_b), cy0 = max(y_lo, (int)ty_a), cy1 = min(y_hi, (int)ty_b);
                    if (cx0 <= cx1 && cy0 <= cy1) bx0 = (uint32_t)cx0, bx1 = (uint32_t)cx1, by0 = (uint32_t)cy0, nt = (uint32_t)((cx1 - cx0 + 1) * (cy1 - cy0 + 1));
                }
                const bool up = e.nay > 0.0f; // E grows with ry (bx >= 0) and with rx iff nay > 0
                const uint32_t longest = wave_max_u32(nt);
                uint32_t tx = bx0, ty = by0;
                for (uint32_t w = 0; w < longest; ++w) {
                    const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile), q0y = ty0 + ry_first;
                    const float c = e.bx * (ty0 - e.lo_y) + e.nay * (tx0 - e.lo_x);
                    const bool gmax = accepts(fmaf(r_last, e.bx, fmaf(up ? r_last : 0.0f, e.nay, c)), e.tl), gmin = accepts(fmaf(ry_first, e.bx, fmaf(up ? 0.0f : r_last, e.nay, c)), e.tl);
                    const bool hit = w < nt && gmax != gmin && e.ymin <= ty0 + r_last && e.ymax >= q0y && e.lo_x <= tx0 + r_last && e.hi_x >= tx0;
                    visit(hit, tx, ty);
                    if (++tx > bx1) tx = bx0, ++ty;
                }
            };
            CRH_PHASE(2) // rectangle, LDS table cleared
            for (uint32_t i0 = 0; i0 < n_edges; i0 += 64u) { // ---- pass 1
                const BinEdge e = edge_of(i0 + lane);
                // backdrop rows: the tile rows whose line q0y lies in the edge's half-open y range; a conservative integer range first
                uint32_t row = ty_a, rows_mine = 0;
                if (e.valid) {
                    const int lo = (int)ceilf((e.ymin - ry_first) * (1.0f / (float)kTile) - 0.01f), hi = (int)floorf((e.ymax - ry_first) * (1.0f / (float)kTile) + 0.01f);
                    const int first = max(lo, (int)ty_a), last = min(hi, (int)ty_b);
                    if (first <= last) row = (uint32_t)first, rows_mine = (uint32_t)(last - first + 1);
                }
                const uint32_t most_rows = wave_max_u32(rows_mine);
                for (uint32_t rr = 0; rr < most_rows; ++rr) {
                    const uint32_t ty = row + rr;
                    const float ty0 = (float)(ty * kTile), q0y = ty0 + ry_first;
                    const bool crosses = rr < rows_mine && e.ymin <= q0y && q0y < e.ymax; // Y_e at the backdrop row
                    if (!__any(crosses)) continue;
                    int* const table = (e.hull ? rect_hbd : rect_bd) + (ty - ty_a) * nx;
                    for (uint32_t cx = 0; cx < nx; ++cx) {
                        const float tx0 = (float)((tx_a + cx) * kTile);
                        const float c = e.bx * (ty0 - e.lo_y) + e.nay * (tx0 - e.lo_x);
                        const bool gq0 = accepts(fmaf(ry_first, e.bx, fmaf(0.0f, e.nay, c)), e.tl);
                        const int term = e.sigma * ((gq0 ? 1 : 0) - e.down); // sigma * Y(q0) * (g(q0) - down)
                        if (crosses && term != 0) atomicAdd(&table[cx], term);
                    }
                }
                walk(e, [&](bool hit, uint32_t tx, uint32_t ty) {
                    if (hit) {
                        const uint32_t q = (ty - ty_a) * nx + (tx - tx_a);
                        atomicAdd(&rect_cursor[q], 1u);
                        if (e.hull) atomicOr(&rect_hull_touch[q >> 5], 1u << (q & 31u));
                    }
                });
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            CRH_PHASE(3) // pass 1
            for (uint32_t base = 0; base < n_rect; base += 64u) { // ---- pass 2, lane = tile (the COVER entry carries one unit of either backdrop)
                const uint32_t q = base + lane, qy = q / nx, qx = q - qy * nx;
                const bool active = q < n_rect;
                const uint32_t tile = (ty_a + qy) * r.tiles_x + tx_a + qx;
                const int bd = active ? rect_bd[q] : 0, hbd = active ? rect_hbd[q] : 0;
                const uint32_t n_touching = active ? rect_cursor[q] : 0u;
                const bool hull_touch = active && ((rect_hull_touch[q >> 5] >> (q & 31u)) & 1u) != 0u;
                const uint32_t abd = (uint32_t)(bd < 0 ? -bd : bd), ahbd = (uint32_t)(hbd < 0 ? -hbd : hbd);
                uint32_t n_cover = (active && n_hull_chain != 0u && (hbd != 0 || hull_touch)) ? 1u : 0u; // the tile is inside the hull or its boundary crosses it
                const int cbd = bd > 0 ? 1 : (bd < 0 ? -1 : 0), chbd = hbd > 0 ? 1 : (hbd < 0 ? -1 : 0);
                const bool hull_over_tile = n_cover != 0u && hbd != 0 && !hull_touch;
                const bool replaces_tile = hull_over_tile && opaque_item && n_touching == 0u && (bd & (int)r.winding_mask) != 0;
                const uint32_t cover_key = synth_b + (uint32_t)(cbd + 1) + 3u * (uint32_t)(chbd + 1) + (replaces_tile ? kCoverOpaque : (hull_over_tile ? kCoverHull : 0u));
                if (const unsigned long long opaque = __ballot(replaces_tile)) // the host's statistic: are there tiles to start late in? (overflow[4])
                    if (lane == 0u) atomicAdd(&r.overflow[4], (uint32_t)__popcll(opaque));
                uint32_t n_bd = n_cover ? (abd ? abd - 1u : 0u) : abd;
                uint32_t n_hbd = n_cover ? (ahbd ? ahbd - 1u : 0u) : 0u;
                const uint32_t bd_key = synth_a + (bd > 0 ? 0u : 1u), hbd_key = synth_a + (hbd > 0 ? 2u : 3u);
                uint32_t left = n_cover + n_bd + n_hbd, pos = 0;
#ifdef CRH_ABLATE
                if (r.debug & 131072u) pos = tile & 7u; else
#endif
                if (left + n_touching) pos = atomicAdd(&r.tile_count[tile], left + n_touching);
                if (active) rect_cursor[q] = pos + left; // where the edges' entries go
                for (;;) {
                    const unsigned long long ballot = __ballot(left != 0u);
                    if (!ballot) break;
                    uint32_t key = 0;
                    if (left) {
                        if (n_cover)
                            n_cover = 0, key = cover_key;
                        else if (n_bd)
                            --n_bd, key = bd_key;
                        else
                            --n_hbd, key = hbd_key;
                    }
                    stage_append(st, r, lane, ballot, tile, pos, key);
                    if (left) ++pos, --left;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            CRH_PHASE(4) // pass 2
            for (uint32_t i0 = 0; i0 < n_edges; i0 += 64u) { // ---- pass 3
                const uint32_t i = i0 + lane;
                const BinEdge e = edge_of(i);
                const uint32_t key = i < k.n_fe ? fe_slot0 + i : hull_slot0 + (i - k.n_fe);
                walk(e, [&](bool hit, uint32_t tx, uint32_t ty) {
                    const unsigned long long ballot = __ballot(hit);
                    if (ballot) {
                        uint32_t pos = 0;
                        if (hit) pos = atomicAdd(&rect_cursor[(ty - ty_a) * nx + (tx - tx_a)], 1u);
                        stage_append(st, r, lane, ballot, ty * r.tiles_x + tx, pos, key);
                    }
                });
            }
        } else if (in_frame) {
            for (uint32_t base = 0; base < n_rect; base += 64u) {
                const uint32_t q = base + lane, qy = q / nx, qx = q - qy * nx;
                const bool active = q < n_rect;
                const uint32_t tx = tx_a + qx, ty = ty_a + qy, tile = ty * r.tiles_x + tx;
                const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile), q0y = ty0 + ry_first;
                int bd = 0, hbd = 0;
                bool hull_touch = false;
                for (uint32_t i0 = 0; i0 < n_edges; i0 += 64u) {
                    if (!single) stage_chunk(i0, false);
                    const uint32_t count = min(64u, n_edges - i0);
                    unsigned long long mask = 0;
#ifdef CRH_ABLATE
                    if (r.debug & 16384u) continue;
#endif
                    for (uint32_t j = 0; j < count; ++j) {
                        const float4 A = edge_a[j], B = edge_b[j];
                        const uint32_t flags = __builtin_amdgcn_readfirstlane(__float_as_uint(B.w));
                        if (!(flags & 0x100u)) continue;
                        const uint32_t tl = flags & kEdgeTl;
                        const float c = A.z * (ty0 - A.y) + A.w * (tx0 - A.x);
                        const bool gq0 = accepts(fmaf(ry_first, A.z, fmaf(0.0f, A.w, c)), tl);
                        const bool y0_in = B.x <= q0y && q0y < B.y; // Y_e at the backdrop row
                        const int sigma = (flags & kEdgeSigmaPos) ? 1 : -1, down = (flags >> 3) & 1;
                        const int term = y0_in ? sigma * ((gq0 ? 1 : 0) - down) : 0; // sigma * Y(q0) * (g(q0) - down)
                        const bool up = A.w > 0.0f; // E grows with ry (bx >= 0) and with rx iff nay > 0
                        const bool gmax = accepts(fmaf(r_last, A.z, fmaf(up ? r_last : 0.0f, A.w, c)), tl), gmin = accepts(fmaf(ry_first, A.z, fmaf(up ? 0.0f : r_last, A.w, c)), tl);
                        const bool touch = active && gmax != gmin && B.x <= ty0 + r_last && B.y >= q0y && A.x <= tx0 + r_last && B.z >= tx0;
                        if (flags & kEdgeHull) {
                            hbd += term;
                            hull_touch = hull_touch || touch;
                        } else {
                            bd += term;
                        }
                        mask |= touch ? (1ull << j) : 0ull;
                    }
                    // ---- this chunk's entries; the last chunk's go together with the item's synthetic entries
                    const bool last_chunk = i0 + 64u >= n_edges;
                    const uint32_t abd = (uint32_t)(bd < 0 ? -bd : bd), ahbd = (uint32_t)(hbd < 0 ? -hbd : hbd);
                    uint32_t n_cover = 0, n_bd = 0, n_hbd = 0, cover_key = 0;
                    if (last_chunk && active) {
                        n_cover = (n_hull_chain != 0u && (hbd != 0 || hull_touch)) ? 1u : 0u; // the tile is inside the hull or its boundary crosses it
                        const int cbd = bd > 0 ? 1 : (bd < 0 ? -1 : 0), chbd = hbd > 0 ? 1 : (hbd < 0 ? -1 : 0);
                        cover_key = synth_b + (uint32_t)(cbd + 1) + 3u * (uint32_t)(chbd + 1) + ((n_cover != 0u && hbd != 0 && !hull_touch) ? kCoverHull : 0u);
                        n_bd = n_cover ? (abd ? abd - 1u : 0u) : abd; // the COVER entry carries one unit of either backdrop
                        n_hbd = n_cover ? (ahbd ? ahbd - 1u : 0u) : 0u;
                    }
                    const uint32_t bd_key = synth_a + (bd > 0 ? 0u : 1u), hbd_key = synth_a + (hbd > 0 ? 2u : 3u);
                    const uint32_t n_mine = (uint32_t)__popcll(mask) + n_cover + n_bd + n_hbd;
                    uint32_t pos = 0;
                    if (n_mine) pos = atomicAdd(&r.tile_count[tile], n_mine);
                    uint32_t left = n_mine;
                    for (;;) {
                        const unsigned long long ballot = __ballot(left != 0u);
                        if (!ballot) break;
                        uint32_t key = 0;
                        if (left) {
                            if (mask) {
                                const uint32_t i = i0 + (uint32_t)(__ffsll((long long)mask) - 1);
                                mask &= mask - 1ull;
                                key = i < k.n_fe ? fe_slot0 + i : hull_slot0 + (i - k.n_fe);
                            } else if (n_cover) {
                                n_cover = 0, key = cover_key;
                            } else if (n_bd) {
                                --n_bd, key = bd_key;
                            } else {
                                --n_hbd, key = hbd_key;
                            }
                        }
                        stage_append(st, r, lane, ballot, tile, pos, key);
                        if (left) ++pos, --left;
                    }
                }
            }
        }
        if (hull_as_triangles) { // the hull strip, triangle by triangle, as cover triangles (keys behind the fill chain and the backdrop slots)
            for (uint32_t t0 = 0; t0 + 2u < k.n_hull; t0 += 64u) {
                const uint32_t t = t0 + lane;
                PrimRec rec = {};
                bool drawn = false;
                if (t + 2u < k.n_hull) {
                    drawn = setup_plain_triangle(s, r, ctx, k.cb[6] + t, rec);
                    if (drawn) *reinterpret_cast<PrimRec*>(r.slots + (size_t)(hull_slot0 + 4u * t) * 32u) = rec;
                }
                bin_triangles(st, r, lane, drawn, rec.cov, hull_slot0 + 4u * t, ry_first, r_last);
            }
        }
    }
    CRH_PHASE(5) // pass 3 (edges) / nothing (triangles)
    } // items
    stage_flush(st, r, lane);
}


// ---------------------------------------------------------------------------------------------- k_bin_flat
// The same binning with the lanes packed ACROSS draw items. k_bin_edges gives every item a wavefront per role and each of them walks
// item -> ranges -> vertices -> records -> LDS passes -> returning atomics alone: 20 000 wavefronts of 33 us for the benchmark scene, a
// third to two thirds of their lanes idle (18 triangles, 40 edges per item), and that sum of wavefront lifetimes, not arithmetic, was the
// kernel's time. Here a workgroup (kFlatThreads lanes) takes a batch of up to kFlatThreads / 8 consecutive items at once:
//   0  lane = item: the item's record (ItemCtx, slot ranges, counts) into LDS — ONE round of dependent loads for the whole batch;
//   A  lane = triangle / lane = edge over the batch (prefix sums of the items' counts in LDS, five-step search): set-up records written
//      to the heap, the triangle's tile test kept in registers, the edges in the LDS table of the walks, the item's pixel box and the facing of its hull strip gathered with LDS atomics;
//   B  lane = item: the item's tile rectangle and its share of a pool of per-tile tables in LDS;
//   C  (pass 1) every edge adds its backdrop terms and counts, per tile of its own box, whether it matters there; every triangle
//      counts the tiles it reaches — the triangles use the item's table too, so no primitive needs a global atomic of its own;
//   D  (pass 2) lane = tile of the pool: ONE returning atomic on the tile's global counter reserves the list positions of everything the
//      item has there, the synthetic entries (COVER / backdrop units) are emitted;
//   E  (pass 3) edges and triangles walk again and take their positions from the LDS cursors — or, in the instantiations that replay, pass 1 has
//      kept every hit as a 32-bit record in LDS (key, pool cell, index in the cell) and pass 3 is a loop over the records: lane = record.
// A hull strip that folds (k_bin_edges) has its triangles binned the old way at the end. What does not fit a batch — more than 256
// triangles or 512 edges in ONE item, a rectangle beyond the pool — is queued for k_bin_edges<S, true>, which has no such limits.
// Slots, records and keys are exactly those of k_bin_edges; the order of a tile's entries in memory differs, the raster kernel sorts.
#ifndef CRH_FLAT_WAVES
#define CRH_FLAT_WAVES 4 // wavefronts per SIMD the kernel is compiled for, as a minimum AND a maximum (the kernel descriptor asks for registers accordingly). 4 fits since
                         // the set-up keeps no edge and no whole triangle record in registers and the tables take 19.4 KB per 128 lanes: 125 registers, no scratch
                         // memory, eight workgroups per CU, the benchmark scene's 1 663 batches in ONE round of 2 048 resident workgroups. -DCRH_FLAT_WAVES=3
                         // is the same code held at three waves (A/B runs): the step measures the same within its spread — what it gained over the 168-register
                         // kernel it gained from the smaller footprint beside the raster grid, not from the fourth wave.
#endif
#ifndef CRH_FLAT_ROUNDS
#define CRH_FLAT_ROUNDS 3
#endif
#ifndef CRH_FLAT_STAGE
#define CRH_FLAT_STAGE 64 // entries of a wavefront's pair stage: every append goes out at once (128, a flush per 65 to 128 entries, measured within 1.5 %: DESIGN.md §4.3)
#endif
#ifndef CRH_FLAT_THREADS
#define CRH_FLAT_THREADS 128 // threads of a workgroup of k_bin_flat: 256 (four wavefronts, a batch of up to 32 items), 128 or 64 (ONE wavefront, a quarter of every table).
                             // Round 5 (tools/r05b_flat_shape.sh): alone the kernel is fastest with 256 (S10k 0.112 ms; 128: 0.124; 64: 0.200) — but it runs in the gap between
                             // two raster kernels, where a workgroup starts as soon as ALL its wavefronts find registers and LDS on one CU, and a two-wave workgroup finds
                             // them earlier behind the draining raster grid: pipelined step S10k 0.3175 -> 0.3013 ms (64: 0.349), glyphs 0.716 -> 0.696 (0.708), S100k 2.07 -> 2.05 (1.94)
#endif
constexpr uint32_t kFlatThreads = CRH_FLAT_THREADS, kFlatWaveCount = kFlatThreads / 64u;
static_assert(kFlatThreads == 64u || kFlatThreads == 128u || kFlatThreads == 256u, "CRH_FLAT_THREADS: 64, 128 or 256");
#ifndef CRH_FLAT_POOL
#define CRH_FLAT_POOL 6 // tile cells of the batch's rectangles per thread
#endif
#ifndef CRH_FLAT_BATCH
#define CRH_FLAT_BATCH (CRH_FLAT_THREADS / 8) // items of a batch at most
#endif
#ifndef CRH_BIN_LOADS_ITEMS
#define CRH_BIN_LOADS_ITEMS 1 // k_bin_flat's item records: the item_elsewhere byte with the item's other words (0: in front of them, a round trip of its own)
#endif
#ifndef CRH_BIN_LOADS_DIRECT
#define CRH_BIN_LOADS_DIRECT 1 // direct tile lists in a batch that replays: a tile's place and room are fetched once per pool cell, beside the cell's atomic; 0: per entry
#endif
#ifndef CRH_FLAT_HITS
#define CRH_FLAT_HITS 400 // hit records per wavefront in the table of a workgroup that replays (k_bin_flat<S, T, true>): what the 128-thread tables leave of 160 KiB / 7, in whole
                          // LDS blocks — 23 024 of 23 040 B. The batch's free edge places come on top (10 000 paths need up to 1 109 records a batch, glyphs 733).
#endif
// A hit of pass 1 as pass 3 replays it, in 32 bits: the index among the item's edge and triangle entries of its pool cell (bits 0-8: every edge
// and every triangle of a batch enters a cell once at most), the pool cell (9-18), the key relative to the first slot of the batch's first item (19-31).
constexpr uint32_t kHitIndexBits = 9, kHitCellBits = 10, kHitKeyBits = 32u - kHitIndexBits - kHitCellBits;
// kFlatItems: entries of the index tables (find_item searches 32); kFlatBatch: items a batch holds (their LDS records)
constexpr uint32_t kFlatItems = 32, kFlatBatch = CRH_FLAT_BATCH, kFlatTris = kFlatThreads, kFlatEdgeRounds = CRH_FLAT_ROUNDS, kFlatEdges = kFlatThreads * kFlatEdgeRounds, kFlatPool = CRH_FLAT_POOL * kFlatThreads, kFlatStage = CRH_FLAT_STAGE; // 128 threads: 19.4 KB of LDS, static_assert in the kernel
static_assert(kFlatBatch >= 1u && kFlatBatch <= kFlatItems, "CRH_FLAT_BATCH");
constexpr uint32_t kFiOpaque = 1u, kFiSkip = 2u, kFiHullTris = 4u, kFiQueue = 8u; // kFiQueue: not binned here but by k_bin_edges (handed on when the item's turn is over)
struct FlatItem {
    ItemCtx ctx;
    uint32_t slot0, fe_slot0, synth_a, hull_slot0, synth_b; // absolute slot numbers of the item's regions
    uint32_t n_tri, n_fe, n_hull, n_hull_chain;
    uint32_t flags;  // kFi*
    int box[4];      // ordered-int images of the float box of everything the item draws: min x, min y, max x, max y (LDS atomics)
    uint32_t faces;  // bit 0: a strip triangle of the hull faces front, bit 1: one faces back
    uint32_t tx_a, ty_a, tx_b, ty_b, nx, n_rect;
};
CRH_D int ordered_int(float f) { // monotone float -> int (finite values): atomicMin / atomicMax on LDS integers
    const int i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7FFFFFFF);
}
CRH_D float ordered_float(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7FFFFFFF)); }
CRH_D uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}
// the largest j < 32 with begin[j] <= x (begin is non-decreasing, entries behind the batch hold 0xFFFFFFFF)
CRH_D uint32_t find_item(const uint32_t* begin, uint32_t x) {
    uint32_t j = 0;
#pragma unroll
    for (uint32_t step = 16; step > 0; step >>= 1)
        if (begin[j + step] <= x) j += step;
    return j;
}
// A workgroup barrier that orders LDS accesses only. __syncthreads() also waits for the wavefront's global stores (s_waitcnt vmcnt(0):
// gfx950 counts loads and stores with one counter), and the record stores of phase A — 46 MB per frame of the benchmark scene — took
// 50 us to drain at the first barrier behind them, every workgroup waiting at once. Nothing here reads global memory another wavefront
// of the workgroup wrote, so the stores may stay in flight across the barriers.
CRH_D void lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}
// A boundary edge in the LDS tables of k_bin_flat: its end points (one 16-byte access) and, in a table of 16-bit words beside them, its flags —
// five words instead of BinEdge's fourteen (the rest is recomputed with the very expressions load_edge used, so the values are the same bits).
struct PackedEdge {
    float lo_x, lo_y, hi_x, hi_y;
};
// bit 0 valid, 1 top-left, 2 hull, 3 sigma > 0, 4 down; 5 / 6: the strip triangle that starts at a hull edge's position faces front / back
// (the sign of BinEdge::strip_det; neither: none); bits 8-12: the item of the batch
constexpr uint32_t kPeValid = 1u, kPeStripFront = 32u, kPeStripBack = 64u;
CRH_D PackedEdge pack_edge(const BinEdge& e) { return PackedEdge{e.lo_x, e.lo_y, e.hi_x, e.hi_y}; }
CRH_D uint32_t pack_edge_flags(const BinEdge& e, uint32_t item) {
    return (e.valid ? kPeValid : 0u) | (e.tl ? 2u : 0u) | (e.hull ? 4u : 0u) | (e.sigma > 0 ? 8u : 0u) | (e.down ? 16u : 0u) |
           (e.strip_det != 0.0f ? (e.strip_det < 0.0f ? kPeStripFront : kPeStripBack) : 0u) | (item << 8);
}
CRH_D BinEdge unpack_edge(const PackedEdge& p, uint32_t flags) {
    BinEdge e = {};
    e.lo_x = p.lo_x, e.lo_y = p.lo_y, e.hi_x = p.hi_x, e.hi_y = p.hi_y;
    e.bx = p.hi_x - p.lo_x;
    e.nay = -(p.hi_y - p.lo_y);
    e.ymin = fminf(p.lo_y, p.hi_y), e.ymax = fmaxf(p.lo_y, p.hi_y);
    e.valid = (flags & kPeValid) != 0u, e.tl = (flags >> 1) & 1u, e.hull = (flags >> 2) & 1u, e.sigma = (flags & 8u) ? 1 : -1, e.down = (int)((flags >> 4) & 1u);
    return e;
}
// The value, but as one the compiler cannot know to be the same in every turn of a loop (_v: a vector register, _s: a scalar one): what is computed
// from it stays inside the turn instead of being hoisted in front of the loop and kept in registers across all of it.
CRH_D uint32_t per_turn_v(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}
CRH_D uint32_t per_turn_s(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(v));
#endif
    return v;
}
struct FlatTri { // a set-up triangle between the passes: its tile test and tile box
    TileTest test;
    uint32_t bx0, bx1, by0, nt, key, item;
};
#ifdef CRH_ABLATE // tools/bin_phases.py: cycles wavefront 0 of every workgroup of k_bin_flat spends per phase (summed in overflow[80 ...])
#define CRH_FLAT_PHASE(k)                                                                                              \
    if ((r.debug & 65536u) && tid == 0u) {                                                                             \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                  \
        atomicAdd(reinterpret_cast<unsigned long long*>(r.overflow + 80) + (k), now_ - phase_t);                       \
        phase_t = __builtin_amdgcn_s_memtime();                                                                        \
    }                                                                                                                  \
    if ((r.debug >> 24) == (k) + 1u) return; /* tools/ablate_flat.sh: the kernel up to and including phase k */
#else
#define CRH_FLAT_PHASE(k)
#endif
// what a batch holds follows from the workgroup's lanes (the tables of k_bin_flat<S, THREADS>; the host cuts its runs by the same numbers)
struct FlatShape {
    uint32_t threads, batch, tris, edges, pool;
};
constexpr FlatShape flat_shape(uint32_t threads) { return FlatShape{threads, threads / 8u, threads, threads * CRH_FLAT_ROUNDS, CRH_FLAT_POOL * threads}; }
constexpr bool flat_replays(uint32_t threads) { return threads == 128u && kFlatThreads == 128u; } // the instantiations of k_bin_flat whose pass 3 is a replay (k_bin_flat's REPLAY)
// REPLAY: pass 1 keeps every hit of an edge or a triangle as a 32-bit record in LDS and pass 3 is a loop over those records instead of the geometric
// walk a second time; replay_cap: the records a wavefront may keep (CRH_BIN_REPLAY_CAP; at most what its table holds). A batch in which a wavefront
// finds more, or whose keys outgrow the record, walks again — the whole batch: places from the records and places from cursor atomics never mix.
template <int S, uint32_t THREADS, bool REPLAY>
#ifdef CRH_FLAT_VGPRS
#define CRH_FLAT_BUDGET __attribute__((amdgpu_num_vgpr(CRH_FLAT_VGPRS)))
#else
#define CRH_FLAT_BUDGET
#endif
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(CRH_FLAT_WAVES, CRH_FLAT_WAVES))) CRH_FLAT_BUDGET void k_bin_flat(SceneDev s, RasterParams r, uint32_t items_per_group, uint32_t replay_cap) {
    // (the namespace's constants of these names describe the default shape; inside the kernel they are this instantiation's)
    constexpr uint32_t kFlatThreads = THREADS, kFlatWaveCount = THREADS / 64u, kFlatBatch = THREADS / 8u, kFlatTris = THREADS, kFlatEdges = THREADS * kFlatEdgeRounds, kFlatPool = CRH_FLAT_POOL * THREADS;
    static_assert(kFlatBatch >= 1u && kFlatBatch <= kFlatItems, "a batch's index tables hold 32 items");
    __shared__ uint32_t stage_tile[kFlatWaveCount][kFlatStage], stage_pos[kFlatWaveCount][kFlatStage], stage_key[kFlatWaveCount][kFlatStage];
    __shared__ FlatItem items[kFlatBatch];
    __shared__ uint32_t tri_begin[kFlatItems + 1], edge_begin[kFlatItems + 1], pool_begin[kFlatItems + 1];
    // Both backdrop sums of a pool cell in one word, bd + 65536 * hbd: a cell's sums — and every partial sum along its row — are bounded by the batch's edges
    // (one unit per edge and tile row), so each fits sixteen bits and a sum of such words is the word of the sums. Pass 2 puts the tile's verdict there.
    static_assert(kFlatEdges < 32768u, "a backdrop sum of a pool cell fits sixteen bits");
    __shared__ int pool_back[kFlatPool];
    __shared__ uint32_t pool_cursor[kFlatPool]; // pass 1: the entries the item's edges and triangles have in the tile (bits 0-19; bits 20-31: the hull edges among them), then the next list position
    __shared__ uint32_t batch[6];               // items in the batch, its triangles, its edges, tiles of its pool, items of the batch that are binned in this turn, (edge, tile row) pairs
    __shared__ uint32_t wave_opaque[kFlatWaveCount];         // opaque whole-tile covers every wavefront found in pass 2
    __shared__ uint32_t wave_entries[2u * kFlatWaveCount];        // entries every wavefront appends in pass 3 ([0..3]) and in pass 2 ([4..7]); then where its share of the pair stream begins
    __shared__ PackedEdge edge_table[kFlatEdges]; // the batch's boundary edges, from phase A on: the walks are balanced over (edge, tile row) pairs, whoever loaded the edge
    __shared__ uint16_t edge_flags[kFlatEdges];   // (kPe*)
    __shared__ uint32_t row_begin[kFlatEdges + 1]; // exclusive prefix of the tile rows every edge walks
    // The hits pass 1 keeps for pass 3 (REPLAY). An instantiation whose cells or entries per cell outgrow the record's fields, or with more than two
    // wavefronts, does not replay. The table is this array and, behind it, whatever the batch leaves free of the edge table (four records per edge the batch
    // does not have: a batch is full when ONE of its tables is, and with 10 000 cubic paths that is the triangles' — 162 of 384 edges on average, so the
    // 800 records here become 1 690, and the largest batch of that scene has 1 109 hits; 800 alone hold two batches in three). The two wavefronts share it —
    // the first fills it from the bottom, the second from the top, neither knows of the other —, so a wavefront that finds few leaves its share to its
    // neighbour; whether the two have met is seen behind pass 1's barrier from their counts (hit_count), and a batch in which they have walks again.
    constexpr bool kReplay = REPLAY && kFlatWaveCount <= 2u && kFlatPool <= (1u << kHitCellBits) && kFlatEdges + kFlatTris <= (1u << kHitIndexBits);
    constexpr uint32_t kHitRegion = kReplay ? CRH_FLAT_HITS * kFlatWaveCount : 1u;
    static_assert(sizeof(PackedEdge) == 16u, "four hit records in the place of an edge");
    __shared__ uint32_t hit_rec[kHitRegion];
    __shared__ uint32_t hit_count[kFlatWaveCount]; // records every wavefront wanted to keep
    __shared__ uint32_t replay_off;                // a key of this batch does not fit the record: the batch walks again
    // Everything above, against a compute unit's 160 KiB shared by the workgroups its four SIMDs hold at CRH_FLAT_WAVES wavefronts each (128 threads
    // at four waves: eight workgroups of 20 480 B). The hardware hands LDS out in blocks of 1 280 B, so the compiler's own occupancy figure is the last word.
    // A kernel that replays gives one of those workgroups up for its records (128 threads: seven of 23 040 B, which still hold the 1 663 batches of 10 000
    // paths at 4096^2 in one round of 1 792).
    constexpr uint32_t kFlatLds = sizeof(stage_tile) + sizeof(stage_pos) + sizeof(stage_key) + sizeof(items) + sizeof(tri_begin) + sizeof(edge_begin) + sizeof(pool_begin) + sizeof(pool_back) +
                                  sizeof(pool_cursor) + sizeof(batch) + sizeof(wave_opaque) + sizeof(wave_entries) + sizeof(edge_table) + sizeof(edge_flags) + sizeof(row_begin) +
                                  sizeof(hit_rec) + sizeof(hit_count) + sizeof(replay_off);
    constexpr uint32_t kFlatGroupsPerCu = 4u * CRH_FLAT_WAVES / kFlatWaveCount - (kReplay ? 1u : 0u), kLdsBlock = 1280u;
    static_assert(kFlatLds <= 160u * 1024u / kFlatGroupsPerCu / kLdsBlock * kLdsBlock, "k_bin_flat's LDS tables keep it from CRH_FLAT_WAVES wavefronts per SIMD (one workgroup per CU less where it replays)");
    const uint32_t tid0 = threadIdx.x;
    uint32_t turn = 0; // batches this workgroup has binned (the pair sub-stream of a batch follows from it)
    const float ry_first = S == 1 ? 0.5f : 0.125f, r_last = (float)(kTile - 1) + (S == 1 ? 0.5f : 0.875f); // extreme sample offsets inside a tile
    const uint32_t first_item = r.bin_batches ? r.bin_batches[2u * blockIdx.x] : blockIdx.x * items_per_group;
    const uint32_t last_item = r.bin_batches ? r.bin_batches[2u * blockIdx.x + 1u] : min(r.n_items, first_item + items_per_group);
    const bool all_queued = (r.debug & (1u | 2u | 4194304u)) != 0u; // debug bits 0, 1 (tests of k_bin_edges' own code paths), 22: every item takes that kernel
#ifdef CRH_ABLATE
    unsigned long long phase_t = __builtin_amdgcn_s_memtime();
    const unsigned long long born_t = phase_t; // (tools/bin_phases.py: the longest-lived workgroup, overflow[120..121], and the sum, [122..123])
    uint32_t dump_items = 0, dump_tris = 0, dump_edges = 0, dump_pool = 0, dump_work = 0, dump_walk = 0, dump_wave_hits = 0, dump_batch_hits = 0; // (... and what every workgroup held, CRH_BIN_DUMP)
#endif
    for (uint32_t next = first_item; next < last_item;) {
        // What follows from the lane's number and the frame's size is made anew in every turn (nearly every workgroup takes one): computed once in front
        // of the loop, the table addresses of every phase and the frame's size as floats lived in some forty vector registers from the first phase to the last.
        const uint32_t tid = per_turn_v(tid0), lane = tid & 63u, wave = tid >> 6;
        Stage st = {stage_tile[wave], stage_pos[wave], stage_key[wave], 0u, 0u, kFlatStage, 0xFFFFFFFFu}; // (empty between turns: every turn flushes what it staged)
        RasterParams rt = r; // (the set-up functions make the frame's size a float themselves)
        rt.width = per_turn_s(r.width), rt.height = per_turn_s(r.height);
        const float W = (float)rt.width, H = (float)rt.height;
        lds_barrier(); // (the previous batch's readers of the LDS records are through)
        // ---------------- 0: the records of the next items
        const uint32_t n_cand = min(kFlatBatch, last_item - next);
        if (kReplay && tid == 0u) replay_off = 0u;
        if (tid < n_cand) {
            const uint32_t item = next + tid;
#if CRH_BIN_LOADS_ITEMS
            // (a pass with a slab: the item has no tile row in it — neither binned here nor queued.) The byte is asked for with the item's other words, not in
            // front of them: its address is a select — without the table, a byte of the item's slot_begin word, which is read anyway —, its use is the last here.
            const uint8_t* const elsewhere_at = r.item_elsewhere ? r.item_elsewhere + item : reinterpret_cast<const uint8_t*>(r.slot_begin + item);
            const uint32_t elsewhere_byte = *elsewhere_at;
            const DrawItem it = item_of(r, item);
#else
            const DrawItem it = item_of(r, item);
            const bool elsewhere = r.item_elsewhere && r.item_elsewhere[item] != 0u; // (a pass with a slab: the item has no tile row in it — neither binned here nor queued)
#endif
            const ItemSlots k = item_slots(s, it);
            FlatItem& fi = items[tid];
            fi.ctx = item_ctx(s, r, it, k.cb);
            const uint32_t slot0 = r.slot_begin[item];
            fi.slot0 = slot0, fi.fe_slot0 = slot0 + k.fe0, fi.synth_a = slot0 + k.synth_a, fi.hull_slot0 = slot0 + k.hull0, fi.synth_b = slot0 + k.synth_b;
            fi.n_tri = k.n_tri, fi.n_fe = k.n_fe, fi.n_hull = k.n_hull, fi.n_hull_chain = k.n_hull;
            const float* c = fi.ctx.col;
            const bool opaque = c[3] == 1.0f && is_finite(c[0]) && is_finite(c[1]) && is_finite(c[2]) && r.occlude != 0u && (r.debug & 32768u) == 0u;
#if CRH_BIN_LOADS_ITEMS
            const bool elsewhere = r.item_elsewhere && elsewhere_byte != 0u;
#endif
            const bool oversize = k.n_tri > kFlatTris || k.n_fe + k.n_hull > kFlatEdges || all_queued || slot0 + k.total > r.slot_capacity;
            fi.flags = (opaque ? kFiOpaque : 0u) | ((oversize || elsewhere) ? kFiSkip : 0u) | ((oversize && !elsewhere && slot0 + k.total <= r.slot_capacity) ? kFiQueue : 0u);
            fi.box[0] = fi.box[1] = 0x7FFFFFFF, fi.box[2] = fi.box[3] = (int)0x80000000;
            fi.faces = 0u;
            fi.n_rect = 0u;
        }
        lds_barrier();
        if (wave == 0u) { // the batch: the longest run of items whose triangles and edges fit the lanes (an oversize item counts as empty)
            const FlatItem& mine_ = items[min(lane, kFlatBatch - 1u)];
            const bool real = lane < n_cand && lane < kFlatBatch, counted = real && (mine_.flags & kFiSkip) == 0u;
            const uint32_t nt = counted ? mine_.n_tri : 0u, ne = counted ? mine_.n_fe + mine_.n_hull : 0u;
            const uint32_t pt = wave_inclusive_scan(nt, lane), pe = wave_inclusive_scan(ne, lane);
            const unsigned long long fits = __ballot(real && pt <= kFlatTris && pe <= kFlatEdges);
            const uint32_t n_batch = (uint32_t)__builtin_ctzll(~fits); // leading lanes that fit (>= 1: one item alone always does)
            if (lane <= kFlatItems) {
                tri_begin[lane] = lane <= n_batch ? pt - nt : 0xFFFFFFFFu;
                edge_begin[lane] = lane <= n_batch ? pe - ne : 0xFFFFFFFFu;
            }
            const uint32_t total_t = (uint32_t)__shfl((int)pt, (int)n_batch - 1, 64), total_e = (uint32_t)__shfl((int)pe, (int)n_batch - 1, 64);
            if (lane == 0u) {
                batch[0] = n_batch, batch[1] = total_t, batch[2] = total_e;
                tri_begin[n_batch] = 0xFFFFFFFFu, edge_begin[n_batch] = 0xFFFFFFFFu; // (searches stop in front of it; the totals are in batch[])
            }
        }
        lds_barrier();
        const uint32_t n_batch = batch[0], n_tris = batch[1], n_edges = batch[2];
        CRH_FLAT_PHASE(0) // item records + batch
        // ---------------- A: set-up, lane = triangle and lane = edge (two edges per lane), records to the heap, boxes and hull facing to LDS.
        // All loads first, all stores last: gfx950 counts vector loads and stores with ONE counter, in order — a load issued behind the 128-byte
        // record stores can only be waited for together with them, and those take tens of microseconds to drain when every workgroup
        // writes its records at once.
        // A lane keeps nothing of its edges across the triangle's set-up: they go to the LDS tables the walks read anyway as soon as they are loaded
        // (LDS accesses are counted apart from the vector-memory ones) and come back from there for the record stores.
        FlatTri tri;
        tri.nt = 0u, tri.item = 0u, tri.key = 0u, tri.bx0 = tri.bx1 = tri.by0 = 0u;
        tri.test = TileTest{};
        PlainTri corners;
        corners.valid = false;
#if CRH_BIN_LOADS_TRIS
        TriRaw tri_raw = {};
#endif
#if CRH_BIN_LOADS_EDGES
        // Two waits for all of it: the flags of every round's fill edges; then every round's vertices and — issued behind them, in front of the
        // wait — the triangle's.
        {
            uint32_t edge_item[kFlatEdgeRounds], edge_bits[kFlatEdgeRounds];
            EdgeFlags edge_fl[kFlatEdgeRounds];
            EdgeVerts edge_v[kFlatEdgeRounds];
#pragma unroll
            for (int k = 0; k < (int)kFlatEdgeRounds; ++k) {
                const uint32_t e = tid + kFlatThreads * (uint32_t)k;
                const bool active = e < n_edges;
                const uint32_t j = active ? find_item(edge_begin, e) : 0u, i = e - edge_begin[j];
                const FlatItem& fi = items[j];
                edge_item[k] = j;
                edge_fl[k] = load_edge_flags(s, fi.ctx, fi.n_fe, i, active && i < fi.n_fe);
            }
#pragma unroll
            for (int k = 0; k < (int)kFlatEdgeRounds; ++k) hold_edge_flags(edge_fl[k]);
#pragma unroll
            for (int k = 0; k < (int)kFlatEdgeRounds; ++k) {
                const uint32_t e = tid + kFlatThreads * (uint32_t)k, j = edge_item[k];
                const FlatItem& fi = items[j];
                const EdgeWhere w = edge_where(s, fi.ctx, fi.n_fe, fi.n_hull, e - edge_begin[j], edge_fl[k]);
                edge_bits[k] = w.bits;
                edge_v[k] = load_edge_verts(w, e < n_edges);
            }
#if CRH_BIN_LOADS_TRIS
            if (tid < n_tris) {
                const uint32_t j = find_item(tri_begin, tid), t = tid - tri_begin[j];
                const FlatItem& fi = items[j];
                const ItemCtx& ctx = fi.ctx;
                const uint32_t c = t < ctx.cb[1] ? t : t - ctx.cb[1] + ctx.cb[2]; // the Shape's candidate numbering without the solid strips
                issue_plain_triangle(s, ctx, c, tri_raw);
                tri.key = fi.slot0 + 4u * t, tri.item = j;
            }
#endif
#pragma unroll
            for (int k = 0; k < (int)kFlatEdgeRounds; ++k) hold_edge_verts(edge_v[k]);
#if CRH_BIN_LOADS_TRIS
            hold_plain_triangle(tri_raw);
#endif
#pragma unroll
            for (int k = 0; k < (int)kFlatEdgeRounds; ++k) {
                const uint32_t e = tid + kFlatThreads * (uint32_t)k, j = edge_item[k];
                if (e < n_edges) {
                    const BinEdge loaded = finish_edge(rt, items[j].ctx, edge_bits[k], edge_v[k]);
                    edge_table[e] = pack_edge(loaded);
                    edge_flags[e] = (uint16_t)pack_edge_flags(loaded, j);
                }
            }
        }
#else
#pragma unroll
        for (int k = 0; k < (int)kFlatEdgeRounds; ++k) {
            const uint32_t e = tid + kFlatThreads * (uint32_t)k;
            if (e < n_edges) {
                const uint32_t j = find_item(edge_begin, e), i = e - edge_begin[j];
                const FlatItem& fi = items[j];
                const BinEdge loaded = load_edge(s, rt, fi.ctx, fi.n_fe, fi.n_hull, i);
                edge_table[e] = pack_edge(loaded);
                edge_flags[e] = (uint16_t)pack_edge_flags(loaded, j);
            }
        }
#endif
        CRH_FLAT_PHASE(1) // edge set-up (with CRH_BIN_LOADS_TRIS: the wait for the triangle's vertices too)
#if CRH_BIN_LOADS_TRIS && CRH_BIN_LOADS_EDGES
        if (tid < n_tris) finish_plain_triangle(items[tri.item].ctx, tri_raw, corners);
#else
        if (tid < n_tris) {
            const uint32_t j = find_item(tri_begin, tid), t = tid - tri_begin[j];
            const FlatItem& fi = items[j];
            const ItemCtx& ctx = fi.ctx;
            const uint32_t c = t < ctx.cb[1] ? t : t - ctx.cb[1] + ctx.cb[2]; // the Shape's candidate numbering without the solid strips
            load_plain_triangle(s, ctx, c, corners);
            tri.key = fi.slot0 + 4u * t, tri.item = j;
        }
#endif
        // ---- stores and LDS. The triangle's record in two halves whose values do not live at the same time: the coverage half, which the tile test
        // and the boxes are taken from before it is stored, then the fragment half.
#ifdef CRH_ABLATE
        const bool store_records = (r.debug & 8388608u) == 0u; // tools/ablate_flat.sh: no record stores
#else
        constexpr bool store_records = true;
#endif
        if (tid < n_tris) {
            FlatItem& fi = items[tri.item];
            float det;
            ushort4 box;
            if (place_plain_triangle(rt, fi.ctx, corners, det, box)) {
                PrimRec* out = reinterpret_cast<PrimRec*>(r.slots + (size_t)tri.key * 32u);
                { // (what the coverage half is made of goes on living as the tile test and the tile box)
                    PrimCoverage cov;
                    cov.box = box;
                    plain_triangle_coverage(corners, det, cov);
                    tri.test.set(cov, ry_first, r_last);
                    tri.bx0 = box.x / kTile, tri.bx1 = box.y / kTile, tri.by0 = box.z / kTile;
                    tri.nt = (tri.bx1 - tri.bx0 + 1u) * (box.w / kTile - tri.by0 + 1u);
                    atomicMin(&fi.box[0], ordered_int((float)box.x)), atomicMin(&fi.box[1], ordered_int((float)box.z));
                    atomicMax(&fi.box[2], ordered_int((float)box.y)), atomicMax(&fi.box[3], ordered_int((float)box.w));
                    if (store_records) out->cov = cov;
                }
                PrimFragment frag;
                plain_triangle_fragment(fi.ctx, corners, det, frag);
                if (store_records) out->frag = frag;
            }
        }
#pragma unroll
        for (int k = 0; k < (int)kFlatEdgeRounds; ++k) {
            const uint32_t at = tid + kFlatThreads * (uint32_t)k;
            if (at < n_edges) {
                const uint32_t flags = edge_flags[at], j = (flags >> 8) & 31u;
                FlatItem& fi = items[j];
                const BinEdge e = unpack_edge(edge_table[at], flags);
                if (e.valid) {
                    EdgeRec er;
                    er.flags = (EK_EDGE << 4) | (e.tl ? kEdgeTl : 0u) | (e.sigma > 0 ? kEdgeSigmaPos : 0u) | (e.hull ? kEdgeHull : 0u), er.pad0 = 0u;
                    er.lo_x = e.lo_x, er.lo_y = e.lo_y, er.hi_x = e.hi_x, er.hi_y = e.hi_y, er.bx = e.bx, er.nay = e.nay;
                    const uint32_t i = at - edge_begin[j];
                    if (store_records) *reinterpret_cast<EdgeRec*>(r.slots + (size_t)(i < fi.n_fe ? fi.fe_slot0 + i : fi.hull_slot0 + (i - fi.n_fe)) * 32u) = er;
                    atomicMin(&fi.box[0], ordered_int(e.lo_x)), atomicMin(&fi.box[1], ordered_int(e.ymin));
                    atomicMax(&fi.box[2], ordered_int(e.hi_x)), atomicMax(&fi.box[3], ordered_int(e.ymax));
                }
                // (a strip triangle is judged at its first position whether or not that position's chain edge is valid)
                if (flags & (kPeStripFront | kPeStripBack)) atomicOr(&fi.faces, (flags & kPeStripFront) ? 1u : 2u);
            }
        }
        CRH_FLAT_PHASE(2) // triangle set-up, record stores
        for (uint32_t q = tid; q < 31u * n_batch; q += kFlatThreads) { // the items' 4 backdrop + 27 COVER slots (the COVER ones carry the premultiplied source colour, shaders.wgsl:304-309)
            const uint32_t j = q / 31u, l = q - 31u * j;
            const FlatItem& fi = items[j];
            if (fi.flags & kFiSkip) continue;
            SynthRec sr = {};
            sr.flags = (EK_SYNTH << 4) | (l << 8);
            sr.first_slot = fi.slot0, sr.synth_a = fi.synth_a;
            const float* c = fi.ctx.col;
            if (l >= 4u) sr.r = c[0] * c[3], sr.g = c[1] * c[3], sr.b = c[2] * c[3], sr.a = c[3];
            if (store_records) *reinterpret_cast<SynthRec*>(r.slots + (size_t)(l < 4u ? fi.synth_a + l : fi.synth_b + l - 4u) * 32u) = sr;
        }
        lds_barrier();
        CRH_FLAT_PHASE(3) // synthetic records + barrier
        // ---------------- B: lane = item: tile rectangle, its tables in the pool; does the hull strip fold?
        if (wave == 0u) {
            uint32_t n_rect = 0;
            const bool mine = lane < n_batch;
            FlatItem& fi = items[min(lane, kFlatBatch - 1u)];
            if (mine && (fi.flags & kFiSkip) == 0u) {
                const float minx = ordered_float(fi.box[0]), miny = ordered_float(fi.box[1]), maxx = ordered_float(fi.box[2]), maxy = ordered_float(fi.box[3]);
                if (fi.box[0] <= fi.box[2]) { // something is drawn
                    const int px0 = (int)floorf(fminf(fmaxf(minx, 0.0f), W)), px1 = (int)floorf(fmaxf(fminf(maxx, W - 1.0f), -1.0f));
                    const int py0 = (int)floorf(fminf(fmaxf(miny, 0.0f), H)), py1 = (int)floorf(fmaxf(fminf(maxy, H - 1.0f), -1.0f));
                    // (the tile rows of the pass' slab only, crh_frame_set_tile_rows: a tile row's backdrops, counts and entries are its own; an item
                    // without a row in the slab has no rectangle and is not binned)
                    const uint32_t row_a = max((uint32_t)max(py0, 0) / kTile, r.slab_ty0), row_end = min((uint32_t)max(py1, 0) / kTile + 1u, r.slab_ty1);
                    if (px0 <= px1 && py0 <= py1 && row_a < row_end) {
                        fi.tx_a = (uint32_t)px0 / kTile, fi.tx_b = (uint32_t)px1 / kTile, fi.ty_a = row_a, fi.ty_b = row_end - 1u;
                        fi.nx = fi.tx_b - fi.tx_a + 1u;
                        n_rect = fi.nx * (fi.ty_b - fi.ty_a + 1u);
                    }
                }
                if (fi.n_hull != 0u && (fi.faces == 3u || (r.debug & 4u) != 0u)) fi.flags |= kFiHullTris, fi.n_hull_chain = 0u; // debug bit 2 (tests): always
            }
            // (a verified pass: what the item takes of a batch — the host sizes later passes' batches with it)
            if (r.item_cost && mine) {
                const bool skipped = (fi.flags & kFiSkip) != 0u, too_wide = n_rect > kFlatPool; // (too wide: queued once it is the first of a batch — a run of its own)
                r.item_cost[2u * (next + lane)] = skipped ? 0u : (too_wide ? 0xFFFFFFFFu : n_rect);
                r.item_cost[2u * (next + lane) + 1u] = (skipped || too_wide) ? 0x80000000u : (fi.n_tri | ((fi.n_fe + fi.n_hull) << 9) | ((fi.flags & kFiHullTris) ? 1u << 29 : 0u));
            }
            // Pool shares in item order. Items from the first one that does not fit are left to the workgroup's next turn (their records are
            // written again then); an item that does not fit the pool even alone goes to k_bin_edges.
            uint32_t end = wave_inclusive_scan(n_rect, lane);
            uint32_t n_fit = (uint32_t)__builtin_ctzll(~__ballot(mine && end <= kFlatPool)); // leading items that fit
            if (n_fit == 0u) {
                if (lane == 0u) fi.flags |= kFiSkip | kFiQueue;
                n_fit = 1u;
                if (lane == 0u) n_rect = 0u, end = 0u;
            }
            const uint32_t pool_total = (uint32_t)__shfl((int)end, (int)n_fit - 1, 64); // (every lane takes part in the shuffle)
            if (lane >= n_fit) n_rect = 0u, end = pool_total;
            if (mine) fi.n_rect = n_rect;
            if (lane <= kFlatItems) pool_begin[lane] = lane < n_batch ? end - n_rect : (lane == n_batch ? pool_total : 0xFFFFFFFFu);
            if (lane == 0u) batch[3] = pool_total, batch[4] = n_fit;
            // (handed on exactly once: a candidate that is not part of this turn is looked at again in the next one)
            if (lane < n_fit && (fi.flags & kFiQueue) != 0u) r.bin_queue[atomicAdd(&r.overflow[6], 1u)] = next + lane;
        }
        lds_barrier();
        const uint32_t n_pool = batch[3], n_turn = batch[4]; // (items n_turn .. n_batch - 1 are set up but not binned: n_rect == 0)
        for (uint32_t q = tid; q < n_pool; q += kFlatThreads) pool_back[q] = 0, pool_cursor[q] = 0u;
        lds_barrier();
        CRH_FLAT_PHASE(4) // rectangles, pool cleared
        // ---------------- the edges' walks are balanced over (edge, tile row) pairs. A lane that walked ITS edge kept its wavefront in the loop
        // for as long as the longest edge among 64 took (a hull edge across a 256-pixel Shape reaches 40 tiles, a polygon edge 3): nine
        // tenths of the lane-steps of the walks were idle. So every edge goes to an LDS table with the number of tile rows of its own box
        // (clamped to its item's rectangle), the counts are summed, and lane w of a pass takes pair w: the edge by a ten-step search in
        // the prefix sums, then the row. Within its row an edge visits the columns its LINE can reach — a float estimate with a margin
        // (2 px + 4e-6 of the largest coordinate: the distance at which f32 rounding can still flip an edge function is about 1e-7 of it),
        // clamped to the box; whether the edge matters in a tile is decided by the exact test as ever. Coordinates beyond 1e6 and horizontal
        // edges take the whole width of the box.
        struct EdgeBox {
            int bx0, bx1, by0, by1;
        };
        auto edge_box = [&](const BinEdge& e, const FlatItem& fi) {
            const int x_lo = (int)ceilf((e.lo_x - r_last) * (1.0f / (float)kTile) - 0.01f), x_hi = (int)floorf(e.hi_x * (1.0f / (float)kTile) + 0.01f);
            const int y_lo = (int)ceilf((e.ymin - r_last) * (1.0f / (float)kTile) - 0.01f), y_hi = (int)floorf((e.ymax - ry_first) * (1.0f / (float)kTile) + 0.01f);
            return EdgeBox{max(x_lo, (int)fi.tx_a), min(x_hi, (int)fi.tx_b), max(y_lo, (int)fi.ty_a), min(y_hi, (int)fi.ty_b)};
        };
#pragma unroll
        for (int k = 0; k < (int)kFlatEdgeRounds; ++k) {
            const uint32_t e = tid + kFlatThreads * (uint32_t)k;
            if (e < n_edges) {
                const uint32_t flags = edge_flags[e];
                const FlatItem& fi = items[(flags >> 8) & 31u];
                // the edge takes part: valid, its item is drawn here, and — a hull edge — its hull is binned as a chain
                bool live = (flags & kPeValid) != 0u && fi.n_rect != 0u && !((flags & 4u) != 0u && (fi.flags & kFiHullTris) != 0u);
                uint32_t rows = 0;
                if (live) {
                    const EdgeBox box = edge_box(unpack_edge(edge_table[e], flags), fi);
                    live = box.by0 <= box.by1; // (an edge left of the rectangle — a Shape that sticks out of the frame — has no tile to walk but still crosses the rows' backdrop lines)
                    if (live) rows = (uint32_t)(box.by1 - box.by0 + 1);
                }
                if (!live) edge_flags[e] = (uint16_t)(flags & ~kPeValid);
                row_begin[e] = rows;
            }
        }
        lds_barrier();
        if (wave == 0u) { // exclusive prefix of the row counts: twelve consecutive edges per lane
            const uint32_t per = (n_edges + 63u) / 64u, first = lane * per, last = min(n_edges, first + per);
            uint32_t sum = 0;
            for (uint32_t e = first; e < last; ++e) sum += row_begin[e];
            uint32_t run = wave_inclusive_scan(sum, lane) - sum;
            for (uint32_t e = first; e < last; ++e) {
                const uint32_t n = row_begin[e];
                row_begin[e] = run;
                run += n;
            }
            const uint32_t total = (uint32_t)__shfl((int)run, 63, 64);
            if (lane == 0u) row_begin[n_edges] = total, batch[5] = total;
        }
        lds_barrier();
        const uint32_t n_work = batch[5];
        // visit(active, edge, its item, the tile row, the columns x0 .. x1 of that row worth a test, the edge's slot number)
        auto for_edge_rows = [&](auto&& visit) {
            for (uint32_t w0 = 0; w0 < n_work; w0 += kFlatThreads) {
                const uint32_t w = w0 + tid;
                const bool active = w < n_work;
                uint32_t ei = 0; // the largest edge index with row_begin <= w (edges without rows share their successor's entry and are passed over)
#ifdef CRH_ABLATE
                if (r.debug & 4096u) ei = w % max(n_edges, 1u); else // what does the search cost? (the wrong edges: timing only)
#endif
#pragma unroll
                for (uint32_t step = kFlatEdges >= 512u ? 512u : (kFlatEdges >= 256u ? 256u : 128u); step > 0u; step >>= 1)
                    if (ei + step < n_edges && row_begin[ei + step] <= w) ei += step;
                const uint32_t pe_flags = edge_flags[active ? ei : 0u];
                const BinEdge e = unpack_edge(edge_table[active ? ei : 0u], pe_flags);
                const uint32_t j = (pe_flags >> 8) & 31u;
                const FlatItem& fi = items[j];
                const EdgeBox box = edge_box(e, fi);
                const int ty = box.by0 + (int)(w - row_begin[ei]);
                int x0 = box.bx0, x1 = box.bx1;
                const float dy = e.hi_y - e.lo_y, largest = fmaxf(fmaxf(fabsf(e.lo_x), fabsf(e.hi_x)), fmaxf(fabsf(e.lo_y), fabsf(e.hi_y)));
                if (dy != 0.0f && largest < 1.0e6f) {
                    const float xs = (e.hi_x - e.lo_x) / dy, pad = 2.0f + 4.0e-6f * largest;
                    const float ty0 = (float)(ty * kTile), ya = ty0 + ry_first - pad, yb = ty0 + r_last + pad;
                    const float xa = e.lo_x + (ya - e.lo_y) * xs, xb = e.lo_x + (yb - e.lo_y) * xs;
                    const float lo = fminf(xa, xb) - pad - r_last, hi = fmaxf(xa, xb) + pad;
                    // (clamped as floats first: the estimates of a steep row can be far outside anything an int holds)
                    x0 = (int)floorf(fmaxf(lo * (1.0f / (float)kTile), (float)box.bx0));
                    x1 = (int)floorf(fminf(hi * (1.0f / (float)kTile), (float)box.bx1));
                }
                const uint32_t i = ei - edge_begin[j];
                visit(active, e, j, fi, ty, x0, x1, i < fi.n_fe ? fi.fe_slot0 + i : fi.hull_slot0 + (i - fi.n_fe));
            }
        };
        // does the edge matter in tile (tx, ty)? (the exact test of k_bin_edges)
        auto matters = [&](const BinEdge& e, int tx, int ty) {
            const bool up = e.nay > 0.0f; // E grows with ry (bx >= 0) and with rx iff nay > 0
            const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile), q0y = ty0 + ry_first;
            const float c = e.bx * (ty0 - e.lo_y) + e.nay * (tx0 - e.lo_x);
            const bool gmax = accepts(fmaf(r_last, e.bx, fmaf(up ? r_last : 0.0f, e.nay, c)), e.tl), gmin = accepts(fmaf(ry_first, e.bx, fmaf(up ? 0.0f : r_last, e.nay, c)), e.tl);
            return gmax != gmin && e.ymin <= ty0 + r_last && e.ymax >= q0y && e.lo_x <= tx0 + r_last && e.hi_x >= tx0;
        };
        auto walk_tri = [&](const FlatTri& t, bool live, auto&& visit) { // (the triangle's tile box, cut to the rows of its item's rectangle: the slab of a tile split)
            const FlatItem& of = items[t.item];
            const uint32_t nxt = t.bx1 - t.bx0 + 1u, row_a = max(t.by0, of.ty_a), row_end = min(t.by0 + t.nt / nxt, of.ty_b + 1u);
            const uint32_t nt = (live && row_a < row_end) ? nxt * (row_end - row_a) : 0u, longest = wave_max_u32(nt);
            uint32_t tx = t.bx0, ty = row_a;
            for (uint32_t w = 0; w < longest; ++w) {
                visit(w < nt && t.test.hit(tx, ty), tx, ty);
                if (++tx > t.bx1) tx = t.bx0, ++ty;
            }
        };
        // ---------------- C: pass 1
        uint32_t my_entries = 0; // what this lane will append in pass 3
        // (REPLAY) ... and what the wavefront has found so far (uniform). A hit is kept with what the cell's counter held in front of it — the counter's
        // atomic returns it —, which is the entry's index among the item's edge and triangle entries of that tile: pass 2 turns the counter into the first
        // place of those entries in the tile's list, and first place + index is where pass 3 puts the key.
        uint32_t n_hits = 0;
        const uint32_t key0 = kReplay ? items[0].slot0 : 0u; // (a batch's items are consecutive, so are their slots: no key of the batch lies below the first item's first slot)
        const uint32_t hit_room = kReplay ? kHitRegion + 4u * (kFlatEdges - n_edges) : 0u; // records the table holds in this batch: hit_rec, then the edge table behind the batch's edges
        // record `at` of this wavefront (at < hit_room): counted from the bottom of the table by the first wavefront, from its top by the second
        auto hit_slot = [&](uint32_t at) -> uint32_t* {
            const uint32_t place = (wave & 1u) ? hit_room - 1u - at : at;
            return place < kHitRegion ? &hit_rec[place] : reinterpret_cast<uint32_t*>(edge_table + n_edges) + (place - kHitRegion);
        };
        auto remember = [&](bool hit, uint32_t cell, uint32_t counted, uint32_t key) {
            const unsigned long long ballot = __ballot(hit);
            if (!ballot) return;
            const uint32_t at = n_hits + lanes_below(ballot, lane), rel = key - key0;
            if (hit) {
                if (rel >> kHitKeyBits) replay_off = 1u;
                else if (at < hit_room) *hit_slot(at) = (rel << (kHitIndexBits + kHitCellBits)) | (cell << kHitIndexBits) | (counted & ((1u << kHitIndexBits) - 1u));
            }
            n_hits += (uint32_t)__popcll(ballot);
        };
        for_edge_rows([&](bool active, const BinEdge& e, uint32_t j, const FlatItem& fi, int ty, int x0, int x1, uint32_t key) {
            const uint32_t base = pool_begin[j] + ((uint32_t)ty - fi.ty_a) * fi.nx, nx = fi.nx, tx_a = fi.tx_a;
            // Along a tile row the backdrop term of an edge that crosses the row's line is 0 left of the edge and +-1 from some column on (the
            // edge function is monotone in x under fmaf, so the very predicate a tile would evaluate switches once): that column is found
            // by bisection — five exact evaluations instead of one per column — and the unit goes there alone; pass 2 sums along the row.
            const float ty0 = (float)(ty * kTile), q0y = ty0 + ry_first;
            const bool crosses = active && e.ymin <= q0y && q0y < e.ymax; // Y_e at the backdrop row
            const uint32_t widest = wave_max_u32(crosses ? nx : 0u);
            if (widest) {
                uint32_t lo = 0, hi = crosses ? nx : 0u; // the first column with a non-zero term lies in [lo, hi]
                for (uint32_t span = widest; span > 0u; span >>= 1) { // (ceil(log2(widest + 1)) steps settle every lane)
                    const uint32_t mid = (lo + hi) >> 1;
                    const float tx0 = (float)((tx_a + mid) * kTile);
                    const float c = e.bx * (ty0 - e.lo_y) + e.nay * (tx0 - e.lo_x);
                    const bool gq0 = accepts(fmaf(ry_first, e.bx, fmaf(0.0f, e.nay, c)), e.tl);
                    const bool nonzero = ((gq0 ? 1 : 0) - e.down) != 0; // sigma * Y(q0) * (g(q0) - down)
                    if (lo < hi) {
                        if (nonzero) hi = mid; else lo = mid + 1u;
                    }
                }
                if (crosses && lo < nx) atomicAdd(&pool_back[base + lo], (e.down ? -e.sigma : e.sigma) * (e.hull ? 65536 : 1));
            }
            const uint32_t cols = wave_max_u32(active && x0 <= x1 ? (uint32_t)(x1 - x0 + 1) : 0u);
            for (uint32_t c = 0; c < cols; ++c) {
                const int tx = x0 + (int)c;
                if (kReplay) {
                    const bool hit = active && tx <= x1 && matters(e, tx, ty);
                    const uint32_t cell = base + ((uint32_t)tx - tx_a);
                    uint32_t counted = 0;
                    if (hit) counted = atomicAdd(&pool_cursor[cell], e.hull ? 0x00100001u : 1u), ++my_entries;
                    remember(hit, cell, counted, key);
                } else if (active && tx <= x1 && matters(e, tx, ty)) atomicAdd(&pool_cursor[base + ((uint32_t)tx - tx_a)], e.hull ? 0x00100001u : 1u), ++my_entries;
            }
        });
        if (n_tris) {
            const FlatItem& fi = items[tri.item];
            const bool live = tri.nt != 0u && fi.n_rect != 0u;
            const uint32_t base = pool_begin[tri.item], nx = fi.nx, tx_a = fi.tx_a, ty_a = fi.ty_a;
            walk_tri(tri, live, [&](bool hit, uint32_t tx, uint32_t ty) {
                if (kReplay) {
                    const uint32_t cell = base + (ty - ty_a) * nx + (tx - tx_a);
                    uint32_t counted = 0;
                    if (hit) counted = atomicAdd(&pool_cursor[cell], 1u), ++my_entries;
                    remember(hit, cell, counted, tri.key);
                } else if (hit) atomicAdd(&pool_cursor[base + (ty - ty_a) * nx + (tx - tx_a)], 1u), ++my_entries;
            });
        }
        if (kReplay && lane == 0u) hit_count[wave] = n_hits;
        lds_barrier();
        // (REPLAY) does the batch replay? (uniform over the workgroup: LDS words and a kernel argument)
        bool replay = kReplay;
        if (kReplay) {
            replay = replay_off == 0u;
            uint32_t together = 0;
#pragma unroll
            for (uint32_t w = 0; w < kFlatWaveCount; ++w) {
                const uint32_t n = hit_count[w];
                together += n;
                replay = replay && n <= replay_cap;
            }
            replay = replay && together <= hit_room;
            replay = __builtin_amdgcn_readfirstlane((int)replay) != 0; // (a scalar: what depends on it is a branch, not a mask)
            if (!replay && tid == 0u) atomicAdd(&r.overflow[kReplayFallbackWord], 1u);
        }
        CRH_FLAT_PHASE(5) // pass 1
        // ---------------- D: pass 2, lane = tile of the pool (the COVER entry carries one unit of either backdrop).
        // Pass 1 left every edge's backdrop unit at the first column it applies to: summed along the rows first, in place (the lane of a row's
        // first tile walks the row). 2a: what the item has in the tile — COVER entry, backdrop units — and ONE returning atomic on the tile's
        // global counter for all of it plus the edges' and triangles' entries; the atomics of all the lane's tiles are in flight together,
        // and the tile's verdict replaces its backdrops in the LDS tables. Then the workgroup reserves its range of the pair stream with one
        // atomic (every wavefront knows what it will append), and 2b emits the synthetic entries.
        constexpr uint32_t kChunks = kFlatPool / kFlatThreads;
#pragma unroll 1
        for (uint32_t ch = 0; ch * kFlatThreads < n_pool; ++ch) {
            const uint32_t p = ch * kFlatThreads + tid;
            if (p < n_pool) {
                const uint32_t j = find_item(pool_begin, p);
                const uint32_t q = p - pool_begin[j], nx = items[j].nx;
                if (q % nx == 0u)
                    for (uint32_t c = 1; c < nx; ++c) pool_back[p + c] += pool_back[p + c - 1u];
            }
        }
        lds_barrier();
        uint32_t my_synth = 0, my_opaque = 0;
        // Direct tile lists in a batch that replays: where a tile's list lies (r.tile_base) is a property of the pool cell, so 2a asks for it beside the cell's
        // atomic — all of a lane's cells in flight together — and leaves the cell two addresses instead of a position and a tile: where the first entry of the
        // item's edges and triangles goes in r.tile_list (pool_cursor) and where the tile's place ends (pool_back). The synthetic entries are stored then and
        // there, 2b has nothing left to do, and pass 3 is LDS reads and stores: no entry waits for a load. (stage_flush_direct's test, entry by entry, as ever:
        // every position below the room is written, none beyond it or beyond pair_capacity, and an entry that finds no room raises overflow[0].)
        const bool direct_cells = kReplay && CRH_BIN_LOADS_DIRECT != 0 && replay && r.direct != 0u; // (uniform)
        // the keys of a cell's synthetic entries from its verdict (below)
        struct SynthKeys {
            uint32_t cover, bd, hbd;
        };
        auto synth_keys = [&](const FlatItem& fi, uint32_t verdict) {
            const uint32_t cbd1 = 1u + ((verdict >> 25) & 1u) - ((verdict >> 27) & 1u), chbd1 = 1u + ((verdict >> 26) & 1u) - ((verdict >> 28) & 1u); // sign of either backdrop + 1
            return SynthKeys{fi.synth_b + cbd1 + 3u * chbd1 + ((verdict >> 29) & 1u ? kCoverOpaque : ((verdict >> 30) & 1u ? kCoverHull : 0u)),
                             fi.synth_a + ((verdict >> 25) & 1u ? 0u : 1u), fi.synth_a + ((verdict >> 26) & 1u ? 2u : 3u)};
        };
        {
            uint32_t reserved[kChunks], lefts[kChunks], place[kChunks], place_end[kChunks];
#pragma unroll
            for (uint32_t ch = 0; ch < kChunks; ++ch) { // 2a
                reserved[ch] = 0u, lefts[ch] = 0u, place[ch] = 0u, place_end[ch] = 0u;
                const uint32_t p = ch * kFlatThreads + tid;
                if (p >= n_pool) continue;
                const uint32_t j = find_item(pool_begin, p);
                const FlatItem& fi = items[j];
                const uint32_t q = p - pool_begin[j], qy = q / fi.nx, qx = q - qy * fi.nx;
                const uint32_t tile = (fi.ty_a + qy) * r.tiles_x + fi.tx_a + qx;
                const int both = pool_back[p], bd = (int)(short)(both & 0xFFFF), hbd = (both - bd) >> 16;
                const uint32_t counted = pool_cursor[p];
                const uint32_t n_touching = counted & 0x000FFFFFu; // entries of the item's edges and triangles in this tile
                const bool hull_touch = (counted >> 20) != 0u;
                const uint32_t abd = (uint32_t)(bd < 0 ? -bd : bd), ahbd = (uint32_t)(hbd < 0 ? -hbd : hbd);
                const bool cover = fi.n_hull_chain != 0u && (hbd != 0 || hull_touch); // the tile is inside the hull or its boundary crosses it
                const int cbd = bd > 0 ? 1 : (bd < 0 ? -1 : 0), chbd = hbd > 0 ? 1 : (hbd < 0 ? -1 : 0);
                const bool hull_over_tile = cover && hbd != 0 && !hull_touch;
                const bool replaces_tile = hull_over_tile && (fi.flags & kFiOpaque) != 0u && n_touching == 0u && (bd & (int)r.winding_mask) != 0;
                const uint32_t n_bd = cover ? (abd ? abd - 1u : 0u) : abd, n_hbd = cover ? (ahbd ? ahbd - 1u : 0u) : 0u;
                const uint32_t left = (cover ? 1u : 0u) + n_bd + n_hbd;
                lefts[ch] = left;
                my_synth += left;
                my_opaque += replaces_tile ? 1u : 0u;
                if (left + n_touching) reserved[ch] = atomicAdd(&r.tile_count[tile], left + n_touching);
                if (direct_cells) place[ch] = r.tile_base[tile], place_end[ch] = r.tile_base[tile + 1u];
                // the verdict, for 2b: left (bits 0-11), backdrop units (12-23), COVER entry (24), bd > 0 (25), hbd > 0 (26), bd < 0 (27), hbd < 0 (28),
                // the COVER entry replaces the tile (29) or lies over all of it (30) — 2b makes the COVER key of the last six
                pool_back[p] = (int)(left | (n_bd << 12) | (cover ? 1u << 24 : 0u) | (cbd > 0 ? 1u << 25 : 0u) | (chbd > 0 ? 1u << 26 : 0u) | (cbd < 0 ? 1u << 27 : 0u) | (chbd < 0 ? 1u << 28 : 0u) |
                                     (replaces_tile ? 1u << 29 : 0u) | (hull_over_tile ? 1u << 30 : 0u));
            }
            // ONE wait for all of it, here, in front of the first key store (behind a store, every wait for a load is a wait for that store too) and on either
            // path (a register still marked as a load's target at the join below would make the next instruction that touches it wait there)
#pragma unroll
            for (uint32_t ch = 0; ch < kChunks; ++ch) held(reserved[ch]), held(place[ch]), held(place_end[ch]);
            if (direct_cells) {
#pragma unroll
                for (uint32_t ch = 0; ch < kChunks; ++ch) {
                    const uint32_t p = ch * kFlatThreads + tid;
                    if (p >= n_pool) continue;
                    const uint32_t base = place[ch], room = min(place_end[ch] - base, r.pair_capacity > base ? r.pair_capacity - base : 0u), limit = base + room;
                    const uint32_t verdict = (uint32_t)pool_back[p];
                    const SynthKeys keys = synth_keys(items[find_item(pool_begin, p)], verdict);
                    uint32_t at = base + reserved[ch], n_bd = (verdict >> 12) & 4095u;
                    bool cover = (verdict >> 24) & 1u, outgrown = false;
                    for (uint32_t left = lefts[ch]; left != 0u; --left, ++at) {
                        uint32_t key = keys.hbd;
                        if (cover)
                            cover = false, key = keys.cover;
                        else if (n_bd)
                            --n_bd, key = keys.bd;
                        if (at < limit) r.tile_list[at] = key;
                        else outgrown = true;
                    }
                    if (outgrown) r.overflow[0] = 1u; // the tile has outgrown the place the previous frame left it
                    pool_cursor[p] = at, pool_back[p] = (int)limit;
                }
            } else {
#pragma unroll
            for (uint32_t ch = 0; ch < kChunks; ++ch)
                if (ch * kFlatThreads + tid < n_pool) pool_cursor[ch * kFlatThreads + tid] = reserved[ch] + lefts[ch]; // where the edges' and triangles' entries go
            }
        }
        {
            uint32_t a = my_entries, b = my_synth | (my_opaque << 22); // (6 cells per lane, < 4096 entries each: a wavefront's sums stay below 2^22 and 2^10)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) a += (uint32_t)__shfl_xor((int)a, d, 64), b += (uint32_t)__shfl_xor((int)b, d, 64);
            if (lane == 0u) wave_entries[wave] = a, wave_entries[kFlatWaveCount + wave] = b & 0x003FFFFFu, wave_opaque[wave] = b >> 22;
        }
        lds_barrier();
        if (tid == 0u) { // the workgroup's range of the pair stream: wavefront w's pass-2 entries, then its pass-3 entries
            uint32_t total = 0;
            for (uint32_t w = 0; w < 2u * kFlatWaveCount; ++w) total += wave_entries[w];
#ifdef CRH_ABLATE
            { // (tools/bin_phases.py: the hits of pass 1 — pass 3's entries — per wavefront and per batch, the largest of the workgroup's turns)
                uint32_t hits = 0;
                for (uint32_t w = 0; w < kFlatWaveCount; ++w) hits += wave_entries[w], dump_wave_hits = max(dump_wave_hits, wave_entries[w]);
                dump_batch_hits = max(dump_batch_hits, hits);
            }
#endif
            uint32_t opaque = 0;
            for (uint32_t w = 0; w < kFlatWaveCount; ++w) opaque += wave_opaque[w];
            if (opaque) atomicAdd(&r.overflow[4], opaque); // the host's statistic: are there tiles to start late in?
            const uint32_t sub = ((blockIdx.x + 40503u * turn) * 2654435761u) >> 26, region = r.pair_capacity / kSubStreams;
            uint32_t begin = 0xFFFFFFFFu;
            if (r.direct) {
                begin = 0u; // (no pair stream: the entries go straight into the lists)
            } else if (total) {
                const uint32_t got = atomicAdd(&r.pair_cursor[sub], total);
                if (got + total > region)
                    r.overflow[5] = 1u; // this region is full: the host grows the stream and runs the pass again (nothing of this batch is written)
                else
                    begin = sub * region + got;
            }
            for (uint32_t w = 0; w < kFlatWaveCount; ++w) {
                const uint32_t mine = wave_entries[kFlatWaveCount + w] + wave_entries[w];
                wave_entries[w] = begin;
                if (begin != 0xFFFFFFFFu) begin += mine;
            }
        }
        lds_barrier();
        st.at = wave_entries[wave];
#pragma unroll 1
        for (uint32_t ch = 0; !direct_cells && ch * kFlatThreads < n_pool; ++ch) { // 2b
            const uint32_t p = ch * kFlatThreads + tid;
            const bool active = p < n_pool;
            const uint32_t j = active ? find_item(pool_begin, p) : 0u;
            const FlatItem& fi = items[j];
            const uint32_t q = active ? p - pool_begin[j] : 0u, row_len = max(fi.nx, 1u), qy = q / row_len, qx = q - qy * row_len;
            const uint32_t tile = (fi.ty_a + qy) * r.tiles_x + fi.tx_a + qx;
            const uint32_t verdict = active ? (uint32_t)pool_back[p] : 0u;
            const SynthKeys keys = synth_keys(fi, verdict);
            const uint32_t cover_key = keys.cover, bd_key = keys.bd, hbd_key = keys.hbd;
            uint32_t left = verdict & 4095u, n_bd = (verdict >> 12) & 4095u, pos = active ? pool_cursor[p] - left : 0u;
            bool cover = (verdict >> 24) & 1u;
            if (replay && active) pool_back[p] = (int)tile; // (the verdict is read: the cell's word now tells the replay which tile the cell is)
            for (;;) {
                const unsigned long long ballot = __ballot(left != 0u);
                if (!ballot) break;
                uint32_t key = 0;
                if (left) {
                    if (cover)
                        cover = false, key = cover_key;
                    else if (n_bd)
                        --n_bd, key = bd_key;
                    else
                        key = hbd_key;
                }
                stage_append<true>(st, r, lane, ballot, tile, pos, key);
                if (left) ++pos, --left;
            }
        }
        lds_barrier(); // (pass 3 moves the cursors 2b has just read)
        CRH_FLAT_PHASE(6) // pass 2
        // ---------------- E: pass 3: every entry of an edge or a triangle with its place in the tile's list. A replay of the records pass 1 kept, lane = record:
        // no search, no edge box, no exact test, no LDS atomic — the keys go where stage_append<true> would have put them, the wavefront's own
        // records to the wavefront's own share of the workgroup's range ...
        if (replay) {
            stage_flush_reserved(st, r, lane); // (the synthetic entries of 2b)
            for (uint32_t i = lane; i < n_hits; i += 64u) {
                const uint32_t rec = *hit_slot(i), cell = (rec >> kHitIndexBits) & ((1u << kHitCellBits) - 1u);
                // (direct_cells: `pos` is the entry's address in r.tile_list and `tile` the end of the tile's place there)
                const uint32_t tile = (uint32_t)pool_back[cell], pos = pool_cursor[cell] + (rec & ((1u << kHitIndexBits) - 1u)), key = key0 + (rec >> (kHitIndexBits + kHitCellBits));
#ifdef CRH_ABLATE
                if (r.debug & 512u) continue;
#endif
                if (direct_cells) {
                    if (pos < tile) r.tile_list[pos] = key;
                    else r.overflow[0] = 1u; // the tile has outgrown the place the previous frame left it
                } else if (r.direct) { // (stage_flush_direct's store)
                    const uint32_t place = r.tile_base[tile];
                    if (pos < r.tile_base[tile + 1u] - place && place + pos < r.pair_capacity) r.tile_list[place + pos] = key;
                    else r.overflow[0] = 1u; // the tile has outgrown the place the previous frame left it
                } else if (st.at != 0xFFFFFFFFu) {
                    r.pair_tile[st.at + i] = tile, r.pair_pos[st.at + i] = pos, r.pair_key[st.at + i] = key;
                }
            }
            if (st.at != 0xFFFFFFFFu) st.at += n_hits;
        } else {
        // ... or, in a batch that does not replay, the same walk again, the places from the cursors
        for_edge_rows([&](bool active, const BinEdge& e, uint32_t j, const FlatItem& fi, int ty, int x0, int x1, uint32_t key) {
            const uint32_t base = pool_begin[j] + ((uint32_t)ty - fi.ty_a) * fi.nx, tx_a = fi.tx_a;
            const uint32_t cols = wave_max_u32(active && x0 <= x1 ? (uint32_t)(x1 - x0 + 1) : 0u);
            for (uint32_t c = 0; c < cols; ++c) {
                const int tx = x0 + (int)c;
                const bool hit = active && tx <= x1 && matters(e, tx, ty);
                const unsigned long long ballot = __ballot(hit);
                if (ballot) {
                    uint32_t pos = 0;
                    if (hit) pos = atomicAdd(&pool_cursor[base + ((uint32_t)tx - tx_a)], 1u);
                    stage_append<true>(st, r, lane, ballot, (uint32_t)ty * r.tiles_x + (uint32_t)tx, pos, key);
                }
            }
        });
        if (n_tris) {
            const FlatItem& fi = items[tri.item];
            const bool live = tri.nt != 0u && fi.n_rect != 0u;
            const uint32_t base = pool_begin[tri.item], nx = fi.nx, tx_a = fi.tx_a, ty_a = fi.ty_a;
            walk_tri(tri, live, [&](bool hit, uint32_t tx, uint32_t ty) {
                const unsigned long long ballot = __ballot(hit);
                if (ballot) {
                    uint32_t pos = 0;
                    if (hit) pos = atomicAdd(&pool_cursor[base + (ty - ty_a) * nx + (tx - tx_a)], 1u);
                    stage_append<true>(st, r, lane, ballot, ty * r.tiles_x + tx, pos, tri.key);
                }
            });
        }
        stage_flush_reserved(st, r, lane); // (the batch's range is used up exactly)
        }
        CRH_FLAT_PHASE(7) // pass 3
        // ---------------- hull strips that fold: triangle by triangle, as cover triangles (keys behind the fill chain and the backdrop slots);
        // their entries take the ordinary way into the pair stream (a cursor atomic per block)
        bool any_folded = false;
        for (uint32_t j = 0; j < n_turn; ++j) any_folded = any_folded || (items[j].flags & (kFiHullTris | kFiSkip)) == kFiHullTris;
        if (any_folded) { // (uniform: LDS values)
            st.sub = ((kFlatWaveCount * blockIdx.x + wave + 977u * turn) * 2654435761u) >> 26;
            for (uint32_t j = 0; j < n_turn; ++j) {
                const FlatItem& fi = items[j];
                if ((fi.flags & (kFiHullTris | kFiSkip)) != kFiHullTris) continue;
                const ItemCtx& ctx = fi.ctx;
                for (uint32_t t0 = 64u * wave; t0 + 2u < fi.n_hull; t0 += kFlatThreads) { // 64 triangles per wavefront and turn
                    const uint32_t t = t0 + lane;
                    PrimRec rec = {};
                    bool drawn = false;
                    if (t + 2u < fi.n_hull) {
                        drawn = setup_plain_triangle(s, r, ctx, ctx.cb[6] + t, rec);
                        if (drawn) *reinterpret_cast<PrimRec*>(r.slots + (size_t)(fi.hull_slot0 + 4u * t) * 32u) = rec;
                    }
                    bin_triangles(st, r, lane, drawn, rec.cov, fi.hull_slot0 + 4u * t, ry_first, r_last);
                }
            }
            stage_flush(st, r, lane);
        }
#ifdef CRH_ABLATE
        dump_items += n_turn, dump_tris += n_tris, dump_edges += n_edges, dump_pool += n_pool, dump_work += n_work, dump_walk += wave_max_u32(tri.nt);
#endif
        next += n_turn;
        ++turn;
        CRH_FLAT_PHASE(8) // folded hulls
    }
    // (a run the host cut for one turn needed more: the costs it was cut by are stale — the host counts these and measures again, api.hip)
    if (r.bin_batches && turn > 1u && tid0 == 0u) atomicAdd(&r.overflow[kExtraTurnsWord], turn - 1u);
#ifdef CRH_ABLATE
    if ((r.debug & 65536u) && tid0 == 0u) {
        const unsigned long long life = __builtin_amdgcn_s_memtime() - born_t;
        atomicMax(reinterpret_cast<unsigned long long*>(r.overflow + 120), life);
        atomicAdd(reinterpret_cast<unsigned long long*>(r.overflow + 122), life);
        atomicAdd(r.overflow + 124, 1u);
    }
    if ((r.debug & 65536u) && r.item_cost && tid0 == 0u) { // CRH_BIN_DUMP: the workgroup's record behind the items' costs
        uint32_t* rec = r.item_cost + 2u * (size_t)(r.n_items + 1u) + 8u * (size_t)blockIdx.x;
        rec[0] = (uint32_t)(__builtin_amdgcn_s_memtime() - born_t), rec[1] = min(turn, 255u) | (min(dump_wave_hits, 4095u) << 8) | (min(dump_batch_hits, 4095u) << 20), rec[2] = dump_items, rec[3] = dump_tris, rec[4] = dump_edges, rec[5] = dump_pool, rec[6] = dump_work, rec[7] = dump_walk; // ([1]: turns | the most hits of a wavefront << 8 | of a batch << 20)
    }
#endif
}

__global__ __launch_bounds__(256) void k_scatter(RasterParams r) {
    if (r.overflow[0] | r.overflow[5]) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, region = r.pair_capacity / kSubStreams;
    const uint32_t sub = i / region, at = i - sub * region;
    if (sub >= kSubStreams || at >= r.pair_cursor[sub]) return;
    r.tile_list[r.tile_offset[r.pair_tile[i]] + r.pair_pos[i]] = r.pair_key[i];
}

// ---------------------------------------------------------------------------------------------- launchers
// slots per draw item (shapes in the plain pass) and their exclusive scan: slot_begin[n_items + 1]
void launch_slot_ranges(const SceneDev& s, const RasterParams& r, uint32_t n_items, uint32_t* item_nslots, uint32_t* slot_begin, uint32_t* scratch, hipStream_t stream) {
    if (n_items == 0) {
        (void)hipMemsetAsync(slot_begin, 0, 4, stream);
        return;
    }
    hipLaunchKernelGGL(k_item_nslots, dim3((n_items + 255u) / 256u), dim3(256), 0, stream, s, r, n_items, item_nslots);
    launch_scan_u32(item_nslots, slot_begin, scratch, n_items, stream);
}
// The plain pass' two per-Shape ranges at the end of a tessellation — contiguous primitive ids (triangle pass) and slot ranges (edge pass) —
// in three launches instead of six (counts of both, then the two scans side by side): small kernels on a lane that starves beside the
// binning and raster kernels pay for every launch.
// The tail of the tessellation lane — per Shape: candidate triangles and slots, then both prefixes — as SINGLE-WAVE workgroups (round 6). The lane of frame i + 1 runs beside
// the raster kernel of frame i, and frame i + 1's binning waits for its end: as 256-thread workgroups k_shape_counts (6 us of work) found no four free wave slots on one compute
// unit until the seven-wave raster grid had drained — 130 us in the rocprofv3 timeline (gpurun_out/r06_trace_steady.txt) —, and the binning started 37 us behind the raster kernel's end.
__global__ __launch_bounds__(64) void k_shape_counts(SceneDev s, uint32_t* shape_ncand, uint32_t* shape_nslots) {
    const uint32_t shape = blockIdx.x * 64u + threadIdx.x;
    if (shape >= s.n_shapes) return;
    uint32_t c[8];
    shape_ncand[shape] = shape_candidates(s, shape, c);
    RasterParams plain = {}; // items == nullptr: item i is Shape i, Stencil + Color
    shape_nslots[shape] = item_slots(s, item_of(plain, shape)).total;
}
// two exclusive prefixes of n items each (blockIdx.y picks the job; a grid of (blocks, 1) runs job a alone), 512 items per single-wave workgroup; out[n] = the total
struct WaveScan {
    const uint32_t* in;
    uint32_t* out;
    uint32_t* block_sum;
};
constexpr uint32_t kWaveScanItems = 8, kWaveScanBlock = 64 * kWaveScanItems;
__global__ __launch_bounds__(64) void k_wave_scan_local2(WaveScan a, WaveScan b, uint32_t n) {
    const WaveScan j = blockIdx.y ? b : a;
    const uint32_t lane = threadIdx.x, i0 = blockIdx.x * kWaveScanBlock + lane * kWaveScanItems;
    uint32_t v[kWaveScanItems], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWaveScanItems; ++k) v[k] = i0 + k < n ? j.in[i0 + k] : 0u, mine += v[k];
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    uint32_t run = incl - mine;
#pragma unroll
    for (uint32_t k = 0; k < kWaveScanItems; ++k) {
        if (i0 + k < n) j.out[i0 + k] = run;
        run += v[k];
    }
    if (lane == 63u) j.block_sum[blockIdx.x] = incl;
}
__global__ __launch_bounds__(64) void k_wave_scan_add2(WaveScan a, WaveScan b, uint32_t n, uint32_t blocks) {
    const WaveScan j = blockIdx.y ? b : a;
    const uint32_t lane = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t k = lane; k < blockIdx.x; k += 64u) sum += j.block_sum[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    const uint32_t i0 = blockIdx.x * kWaveScanBlock + lane * kWaveScanItems;
#pragma unroll
    for (uint32_t k = 0; k < kWaveScanItems; ++k)
        if (i0 + k < n) j.out[i0 + k] += sum;
    if (blockIdx.x + 1u == blocks && lane == 0u) j.out[n] = sum + j.block_sum[blockIdx.x];
}
// (scratch0 / scratch1: (n_shapes + 511) / 512 block sums each)
void launch_plain_ranges(const SceneDev& s, uint32_t* shape_ncand, uint32_t* shape_prim_begin, uint32_t* shape_nslots, uint32_t* shape_slot_begin, uint32_t* scratch0, uint32_t* scratch1, hipStream_t stream) {
    if (s.n_shapes == 0) {
        (void)hipMemsetAsync(shape_prim_begin, 0, 4, stream);
        (void)hipMemsetAsync(shape_slot_begin, 0, 4, stream);
        return;
    }
    hipLaunchKernelGGL(k_shape_counts, dim3((s.n_shapes + 63u) / 64u), dim3(64), 0, stream, s, shape_ncand, shape_nslots);
    const uint32_t blocks = (s.n_shapes + kWaveScanBlock - 1u) / kWaveScanBlock;
    const WaveScan a = {shape_ncand, shape_prim_begin, scratch0}, b = {shape_nslots, shape_slot_begin, scratch1};
    hipLaunchKernelGGL(k_wave_scan_local2, dim3(blocks, 2), dim3(64), 0, stream, a, b, s.n_shapes);
    hipLaunchKernelGGL(k_wave_scan_add2, dim3(blocks, 2), dim3(64), 0, stream, a, b, s.n_shapes, blocks);
}
// The items of a pass cut into runs of consecutive items that fill ONE batch of k_bin_flat each (cost: what a verified pass wrote to
// RasterParams::item_cost). A workgroup's life is a chain of barrier-separated phases per batch, whatever the batch holds: with equal
// NUMBERS of items per workgroup the ones with large Shapes took two to four batches (10 000 Shapes of 16-256 px: the longest workgroup
// lived 1.84 x the mean, and the kernel lasts as long as that one); with one full batch per workgroup every workgroup lives one chain and
// the hardware's dispatch balances the rest. runs[2 k], runs[2 k + 1] = the first item of run k and the one behind its last.
// The lanes of k_bin_flat's workgroups for a pass of n_items items: 128 (alone the kernel is fastest with 256, in the gap between two raster kernels
// with 128: §4.3 of DESIGN.md), 64 from 65 536 items on (100 000 paths @ 8192^2: pipelined step 2.05 -> 1.94 ms; 50 000 glyphs and the metric's
// 10 000 paths are slower that way). CRH_BIN_FLAT_THREADS pins it (64 / 128; read per pass).
uint32_t flat_threads_for(uint32_t n_items) {
    if (const char* e = getenv("CRH_BIN_FLAT_THREADS")) return atoi(e) == 64 ? 64u : kFlatThreads;
    return (n_items >= 65536u && kFlatThreads != 64u) ? 64u : kFlatThreads;
}
bool bin_itemwise(const RasterParams& r) { // (read per launch: tests and A/B runs switch it inside one process)
    const FlatShape shape = flat_shape(flat_threads_for(r.n_items));
    return getenv("CRH_BIN_ITEMWISE") != nullptr ||
           (getenv("CRH_BIN_FLAT") == nullptr && r.n_items != 0u && (r.hint_tris / r.n_items > shape.tris / 2u || r.hint_edges / r.n_items > shape.edges / 2u));
}
void flat_batches(const uint32_t* cost, uint32_t n_items, std::vector<uint32_t>& runs) {
    const FlatShape shape = flat_shape(flat_threads_for(n_items));
    const uint32_t kFlatBatch = shape.batch, kFlatTris = shape.tris, kFlatEdges = shape.edges, kFlatPool = shape.pool; // (of the kernel that will take these runs)
    struct Run {
        uint32_t first, last;
        float ticks;
    };
    std::vector<Run> all;
    const float cap = getenv("CRH_BIN_BATCH_TICKS") ? (float)atof(getenv("CRH_BIN_BATCH_TICKS")) : 0.0f; // A/B runs: close a run at this predicted life as well
    const uint32_t most = getenv("CRH_BIN_BATCH_ITEMS") ? (uint32_t)std::max(1, atoi(getenv("CRH_BIN_BATCH_ITEMS"))) : kFlatBatch; // ... or at this many items
    uint32_t n = 0, tris = 0, edges = 0, cells = 0, widest = 0, folded = 0, first = 0;
    bool closed = false;
    // a workgroup's life in shader clocks, fitted to the lifetimes tools/bin_phases.py dumps (10 000 Shapes / 50 000 glyphs): the chain of
    // phases, then what grows with the batch — the walks over (edge, tile row) pairs, the pool's cells, the longest triangle's tile box
    // (it goes with the widest rectangle), hull strips that fold (item by item)
    auto ticks = [&]() { return 76000.0f + 2000.0f * (float)n + 40.0f * (float)tris + 250.0f * (float)edges + 60.0f * (float)cells + 45.0f * (float)widest + 8000.0f * (float)folded; };
    for (uint32_t i = 0; i < n_items; ++i) {
        const uint32_t c = cost[2u * i], w = cost[2u * i + 1u];
        const bool alone = c == 0xFFFFFFFFu; // wider than the pool: k_bin_flat hands it on when it is the first of a batch
        const uint32_t t = (w >> 31) ? 0u : (w & 0x1FFu), e = (w >> 31) ? 0u : ((w >> 9) & 0x3FFu);
        if (n != 0u && (alone || closed || n >= std::min(most, kFlatBatch) || tris + t > kFlatTris || edges + e > kFlatEdges || cells + c > kFlatPool || (cap > 0.0f && ticks() > cap))) {
            all.push_back(Run{first, i, ticks()});
            n = tris = edges = cells = widest = folded = 0u, first = i, closed = false;
        }
        n += 1u, tris += t, edges += e, cells += alone ? 0u : c, widest = std::max(widest, alone ? 0u : c), folded += (w >> 29) & 1u;
        if (alone) closed = true; // (the next item opens a run)
    }
    if (n_items) all.push_back(Run{first, n_items, ticks()});
    // the long runs first: the hardware starts workgroups in grid order, and a long one that starts late ends after everything else
    const bool in_order = getenv("CRH_BIN_BATCH_ORDER") != nullptr; // A/B runs: the runs in item order
    if (!in_order) std::stable_sort(all.begin(), all.end(), [](const Run& a, const Run& b) { return a.ticks > b.ticks; });
    runs.clear();
    for (const Run& run : all) runs.push_back(run.first), runs.push_back(run.last);
}
void flat_batch_limits(uint32_t n_items, uint32_t limits[4]) {
    const FlatShape shape = flat_shape(flat_threads_for(n_items));
    limits[0] = shape.batch, limits[1] = shape.tris, limits[2] = shape.edges, limits[3] = shape.pool;
}
// The clear in front of a pass' binning kernels (tile counts, overflow words, cursors: 256 KB for 4096^2) as SINGLE-WAVE workgroups, for the reason k_tile_caps
// has them (below): the runtime's fill kernel behind hipMemsetAsync has 256-thread workgroups — four wavefronts that must find room on ONE compute unit at
// the same moment — and beside k_raster_fill's seven waves per SIMD it waited 121 us for them, k_bin_flat's dispatch behind it (profiles/r06_experiments.txt
// item 7). One wavefront takes the first slot that frees. Eight dwords per lane, each store of a wavefront one contiguous 256 bytes.
// CRH_NO_CLEAR_KERNEL=1 (A/B runs; read per launch): hipMemsetAsync, as before.
constexpr uint32_t kClearWordsPerLane = 8u;
__global__ __launch_bounds__(64) void k_clear_words(uint32_t* words, uint32_t n) {
    const uint32_t first = blockIdx.x * (64u * kClearWordsPerLane) + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < kClearWordsPerLane; ++k) {
        const uint32_t i = first + k * 64u;
        if (i < n) words[i] = 0u;
    }
}
void launch_clear_words(uint32_t* words, size_t n_words, hipStream_t stream) {
    if (n_words == 0) return;
    if (getenv("CRH_NO_CLEAR_KERNEL") != nullptr || n_words > 0x7FFFFFFFu) {
        (void)hipMemsetAsync(words, 0, n_words * sizeof(uint32_t), stream);
        return;
    }
    const uint32_t per_group = 64u * kClearWordsPerLane;
    hipLaunchKernelGGL(k_clear_words, dim3((uint32_t)((n_words + per_group - 1u) / per_group)), dim3(64), 0, stream, words, (uint32_t)n_words);
}
// The edge pass draws msaa 1 and 4 only (edge_pass_samples): for any other count its launchers launch nothing and return 0 (api.hip
// render_impl refuses such a pass before it gets here; choose_pass sends msaa 2 and 8 to the triangle pass).
uint32_t launch_bin_edges(const SceneDev& s, const RasterParams& r, uint32_t samples, hipStream_t stream, MarkFn mark, void* ctx, hipEvent_t after_bin) {
    if (!edge_pass_samples(samples)) return 0u;
    // tile_count and, right behind it, the overflow words (overflow[8 ...] are the cursors of the pair sub-streams): one clear (tile_cursor, in front, is the triangle pass')
    launch_clear_words(r.tile_count, (size_t)r.n_tiles + 8u + kSubStreams + 8u, stream); // (... and kExtraTurnsWord behind them)
    // Items per workgroup. One is best while the grid is small (S10k: 0.169 ms; two: 0.189, four: 0.21 — an item is a chain of dependent
    // memory operations, and a wavefront that takes a second item doubles it); tens of thousands of small items are bound by workgroup
    // turnover instead (50 000 glyphs: one 0.45, two 0.31, four 0.31, eight 0.33 ms). So: about 12 000 workgroups.
    const uint32_t pinned = getenv("CRH_BIN_ITEMS") ? max(1, atoi(getenv("CRH_BIN_ITEMS"))) : 0u; // (read per launch: tests and A/B runs switch it inside one process)
    // k_bin_edges for every item: CRH_BIN_ITEMWISE (A/B runs, tests), or a pass whose AVERAGE item is beyond what a batch of k_bin_flat holds
    // (the dashed strokes of config 5: a thousand line triangles per Shape) — every item would be queued anyway
    const bool itemwise = bin_itemwise(r);
    auto by_samples = [&](auto launch) { samples == 4 ? launch(std::integral_constant<int, 4>{}) : launch(std::integral_constant<int, 1>{}); }; // a launch ladder, written once for both sample counts
    uint32_t route = r.n_items == 0u ? 0u : (itemwise ? kBinItemwise : (r.bin_batches ? kBinFlatBatches : kBinFlatItems)); // (0: no item, nothing launched)
    if (r.n_items && itemwise) {
        const uint32_t items_per_group = pinned ? pinned : min(8u, max(1u, (r.n_items + 12287u) / 12288u));
        route |= min(items_per_group, 255u) << 16;
        const uint32_t bin_grid = (r.n_items + items_per_group - 1u) / items_per_group;
        by_samples([&](auto S) { hipLaunchKernelGGL((k_bin_edges<S(), false>), dim3(bin_grid), dim3(128), 0, stream, s, r); });
    } else if (r.n_items) {
        // k_bin_flat: a batch of items per 256-thread workgroup. A workgroup lives about as long whether it holds two items or twenty (the
        // same chain of phases), so the grid is sized to ONE round of resident workgroups — three per CU — as long as that leaves a batch
        // within the kernel's 32 items; what a batch cannot hold is queued and binned item by item behind it.
        const FlatShape shape = flat_shape(flat_threads_for(r.n_items));
        const uint32_t resident = (getenv("CRH_BIN_CUS") ? (uint32_t)max(1, atoi(getenv("CRH_BIN_CUS"))) : 256u) * (4u * CRH_FLAT_WAVES) / (shape.threads / 64u); // workgroups the CUs of the binning lane hold at once (four SIMDs of CRH_FLAT_WAVES wavefronts each)
        // ... and within what the lanes of a batch hold (threads triangles, three times as many edges): an item that does not fit is left to the
        // workgroup's next turn, which doubles the workgroup's life — the averages of the scene keep a batch nine tenths full
        const uint32_t by_tris = r.hint_tris ? (uint32_t)((uint64_t)shape.tris * 9u / 10u * r.n_items / r.hint_tris) : shape.batch;
        const uint32_t by_edges = r.hint_edges ? (uint32_t)((uint64_t)shape.edges * 9u / 10u * r.n_items / r.hint_edges) : shape.batch;
        const uint32_t fitting = max(1u, min(shape.batch, min(by_tris, by_edges)));
        const uint32_t items_per_group = pinned ? min(pinned, shape.batch) : min(fitting, max(1u, (r.n_items + resident - 1u) / resident));
        const uint32_t flat_grid = r.bin_batches ? r.n_bin_batches : (r.n_items + items_per_group - 1u) / items_per_group, queue_grid = min(r.n_items, 4096u);
        if (!r.bin_batches) route |= min(items_per_group, 255u) << 16;
        // Pass 3 as a replay of pass 1's hits, where the instantiation has the LDS for the records: the default workgroup of 128 threads (the 64-thread
        // kernel is at its LDS limit for four waves per SIMD without them). CRH_BIN_REPLAY=0: the walk again, as before; CRH_BIN_REPLAY_CAP=<n> (tests):
        // a wavefront keeps at most n records, 0 makes every batch walk again. Both read per launch.
        const char* const replay_env = getenv("CRH_BIN_REPLAY");
        const bool replay = flat_replays(shape.threads) && !(replay_env && atoi(replay_env) == 0);
        const uint32_t replay_cap = getenv("CRH_BIN_REPLAY_CAP") ? (uint32_t)max(0, atoi(getenv("CRH_BIN_REPLAY_CAP"))) : 0xFFFFFFFFu;
        if (replay) route |= kBinReplayed;
        by_samples([&](auto S) {
            if (shape.threads == 64u) hipLaunchKernelGGL((k_bin_flat<S(), 64u, false>), dim3(flat_grid), dim3(64), 0, stream, s, r, items_per_group, replay_cap);
            else if (replay) hipLaunchKernelGGL((k_bin_flat<S(), kFlatThreads, kFlatThreads == 128u>), dim3(flat_grid), dim3(kFlatThreads), 0, stream, s, r, items_per_group, replay_cap);
            else hipLaunchKernelGGL((k_bin_flat<S(), kFlatThreads, false>), dim3(flat_grid), dim3(kFlatThreads), 0, stream, s, r, items_per_group, replay_cap);
            if (!r.skip_queue) hipLaunchKernelGGL((k_bin_edges<S(), true>), dim3(queue_grid), dim3(128), 0, stream, s, r);
        });
    }
    if (after_bin) (void)hipEventRecord(after_bin, stream);
    if (mark) mark(ctx, "raster_bin", 0);
    if (!r.direct) launch_scan_tiles(r, stream);
    if (mark) mark(ctx, "raster_tile_scan", 0);
    return route;
}
void launch_scatter(const RasterParams& r, hipStream_t stream, MarkFn mark, void* ctx) {
    if (r.pair_capacity && !r.direct) hipLaunchKernelGGL(k_scatter, dim3((r.pair_capacity + 255u) / 256u), dim3(256), 0, stream, r);
    if (mark) mark(ctx, "raster_scatter", 0);
}
// the places of the next frames' lists: caps[t] = count[t] + count[t] / 2 + 64, summed into tile_base[0 .. n_tiles] (tile_base[n_tiles] = all of them)
// (+ 64: a Shape whose boundary moves into an empty tile brings a dozen or two entries at once — with + 16, rounds 3 and 4, a zoom of 1 % per
// frame outgrew some list every few frames)
constexpr uint32_t kListSlack = 64u;
// ... of the LONGEST list within `radius` tiles (round 5): a camera that moves shifts the content by whole tiles between two passes into the same target —
// a zoom of 1 % per frame about the centre of 4096^2 moves the border by 40 pixels from one pass into a target to the next —, so a tile's next
// list resembles a neighbour's, not its own. 49 counts per tile out of L2, beside the raster kernel.
// SINGLE-WAVE workgroups, all three kernels of the chain (round 6): they run beside the raster kernel of the pass whose counts they read, and behind them on the same stream
// wait the next pass' instance copies and its binning. With k_raster_fill at seven waves per SIMD (504 of a SIMD's 512 registers) a 256-thread workgroup — four wavefronts that
// must find room on ONE compute unit at the same moment — got no slot until that grid had drained: k_tile_caps lasted 138 us, exactly as long as the raster kernel beside it
// (rocprofv3 timeline, gpurun_out/r06_trace_moved.txt), and a scene that moves paid 0.32 - 0.34 ms per step where round 5's five-wave raster kernel had left it 0.30.
// One wavefront takes the first slot that frees.
__global__ __launch_bounds__(64) void k_tile_caps(const uint32_t* count, uint32_t* caps, uint32_t n, uint32_t tiles_x, uint32_t radius) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n) return;
    uint32_t longest = count[t];
    if (radius) {
        const uint32_t tiles_y = n / tiles_x, ty = t / tiles_x, tx = t - ty * tiles_x;
        const uint32_t x0 = tx > radius ? tx - radius : 0u, x1 = min(tiles_x - 1u, tx + radius), y0 = ty > radius ? ty - radius : 0u, y1 = min(tiles_y - 1u, ty + radius);
        for (uint32_t y = y0; y <= y1; ++y)
            for (uint32_t x = x0; x <= x1; ++x) longest = max(longest, count[y * tiles_x + x]);
    }
    caps[t] = longest + (longest >> 1) + kListSlack;
}
// exclusive prefix of caps -> tile_base[0 .. n_tiles], tile_base[n_tiles] = the total: the single-wave scan of launch_plain_ranges with one job (scratch: (n_tiles + 511) / 512 block sums)
void launch_tile_bases(const uint32_t* tile_count, uint32_t* caps, uint32_t* tile_base, uint32_t* scratch, uint32_t n_tiles, uint32_t tiles_x, uint32_t radius, hipStream_t stream) {
    const uint32_t blocks = (n_tiles + kWaveScanBlock - 1u) / kWaveScanBlock;
    const WaveScan job = {caps, tile_base, scratch};
    hipLaunchKernelGGL(k_tile_caps, dim3((n_tiles + 63u) / 64u), dim3(64), 0, stream, tile_count, caps, n_tiles, tiles_x, radius);
    hipLaunchKernelGGL(k_wave_scan_local2, dim3(blocks, 1), dim3(64), 0, stream, job, job, n_tiles);
    hipLaunchKernelGGL(k_wave_scan_add2, dim3(blocks, 1), dim3(64), 0, stream, job, job, n_tiles, blocks);
}

} // namespace crh
