// csrc/edge_slots.hpp — what the two halves of the edge pass share: the formulation both implement and the 32-byte slot records through which
// they meet. bin_edges.hip writes the slots and bins their keys per tile; raster_edges.hip reads them tile by tile. The edge pass is the plain
// Stencil + Color pass (Shape::render renderer.rs:267-355 with the stencil states renderer.rs:565-582, 736-754 and the fragment stages
// shaders.wgsl:233-309) as boundary edges + backdrop.
//
// The reference draws the interior of a filled path as a triangle strip (triangle_fan_to_strip, vertex.rs:28-35; renderer.rs:304-318) and
// covers the Shape with the strip of its convex hull (renderer.rs:340-354). Both strips are long thin triangles across the whole Shape —
// five of six (tile, triangle) pairs of the benchmark scene. Their sum is the winding number of the strip's BOUNDARY chain (interior strip
// edges are shared by two triangles that see exactly negated edge functions under the top-left rule, so they cancel sample by sample), and
// that is what the edge pass evaluates, with the same canonical-orientation edge function  E = fma(ry, bx, fma(rx, nay, c))  per boundary edge:
//
//   g_e(p) = E_e(p) > 0 || (E_e(p) == 0 && top-left of the canonical direction)          (what a strip triangle on that side would accept)
//   w(p)   = sum_e sigma_e * Y_e(p.y) * (g_e(p) - down_e)                                 ray to -x; Y = half-open y range, sigma = chain direction
//
// per 16x16 tile T with q_k = (left tile boundary, y of sample row k):
//   w(p)   = BD(T) + sum_{e touching T} sigma_e * [ xr_e * (g_e(q_k) - g_e(q_0)) + Y_e(k) * (g_e(p) - g_e(q_k)) ]
//   BD(T)  = w(q_0), the backdrop, summed over ALL edges of the chain by the binning kernel (one lane per edge, ballots);
//   the bracket is the crossing count of the path q_0 -> q_k -> p with e, non-zero only for edges whose g is not constant over the tile.
// Every term is an evaluation of the same f32 expression the triangle path uses, at sample positions or at q_k, so the result equals the
// strip's sample for sample (tools/proto_edges.cpp checks this formulation against oracle/raster.hpp on the CPU, bit for bit; the GPU
// parity tests check the kernels). Curve and stroke triangles stay triangles.
// Keys are slot numbers of a 32-byte primitive heap (a triangle owns four slots = its 128-byte record); they ascend in draw order.
#pragma once
#include "raster_common.hpp"

namespace crh {

constexpr uint32_t EK_EDGE = 0, EK_SYNTH = 7, EK_COVER_TRI = 8; // kinds 1..6 = KIND_IQ .. KIND_JOINT as in raster_common.hpp (flags bits 4-7)
// Two refinements of a COVER entry's code, decided by the bin kernel per (item, tile):
//   + kCoverHull    the whole tile lies inside the item's hull (no hull edge matters there, hull backdrop non-zero): the cover resets the
//                   winding of EVERY sample of the tile;
//   + kCoverOpaque  also: the item is opaque and the whole tile lies inside its fill (no fill edge matters, backdrop winding non-zero under
//                   the winding rule): unless a sample inherits a winding that cancels the backdrop, the cover REPLACES the tile.
// k_raster_edges uses them to start a tile's list late (see there): painter's-order occlusion, verified per tile, exact.
constexpr uint32_t kCoverHull = 9u, kCoverOpaque = 18u;
constexpr uint32_t kEdgeTl = 1u, kEdgeSigmaPos = 2u, kEdgeHull = 4u;
// Synthetic slots of an item (flags bits 8-11 = code): 0 BD+1, 1 BD-1 (fill winding of the whole tile), 2 HBD+1, 3 HBD-1 (hull winding of the
// whole tile); 4 + (bd + 1) + 3 * (hbd + 1): COVER with one unit of both backdrops folded in (bd, hbd in -1..1).
// Slot layout of an item, in key (= draw) order, every region a multiple of 4 slots:
//   triangles (stroke lines, joints, the four curve lists; 4 slots each) | fill chain edges | BD / HBD slots (4) |
//   hull region: the hull chain's edges (1 slot each) or — a hull strip whose triangles do not all face the same way — its triangles as
//   cover triangles (4 slots each; the region is sized for those) | the 9 COVER slots (12)
struct EdgeRec {
    uint32_t flags, pad0;
    float lo_x, lo_y, hi_x, hi_y, bx, nay;
};
struct SynthRec {
    uint32_t flags, first_slot; // first_slot: the item's first slot (its triangles and fill edges lie in [first_slot, synth_a))
    float r, g, b, a;
    uint32_t synth_a, pad;      // the item's first backdrop slot
};
static_assert(sizeof(EdgeRec) == 32 && sizeof(SynthRec) == 32, "slots");

// The layout above as code (today only the binning side calls it; it is kept beside the layout it states).
struct ItemSlots {
    uint32_t n_tri, n_fe, n_hull; // triangles, fill chain edges (= polygon vertices), hull vertices (0: no cover)
    uint32_t fe0, synth_a, hull0, synth_b, total; // region offsets from the item's first slot
    uint32_t cb[8];
};
CRH_D ItemSlots item_slots(const SceneDev& s, const DrawItem& it) {
    ItemSlots k;
    shape_candidates(s, it.shape, k.cb);
    const uint32_t* b0 = s.shape_base + it.shape * kShapeRow;
    const bool stencil = (it.ops & 1u) != 0u, cover = (it.ops >> 4) != 0u;
    const uint32_t hn = s.hull_count[it.shape];
    k.n_tri = stencil ? k.cb[1] + (k.cb[6] - k.cb[2]) : 0u; // stroke line + joint triangles, then the four curve lists
    k.n_fe = stencil ? b0[NCH + CH_SOLID_V] - b0[CH_SOLID_V] : 0u; // one boundary edge per polygon vertex
    k.n_hull = (cover && hn >= 3u) ? hn : 0u;
    k.fe0 = 4u * k.n_tri;
    k.synth_a = k.fe0 + ((k.n_fe + 3u) & ~3u);
    k.hull0 = k.synth_a + 4u;
    k.synth_b = k.hull0 + (k.n_hull ? 4u * (k.n_hull - 2u) : 0u);
    k.total = k.synth_b + 28u; // 9 COVER codes, the same 9 as "the whole tile inside the hull" (kCoverHull) and as "opaque over the whole tile" (kCoverOpaque)
    return k;
}

} // namespace crh
