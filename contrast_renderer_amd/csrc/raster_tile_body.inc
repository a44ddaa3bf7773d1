// csrc/raster_tile_body.inc — the body of k_raster_tile<S, ROWS, OPS, STROKES>, k_raster_blend<S, STROKES>, k_raster_paint<S, STROKES> and
// k_raster_image<S, STROKES> (raster.hip), included into the four kernels with S, ROWS, OPS, STROKES, BLEND, the blend form `bf`, PAINT, the paint
// tables `pa`, IMAGES and the image paints `ia` in scope. Included rather than shared as a __device__ function:
// the instruction stream of k_raster_tile stays what it was (an inlined body changed its register allocation and scheduling). The steps in
// front of the walk that every tile kernel takes — the tile of the workgroup's place, the sort of a list in place — are the helpers of
// raster_tile_list.hpp: tools/resource_usage.py shows the same registers, scratch, occupancy and LDS for every instantiation with them.
    extern __shared__ uint32_t sort_buffer[]; // [waves][r.sort_capacity], wave-private; only used by tiles with more than 64 primitives
    __shared__ float4 entry_buffer[4 / ROWS][64 * 3];        // wave-private: the set-up values of the current chunk's 64 entries
    uint32_t tx, ty;
    if (!tile_of_place(r, blockIdx.x, tx, ty)) return;
    const uint32_t tile = ty * r.tiles_x + tx;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* __restrict__ keys = sort_buffer + wave * r.sort_capacity;
    const uint32_t px = lane & 15u, rq = lane >> 4;
    const uint32_t first_row = 4u * ROWS * wave; // local row b of this lane is pixel row first_row + 4b + rq (ROWS == 4: one wavefront, wave == 0)
    static_assert(ROWS == tile_rows(S), "the lane layout of msaa S");
    const uint32_t gx = tx * kTile + px;
    const float tx0 = (float)(tx * kTile), ty0 = (float)(ty * kTile);
    const int tpx = (int)(tx * kTile), tpy = (int)(ty * kTile);

    float sx[S], sy0[S]; // sample positions of the lane's first row (the pattern of msaa S, raster_common.hpp); local row b adds 4b (exact in f32)
    if (S == 1) { // (written out: the one-trip loop lets the msaa 1 kernels schedule these two adds the other way round)
        sx[0] = (float)px + sample_dx(S, 0);
        sy0[0] = (float)(first_row + rq) + sample_dy(S, 0);
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            sx[k] = (float)px + sample_dx(S, k);
            sy0[k] = (float)(first_row + rq) + sample_dy(S, k);
        }
    }
    const uint32_t row_shift = first_row + rq; // the lane's row b is bit row_shift + 4b of a 16-bit row mask
    int winding[ROWS][S];
    int clipc[OPS ? ROWS : 1][OPS ? S : 1];                        // clip nesting counter (the upper stencil bits, renderer.rs:565)
    float saved[OPS ? ROWS : 1][OPS ? S : 1][kMaxAlphaLayers];     // alpha-context layers (renderer.rs:892-927)
#pragma unroll
    for (int b = 0; b < (OPS ? ROWS : 1); ++b)
#pragma unroll
        for (int k = 0; k < (OPS ? S : 1); ++k) {
            clipc[OPS ? b : 0][OPS ? k : 0] = 0;
#pragma unroll
            for (int l = 0; l < kMaxAlphaLayers; ++l) saved[b][k][l] = 0.0f;
        }
    float col[ROWS][S][4];
#pragma unroll
    for (int b = 0; b < ROWS; ++b)
#pragma unroll
        for (int k = 0; k < S; ++k) {
            winding[b][k] = 0;
            col[b][k][0] = col[b][k][1] = col[b][k][2] = col[b][k][3] = 0.0f;
        }
    // the depth attachment (OPS only): tested / written by the colour cover alone (renderer.rs:743-745)
    float depth[OPS ? ROWS : 1][OPS ? S : 1];
    const bool has_depth = OPS && r.depth != nullptr;
    if (OPS) {
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
#pragma unroll
            for (int k = 0; k < S; ++k)
                depth[OPS ? b : 0][OPS ? k : 0] = (has_depth && gx < r.width && gy < r.height) ? r.depth[((size_t)gy * r.width + gx) * S + k] : 0.0f;
        }
    }
    if (r.load_existing) {
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
            if (gx < r.width && gy < r.height) {
                const float4 d = load_px<XFMT>(r, gx, gy);
#pragma unroll
                for (int k = 0; k < S; ++k) col[b][k][0] = d.x, col[b][k][1] = d.y, col[b][k][2] = d.z, col[b][k][3] = d.w;
            }
        }
    }

    const uint32_t list_begin = r.tile_offset[tile];
    uint32_t n = r.overflow[0] ? 0u : r.tile_offset[tile + 1] - list_begin;
    constexpr uint32_t kLdsSortMax = kSortBytesMax / (4u * (4u / ROWS));
    if (n > r.sort_capacity && n <= kLdsSortMax) n = 0; // the host sizes the sort buffer from overflow[3] (the longest list) and runs the frame again
    // Pass state kept with the frame (renderer.rs:148-158, 257-266: the stencil attachment and the alpha layers outlive a Shape::render call):
    // the tile starts from what the earlier passes left — stencil byte = clip nesting counter << winding bits | winding counter
    // (renderer.rs:565-566, 936), the saved alphas, the colour of every SAMPLE — and leaves its own behind (below, in front of the resolve).
    const bool keeps_state = OPS && r.state_stencil != nullptr;
    if (keeps_state && r.state_load) {
        if (n == 0u && r.load_existing) return; // nothing of this pass touches the tile: planes and pixels stay as they are (a cleared frame's tiles are all written)
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
            if (gx < r.width && gy < r.height) {
                const size_t at = ((size_t)gy * r.width + gx) * S;
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const uint32_t st = r.state_stencil[at + k];
                    winding[b][k] = (int)(st & r.winding_mask);
                    clipc[OPS ? b : 0][OPS ? k : 0] = (int)((st >> r.winding_bits) & r.clip_mask_count);
                    const float4 c = reinterpret_cast<const float4*>(r.state_color)[at + k];
                    col[b][k][0] = c.x, col[b][k][1] = c.y, col[b][k][2] = c.z, col[b][k][3] = c.w;
#pragma unroll
                    for (int l = 0; l < kMaxAlphaLayers; ++l)
                        if ((uint32_t)l < r.state_layers) saved[OPS ? b : 0][OPS ? k : 0][l] = r.state_alpha[(size_t)l * r.width * r.height * S + at + k];
                }
            }
        }
    }
    // ---- draw order = ascending prim id: bitonic network in registers (<= 64 entries), in LDS, or — a list longer than LDS holds — in
    //      place in global memory
    uint32_t my_key = 0xFFFFFFFFu;
    const bool sorted_in_place = n > kLdsSortMax;
    uint32_t* const segment = r.tile_list + list_begin;
    if (sorted_in_place) {
        sort_list_in_place(segment, n, threadIdx.x, 64u * (4u / ROWS));
    } else if (n <= 64u) {
        if (lane < n) my_key = r.tile_list[list_begin + lane];
#pragma unroll
        for (uint32_t k = 2; k <= 64u; k <<= 1) {
#pragma unroll
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                const uint32_t other = __shfl_xor(my_key, j, 64);
                const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
                my_key = keep_min ? min(my_key, other) : max(my_key, other);
            }
        }
    } else {
        // sort_list_in_lds (raster_tile_list.hpp) written out: with the helper k_raster_tile<1, 4, false, false, true> takes 78 registers instead of 80
        uint32_t padded = 128;
        while (padded < n) padded <<= 1;
        for (uint32_t i = lane; i < padded; i += 64u) keys[i] = i < n ? r.tile_list[list_begin + i] : 0xFFFFFFFFu;
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

    const PrimRec* recs = r.prim_rec;
    const int wmask = (int)r.winding_mask;
    for (uint32_t q0 = 0; q0 < n; q0 += 64u) {
        if (sorted_in_place)
            my_key = q0 + lane < n ? __hip_atomic_load(segment + q0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xFFFFFFFFu;
        else if (n > 64u)
            my_key = q0 + lane < n ? keys[q0 + lane] : 0xFFFFFFFFu;
        const uint32_t count = min(64u, n - q0);
        // ---- entry setup, vectorised across the chunk: lane j prepares entry j (one gathered 64-byte record per lane)
        uint32_t e_bits = 0, e_flags = 0, e_desc = 0;
        float e_c[3] = {0.0f, 0.0f, 0.0f}, e_bx[3] = {0.0f, 0.0f, 0.0f}, e_nay[3] = {0.0f, 0.0f, 0.0f};
        if (lane < count) {
            const PrimCoverage mine = recs[my_key].cov;
            const int bx0 = max((int)mine.box.x, tpx) - tpx, bx1 = min((int)mine.box.y, tpx + kTile - 1) - tpx;
            const int by0 = max((int)mine.box.z, tpy) - tpy, by1 = min((int)mine.box.w, tpy + kTile - 1) - tpy;
            const uint32_t col_bits = bx1 >= bx0 ? (2u << bx1) - (1u << bx0) : 0u, row_bits = by1 >= by0 ? (2u << by1) - (1u << by0) : 0u;
            e_bits = col_bits | (row_bits << 16); // columns / rows of the tile inside the triangle's clamped pixel box
            e_flags = mine.flags;
            e_desc = mine.desc;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                e_c[i] = mine.bx[i] * (ty0 - mine.lo_y[i]) + mine.nay[i] * (tx0 - mine.lo_x[i]);
                e_bx[i] = mine.bx[i];
                e_nay[i] = mine.nay[i];
            }
        }
        // staged in LDS so that the loop reads entry j with three uniform-address (broadcast) ds_read_b128 — the LDS pipe instead of a
        // dozen v_readlane on the VALU pipe, which is what bounds this kernel
        float4* __restrict__ entries = entry_buffer[wave];
        __builtin_amdgcn_wave_barrier(); // the previous chunk's reads are done
        entries[lane * 3u + 0u] = make_float4(e_c[0], e_c[1], e_c[2], __uint_as_float(e_bits));
        entries[lane * 3u + 1u] = make_float4(e_bx[0], e_bx[1], e_bx[2], __uint_as_float(e_flags));
        entries[lane * 3u + 2u] = make_float4(e_nay[0], e_nay[1], e_nay[2], __uint_as_float(e_desc));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t prim = __builtin_amdgcn_readlane(my_key, j);
            const float4 ea4 = entries[j * 3u + 0u], eb4 = entries[j * 3u + 1u], ec4 = entries[j * 3u + 2u];
            const uint32_t flags = __builtin_amdgcn_readfirstlane(__float_as_uint(eb4.w));
            const uint32_t kind = (flags >> 4) & 7u;
            const int clip_ref = OPS ? (int)((flags >> 16) & 255u) : 0; // the stencil reference of this draw: its clip depth
#ifndef CRH_NO_DEAD_COVER_SKIP
            // A colour cover over a tile in which no sample can pass its stencil test (Less: a non-zero winding, or a deeper clip level)
            // changes nothing: the blend needs a pass and the Zero operation leaves a winding that is already zero modulo the counter.
            // The long thin triangles of a hull strip mostly find the tile already cleared by their predecessors.
            if (kind == KIND_COVER && (!OPS || ((flags >> 7) & 7u) == (uint32_t)CRH_OP_COLOR)) {
                int live = 0;
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < S; ++k) live |= OPS ? (int)((winding[b][k] & wmask) != 0 || clipc[OPS ? b : 0][OPS ? k : 0] > clip_ref) : (winding[b][k] & wmask);
                if (!__any(live != 0)) continue;
            }
#endif
            // the second half of the record (attribute planes / cover colour) comes through a scalar load issued up front
            PrimFragment frag;
            if (kind != KIND_SOLID) frag = load_uniform(&recs[prim].frag);
            // inside[b][k]  <=>  sample k of pixel (px, 4b + rq) is covered:
            //   edge i accepts e  <=>  e > 0 || (e == 0 && top_left_i)  <=>  as_int(e) >= 1 - top_left_i
            //   (edge values are finite and never -0: an exact zero sum rounds to +0 unless both addends are -0, which would need
            //    bx == nay == 0, i.e. a zero-length edge, and those triangles have det == 0 and are never set up)
            // Two (row, sample) combinations are evaluated together with packed f32 FMAs (v_pk_fma_f32: two IEEE fmas
            // per instruction, bit-identical to the scalar ones); the three compares produce lane masks that are combined on the scalar
            // unit; "the pixel is inside the clamped box" is a bit lookup in (column mask, row mask).
            bool inside[ROWS][S];
            {
                const uint32_t bits = __float_as_uint(ea4.w);
                const float c0 = ea4.x, c1 = ea4.y, c2 = ea4.z, bx_0 = eb4.x, bx_1 = eb4.y, bx_2 = eb4.z, nay_0 = ec4.x, nay_1 = ec4.y, nay_2 = ec4.z;
                const uint32_t lane_rows = ((bits >> px) & 1u) ? (bits >> 16) >> row_shift : 0u; // bit 4b: the lane's row b is inside the box
                const int thr0 = 1 - (int)(flags & 1u), thr1 = 1 - (int)((flags >> 1) & 1u), thr2 = 1 - (int)((flags >> 2) & 1u);
                // E = fma(ry, bx, fma(rx, nay, c)): the column term is shared by the rows of the lane (one fma per edge and sample position)
                float ha[S], hb[S], hc[S];
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    ha[k] = fmaf(sx[k], nay_0, c0);
                    hb[k] = fmaf(sx[k], nay_1, c1);
                    hc[k] = fmaf(sx[k], nay_2, c2);
                }
                // the ROWS * S (row, sample) combinations are taken two at a time
#pragma unroll
                for (int c = 0; c < ROWS * S; c += 2) {
                    const int b0 = c / S, k0 = c % S, b1 = (c + 1) / S, k1 = (c + 1) % S;
                    const f32x2 y = {sy0[k0] + (float)(4 * b0), sy0[k1] + (float)(4 * b1)};
                    const f32x2 ea = fma2(y, splat2(bx_0), f32x2{ha[k0], ha[k1]});
                    const f32x2 eb = fma2(y, splat2(bx_1), f32x2{hb[k0], hb[k1]});
                    const f32x2 ec = fma2(y, splat2(bx_2), f32x2{hc[k0], hc[k1]});
                    inside[b0][k0] = (__float_as_int(ea[0]) >= thr0) & (__float_as_int(eb[0]) >= thr1) & (__float_as_int(ec[0]) >= thr2) & ((lane_rows & (1u << (4 * b0))) != 0u);
                    inside[b1][k1] = (__float_as_int(ea[1]) >= thr0) & (__float_as_int(eb[1]) >= thr1) & (__float_as_int(ec[1]) >= thr2) & ((lane_rows & (1u << (4 * b1))) != 0u);
                }
            }
            // projective instances (oracle/raster.hpp raster_projective): per-sample near / far test on z/w, and 1 / (1/w) for the attributes
            float rw[OPS ? ROWS : 1][OPS ? S : 1], zs[OPS ? ROWS : 1][OPS ? S : 1];
            if (OPS) {
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        rw[OPS ? b : 0][OPS ? k : 0] = 1.0f;
                        zs[OPS ? b : 0][OPS ? k : 0] = 0.0f;
                    }
                if (flags & kFlagProjective) { // wave uniform
                    const PrimProj pp = load_uniform(&r.prim_proj[prim]);
                    const float dxa = tx0 - pp.ax, dya = ty0 - pp.ay;
                    const float zc = fmaf(dya, pp.zgy, fmaf(dxa, pp.zgx, pp.z0)), qc = fmaf(dya, pp.qgy, fmaf(dxa, pp.qgx, pp.q0));
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int k = 0; k < S; ++k) {
                            const float y = sy0[k] + (float)(4 * b);
                            const float z = fmaf(y, pp.zgy, fmaf(sx[k], pp.zgx, zc));
                            const float q = fmaf(y, pp.qgy, fmaf(sx[k], pp.qgx, qc));
                            inside[b][k] = inside[b][k] & (z >= 0.0f) & (z <= 1.0f); // unclipped_depth: false (renderer.rs:478)
                            zs[OPS ? b : 0][OPS ? k : 0] = z;
                            rw[OPS ? b : 0][OPS ? k : 0] = 1.0f / q;
                        }
                }
            }
            const int delta = (flags & 8u) ? 1 : -1; // front (ccw on screen) increments, back decrements (renderer.rs:577-582)
            // Every kind only produces the change of the winding counters (dw) and, for the colour cover, which samples blend; the state
            // itself is updated once after the dispatch. (Updating winding / colour inside the multi-way dispatch made every iteration end
            // with ~18 register-pair copies: the SSA join of 20 state registers over all kinds.)
            int dw[ROWS][S];
            bool blend[ROWS][S];
#pragma unroll
            for (int b = 0; b < ROWS; ++b)
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    dw[b][k] = 0;
                    blend[b][k] = false;
                }
            const uint32_t cover_op = OPS ? (flags >> 7) & 7u : (uint32_t)CRH_OP_COLOR;
            const bool color_cover = kind == KIND_COVER && cover_op == CRH_OP_COLOR;
            if (kind == KIND_SOLID) { // stencil_solid
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < S; ++k) dw[b][k] = (inside[b][k] && (!OPS || clipc[OPS ? b : 0][OPS ? k : 0] >= clip_ref)) ? delta : 0; // LessEqual(ref <= stencil)
            } else if (kind == KIND_COVER) {
                if (cover_op == CRH_OP_COLOR) { // stencil Less / Zero of color_cover (renderer.rs:747-752); the blend itself follows the dispatch
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int k = 0; k < S; ++k) {
                            // Less(ref < stencil) on clip | winding: a deeper clip level, or this level with a non-zero winding
                            const bool stencil_pass = OPS ? (clipc[OPS ? b : 0][OPS ? k : 0] > clip_ref || (clipc[OPS ? b : 0][OPS ? k : 0] == clip_ref && (winding[b][k] & wmask) != 0)) : (winding[b][k] & wmask) != 0;
                            if (OPS) {
                                // the depth test follows the stencil test; depth_fail_op = Keep (renderer.rs:442): the winding survives a depth fail
                                const float z = (flags & kFlagProjective) ? zs[OPS ? b : 0][OPS ? k : 0] : frag.gx[0];
                                const float stored = depth[OPS ? b : 0][OPS ? k : 0];
                                const uint32_t relation = (z < stored ? 1u : 0u) | (z == stored ? 2u : 0u) | (z > stored ? 4u : 0u) | 8u;
                                const bool depth_pass = !has_depth || (relation & r.depth_pass_mask) != 0u;
                                const bool depth_fail = inside[b][k] && stencil_pass && !depth_pass;
                                blend[b][k] = inside[b][k] && stencil_pass && depth_pass;
                                dw[b][k] = (inside[b][k] && !depth_fail) ? -winding[b][k] : 0;
                                depth[OPS ? b : 0][OPS ? k : 0] = (blend[b][k] && has_depth && r.depth_write != 0u) ? z : stored;
                            } else {
                                blend[b][k] = inside[b][k] && stencil_pass;
                                dw[b][k] = inside[b][k] ? -winding[b][k] : 0; // pass -> Zero, fail -> Zero
                            }
                        }
                } else if (OPS) {
                    // Clip / UnClip / the alpha-context covers, branch-free per sample (the operation is wave uniform)
                    const uint32_t layer = (flags >> 24) & 15u;
                    const float ca = frag.a0[3]; // the instance colour's alpha
                    const bool is_clip = cover_op == CRH_OP_CLIP, is_unclip = cover_op == CRH_OP_UNCLIP, is_save = cover_op == CRH_OP_SAVE_ALPHA_CONTEXT;
                    const bool is_scale = cover_op == CRH_OP_SCALE_ALPHA_CONTEXT, is_restore = cover_op == CRH_OP_RESTORE_ALPHA_CONTEXT;
                    const float scale_src = 1.0f - ca; // scale_alpha_context_cover: src = (0, 0, 0, 1 - a), shaders.wgsl:311-316
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int k = 0; k < S; ++k) {
                            const int cb_ = OPS ? b : 0, ck_ = OPS ? k : 0;
                            const bool in = inside[b][k];
                            const int clip_now = clipc[cb_][ck_];
                            // Clip: NotEqual on the winding bits -> Replace(ref) (renderer.rs:703-708); UnClip: Less on the clip bits (ref < stencil)
                            // -> Replace(ref) (renderer.rs:722-727); both rewrite clip | winding
                            const bool replace = in && ((is_clip && (winding[b][k] & wmask) != 0) || (is_unclip && clip_ref < clip_now));
                            clipc[cb_][ck_] = replace ? clip_ref : clip_now;
                            dw[b][k] = replace ? -winding[b][k] : 0;
                            // alpha-context covers: LessEqual(ref <= stencil), stencil untouched (renderer.rs:761-766)
                            const bool pass = in && clip_now >= clip_ref;
                            const float alpha = col[b][k][3];
                            float mine = 0.0f;
#pragma unroll
                            for (int l = 0; l < kMaxAlphaLayers; ++l) mine = (uint32_t)l == layer ? saved[cb_][ck_][l] : mine;
                            const float scaled = scale_src + alpha * (1.0f - scale_src);      // alpha' = src.a * One + dst.a * (1 - src.a), renderer.rs:803-828
                            const float restored = alpha - (1.0f - mine) * (1.0f - ca);        // alpha' = dst.a - (1 - saved)(1 - a), renderer.rs:829-861
                            float next = is_scale ? scaled : (is_restore ? restored : alpha);
                            if (rounds_writes<XFMT>(r)) next = attachment<XFMT>(r, 3, next); // an Rgba8Unorm attachment keeps 8 bits of what the blender writes
                            col[b][k][3] = pass ? next : alpha;
#pragma unroll
                            for (int l = 0; l < kMaxAlphaLayers; ++l) // save_alpha_context_cover: the layer receives the frame's alpha, shaders.wgsl:326-331
                                saved[cb_][ck_][l] = (pass && is_save && (uint32_t)l == layer) ? alpha : saved[cb_][ck_][l];
                        }
                }
            } else {
            // attribute planes, tile relative: ac = fma(ty0 - v0y, gy, fma(tx0 - v0x, gx, a0)); a = fma(sy, gy, fma(sx, gx, ac))
            const float dx0 = tx0 - frag.v0x, dy0 = ty0 - frag.v0y;
            float hx[4][S]; // the row-independent inner fma
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float ac = fmaf(dy0, frag.gy[t], fmaf(dx0, frag.gx[t], frag.a0[t]));
#pragma unroll
                for (int k = 0; k < S; ++k) hx[t][k] = fmaf(sx[k], frag.gx[t], ac);
            }
            if (kind <= KIND_RC) { // the four implicit-curve tests (shaders.wgsl:236-266)
#pragma unroll
                for (int b = 0; b < ROWS; ++b) {
                    bool row_touched = false;
#pragma unroll
                    for (int k = 0; k < S; ++k) row_touched = row_touched | inside[b][k];
                    if (!__any(row_touched)) continue; // curve triangles are small: most rows of the tile are not touched
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        const float y = sy0[k] + (float)(4 * b);
                        // (x * 1.0f is exact, so the plain instances of an OPS pass keep their bits)
                        const float w = OPS ? rw[OPS ? b : 0][OPS ? k : 0] : 1.0f;
                        const float a0 = OPS ? fmaf(y, frag.gy[0], hx[0][k]) * w : fmaf(y, frag.gy[0], hx[0][k]);
                        const float a1 = OPS ? fmaf(y, frag.gy[1], hx[1][k]) * w : fmaf(y, frag.gy[1], hx[1][k]);
                        const float a2 = OPS ? fmaf(y, frag.gy[2], hx[2][k]) * w : fmaf(y, frag.gy[2], hx[2][k]);
                        const float a3 = OPS ? fmaf(y, frag.gy[3], hx[3][k]) * w : fmaf(y, frag.gy[3], hx[3][k]);
                        const float lhs = (kind == KIND_IQ || kind == KIND_RQ) ? a0 * a0 : a0 * a0 * a0;
                        const float rhs = kind == KIND_IQ ? a1 : (kind == KIND_RC ? a1 * a2 * a3 : a1 * a2);
                        dw[b][k] = (inside[b][k] && (!OPS || clipc[OPS ? b : 0][OPS ? k : 0] >= clip_ref) && lhs - rhs <= 0.0f) ? delta : 0;
                    }
                }
            } else if (STROKES) { // KIND_LINE / KIND_JOINT: the stroke fragment stages
                int any_inside = 0;
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < S; ++k) any_inside |= (int)inside[b][k];
                if (__any(any_inside)) {
                    const crh_dynamic_stroke_descriptor d = load_uniform(&s.descriptors[__builtin_amdgcn_readfirstlane(__float_as_uint(ec4.w))]); // 48 B, scalar loads
                    const uint32_t caps = d.caps, count_dashed_join = d.count_dashed_join; // wave uniform
                    const uint32_t flat_u = frag.flat_u;
                    const float end_y = frag.end_y;
                    const bool dashed = (count_dashed_join & 4u) != 0u;
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int k = 0; k < S; ++k) {
                            // stroke stencil: Equal(0) -> IncrementWrap, both faces (renderer.rs:571-576)
                            if (inside[b][k] && (winding[b][k] & wmask) == 0 && (!OPS || clipc[OPS ? b : 0][OPS ? k : 0] == clip_ref)) { // Equal(ref) on clip | winding
                                const float y = sy0[k] + (float)(4 * b);
                                const float w = OPS ? rw[OPS ? b : 0][OPS ? k : 0] : 1.0f;
                                const float a0 = OPS ? fmaf(y, frag.gy[0], hx[0][k]) * w : fmaf(y, frag.gy[0], hx[0][k]);
                                const float a1 = OPS ? fmaf(y, frag.gy[1], hx[1][k]) * w : fmaf(y, frag.gy[1], hx[1][k]);
                                const float a2 = OPS ? fmaf(y, frag.gy[2], hx[2][k]) * w : fmaf(y, frag.gy[2], hx[2][k]);
                                bool fill;
                                if (kind == KIND_LINE) { // stencil_stroke_line, shaders.wgsl:268-285
                                    if (dashed)
                                        fill = stroke_dashed(d, a0, a1);
                                    else if ((flat_u & 65536u) != 0u)
                                        fill = cap_test(a0, a1 - end_y, caps >> 4);
                                    else if (a1 < 0.0f)
                                        fill = cap_test(a0, -a1, caps);
                                    else
                                        fill = true;
                                } else { // stencil_stroke_joint, shaders.wgsl:287-300
                                    const float radius = sqrtf(a0 * a0 + a1 * a1);
                                    const uint32_t join = count_dashed_join & 3u;
                                    fill = join == 1u ? (flat_u & 65536u) != 0u : (join == 2u ? radius <= 0.5f : true);
                                    if (fill && dashed) fill = stroke_dashed_joint(d, radius, a0, a1, a2);
                                }
                                dw[b][k] = fill ? 1 : 0;
                            }
                        }
                }
            }
            } // kinds with attribute planes
#pragma unroll
            for (int b = 0; b < ROWS; ++b)
#pragma unroll
                for (int k = 0; k < S; ++k) winding[b][k] += dw[b][k];
            if (PAINT && BLEND && color_cover && frag.flat_u != 0u) {
                // color_cover of a painted item (k_paint_items left item + 1 in flat_u; wave uniform): the source is paint(t) * instance colour per
                // SAMPLE (include/contrast_hip.h crh_scene_set_paints states the model), premultiplied and blended as the block below blends its
                // wave-uniform one. Four samples at a time — msaa 8 takes two turns — so that t and the paint's colour of four samples are live at once.
                const PaintItem pi = load_uniform(&pa.items[frag.flat_u - 1u]);
                const PaintHead ph = load_uniform(&pa.heads[pi.paint]);
#pragma unroll
                for (int g = 0; g < ROWS * S; g += 4) {
                    int any_blend = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) any_blend |= (int)blend[(g + c) / S][(g + c) % S];
                    if (!__any(any_blend)) continue;
                    float t[4], pc[4][4] = {};
                    if (IMAGES && pi.pad != 0u) { // wave uniform: an image paint (k_paint_items_images left image paint + 1 in pad)
                        // (include/contrast_hip.h crh_scene_set_paints_with_images states the model.) The texels of a turn's samples — one each, or four for
                        // LINEAR — are fetched together, every address from wrapped indices, and unpacked behind the last load: the loads of divergent
                        // addresses are in flight at once instead of one round trip per sample.
                        const ImagePaintRec im = load_uniform(&ia.paints[pi.pad - 1u]);
                        if (MIPS && (im.filter & CRH_FILTER_MIPMAP) != 0u && im.levels > 1u) { // wave uniform; the host leaves the flag only on a paint whose image has a chain
                            // (include/contrast_hip.h crh_image_generate_mipmaps states the model; raster.hip mip_samples is the block.) lod once per painted
                            // cover for an affine item — this turn is the only one below msaa 8 — and per sample for a projective one.
                            MipUniform uni = {};
                            if (pi.affine) uni = mip_uniform(pi, im);
                            constexpr int kTogether = CRH_IMAGE_FETCH_TOGETHER(S), kLevels = CRH_MIP_LEVELS_TOGETHER(S);
#pragma unroll
                            for (int c0 = 0; c0 < 4; c0 += kTogether) {
                                float fx[kTogether], fy[kTogether], value[kTogether][4];
#pragma unroll
                                for (int c = c0; c < c0 + kTogether; ++c) {
                                    const int b = (g + c) / S, k = (g + c) % S;
                                    fx[c - c0] = tx0 + sx[k], fy[c - c0] = ty0 + (sy0[k] + (float)(4 * b)); // the sample's place on the frame (exact)
                                }
                                if (pi.affine) mip_samples<kTogether, kLevels, true>(pi, im, uni, fx, fy, value);
                                else mip_samples<kTogether, kLevels, false>(pi, im, uni, fx, fy, value);
#pragma unroll
                                for (int c = c0; c < c0 + kTogether; ++c)
#pragma unroll
                                    for (int ch = 0; ch < 4; ++ch) pc[c][ch] = value[c - c0][ch];
                            }
                        } else {
                        const int iw = (int)im.width, ih = (int)im.height;
                        const bool linear = im.filter == CRH_FILTER_LINEAR;
                        constexpr int kTogether = CRH_IMAGE_FETCH_TOGETHER(S);
#pragma unroll
                        for (int c0 = 0; c0 < 4; c0 += kTogether) {
                            uint32_t tex[kTogether][4];
                            float frac[kTogether][2];
#pragma unroll
                            for (int c = c0; c < c0 + kTogether; ++c) {
                                const int b = (g + c) / S, k = (g + c) % S;
                                const float fx = tx0 + sx[k], fy = ty0 + (sy0[k] + (float)(4 * b)); // the sample's place on the frame (exact)
                                float X = fmaf(fy, pi.h[1], fmaf(fx, pi.h[0], pi.h[2])), Y = fmaf(fy, pi.h[4], fmaf(fx, pi.h[3], pi.h[5]));
                                if (!pi.affine) { // wave uniform
                                    const float W = fmaf(fy, pi.h[7], fmaf(fx, pi.h[6], pi.h[8]));
                                    X = X / W;
                                    Y = Y / W;
                                }
                                const float u = image_coord(fmaf(Y, im.m[1], fmaf(X, im.m[0], im.m[2]))), v = image_coord(fmaf(Y, im.m[4], fmaf(X, im.m[3], im.m[5])));
                                if (linear) {
                                    const float au = u - 0.5f, av = v - 0.5f;
                                    const float fu = floorf(au), fv = floorf(av);
                                    frac[c - c0][0] = au - fu, frac[c - c0][1] = av - fv;
                                    const int i0 = image_wrap((int)fu, iw, im.spread_x), i1 = image_wrap((int)fu + 1, iw, im.spread_x);
                                    const int j0 = image_wrap((int)fv, ih, im.spread_y), j1 = image_wrap((int)fv + 1, ih, im.spread_y);
                                    tex[c - c0][0] = im.texels[(uint32_t)j0 * im.width + (uint32_t)i0];
                                    tex[c - c0][1] = im.texels[(uint32_t)j0 * im.width + (uint32_t)i1];
                                    tex[c - c0][2] = im.texels[(uint32_t)j1 * im.width + (uint32_t)i0];
                                    tex[c - c0][3] = im.texels[(uint32_t)j1 * im.width + (uint32_t)i1];
                                } else {
                                    const int i0 = image_wrap((int)floorf(u), iw, im.spread_x), j0 = image_wrap((int)floorf(v), ih, im.spread_y);
                                    tex[c - c0][0] = im.texels[(uint32_t)j0 * im.width + (uint32_t)i0];
                                }
                            }
#pragma unroll
                            for (int c = c0; c < c0 + kTogether; ++c) {
#pragma unroll
                                for (int ch = 0; ch < 4; ++ch) {
                                    const float t00 = texel_channel(tex[c - c0][0], ch);
                                    if (linear) {
                                        const float t01 = texel_channel(tex[c - c0][1], ch), t10 = texel_channel(tex[c - c0][2], ch), t11 = texel_channel(tex[c - c0][3], ch);
                                        const float top = t00 + frac[c - c0][0] * (t01 - t00), bottom = t10 + frac[c - c0][0] * (t11 - t10);
                                        pc[c][ch] = top + frac[c - c0][1] * (bottom - top);
                                    } else {
                                        pc[c][ch] = t00;
                                    }
                                }
                            }
                        }
                        } // one level
                    } else {
                    // The kind is chosen once per turn of four samples, not per sample: the loop of the linear and radial kinds is the one the kernel had
                    // before the conic kind, so their code does not pay for it (chosen inside the loop, it became a chain of scalar branches per sample).
                    if (ph.kind == CRH_PAINT_CONIC) { // wave uniform. d = (s, k), dd = +-1 the direction (raster_params.hpp PaintHead)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int b = (g + c) / S, k = (g + c) % S;
                        const float fx = tx0 + sx[k], fy = ty0 + (sy0[k] + (float)(4 * b)); // the sample's place on the frame (exact)
                        float X = fmaf(fy, pi.h[1], fmaf(fx, pi.h[0], pi.h[2])), Y = fmaf(fy, pi.h[4], fmaf(fx, pi.h[3], pi.h[5]));
                        if (!pi.affine) { // wave uniform
                            const float W = fmaf(fy, pi.h[7], fmaf(fx, pi.h[6], pi.h[8]));
                            X = X / W;
                            Y = Y / W;
                        }
                        const float ux = X - ph.p0[0], uy = Y - ph.p0[1];
                        const float bt = (paint_turns(uy, ux) - ph.d[0]) * ph.dd;
                        float v = (bt < 0.0f ? bt + 1.0f : bt) * ph.d[1];
                        if (ph.spread == CRH_SPREAD_REPEAT) {
                            v = v - floorf(v);
                        } else if (ph.spread == CRH_SPREAD_REFLECT) {
                            const float u = v - 2.0f * floorf(v * 0.5f);
                            v = u <= 1.0f ? u : 2.0f - u;
                        } else {
                            v = clamp_unit(v);
                        }
                        t[c] = v;
                    }
                    } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int b = (g + c) / S, k = (g + c) % S;
                        const float fx = tx0 + sx[k], fy = ty0 + (sy0[k] + (float)(4 * b)); // the sample's place on the frame (exact)
                        float X = fmaf(fy, pi.h[1], fmaf(fx, pi.h[0], pi.h[2])), Y = fmaf(fy, pi.h[4], fmaf(fx, pi.h[3], pi.h[5]));
                        if (!pi.affine) { // wave uniform
                            const float W = fmaf(fy, pi.h[7], fmaf(fx, pi.h[6], pi.h[8]));
                            X = X / W;
                            Y = Y / W;
                        }
                        const float ux = X - ph.p0[0], uy = Y - ph.p0[1];
                        float v = ph.kind == CRH_PAINT_LINEAR ? fmaf(ux, ph.d[0], uy * ph.d[1]) / ph.dd : sqrtf(fmaf(ux, ux, uy * uy)) / ph.d[0];
                        if (ph.spread == CRH_SPREAD_REPEAT) {
                            v = v - floorf(v);
                        } else if (ph.spread == CRH_SPREAD_REFLECT) {
                            const float u = v - 2.0f * floorf(v * 0.5f);
                            v = u <= 1.0f ? u : 2.0f - u;
                        } else {
                            v = clamp_unit(v);
                        }
                        t[c] = v;
                    }
                    }
                    for (uint32_t i = 0; i < ph.n_stops; ++i) { // wave uniform: the stop's record in scalar registers, a select per sample
                        const PaintStop st = load_uniform(&pa.stops[ph.first_stop + i]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const bool here = i == 0u || t[c] >= st.o;
                            const float f = fmaxf((t[c] - st.o) * st.inv, 0.0f);
#pragma unroll
                            for (int ch = 0; ch < 4; ++ch) pc[c][ch] = here ? fmaf(f, st.dc[ch], st.c[ch]) : pc[c][ch];
                        }
                    }
                    } // a gradient
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int b = (g + c) / S, k = (g + c) % S;
                        float src[4], us[4], ud[4];
                        const float sa = pc[c][3] * pi.tint[3];
                        if (IMAGES && pi.pad != 0u) { // texels are premultiplied: the tint is premultiplied first, (rgb * a, a) as k_prim_setup does
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) src[ch] = clamp_unit(pc[c][ch] * (pi.tint[ch] * pi.tint[3]));
                        } else {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) src[ch] = clamp_unit((pc[c][ch] * pi.tint[ch]) * sa); // (rgb * a, a) as k_prim_setup premultiplies the solid colour
                        }
                        src[3] = clamp_unit(sa);
#pragma unroll
                        for (int ch = 0; ch < 4; ++ch) {
                            const int cc = ch == 3 ? 1 : 0;
                            us[ch] = (bf.src.c0[ch] + bf.src.s[cc] * src[ch]) + bf.src.sa[cc] * src[3];
                            ud[ch] = (bf.dst.c0[ch] + bf.dst.s[cc] * src[ch]) + bf.dst.sa[cc] * src[3];
                        }
                        const float ad = col[b][k][3];
#pragma unroll
                        for (int ch = 0; ch < 4; ++ch) {
                            const int cc = ch == 3 ? 1 : 0;
                            const float dc = col[b][k][ch];
                            const float fs = fminf((us[ch] + bf.src.d[cc] * dc) + bf.src.da[cc] * ad, bf.src.cap0[cc] + bf.src.cap1[cc] * ad);
                            const float fd = fminf((ud[ch] + bf.dst.d[cc] * dc) + bf.dst.da[cc] * ad, bf.dst.cap0[cc] + bf.dst.cap1[cc] * ad);
                            const float ps = src[ch] * fs, qd = dc * fd;
                            const float lin = bf.os[cc] * ps + bf.od[cc] * qd;
                            const uint32_t bkind = bf.kind[cc]; // wave uniform
                            float v = bkind == 0u ? lin : (bkind == 1u ? fminf(src[ch], dc) : (bkind == 2u ? fmaxf(src[ch], dc) : src[ch]));
                            v = clamp_unit(v);
                            if (rounds_writes<XFMT>(r)) v = attachment<XFMT>(r, ch, v);
                            col[b][k][ch] = (blend[b][k] && ((bf.write_mask >> ch) & 1u) != 0u) ? v : dc;
                        }
                    }
                }
            } else if (BLEND && color_cover) { // color_cover with the renderer's blend state (api.hip blend_form; the target stands for an Rgba8Unorm attachment)
                float src[4], us[4], ud[4];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) src[ch] = clamp_unit(frag.a0[ch]);
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) { // the terms of the factors that do not depend on the target (wave uniform)
                    const int c = ch == 3 ? 1 : 0;
                    us[ch] = (bf.src.c0[ch] + bf.src.s[c] * src[ch]) + bf.src.sa[c] * src[3];
                    ud[ch] = (bf.dst.c0[ch] + bf.dst.s[c] * src[ch]) + bf.dst.sa[c] * src[3];
                }
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        const float ad = col[b][k][3];
#pragma unroll
                        for (int ch = 0; ch < 4; ++ch) {
                            const int c = ch == 3 ? 1 : 0;
                            const float dc = col[b][k][ch];
                            const float fs = fminf((us[ch] + bf.src.d[c] * dc) + bf.src.da[c] * ad, bf.src.cap0[c] + bf.src.cap1[c] * ad);
                            const float fd = fminf((ud[ch] + bf.dst.d[c] * dc) + bf.dst.da[c] * ad, bf.dst.cap0[c] + bf.dst.cap1[c] * ad);
                            const float ps = src[ch] * fs, qd = dc * fd;
                            const float lin = bf.os[c] * ps + bf.od[c] * qd;
                            const uint32_t kind = bf.kind[c]; // wave uniform
                            float v = kind == 0u ? lin : (kind == 1u ? fminf(src[ch], dc) : (kind == 2u ? fmaxf(src[ch], dc) : src[ch]));
                            v = clamp_unit(v);
                            if (rounds_writes<XFMT>(r)) v = attachment<XFMT>(r, ch, v);
                            col[b][k][ch] = (blend[b][k] && ((bf.write_mask >> ch) & 1u) != 0u) ? v : dc; // a masked channel keeps the target's value
                        }
                    }
            } else if (color_cover) { // color_cover: premultiplied "over" (shaders.wgsl:304-309, blending of examples/showcase/main.rs:32-43)
                const float s0 = frag.a0[0], s1 = frag.a0[1], s2 = frag.a0[2], ca = frag.a0[3];
                const float one_minus_a = 1.0f - ca;
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        const float n0 = s0 + col[b][k][0] * one_minus_a, n1 = s1 + col[b][k][1] * one_minus_a;
                        const float n2 = s2 + col[b][k][2] * one_minus_a, n3 = ca + col[b][k][3] * one_minus_a;
                        col[b][k][0] = blend[b][k] ? n0 : col[b][k][0];
                        col[b][k][1] = blend[b][k] ? n1 : col[b][k][1];
                        col[b][k][2] = blend[b][k] ? n2 : col[b][k][2];
                        col[b][k][3] = blend[b][k] ? n3 : col[b][k][3];
                    }
                if (rounds_writes<XFMT>(r)) { // an Rgba8Unorm attachment keeps 8 bits of what the blender writes (idempotent on the others)
#pragma unroll
                    for (int b = 0; b < ROWS; ++b)
#pragma unroll
                        for (int k = 0; k < S; ++k)
#pragma unroll
                            for (int ch = 0; ch < 4; ++ch) col[b][k][ch] = attachment<XFMT>(r, ch, col[b][k][ch]);
                }
            }
        }
    }
    if (OPS && has_depth && r.depth_write != 0u) {
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
            if (gx < r.width && gy < r.height) {
#pragma unroll
                for (int k = 0; k < S; ++k) r.depth[((size_t)gy * r.width + gx) * S + k] = depth[OPS ? b : 0][OPS ? k : 0];
            }
        }
    }
    if (keeps_state) { // what this pass leaves to the next one (the winding counter wraps inside its bits: IncrementWrap / DecrementWrap under the write mask, renderer.rs:577-582)
#pragma unroll
        for (int b = 0; b < ROWS; ++b) {
            const uint32_t gy = ty * kTile + first_row + 4u * b + rq;
            if (gx < r.width && gy < r.height) {
                const size_t at = ((size_t)gy * r.width + gx) * S;
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    r.state_stencil[at + k] = (uint8_t)(((uint32_t)winding[b][k] & r.winding_mask) | (((uint32_t)clipc[OPS ? b : 0][OPS ? k : 0] & r.clip_mask_count) << r.winding_bits));
                    reinterpret_cast<float4*>(r.state_color)[at + k] = make_float4(col[b][k][0], col[b][k][1], col[b][k][2], col[b][k][3]);
#pragma unroll
                    for (int l = 0; l < kMaxAlphaLayers; ++l)
                        if ((uint32_t)l < r.state_layers) r.state_alpha[(size_t)l * r.width * r.height * S + at + k] = saved[OPS ? b : 0][OPS ? k : 0][l];
                }
            }
        }
    }
    // ---- MSAA resolve (box average) + RGBA8 unorm store
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
                for (int k = 0; k < S; ++k) sum = sum + col[b][k][ch];
                avg[ch] = sum * inv;
            }
            store_px<XFMT>(r, gx, gy, avg[0], avg[1], avg[2], avg[3]);
        }
    }
