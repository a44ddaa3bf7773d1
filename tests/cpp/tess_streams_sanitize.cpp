// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_tess_streams_cpu.py: a stand-alone
// host program around csrc/tess_streams.hpp, the one table of the eleven output streams that sizes them, reports a tessellation's traffic
// and cuts the parity taps' byte images (no library, no device). For synthetic rows of shape_base, hull counts and totals it compares the
// header's per-Shape offsets, per-stream totals, emitted bytes and assembled images with a plain restatement that carries the record
// sizes as literals — 20, 120, 8, 48, 20, 60, 24, 8 and 2, 12, 2, and the two channel sums — on heap buffers that end exactly where the
// streams and the images do: a slice cut a byte too long is the sanitizer's to see. With -DTESS_STREAMS_RESTATEMENT_ONLY the header is
// left out and the restatement runs against its hand-computed figures alone (it builds where the header does not exist).
// Exit status 0 = all equal.
#include <cstdint>
uint32_t atomicMin(uint32_t*, uint32_t); // (scene.hpp, read as plain C++: its one device helper names it; nothing here calls either)
#ifndef TESS_STREAMS_RESTATEMENT_ONLY
#include <tess_streams.hpp>
#else
#include <scene.hpp>
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
using namespace crh;

long long failures = 0, checks = 0;

void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
    ++checks;
    if (ok) return;
    ++failures;
    std::printf("FAILED %s (%lld, %lld)\n", what, a, b);
}

// ---- the restatement: the layout with its literals written out, stream by stream
void restated_offsets(const uint32_t* a, uint32_t hull_count, uint64_t vo[8], uint64_t io[3]) {
    const uint32_t* b = a + NCH; // a: begin[NCH], b: end[NCH]
    auto n = [&](int c) { return (uint64_t)(b[c] - a[c]); };
    uint64_t v = 0;
    vo[0] = v += n(CH_LINE_V) * 20;
    vo[1] = v += n(CH_JOINT) * 120;
    vo[2] = v += n(CH_SOLID_V) * 8;
    vo[3] = v += n(CH_IQ) * 48;
    vo[4] = v += n(CH_IC_V) * 20;
    vo[5] = v += n(CH_RQ) * 60;
    vo[6] = v += n(CH_RC_V) * 24;
    vo[7] = v += (uint64_t)hull_count * 8;
    uint64_t i = 0;
    io[0] = i += (n(CH_LINE_V) + n(CH_LINE_CUT)) * 2;
    io[1] = i += n(CH_JOINT) * 12;
    io[2] = i += (n(CH_SOLID_V) + n(CH_SOLID_END)) * 2;
}
// the bytes of the eleven scene-wide streams for these counts (totals, or a Shape's begin row: where its slices begin)
void restated_stream_bytes(const uint32_t* t, uint64_t out[11]) {
    out[0] = (uint64_t)t[CH_LINE_V] * 20, out[1] = (uint64_t)t[CH_JOINT] * 120, out[2] = (uint64_t)t[CH_SOLID_V] * 8, out[3] = (uint64_t)t[CH_IQ] * 48;
    out[4] = (uint64_t)t[CH_IC_V] * 20, out[5] = (uint64_t)t[CH_RQ] * 60, out[6] = (uint64_t)t[CH_RC_V] * 24, out[7] = (uint64_t)t[CH_HULL] * 8;
    out[8] = ((uint64_t)t[CH_LINE_V] + t[CH_LINE_CUT]) * 2, out[9] = (uint64_t)t[CH_JOINT] * 12, out[10] = ((uint64_t)t[CH_SOLID_V] + t[CH_SOLID_END]) * 2;
}
uint64_t restated_emitted(const uint32_t* t) {
    return (uint64_t)t[CH_LINE_V] * 20 + ((uint64_t)t[CH_LINE_V] + t[CH_LINE_CUT]) * 2 + (uint64_t)t[CH_JOINT] * (120 + 12) + (uint64_t)t[CH_SOLID_V] * 8 +
           ((uint64_t)t[CH_SOLID_V] + t[CH_SOLID_END]) * 2 + (uint64_t)t[CH_IQ] * 48 + (uint64_t)t[CH_IC_V] * 20 + (uint64_t)t[CH_RQ] * 60 + (uint64_t)t[CH_RC_V] * 24;
}
void restated_assemble(const uint32_t* a, uint32_t hull_count, const uint8_t* const stream[11], uint8_t* vb, uint8_t* ib) {
    uint64_t begin[11], vo[8], io[3];
    restated_stream_bytes(a, begin);
    restated_offsets(a, hull_count, vo, io);
    for (int k = 0; k < 11; ++k) {
        uint8_t* const dst = k < 8 ? vb : ib;
        const uint64_t from = k == 0 || k == 8 ? 0 : k < 8 ? vo[k - 1] : io[k - 9], to = k < 8 ? vo[k] : io[k - 8];
        for (uint64_t j = from; dst && j < to; ++j) dst[j] = stream[k][begin[k] + (j - from)];
    }
}

// ---- a synthetic tessellation: counts[s][c] records of channel c for Shape s, hull[s] <= counts[s][CH_HULL] hull vertices
struct Scene {
    uint32_t n_shapes;
    std::vector<uint32_t> rows, hull; // shape_base: [n_shapes][2][NCH]
    uint32_t totals[NCH];
    std::vector<uint8_t> stream[11]; // exactly the streams' bytes
    const uint8_t* at[11];
};
Scene make_scene(uint32_t n_shapes, const uint32_t (*counts)[NCH], const uint32_t* hull, unsigned seed) {
    Scene s;
    s.n_shapes = n_shapes;
    std::memset(s.totals, 0, sizeof(s.totals));
    for (uint32_t k = 0; k < n_shapes; ++k) {
        for (int c = 0; c < NCH; ++c) s.rows.push_back(s.totals[c]);
        for (int c = 0; c < NCH; ++c) s.rows.push_back(s.totals[c] += counts[k][c]);
        s.hull.push_back(hull[k]);
    }
    uint64_t bytes[11];
    restated_stream_bytes(s.totals, bytes);
    std::srand(seed);
    for (int k = 0; k < 11; ++k) {
        s.stream[k].resize(bytes[k]);
        s.stream[k].shrink_to_fit();
        for (uint8_t& v : s.stream[k]) v = (uint8_t)(std::rand() >> 7);
        s.at[k] = s.stream[k].data();
    }
    return s;
}

void check_scene(const Scene& s) {
    uint64_t total_v = 0, total_i = 0;
    std::vector<uint64_t> all_vo((size_t)s.n_shapes * 8), all_io((size_t)s.n_shapes * 3);
    for (uint32_t k = 0; k < s.n_shapes; ++k) {
        restated_offsets(&s.rows[(size_t)k * 2 * NCH], s.hull[k], &all_vo[(size_t)k * 8], &all_io[(size_t)k * 3]);
        total_v += all_vo[(size_t)k * 8 + 7], total_i += all_io[(size_t)k * 3 + 2];
    }
    // the restatement against itself: what the Shapes hold in front of their hulls and in their index buffers is what the run emitted
    uint64_t in_front = 0;
    for (uint32_t k = 0; k < s.n_shapes; ++k) in_front += all_vo[(size_t)k * 8 + 6] + all_io[(size_t)k * 3 + 2];
    expect(in_front == restated_emitted(s.totals), "the emitted bytes are the Shapes' slices", (long long)in_front, (long long)restated_emitted(s.totals));
    // the images of all Shapes one behind the other (crh_scene_download_all), on buffers of exactly their size
    std::vector<uint8_t> want_v(total_v), want_i(total_i);
    uint64_t v = 0, i = 0;
    for (uint32_t k = 0; k < s.n_shapes; ++k) {
        restated_assemble(&s.rows[(size_t)k * 2 * NCH], s.hull[k], s.at, want_v.data() + v, want_i.data() + i);
        v += all_vo[(size_t)k * 8 + 7], i += all_io[(size_t)k * 3 + 2];
    }
    expect(v == total_v && i == total_i, "the images fill their buffers");
#ifndef TESS_STREAMS_RESTATEMENT_ONLY
    static_assert(kTessStreams == 11 && kTessVertexStreams == 8 && kTessIndexStreams == 3 && kShapeRow == 2 * NCH, "the shape of the table");
    uint64_t bytes[11];
    restated_stream_bytes(s.totals, bytes);
    for (int k = 0; k < 11; ++k) expect(tess_stream_bytes(k, s.totals) == bytes[k], "a stream's bytes", k, (long long)tess_stream_bytes(k, s.totals));
    expect(tess_emitted_bytes(s.totals) == restated_emitted(s.totals), "the emitted bytes", (long long)tess_emitted_bytes(s.totals), (long long)restated_emitted(s.totals));
    for (int pass = 0; pass < 3; ++pass) { // both buffers, the vertex buffer alone (ib null), the index buffer alone (vb null)
        std::vector<uint8_t> got_v(pass == 2 ? 0 : total_v), got_i(pass == 1 ? 0 : total_i);
        got_v.shrink_to_fit(), got_i.shrink_to_fit();
        uint8_t* pv = pass == 2 ? nullptr : got_v.data();
        uint8_t* pi = pass == 1 ? nullptr : got_i.data();
        for (uint32_t k = 0; k < s.n_shapes; ++k) {
            const uint32_t* row = &s.rows[(size_t)k * kShapeRow];
            uint64_t vo[8], io[3];
            tess_shape_offsets(row, s.hull[k], vo, io);
            for (int j = 0; j < 8; ++j) expect(vo[j] == all_vo[(size_t)k * 8 + j], "a vertex offset", k, j);
            for (int j = 0; j < 3; ++j) expect(io[j] == all_io[(size_t)k * 3 + j], "an index offset", k, j);
            tess_assemble_shape(row, s.hull[k], s.at, pv, pi);
            if (pv) pv += vo[7];
            if (pi) pi += io[2];
        }
        if (pass != 2) expect(got_v == want_v, "the vertex images", pass);
        if (pass != 1) expect(got_i == want_i, "the index images", pass);
    }
#endif
}

// the restatement against figures worked out by hand: 2 line vertices + 1 cut, 1 join, 3 + 1 polygon records, 1 + 3 + 1 + 3 curve records, 4 of 5 hull candidates
void check_by_hand() {
    const uint32_t row[2 * NCH] = {7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7 + 2, 7 + 5, 7 + 1, 7 + 1, 7 + 3, 7 + 1, 7 + 1, 7 + 3, 7 + 1, 7 + 3};
    uint64_t vo[8], io[3], begin[11];
    restated_offsets(row, 4, vo, io);
    const uint64_t want_vo[8] = {40, 160, 184, 232, 292, 352, 424, 456}, want_io[3] = {6, 18, 26};
    for (int j = 0; j < 8; ++j) expect(vo[j] == want_vo[j], "a vertex offset by hand", j, (long long)vo[j]);
    for (int j = 0; j < 3; ++j) expect(io[j] == want_io[j], "an index offset by hand", j, (long long)io[j]);
    restated_stream_bytes(row, begin);
    const uint64_t want_begin[11] = {140, 840, 56, 336, 140, 420, 168, 56, 28, 84, 28};
    for (int k = 0; k < 11; ++k) expect(begin[k] == want_begin[k], "a slice's begin by hand", k, (long long)begin[k]);
    expect(restated_emitted(row + NCH) == 180 + 1056 + 80 + 384 + 200 + 480 + 240 + 34 + 36, "the emitted bytes by hand", (long long)restated_emitted(row + NCH));
}

} // namespace

int main() {
    check_by_hand();
    //                              LINE_V HULL CUT JOINT SOLID_V SOLID_END IQ IC_V RQ RC_V
    const uint32_t full[1][NCH] = {{6, 9, 2, 3, 5, 2, 2, 6, 1, 3}};
    const uint32_t full_hull[1] = {7};
    check_scene(make_scene(1, full, full_hull, 1));
    const uint32_t nothing[1][NCH] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
    const uint32_t no_hull[1] = {0};
    check_scene(make_scene(1, nothing, no_hull, 2));
    // three Shapes: strokes and curves; one that is empty in every stream; one with a single restart marker of the last stream (solid_i) and nothing else
    const uint32_t three[3][NCH] = {{4, 11, 1, 2, 0, 0, 1, 3, 2, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 1, 0, 0, 0, 0}};
    const uint32_t three_hull[3] = {5, 0, 0};
    check_scene(make_scene(3, three, three_hull, 3));
    // ... and with the empty Shape first, candidates that all stay on the hull, a Shape of polygons only
    const uint32_t again[3][NCH] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {2, 3, 0, 0, 7, 2, 0, 0, 0, 6}, {0, 4, 0, 0, 4, 1, 0, 0, 0, 0}};
    const uint32_t again_hull[3] = {0, 3, 4};
    check_scene(make_scene(3, again, again_hull, 4));
    std::printf("%lld checks, %lld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
