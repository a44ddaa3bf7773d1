// csrc/tess_streams.hpp — the byte layout of the eleven output streams of a tessellation, written once: which scan channel (or sum of two)
// counts a stream's records and how many bytes a record has, in the order of the reference's byte image of a Shape (renderer.rs:198-209: the
// vertex buffer holds eight slices, the index buffer three). Host code over plain arrays: the C ABI sizes the streams, reports the traffic and
// cuts the parity taps' images with it (api.hip), and tests/cpp/tess_streams_sanitize.cpp runs it without a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "scene.hpp"

namespace crh {

enum { TS_LINE_V, TS_JOINT_V, TS_SOLID_V, TS_IQ_V, TS_IC_V, TS_RQ_V, TS_RC_V, TS_HULL_V, TS_LINE_I, TS_JOINT_I, TS_SOLID_I, kTessStreams };
constexpr int kTessVertexStreams = 8, kTessIndexStreams = 3; // the slices of a Shape's vertex and index buffer

struct TessStream {
    int ch, plus;   // its records: those of channel ch, and of channel plus where that is one (the restart markers of an index stream)
    uint32_t bytes; // per record
};
constexpr int kNoChannel = -1;
constexpr TessStream kTessStream[kTessStreams] = {
    {CH_LINE_V, kNoChannel, 20},     // line_v: a Vertex2f1i
    {CH_JOINT, kNoChannel, 120},     // joint_v: 5 x Vertex3f1i
    {CH_SOLID_V, kNoChannel, 8},     // solid_v: a Vertex0
    {CH_IQ, kNoChannel, 48},         // iq_v: 3 x Vertex2f
    {CH_IC_V, kNoChannel, 20},       // ic_v: a Vertex3f
    {CH_RQ, kNoChannel, 60},         // rq_v: 3 x Vertex3f
    {CH_RC_V, kNoChannel, 24},       // rc_v: a Vertex4f
    {CH_HULL, kNoChannel, 8},        // hull_v: a Vertex0. The channel counts the CANDIDATES (what the stream is sized for and where a Shape's hull begins); how
                                     // many of them are the Shape's hull is hull_count
    {CH_LINE_V, CH_LINE_CUT, 2},     // line_i: a u16 per line vertex and per restart marker
    {CH_JOINT, kNoChannel, 12},      // joint_i: 6 x u16
    {CH_SOLID_V, CH_SOLID_END, 2},   // solid_i: a u16 per polygon vertex and per closed path
};
static_assert(kTessVertexStreams + kTessIndexStreams == kTessStreams, "the byte image has eight vertex and three index slices");
static_assert(kTessStream[TS_LINE_V].bytes == sizeof(Vertex2f1i) && kTessStream[TS_JOINT_V].bytes == 5 * sizeof(Vertex3f1i), "stroke records");
static_assert(kTessStream[TS_SOLID_V].bytes == sizeof(Vertex0) && kTessStream[TS_HULL_V].bytes == sizeof(Vertex0), "polygon and hull records");
static_assert(kTessStream[TS_IQ_V].bytes == 3 * sizeof(Vertex2f) && kTessStream[TS_IC_V].bytes == sizeof(Vertex3f), "integral curve records");
static_assert(kTessStream[TS_RQ_V].bytes == 3 * sizeof(Vertex3f) && kTessStream[TS_RC_V].bytes == sizeof(Vertex4f), "rational curve records");
static_assert(kTessStream[TS_LINE_I].bytes == sizeof(uint16_t) && kTessStream[TS_JOINT_I].bytes == 6 * sizeof(uint16_t) && kTessStream[TS_SOLID_I].bytes == sizeof(uint16_t), "index records");

// the records of stream k among the per-channel counts n[NCH] (totals, capacities, or where a Shape begins: a row of shape_base)
inline uint64_t tess_stream_records(int k, const uint32_t* n) {
    const TessStream& s = kTessStream[k];
    return (uint64_t)n[s.ch] + (s.plus != kNoChannel ? n[s.plus] : 0u);
}
inline uint64_t tess_stream_bytes(int k, const uint32_t* n) { return tess_stream_records(k, n) * kTessStream[k].bytes; }

// What a tessellation with these totals writes for the passes to read: every stream but the hull's (its bytes are the hull kernels' to account for).
inline uint64_t tess_emitted_bytes(const uint32_t* totals) {
    uint64_t bytes = 0;
    for (int k = 0; k < kTessStreams; ++k)
        if (k != TS_HULL_V) bytes += tess_stream_bytes(k, totals);
    return bytes;
}

// One Shape's slice of stream k, in bytes — row: its begin[NCH], end[NCH] of shape_base, so it begins tess_stream_bytes(k, row) into the scene-wide stream.
inline uint64_t tess_shape_bytes(int k, const uint32_t* row, uint32_t hull_count) {
    if (k == TS_HULL_V) return (uint64_t)hull_count * kTessStream[k].bytes;
    uint32_t n[NCH];
    for (int c = 0; c < NCH; ++c) n[c] = row[NCH + c] - row[c];
    return tess_stream_bytes(k, n);
}

// Where each slice ENDS in the Shape's vertex buffer (vo[8]) and index buffer (io[3]): the last entries are the buffers' sizes.
inline void tess_shape_offsets(const uint32_t* row, uint32_t hull_count, uint64_t vo[kTessVertexStreams], uint64_t io[kTessIndexStreams]) {
    uint64_t at = 0;
    for (int k = 0; k < kTessStreams; ++k) {
        if (k == kTessVertexStreams) at = 0;
        at += tess_shape_bytes(k, row, hull_count);
        (k < kTessVertexStreams ? vo[k] : io[k - kTessVertexStreams]) = at;
    }
}

// The byte image of one Shape cut out of host copies of the eleven scene-wide streams (stream[k]: all of stream k); a null vb or ib is left out.
inline void tess_assemble_shape(const uint32_t* row, uint32_t hull_count, const uint8_t* const stream[kTessStreams], uint8_t* vb, uint8_t* ib) {
    for (int k = 0; k < kTessStreams; ++k) {
        uint8_t*& dst = k < kTessVertexStreams ? vb : ib;
        const uint64_t bytes = tess_shape_bytes(k, row, hull_count);
        if (dst && bytes) {
            std::memcpy(dst, stream[k] + tess_stream_bytes(k, row), bytes);
            dst += bytes;
        }
    }
}

} // namespace crh
