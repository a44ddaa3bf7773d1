// Compiled as host code under the address and undefined-behaviour sanitizers and run once by tests/test_resize_cpu.py: a stand-alone host
// program around the rule of csrc/resize.hpp, the code crh_resize_taps and crh_resize_texels run (no library, no device). It builds the
// taps of every filter over the edge sizes — 1 and 16384 on either side, the pairs just inside the tap cap, every small pair — checks what
// the rule promises of them (sum q = 16384, sum |q| <= 32768, every index inside the source, the kernels' table inside the source but for
// the zero tap one past an odd axis) and resizes images from and into heap buffers that end exactly where the image and the result do, at
// odd addresses, against a plain restatement of the two sums in 64-bit integers. An index that left the source, or a sum that
// overflowed 32 bits, would be the sanitizer's to see. Exit status 0 = all equal.
#include <resize.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

long long failures = 0, texels = 0;

void expect(bool ok, const char* what, unsigned filter, unsigned n, unsigned m) {
    if (ok) return;
    ++failures;
    std::printf("FAILED %s: filter %u, %u -> %u\n", what, filter, n, m);
}

// the promises of an axis; -> false where the rule refuses it
bool check_axis(unsigned n, unsigned m, unsigned filter, crh::ResizeAxis* axis) {
    const crh::ResizeAxisStatus st = crh::resize_axis(n, m, filter, axis, nullptr);
    if (st != crh::kResizeAxisOk) return false;
    for (unsigned o = 0; o < m; ++o) {
        long long sum = 0, gain = 0;
        for (unsigned t = 0; t < axis->count[o]; ++t) {
            const long long q = axis->taps[axis->offset[o] + t];
            sum += q, gain += q < 0 ? -q : q;
        }
        expect(sum == 16384 && gain <= 32768, "the sums of an output's taps", filter, n, m);
        expect(axis->first[o] >= 0 && axis->count[o] >= 1 && axis->count[o] <= 512 && (unsigned)axis->first[o] + axis->count[o] <= n, "the window", filter, n, m);
    }
    crh::ResizeTable table;
    expect(crh::resize_table(*axis, n, &table), "the table's indices", filter, n, m);
    for (unsigned o = 0; o < m; ++o) {
        const unsigned first = table.words[o], count = table.words[m + o];
        expect(first % 2u == 0u && count % 2u == 0u && count <= 2u * table.pairs && first + count <= n + 1u, "the table's window", filter, n, m);
        for (unsigned t = 0; t < count; ++t) { // the table holds the same taps at the same indices, and zeros around them
            const int16_t q = (int16_t)(table.words[2u * m + o * table.pairs + t / 2u] >> (t % 2u ? 16 : 0));
            const long long at = (long long)first + t - axis->first[o];
            const int16_t want = at >= 0 && at < axis->count[o] ? axis->taps[axis->offset[o] + (unsigned)at] : (int16_t)0;
            expect(q == want, "the table's taps", filter, n, m);
        }
    }
    return true;
}

void check_image(unsigned w, unsigned h, unsigned out_w, unsigned out_h, unsigned filter, unsigned seed) {
    crh::ResizeAxis ax, ay;
    if (!check_axis(w, out_w, filter, &ax) || !check_axis(h, out_h, filter, &ay)) {
        expect(false, "an image's axis is refused", filter, w, out_w);
        return;
    }
    // heap buffers that end exactly where the image and the result do, one byte off alignment
    std::vector<uint8_t> raw_in((size_t)w * h * 4u + 1u), raw_out((size_t)out_w * out_h * 4u + 1u);
    uint8_t* in = raw_in.data() + 1;
    uint8_t* out = raw_out.data() + 1;
    uint32_t state = seed * 2654435761u + 1u;
    for (size_t k = 0; k < (size_t)w * h; ++k) {
        state = state * 1664525u + 1013904223u;
        const unsigned a = (state >> 8) % 3u == 0u ? 255u : (state >> 8) % 3u == 1u ? 0u : (state >> 16) & 255u;
        for (int c = 0; c < 3; ++c) in[k * 4u + c] = (uint8_t)(((state >> (4 + 7 * c)) & 1u) * a); // colours 0 or alpha: the hardest edges
        in[k * 4u + 3u] = (uint8_t)a;
    }
    crh::resize_run(in, w, h, ax, ay, out_w, out_h, out);
    std::vector<long long> tmp((size_t)out_w * h * 4u);
    for (unsigned j = 0; j < h; ++j)
        for (unsigned o = 0; o < out_w; ++o)
            for (unsigned c = 0; c < 4u; ++c) {
                long long sum = 0;
                for (unsigned t = 0; t < ax.count[o]; ++t) sum += (long long)ax.taps[ax.offset[o] + t] * in[((size_t)j * w + (unsigned)ax.first[o] + t) * 4u + c];
                long long v = (sum + 32) >> 6;
                tmp[((size_t)j * out_w + o) * 4u + c] = v < 0 ? 0 : v > 65280 ? 65280 : v;
            }
    for (unsigned i = 0; i < out_h; ++i)
        for (unsigned o = 0; o < out_w; ++o) {
            long long v[4];
            for (unsigned c = 0; c < 4u; ++c) {
                long long sum = 0;
                for (unsigned t = 0; t < ay.count[i]; ++t) sum += (long long)ay.taps[ay.offset[i] + t] * tmp[((size_t)((unsigned)ay.first[i] + t) * out_w + o) * 4u + c];
                if (sum + (1ll << 21) >= (1ll << 31) || sum + (1ll << 21) < -(1ll << 31)) expect(false, "the vertical sum leaves 32 bits", filter, h, out_h);
                v[c] = (sum + (1ll << 21)) >> 22;
                v[c] = v[c] < 0 ? 0 : v[c] > 255 ? 255 : v[c];
            }
            for (unsigned c = 0; c < 4u; ++c) {
                const long long want = c < 3u && v[c] > v[3] ? v[3] : v[c];
                if (out[((size_t)i * out_w + o) * 4u + c] != want) expect(false, "a byte", filter, w, out_w);
            }
            ++texels;
        }
}

} // namespace

int main() {
    crh::ResizeAxis axis;
    const unsigned edges[][2] = {{1, 1}, {1, 16384}, {16384, 1}, {16384, 16384}, {16384, 33}, {33, 16384}, {16384, 32}, {16384, 65}, {16384, 64}, {16384, 129}, {16384, 128}, {16384, 193}, {16384, 192}, {16383, 511}, {2, 16383}};
    for (unsigned filter = 0; filter < crh::kResizeFilters; ++filter) {
        for (const auto& e : edges) (void)check_axis(e[0], e[1], filter, &axis);
        for (unsigned n = 1; n <= 12; ++n)
            for (unsigned m = 1; m <= 12; ++m) expect(check_axis(n, m, filter, &axis), "a small axis is refused", filter, n, m);
        // the caps: 16384 texels go to no fewer outputs than these
        const unsigned least[] = {33, 65, 129, 129, 193};
        expect(check_axis(16384, least[filter], filter, &axis) && !check_axis(16384, least[filter] - 1u, filter, &axis), "the cap", filter, 16384, least[filter]);
        check_image(1, 1, 1, 1, filter, 1), check_image(1, 1, 37, 21, filter, 2), check_image(37, 21, 1, 1, filter, 3);
        check_image(8, 5, 21, 13, filter, 4), check_image(11, 6, 5, 4, filter, 5), check_image(64, 3, 63, 5, filter, 6), check_image(129, 2, 31, 2, filter, 7);
        check_image(600, 2, 8, 3, filter, 8), check_image(2, 600, 3, 8, filter, 9), check_image(3, 2, 16384, 1, filter, 10), check_image(1, 3, 1, 16384, filter, 11);
    }
    check_image(16384, 1, 33, 1, crh::kResizeBox, 12), check_image(1, 16384, 1, 193, crh::kResizeLanczos3, 13);
    std::printf("%lld texels, %lld failures\n", texels, failures);
    return failures == 0 ? 0 : 1;
}
