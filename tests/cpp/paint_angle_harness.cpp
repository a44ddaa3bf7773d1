// Compiled by tests/test_conic_cpu.py and tests/test_gpu_conic.py from csrc/paint_angle.hpp alone, with the host compiler and -ffp-contract=off:
//   paint_angle_harness IN OUT        IN holds f32 pairs (y, x); OUT receives paint_turns(y, x) of each, as f32
//   paint_angle_harness --measure N   the largest error in turns against binary64 atan2 over a dense sweep (N ratios per octant and magnitude).
//                                     The mantissas and half of the ratios are random and their sequence depends on N: the figure is that of a
//                                     sample and differs a little from one N to the next
#include <paint_angle.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static double turns64(double y, double x) {
    const double a = std::atan2(y, x) / 6.283185307179586476925286766559;
    return a < 0.0 ? a + 1.0 : a;
}

static double error_of(float y, float x) {
    const double d = std::fabs((double)crh::paint_turns(y, x) - turns64((double)y, (double)x));
    return d > 0.5 ? 1.0 - d : d; // round the circle: 1 and 0 are one angle
}

static int measure(long n) {
    double worst = 0.0;
    float worst_y = 0.0f, worst_x = 0.0f;
    unsigned long long points = 0;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto uniform = [&]() { // xorshift64*: [0, 1)
        state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
        return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
    };
    auto visit = [&](float lo, float hi) {
        for (int octant = 0; octant < 8; ++octant) {
            float x = (octant & 1) ? lo : hi, y = (octant & 1) ? hi : lo;
            if (octant & 2) x = -x;
            if (octant & 4) y = -y;
            const double e = error_of(y, x);
            points += 1;
            if (e > worst) worst = e, worst_y = y, worst_x = x;
        }
    };
    for (int e = -149; e <= 24; ++e) {
        for (long i = 0; i <= n; ++i) { // ratios dense in [0, 1], the ends included, under a random mantissa of the magnitude (a denormal
                                        // magnitude keeps 149 + e bits of it: at 2^-149 there is one value, and the ratios are 0 or 1)
            const float hi = (float)std::ldexp(i == 0 || e == 24 ? 1.0 : 1.0 + uniform(), e);
            visit((float)((double)hi * ((double)i / (double)n)), hi);
            visit((float)((double)hi * uniform()), hi);
        }
        for (int k = 0; k <= 173; ++k) // small ratios: 2^-k under a random mantissa
            visit((float)std::ldexp(1.0 + uniform(), e - k), (float)std::ldexp(1.0, e));
    }
    std::printf("points %llu worst %.6e at y %a x %a bound %.6e\n", points, worst, (double)worst_y, (double)worst_x, (double)crh::kPaintTurnsError);
    return worst <= (double)crh::kPaintTurnsError ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "--measure") == 0) return measure(std::atol(argv[2]));
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<float> pairs;
    float buffer[4096];
    for (size_t got; (got = std::fread(buffer, sizeof(float), 4096, in)) != 0;) pairs.insert(pairs.end(), buffer, buffer + got);
    std::fclose(in);
    std::vector<float> out(pairs.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = crh::paint_turns(pairs[2 * i], pairs[2 * i + 1]);
    std::FILE* to = std::fopen(argv[2], "wb");
    if (!to) return 3;
    const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), to) == out.size();
    return std::fclose(to) == 0 && ok ? 0 : 4;
}
