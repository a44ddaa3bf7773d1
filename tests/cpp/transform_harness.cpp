// Compiled and run by tests/test_transform_cpu.py: the C++ mirror's transform against the C ABI. main() reads a width x height RGBA8 source
// from the file argv[1] (argv[2], argv[3] = the size), fits the forward matrix (0.75 -0.5 3; 0.5 0.75 -1; 0 0 1) — a turn with a scale,
// in entries that are exact in binary — and prints the fitted size and origin, the nine entries of the fitted matrix as hexadecimal
// floats, one line of hex bytes of transform_texels per filter under the Reflect edge, and the position and visibility of two texels of
// a projective call; host only: no device is touched. device_side() is only compiled.
#include <contrast_renderer.hpp>

#include <cstdio>
#include <cstdlib>

int device_side(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    Image layer = Image::from_frame(frame, 0, 0, 2u, 2u);
    Image turned = layer.rotate(30.0, TransformFilter::Cubic);
    Image flipped = layer.transform({1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.001, 0.0, 1.0});
    Transform raw;
    raw.width = 2, raw.height = 2;
    Image same = layer.resample(raw);
    (void)renderer;
    static_assert(sizeof(crh_transform) == 88, "crh_transform is nine doubles and four 32-bit words");
    return (int)(turned.origin()[0] + flipped.width() + same.height());
}

int main(int argc, char** argv) {
    using namespace contrast_renderer;
    if (argc != 4) return 2;
    std::FILE* file = std::fopen(argv[1], "rb");
    if (!file) return 3;
    std::vector<uint8_t> texels;
    for (int c; (c = std::fgetc(file)) != EOF;) texels.push_back((uint8_t)c);
    std::fclose(file);
    const uint32_t width = (uint32_t)std::atol(argv[2]), height = (uint32_t)std::atol(argv[3]);
    if (texels.size() != (size_t)width * height * 4u) return 4;
    TransformFit fit = transform_fit(width, height, {0.75, -0.5, 3.0, 0.5, 0.75, -1.0, 0.0, 0.0, 1.0}, TransformFilter::Linear, BlurEdge::Reflect);
    std::printf("%u %u %d %d\n", fit.transform.width, fit.transform.height, fit.origin[0], fit.origin[1]);
    for (double m : fit.transform.matrix) std::printf("%a ", m);
    std::printf("\n");
    const TransformFilter filters[3] = {TransformFilter::Nearest, TransformFilter::Linear, TransformFilter::Cubic};
    for (TransformFilter filter : filters) {
        fit.transform.filter = filter;
        transform_validate(fit.transform);
        for (uint8_t v : transform_texels(width, height, texels, fit.transform)) std::printf("%02x", v);
        std::printf("\n");
    }
    Transform tilted;
    tilted.matrix = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.25, 0.0, 1.0};
    tilted.width = 8, tilted.height = 2;
    for (uint32_t i : {1u, 6u}) {
        const TransformPosition at = transform_position(tilted, i, 1u);
        std::printf("%d %d %d\n", at.position[0], at.position[1], at.visible ? 1 : 0);
    }
    try {
        tilted.matrix[4] = 2e12;
        transform_validate(tilted);
        return 5; // (an entry above 2^40 must throw)
    } catch (const Error&) {
    }
    try {
        (void)transform_fit(width, height, {1.0, 2.0, 0.0, 2.0, 4.0, 0.0, 0.0, 0.0, 1.0});
        return 6; // (a singular forward must throw)
    } catch (const Error&) {
    }
    return 0;
}
