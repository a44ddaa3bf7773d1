// Compiled and run by tests/test_color_filter_cpu.py: the C++ mirror's colour-filter interface against the C ABI. main() reads texels from the
// file argv[1] (n * 4 bytes) and prints, for each of the mirror's matrices without tables and with inverting tables, one line
// "name tables hex-bytes" of color_filter_texels (host only: no device is touched), and one line "matrix name 20 floats" per constructor.
// device_side() is only compiled.
#include <contrast_renderer.hpp>

#include <cstdio>
#include <cstdlib>

int device_side(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image layer(renderer, 2, 2, texels);
    Image soft = layer.blur(1.5f);
    const ColorMatrixValues black = ColorMatrix::flood(0.0, 0.0, 0.0, 0.5);
    Image shadow = soft.color_filter(&black);
    const std::array<uint32_t, 2> origin = shadow.origin();
    Image under = layer.composite(shadow, CompositeOp::DstOver, BlendMode::Normal, 1.0f, {4 - (int32_t)origin[0], 3 - (int32_t)origin[1]});
    ColorTables invert;
    for (size_t n = 0; n < invert.size(); ++n) invert[n] = (uint8_t)(255u - n % 256u);
    Image negative = under.color_filter(nullptr, &invert);
    Image copy = negative.color_filter();
    copy.generate_mipmaps();
    frame.load_image(copy);
    static_assert(CRH_COLOR_MATRIX_MAX == 16.0f, "the bound of the header");
    return (int)(copy.levels() + negative.width() + shadow.origin()[0]);
}

int main(int argc, char** argv) {
    using namespace contrast_renderer;
    if (argc < 2) return 2;
    std::FILE* file = std::fopen(argv[1], "rb");
    if (!file) return 3;
    std::vector<uint8_t> texels;
    for (int c; (c = std::fgetc(file)) != EOF;) texels.push_back((uint8_t)c);
    std::fclose(file);
    if (texels.empty() || texels.size() % 4u) return 4;
    const std::pair<const char*, ColorMatrixValues> matrices[] = {{"identity", ColorMatrix::identity()},       {"saturate", ColorMatrix::saturate(2.0)},
                                                                   {"hue_rotate", ColorMatrix::hue_rotate(90.0)}, {"luminance_to_alpha", ColorMatrix::luminance_to_alpha()},
                                                                   {"flood", ColorMatrix::flood(0.2, 0.4, 0.9, 0.6)}, {"opacity", ColorMatrix::opacity(0.25)}};
    ColorTables invert;
    for (size_t n = 0; n < invert.size(); ++n) invert[n] = (uint8_t)(255u - n % 256u);
    for (const auto& named : matrices) {
        std::printf("matrix %s", named.first);
        for (float v : named.second) std::printf(" %.9g", (double)v);
        std::printf("\n");
        for (int with_tables = 0; with_tables < 2; ++with_tables) {
            const std::vector<uint8_t> out = color_filter_texels(texels, &named.second, with_tables ? &invert : nullptr);
            std::printf("%s %d ", named.first, with_tables);
            for (uint8_t v : out) std::printf("%02x", v);
            std::printf("\n");
        }
    }
    if (color_filter_texels(texels) != color_filter_texels(texels, &matrices[0].second)) return 6; // (no matrix is the identity)
    ColorMatrixValues bad = ColorMatrix::identity();
    bad[7] = 16.5f;
    try {
        (void)color_filter_texels(texels, &bad);
        return 5; // (a coefficient above CRH_COLOR_MATRIX_MAX must throw)
    } catch (const Error&) {
    }
    return 0;
}
