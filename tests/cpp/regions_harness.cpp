// Compiled and run by tests/test_regions_cpu.py: the C++ mirror's regions and statistics against the C ABI. main() reads a width x height
// image of RGBA8 from the file argv[1] (argv[2], argv[3] = its size) and prints, for every following group of four arguments x y w h,
// one line "crop hex-bytes" of crop_texels, then two lines "statistics x0 y0 x1 y1 count hex-words" of statistics_texels (alpha >= 1,
// red >= 128), host only: no device is touched. device_side() is only compiled.
#include <contrast_renderer.hpp>

#include <cstdio>
#include <cstdlib>

int device_side(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image layer(renderer, 2, 2, texels);
    Image canvas = layer.crop(-700, -400, 1024u, 1024u);
    Image trimmed = canvas.trim(Channel::A, 1u, 2u);
    Image part = Image::from_frame(frame, 10, -3, 40u, 30u);
    Image shadow = trimmed.blur(2.0f);
    const std::array<uint32_t, 2> origin = shadow.origin();
    Image under = canvas.composite(shadow, CompositeOp::DstOver, BlendMode::Normal, 0.5f, {4 - (int32_t)origin[0], 3 - (int32_t)origin[1]});
    const ImageStatistics stats = under.statistics(Channel::G, 200u);
    const std::array<uint32_t, 4> bounds = part.bounds();
    static_assert(sizeof(crh_image_stats) == 4116, "crh_image_stats is 1024 + 5 32-bit words");
    static_assert(sizeof(ImageStatistics) == sizeof(crh_image_stats), "the mirror's statistics are the C ABI's");
    return (int)(stats.count + stats.histogram[256u * 3u] + bounds[2] + (uint32_t)(int32_t)part.origin()[1]);
}

int main(int argc, char** argv) {
    using namespace contrast_renderer;
    if (argc < 4 || (argc - 4) % 4 != 0) return 2;
    std::FILE* file = std::fopen(argv[1], "rb");
    if (!file) return 3;
    std::vector<uint8_t> texels;
    for (int c; (c = std::fgetc(file)) != EOF;) texels.push_back((uint8_t)c);
    std::fclose(file);
    const uint32_t width = (uint32_t)std::atol(argv[2]), height = (uint32_t)std::atol(argv[3]);
    if (texels.size() != (size_t)width * height * 4u) return 4;
    for (int at = 4; at < argc; at += 4) {
        const std::vector<uint8_t> out =
            crop_texels(width, height, texels, (int32_t)std::atoll(argv[at]), (int32_t)std::atoll(argv[at + 1]), (uint32_t)std::atol(argv[at + 2]), (uint32_t)std::atol(argv[at + 3]));
        std::printf("crop ");
        for (uint8_t v : out) std::printf("%02x", v);
        std::printf("\n");
    }
    const Channel channels[2] = {Channel::A, Channel::R};
    const uint32_t thresholds[2] = {1u, 128u};
    for (int k = 0; k < 2; ++k) {
        const ImageStatistics s = statistics_texels(width, height, texels, channels[k], thresholds[k]);
        std::printf("statistics %u %u %u %u %u ", s.x0, s.y0, s.x1, s.y1, s.count);
        for (uint32_t word : s.histogram) std::printf("%02x%02x%02x%02x", word & 255u, (word >> 8) & 255u, (word >> 16) & 255u, word >> 24);
        std::printf("\n");
    }
    try {
        (void)crop_texels(width, height, texels, 0, 0, 0u, 1u);
        return 5; // (an empty result must throw)
    } catch (const Error&) {
    }
    try {
        (void)statistics_texels(width, height, texels, Channel::A, 0u);
        return 6; // (a threshold of 0 must throw)
    } catch (const Error&) {
    }
    return 0;
}
