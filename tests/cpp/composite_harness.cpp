// Compiled and run by tests/test_composite_cpu.py: the C++ mirror's compositing interface against the C ABI. main() reads texel pairs from the
// file argv[1] ([n * 4 bytes of sources | n * 4 bytes of backdrops]) and prints, for every operator and mode at the opacity argv[2], one line
// "op mode hex-bytes" of composite_texels (host only: no device is touched). device_side() is only compiled.
#include <contrast_renderer.hpp>

#include <cstdio>
#include <cstdlib>

int device_side(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image layer(renderer, 2, 2, texels);
    Image soft = layer.blur(1.5f);
    Image black = Image::from_frame(frame);
    Image shadow = black.composite(soft, CompositeOp::SrcIn);
    const std::array<uint32_t, 2> origin = soft.origin();
    Image under = layer.composite(shadow, CompositeOp::DstOver, BlendMode::Normal, 0.5f, {4 - (int32_t)origin[0], 3 - (int32_t)origin[1]});
    Image lit = layer.composite(layer, CompositeOp::SrcAtop, BlendMode::HardLight);
    under.generate_mipmaps();
    frame.load_image(under);
    static_assert((uint32_t)CompositeOp::Clear == 0u && (uint32_t)CompositeOp::SrcOver == 3u && (uint32_t)CompositeOp::Plus == 12u, "CompositeOp mirrors crh_composite_op");
    static_assert((uint32_t)BlendMode::Normal == 0u && (uint32_t)BlendMode::HardLight == 6u && (uint32_t)BlendMode::Exclusion == 8u, "BlendMode mirrors crh_blend_mode");
    static_assert(sizeof(crh_composite) == 20, "crh_composite is five 32-bit words");
    return (int)(under.levels() + lit.width() + under.origin()[0]);
}

int main(int argc, char** argv) {
    using namespace contrast_renderer;
    if (argc < 3) return 2;
    std::FILE* file = std::fopen(argv[1], "rb");
    if (!file) return 3;
    std::vector<uint8_t> bytes;
    for (int c; (c = std::fgetc(file)) != EOF;) bytes.push_back((uint8_t)c);
    std::fclose(file);
    if (bytes.empty() || bytes.size() % 8u) return 4;
    const std::vector<uint8_t> source(bytes.begin(), bytes.begin() + (long)(bytes.size() / 2u)), backdrop(bytes.begin() + (long)(bytes.size() / 2u), bytes.end());
    const float opacity = (float)std::atof(argv[2]);
    for (uint32_t op = 0; op <= (uint32_t)CompositeOp::Plus; ++op)
        for (uint32_t mode = 0; mode <= (uint32_t)BlendMode::Exclusion; ++mode) {
            const std::vector<uint8_t> out = composite_texels(source, backdrop, (CompositeOp)op, (BlendMode)mode, opacity);
            std::printf("%u %u ", op, mode);
            for (uint8_t v : out) std::printf("%02x", v);
            std::printf("\n");
        }
    try {
        (void)composite_texels(source, backdrop, CompositeOp::SrcOver, BlendMode::Normal, 1.5f);
        return 5; // (an opacity above 1 must throw)
    } catch (const Error&) {
    }
    return 0;
}
