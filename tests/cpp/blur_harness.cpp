// Compiled by tests/test_blur_cpu.py: the C++ mirror's blur interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int blur_of(contrast_renderer::Renderer& renderer, contrast_renderer::Scene& scene, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image image(renderer, 2, 2, texels);
    Image soft = image.blur(1.5f);
    Image wide = image.blur(4.0f, 0.0f, BlurEdge::Reflect);
    Image shadow = Image::from_frame(frame).blur(3.0f, -1.0f, BlurEdge::Transparent);
    shadow.generate_mipmaps();
    const std::vector<uint32_t> taps = blur_taps(2.0f);
    const std::array<uint32_t, 2> origin = shadow.origin();
    static_assert((uint32_t)BlurEdge::Transparent == 0u && (uint32_t)BlurEdge::Pad == 1u && (uint32_t)BlurEdge::Repeat == 2u && (uint32_t)BlurEdge::Reflect == 3u, "BlurEdge mirrors crh_blur_edge");
    static_assert(CRH_MAX_BLUR_RADIUS == 192u && CRH_MAX_BLUR_SIGMA == 64.0f, "the limits of crh_image_blur");
    const ImagePaint paint(shadow, {1.0f, 0.0f, (float)origin[0], 0.0f, 1.0f, (float)origin[1]}, Filter::Linear);
    scene.set_paints({}, {paint}, {0});
    Image moved = std::move(soft);
    return (int)(taps.size() + origin[0] + origin[1] + wide.origin()[0] + moved.width() + shadow.levels());
}

int main() { return 0; }
