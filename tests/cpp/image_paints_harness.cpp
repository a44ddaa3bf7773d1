// Compiled by tests/test_image_paints_cpu.py: the C++ mirror's image paint interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int image_paints_of(contrast_renderer::Renderer& renderer, contrast_renderer::Scene& scene, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image image(renderer, 2, 2, texels);
    Image snapshot = Image::from_frame(frame);
    const ImagePaint nearest(image, {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f}, Filter::Nearest, Spread::Repeat, Spread::Reflect);
    const ImagePaint fitted = ImagePaint::fit(snapshot, {-1.0f, -1.0f}, {1.0f, 1.0f});
    nearest.validate();
    const Paint radial = Paint::radial({0.25f, 0.25f}, 0.75f, {{0.5f, {1.0f, 1.0f, 1.0f, 1.0f}}});
    scene.set_paints({radial}, {nearest, fitted}, {0, -1, 1, 2});
    RenderPass pass(renderer, frame);
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, white[4] = {1, 1, 1, 1};
    const uint32_t solid = pass.push_instance(identity, white), textured = pass.push_instance(identity, white, fitted), graded = pass.push_instance(identity, white, radial);
    for (uint32_t i : {solid, textured, graded}) {
        pass.render(scene, 0, i, i + 1, RenderOperation::Stencil);
        pass.render(scene, 0, i, i + 1, RenderOperation::Color);
    }
    pass.submit();
    scene.set_paints({}, {});
    return (int)(image.width() + snapshot.height() + fitted.to_c().filter);
}

int main() { return 0; }
