// Compiled by tests/test_paints_cpu.py: the C++ mirror's paint interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int paints_of(contrast_renderer::Renderer& renderer, contrast_renderer::Scene& scene, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const Paint linear = Paint::linear({0.0f, 0.0f}, {1.0f, 0.5f}, {{0.0f, {1.0f, 0.0f, 0.0f, 1.0f}}, {1.0f, {0.0f, 0.0f, 1.0f, 0.5f}}}, Spread::Reflect);
    const Paint radial = Paint::radial({0.25f, 0.25f}, 0.75f, {{0.5f, {1.0f, 1.0f, 1.0f, 1.0f}}});
    linear.validate();
    scene.set_paints({linear, radial}, {0, -1, 1});
    RenderPass pass(renderer, frame);
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, white[4] = {1, 1, 1, 1};
    const uint32_t solid = pass.push_instance(identity, white), painted = pass.push_instance(identity, white, radial);
    pass.render(scene, 0, painted, painted + 1, RenderOperation::Stencil);
    pass.render(scene, 0, painted, painted + 1, RenderOperation::Color);
    pass.submit();
    RenderPass plain(renderer, frame); // a pass without paints removes the table the pass before installed
    const uint32_t again = plain.push_instance(identity, white);
    plain.render(scene, 0, again, again + 1, RenderOperation::Stencil);
    plain.render(scene, 0, again, again + 1, RenderOperation::Color);
    plain.submit();
    scene.set_paints({}, {});
    return (int)(solid + linear.to_c().n_stops);
}

int main() { return 0; }
