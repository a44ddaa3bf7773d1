// Compiled by tests/test_lighting_cpu.py: the C++ mirror's lighting interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int lighting_of(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image image(renderer, 2, 2, texels);
    Image lit = image.lighting(DistantLight{225.0f, 45.0f});
    Lighting gloss;
    gloss.op = LightingOp::Specular, gloss.surface_scale = 4.0f, gloss.constant = 1.5f, gloss.specular_exponent = 20.0f, gloss.color = {1.0f, 0.9f, 0.8f}, gloss.edge = BlurEdge::Reflect;
    Image shine = image.lighting(PointLight{1.0f, 1.0f, 8.0f}, gloss);
    SpotLight lamp;
    lamp.position = {0.0f, 0.0f, 10.0f}, lamp.points_at = {1.0f, 1.0f, 0.0f}, lamp.exponent = 2.0f, lamp.cone_angle = 30.0f;
    Image bevel = Image::from_frame(frame).blur(2.0f).specular_lighting(lamp, 5.0f, 1.0f, 16.0f);
    Image shade = bevel.diffuse_lighting(DistantLight{}, 2.0f, 0.8f, {1.0f, 1.0f, 1.0f}, BlurEdge::Transparent);
    shade.generate_mipmaps();
    frame.load_image(shade.lighting(lamp));
    const std::vector<uint8_t> host = lighting_texels(2, 2, std::vector<uint8_t>(texels, texels + 16), lamp, gloss);
    const std::vector<uint8_t> plain = lighting_texels(2, 2, std::vector<uint8_t>(texels, texels + 16), DistantLight{0.0f, 90.0f});
    static_assert(CRH_LIGHTING_SPECULAR == 1 && CRH_LIGHT_SPOT == 2 && sizeof(crh_lighting) == 19 * 4, "the layout of crh_lighting");
    return (int)(host.size() + plain.size() + lit.width() + shine.origin()[0] + bevel.height() + shade.levels());
}

int main() { return 0; }
