// Compiled by tests/test_displace_cpu.py: the C++ mirror's displacement interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int displace_of(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    Turbulence waves;
    waves.base_frequency = {0.01f, 0.02f}, waves.octaves = 2, waves.opaque = true;
    Image map = Image::turbulence(renderer, 256, 128, waves);
    Image layer = Image::from_frame(frame);
    Displace haze;
    haze.scale = {32.0f, 32.0f}, haze.x_channel = Channel::R, haze.y_channel = Channel::G;
    Image wobbly = layer.displace(map, haze);
    Displace torn;
    torn.scale = {0.0f, -12.5f}, torn.y_channel = Channel::B, torn.filter = Filter::Nearest, torn.edge = BlurEdge::Reflect;
    Image edges = wobbly.displace(map, torn).blur(1.0f);
    edges.generate_mipmaps();
    frame.load_image(wobbly);
    const std::vector<uint8_t> texels(4 * 2 * 4, 0x40), codes(4 * 2 * 4, 0x80);
    const std::vector<uint8_t> host = displace_texels(4, 2, texels, codes, haze);
    const std::array<int32_t, 2> q = displace_offset(haze, 255, 0);
    static_assert(CRH_CHANNEL_R == 0 && CRH_CHANNEL_A == 3 && sizeof(crh_displace) == 6 * 4, "the layout of crh_displace");
    return (int)(host.size() + (size_t)q[0] + wobbly.width() + edges.levels());
}

int main() { return 0; }
