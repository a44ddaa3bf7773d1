// Compiled by tests/test_distance_cpu.py: the C++ mirror's distance-field interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int distance_of(contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    Image layer = Image::from_frame(frame);
    Distance outline;
    outline.spread = 8;
    Image field = layer.distance_field(outline);
    Distance chisel;
    chisel.spread = 12, chisel.mode = DistanceMode::Inside, chisel.channel = Channel::A, chisel.threshold = 200, chisel.edge = BlurEdge::Pad;
    Image height = layer.distance_field(chisel).blur(1.0f);
    height.generate_mipmaps();
    frame.load_image(height);
    const std::vector<uint8_t> texels(4 * 2 * 4, 0xC0);
    const std::vector<uint8_t> host = distance_texels(4, 2, texels, outline);
    const std::array<uint32_t, 2> size = distance_size(4, 2, outline);
    const uint32_t code = distance_code(outline, 5);
    static_assert(CRH_DISTANCE_OUTSIDE == 0 && CRH_DISTANCE_INSIDE == 1 && CRH_MAX_DISTANCE_SPREAD == 255u && sizeof(crh_distance) == 5 * 4, "the layout of crh_distance");
    return (int)(host.size() + size[0] + code + field.width() + field.origin()[0] + height.levels());
}

int main() { return 0; }
