// Compiled by tests/test_morphology_cpu.py: the C++ mirror's morphology interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int morphology_of(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image image(renderer, 2, 2, texels);
    Image grown = image.dilate(2);
    Image choked = image.erode(1, 0, BlurEdge::Reflect);
    Image wide = image.morphology(MorphologyOp::Dilate, 192, 0, BlurEdge::Pad);
    Image outline = Image::from_frame(frame).dilate(3, 3, BlurEdge::Transparent);
    outline.generate_mipmaps();
    const ColorMatrixValues black = ColorMatrix::flood(0, 0, 0, 1);
    Image stroked = Image::from_frame(frame).composite(outline.color_filter(&black), CompositeOp::DstOver, BlendMode::Normal, 1.0f, {-(int32_t)outline.origin()[0], -(int32_t)outline.origin()[1]});
    frame.load_image(stroked);
    const std::array<uint32_t, 2> size = morphology_size(2, 2, MorphologyOp::Dilate, 2, 2);
    const std::vector<uint8_t> host = morphology_texels(2, 2, std::vector<uint8_t>(texels, texels + 16), MorphologyOp::Erode, 1, 1, BlurEdge::Repeat);
    static_assert((uint32_t)MorphologyOp::Erode == 0u && (uint32_t)MorphologyOp::Dilate == 1u, "MorphologyOp mirrors crh_morphology_op");
    static_assert(CRH_MAX_MORPHOLOGY_RADIUS == 192u, "the limit of crh_image_morphology");
    return (int)(size[0] + host.size() + grown.origin()[0] + choked.origin()[1] + wide.width() + outline.levels());
}

int main() { return 0; }
