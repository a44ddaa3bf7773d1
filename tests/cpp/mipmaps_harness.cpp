// Compiled by tests/test_mipmaps_cpu.py: the C++ mirror's mipmap interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int mipmaps_of(contrast_renderer::Renderer& renderer, contrast_renderer::Scene& scene, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image image(renderer, 2, 2, texels);
    image.generate_mipmaps();
    Image snapshot = Image::from_frame(frame);
    snapshot.generate_mipmaps();
    uint32_t w = 0, h = 0;
    const std::vector<uint8_t> last = image.download_level(image.levels() - 1, &w, &h);
    const ImagePaint trilinear(image, {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f}, Filter::LinearMipmap, Spread::Repeat, Spread::Reflect);
    const ImagePaint nearest = ImagePaint::fit(snapshot, {-1.0f, -1.0f}, {1.0f, 1.0f}, Filter::NearestMipmap);
    trilinear.validate();
    static_assert((uint32_t)Filter::NearestMipmap == 0x100u && (uint32_t)Filter::LinearMipmap == 0x101u && CRH_FILTER_MIPMAP == 0x100, "the flag is OR-ed onto the base filter");
    static_assert(sizeof(crh_image_paint) == 48, "crh_image_paint keeps its size");
    scene.set_paints({}, {trilinear, nearest}, {0, 1});
    return (int)(last.size() + w + h + snapshot.levels() + trilinear.to_c().filter);
}

int main() { return 0; }
