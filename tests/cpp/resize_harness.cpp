// Compiled by tests/test_resize_cpu.py: the C++ mirror's resize interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int resize_of(contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    Image big = Image::from_frame(frame);
    Image display = big.resize(big.width() / 2u, big.height() / 2u);                                        // a 2x supersampled frame down to the display's size
    Image soft = big.resize(big.width() / 2u, big.height() / 2u, ResizeFilter::Box).blur(2.0f).resize(big.width(), big.height(), ResizeFilter::Triangle); // the half-resolution blur
    Image thumbnail = big.resize(37, 21, ResizeFilter::Mitchell);
    thumbnail.generate_mipmaps();
    frame.load_image(soft);
    const std::vector<uint8_t> texels(4 * 2 * 4, 0xC0);
    const std::vector<uint8_t> host = resize_texels(4, 2, texels, 7, 3, ResizeFilter::CatmullRom);
    const ResizeTaps taps = resize_taps(4, 7);
    static_assert(CRH_RESIZE_BOX == 0 && CRH_RESIZE_TRIANGLE == 1 && CRH_RESIZE_CATMULL_ROM == 2 && CRH_RESIZE_MITCHELL == 3 && CRH_RESIZE_LANCZOS3 == 4 && CRH_MAX_RESIZE_TAPS == 512u,
                  "the filters and the cap");
    return (int)(host.size() + taps.first.size() + taps.count.size() + taps.taps.size() + display.width() + display.origin()[0] + thumbnail.levels());
}

int main() { return 0; }
