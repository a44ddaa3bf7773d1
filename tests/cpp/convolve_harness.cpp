// Compiled by tests/test_convolve_cpu.py: the C++ mirror's convolution interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int convolve_of(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t texels[2 * 2 * 4] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 128, 128, 128, 128};
    Image image(renderer, 2, 2, texels);
    Image same = image.convolve(ConvolveKernel::identity());
    Image sharp = image.convolve(ConvolveKernel::sharpen(0.5f), BlurEdge::Reflect, true);
    Image mean = image.convolve(ConvolveKernel::box(15), BlurEdge::Repeat);
    ConvolveKernel edges = ConvolveKernel::sobel_x();
    edges.bias = 0.5f, edges.target_x = 0, edges.target_y = 2;
    Image outline = Image::from_frame(frame).convolve(edges, BlurEdge::Transparent, true);
    outline.generate_mipmaps();
    Image again = outline.convolve(ConvolveKernel::laplacian()).convolve(ConvolveKernel::emboss()).convolve(ConvolveKernel::sobel_y());
    frame.load_image(again);
    const std::vector<int32_t> k = convolve_coefficients(ConvolveKernel::box(3));
    const std::vector<uint8_t> host = convolve_texels(2, 2, std::vector<uint8_t>(texels, texels + 16), ConvolveKernel(2, 1, {1.0f, 3.0f}, 4.0f), BlurEdge::Pad, false);
    static_assert(CRH_MAX_CONVOLVE_ORDER == 15u && CRH_CONVOLVE_MAX_GAIN == 64.0f, "the limits of crh_image_convolve");
    return (int)(k.size() + host.size() + same.width() + sharp.origin()[0] + mean.height() + outline.levels());
}

int main() { return 0; }
