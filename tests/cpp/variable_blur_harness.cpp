// Compiled and run by tests/test_variable_blur_cpu.py: the C++ mirror's variable blur against the C ABI. main() reads a width x height
// source and a mask of the same size, RGBA8 each, from the file argv[1] (argv[2], argv[3] = the size) and prints one line of hex bytes of
// variable_blur_texels per edge, x from 0 to 2.5 and y from 4 to 0 over the mask's red channel, then the sigmas of code 100, host only:
// no device is touched. device_side() is only compiled.
#include <contrast_renderer.hpp>

#include <cstdio>
#include <cstdlib>

int device_side(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    const uint8_t ramp[2 * 2 * 4] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 255, 0, 0, 0, 255};
    Image mask(renderer, 2, 2, ramp);
    Image backdrop = Image::from_frame(frame, 0, 0, 2u, 2u);
    VariableBlur how;
    how.sigma_x = {0.0f, 24.0f}, how.sigma_y = {0.0f, 24.0f};
    Image soft = backdrop.variable_blur(mask, how);
    frame.load_image(soft);
    static_assert(sizeof(crh_variable_blur) == 24, "crh_variable_blur is four floats and two 32-bit words");
    return (int)(soft.origin()[0] + soft.width());
}

int main(int argc, char** argv) {
    using namespace contrast_renderer;
    if (argc != 4) return 2;
    std::FILE* file = std::fopen(argv[1], "rb");
    if (!file) return 3;
    std::vector<uint8_t> bytes;
    for (int c; (c = std::fgetc(file)) != EOF;) bytes.push_back((uint8_t)c);
    std::fclose(file);
    const uint32_t width = (uint32_t)std::atol(argv[2]), height = (uint32_t)std::atol(argv[3]);
    const size_t size = (size_t)width * height * 4u;
    if (bytes.size() != 2u * size) return 4;
    const std::vector<uint8_t> texels(bytes.begin(), bytes.begin() + (long)size), mask(bytes.begin() + (long)size, bytes.end());
    VariableBlur how;
    how.sigma_x = {0.0f, 2.5f}, how.sigma_y = {4.0f, 0.0f}, how.channel = Channel::R;
    const BlurEdge edges[4] = {BlurEdge::Transparent, BlurEdge::Pad, BlurEdge::Repeat, BlurEdge::Reflect};
    for (BlurEdge edge : edges) {
        how.edge = edge;
        variable_blur_validate(how);
        for (uint8_t v : variable_blur_texels(width, height, texels, mask, how)) std::printf("%02x", v);
        std::printf("\n");
    }
    const std::array<float, 2> sigma = variable_blur_sigma(how, 100u);
    std::printf("%.9g %.9g\n", (double)sigma[0], (double)sigma[1]);
    try {
        how.sigma_x[1] = 65.0f;
        variable_blur_validate(how);
        return 5; // (a sigma above the limit must throw)
    } catch (const Error&) {
    }
    try {
        how.sigma_x[1] = 1.0f;
        (void)variable_blur_sigma(how, 256u);
        return 6; // (a code above 255 must throw)
    } catch (const Error&) {
    }
    return 0;
}
