// Compiled by tests/test_turbulence_cpu.py: the C++ mirror's turbulence interface against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int turbulence_of(contrast_renderer::Renderer& renderer, contrast_renderer::Frame& frame) {
    using namespace contrast_renderer;
    Turbulence clouds;
    clouds.base_frequency = {0.01f, 0.02f}, clouds.octaves = 6, clouds.seed = 42, clouds.kind = TurbulenceKind::FractalNoise, clouds.stitch = true, clouds.offset = {128.0f, -64.0f};
    Image sky = Image::turbulence(renderer, 256, 128, clouds);
    Turbulence grain;
    grain.base_frequency = {0.8f, 0.8f}, grain.opaque = true;
    Image rough = Image::turbulence(renderer, 256, 128, grain).blur(1.0f, -1.0f, BlurEdge::Repeat).diffuse_lighting(DistantLight{225.0f, 45.0f}, 3.0f);
    rough.generate_mipmaps();
    frame.load_image(sky);
    const std::vector<uint8_t> host = turbulence_texels(4, 2, clouds);
    const TurbulenceTables tables = turbulence_tables(clouds.seed);
    static_assert(CRH_TURBULENCE_TURBULENCE == 1 && CRH_MAX_TURBULENCE_OCTAVES == 12 && sizeof(crh_turbulence) == 9 * 4, "the layout of crh_turbulence");
    return (int)(host.size() + tables.lattice[0] + sky.width() + rough.levels());
}

int main() { return 0; }
