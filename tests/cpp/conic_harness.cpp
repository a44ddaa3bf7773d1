// Compiled by tests/test_conic_cpu.py: Paint::conic of the C++ mirror against the C ABI (nothing runs).
#include <contrast_renderer.hpp>

int conic_of(contrast_renderer::Scene& scene) {
    using namespace contrast_renderer;
    const std::vector<GradientStop> stops = {{0.0f, {1.0f, 0.0f, 0.0f, 1.0f}}, {0.5f, {0.0f, 1.0f, 0.0f, 1.0f}}, {1.0f, {0.0f, 0.0f, 1.0f, 0.5f}}};
    const Paint wheel = Paint::conic({0.0f, 0.0f}, 0.0f, 6.2831855f, stops);
    const Paint wedge = Paint::conic({0.25f, -0.5f}, 1.5f, 0.5f, stops, Spread::Reflect); // clockwise
    const Paint radial = Paint::radial({0.25f, 0.25f}, 0.75f, stops);
    wheel.validate();
    wedge.validate();
    static_assert(CRH_PAINT_CONIC == 4 && sizeof(crh_paint) == 188, "the conic kind lives in crh_paint as it is");
    scene.set_paints({wheel, radial, wedge}, {0, -1, 2, 1});
    return (int)(wheel.to_c().kind + wedge.to_c().n_stops);
}

int main() { return 0; }
