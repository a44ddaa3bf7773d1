// tests/cpp/blend_harness.cpp — Configuration::blending through the C++ host mirror (include/contrast_renderer.hpp). Prints the C struct the
// mirror builds for a few states, one line each, and the status Renderer's constructor throws for states the C ABI refuses (validated
// before any device is touched, so this runs without a GPU). tests/test_blending_cpu.py compares the lines with the Python mirror.
//   usage: blend_harness
#include <cstdio>

#include "contrast_renderer.hpp"

using namespace contrast_renderer;

static void print(const char* name, const crh_color_target_state& c) {
    std::printf("%s %u %u %u %u %u %u %u %u %.9g %.9g %.9g %.9g\n", name, c.blend_enabled, c.color.src_factor, c.color.dst_factor, c.color.operation, c.alpha.src_factor,
                c.alpha.dst_factor, c.alpha.operation, c.write_mask, (double)c.constant[0], (double)c.constant[1], (double)c.constant[2], (double)c.constant[3]);
}

static int refused(const ColorTargetState& state) {
    Configuration config{1, 4, 4, 0};
    config.blending = state;
    try {
        Renderer renderer(0, config);
    } catch (const Error& e) {
        return (int)e.status;
    }
    return 0;
}

int main() {
    print("premultiplied", ColorTargetState{BlendState::PREMULTIPLIED_ALPHA_BLENDING, ColorWrites::ALL, {0.0f, 0.0f, 0.0f, 0.0f}}.to_c());
    print("alpha", ColorTargetState{BlendState::ALPHA_BLENDING, ColorWrites::RED | ColorWrites::ALPHA, {0.25f, 0.5f, 0.75f, 1.0f}}.to_c());
    print("replace", ColorTargetState{}.to_c());
    const BlendComponent add{BlendFactor::One, BlendFactor::One, BlendOperation::Add};
    const BlendComponent constant{BlendFactor::Constant, BlendFactor::OneMinusConstant, BlendOperation::ReverseSubtract};
    print("mixed", ColorTargetState{BlendState{add, constant}, ColorWrites::COLOR, {0.125f, 0.0f, 1.0f, 0.5f}}.to_c());
    // Configuration keeps its positional initialisers; blending is the last member and defaults to "over"
    const Configuration plain{4, 4, 4, 1};
    std::printf("plain %d\n", plain.blending.has_value() ? 1 : 0);
    // refused before any device is touched
    const BlendComponent min_scaled{BlendFactor::SrcAlpha, BlendFactor::One, BlendOperation::Min};
    const BlendComponent dual{BlendFactor::Src1, BlendFactor::Zero, BlendOperation::Add};
    std::printf("refused %d %d %d\n", refused(ColorTargetState{BlendState{min_scaled, add}, ColorWrites::ALL, {}}),
                refused(ColorTargetState{BlendState{add, dual}, ColorWrites::ALL, {}}), refused(ColorTargetState{BlendState{add, add}, 16u, {}}));
    return 0;
}
