// csrc/api_internal.hpp — the interface between the host translation units (api.hip, image.hip, comm.hip), as launch.hpp is the interface
// to the kernels. Included by the callers AND by the file that defines each of these, so that the compiler checks every definition against
// its declaration. Nothing of crh_renderer, crh_frame or crh_scene is here: what needs more of them than this belongs in api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/contrast_hip.h"
#include "last_error.hpp"
#include "raster_params.hpp"

// The texels of a crh_image on the device, shared by the image and by every paint table that names it (crh_scene_set_paints_with_images):
// freed with the last of them, so that no kernel of a pass reads an image its caller has destroyed.
// Its mipmaps (crh_image_generate_mipmaps) are one more allocation of the same object — the level table at its head, the levels >= 1 behind it —
// so a table keeps them alive exactly as it keeps level 0.
struct ImagePixels {
    void* p = nullptr;
    void* chain = nullptr;               // [kImageLevelTableWords | level 1 | level 2 | ...] 32-bit words, or nullptr: one level
    std::vector<crh::ImageLevel> levels; // the table as the host wrote it (empty: one level)
    ~ImagePixels() {
        if (p) (void)hipFree(p);
        if (chain) (void)hipFree(chain);
    }
};
struct crh_image {
    crh_renderer* renderer = nullptr;
    uint32_t width = 0, height = 0;
    std::shared_ptr<ImagePixels> pixels;
};

namespace crh {
inline bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
#define HIP_TRY(expr)                                         \
    do {                                                      \
        if (!crh::hip_ok((expr), #expr)) return CRH_ERR_HIP; \
    } while (0)

// image.hip
constexpr uint32_t kMaxImageSize = 16384;
crh_status new_image(crh_renderer* r, uint32_t width, uint32_t height, crh_image** out); // the texels' hipMalloc, on the current device
// api.hip: what image.hip needs of a renderer (its device: crh_internal_renderer_device below)
hipStream_t renderer_stream(crh_renderer* r); // the raster kernel's, and the copies'
hipError_t renderer_sync(crh_renderer* r);    // waits for every stream
} // namespace crh

// api.hip: the accessors comm.hip (the multi-GPU exchange) reads frames through; not part of the public header
extern "C" {
crh_status crh_internal_frame_geometry(crh_frame* f, uint32_t* width, uint32_t* height, uint32_t* format, int* device);
crh_status crh_internal_frame_info(crh_frame* f, void** rgba8, uint32_t* width, uint32_t* height, int* device);
crh_status crh_internal_frame_touched(crh_frame* f, void* stream, int written);
crh_status crh_internal_frame_order(crh_frame* f, void* stream, int will_write);
crh_status crh_internal_frame_slab(crh_frame* f, uint32_t* row_begin, uint32_t* row_end);
crh_status crh_internal_frame_tile_counts(crh_frame* f, const uint32_t** counts, uint32_t* n_tiles, uint32_t* first_tile, uint32_t* end_tile);
int crh_internal_renderer_device(crh_renderer* r);
int crh_internal_frame_blends_over(crh_frame* f);
}
