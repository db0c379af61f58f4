// The f64 compilation's side of f32_bridge.hpp (included by render.hip proper): the flat arrays, converted field by
// field by host/f32_layout.hpp, handed to the f32 compilation.
#include "../host/f32_layout.hpp"

namespace rtx {

static rtx_status upload_as_f32(const FlatScene& fs, void** device_scene) {
  std::vector<unsigned char> img[RTX32_N_ARRAYS];
  RtxF32Blobs b;
  if (!f32_images(fs, img, &b)) { set_error("rtx_scene_upload_f32: a layout descriptor of f32_layout.hpp does not match its struct"); return RTX_EINVAL; }
  return rtx_f32_upload(&b, device_scene);
}

}  // namespace rtx

void rtx_f32_set_error(const char* msg) { rtx::set_error(msg); }
