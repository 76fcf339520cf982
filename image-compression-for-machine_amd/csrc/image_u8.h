// The 8-bit value of an f32 sample, gfx950: one statement for every kernel that needs it (imageio.hip writes the bytes
// of a decoded image with it; qstep.hip derives a training crop's quality map from the bytes the codec would see).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace icm {

// clamp(0, 1).mul(255).to(uint8): one f32 multiplication, correctly rounded on every target, then truncation.  Every
// value fl32(k / 255) comes back as k.  NaN is unspecified.
__device__ __forceinline__ uint32_t quantise_u8(float v) {
  return (uint32_t)(int)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

}  // namespace icm
