// pixel.h — the two pixel rules between a uint8 image and the unit-range fp32 tensor, each written once (kernels_layout.hip, colorfix.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace {

// img2tensor(...) / 255. (basicsr/utils/img_util.py:9-35, inference_femasr.py:55): one IEEE division
__device__ __forceinline__ float pixel_byte_to_unit(unsigned char b) { return (float)b / 255.0f; }

// tensor2img (img_util.py:38-94): clamp to [0,1], then NaN -> 0 (a NaN passes both comparisons of the clamp), (v * 255).round(), half to even
__device__ __forceinline__ unsigned char pixel_unit_to_byte(float v)
{
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    if (!(v == v)) v = 0.f;
    return (unsigned char)rintf(v * 255.0f);
}

}  // namespace
