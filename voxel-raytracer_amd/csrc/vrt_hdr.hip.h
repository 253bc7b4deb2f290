// vrt_hdr.hip.h -- the two pieces of HDR arithmetic every HDR kernel shares (include/vrt.h vrt_accum_keep_hdr points 1 and 4): the
// clamp of a float colour and the tone map of a float mean. One definition, so the accumulation's resolve (vrt_accum_hdr.hip.h), the
// ray batches (vrt_rays.hip.h) and the HDR display pass (vrt_denoise.hip.h) evaluate the same expressions.
#pragma once
#include "vrt_common.hip.h"
#include "vrt_accum.h"

namespace vrt {
namespace accum {

// h(c) of include/vrt.h: [0, kHdrMax], NaN -> +0 (0 < NaN is false); unorm8(hdr_value(c)) == unorm8(c) for every float
VRT_DEV float hdr_value(float c) { return fmin_c(fmax_c(0.0f, c), kHdrMax); }

// The tone map of include/vrt.h vrt_tonemap on one channel of the mean: every operation rounded on its own
VRT_DEV float tone_map(float x, int op, float e) {
    const float xe = e * x;
    return op == 1 ? xe / (1.0f + xe) : xe;   // VRT_TONEMAP_REINHARD : _CLAMP (unorm8 clamps)
}

}  // namespace accum
}  // namespace vrt
