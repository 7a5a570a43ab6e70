// rt_accum.h — the per-pixel arithmetic of a frame's sample sums, shared by the trace kernel's
// resolve, the fold kernel of rt_accumulate (accum_fold_kernel, rt_kernels.hip) and the host test
// (tests/accum_host.cpp): one definition of clamp1, mean and pack, so that a frame folded one
// sample per call performs the float32 operations of the frame traced in one call.
// A frame of n samples is the in-order sum ((0 + c_0) + c_1) + ... of its samples' radiance c_k,
// kept twice: clamped per sample (clamp1, raytracer.cu:37-40) for RGBA8, raw for `radiance`; then
// the mean (x 2^-k for n = 2^k, x / n otherwise) and Color's truncation to bytes.
#pragma once

#include <stdint.h>

#include "rt_math.h"

namespace rta {

using rtm::V4;

// raytracer.cu:37-40: each channel above 1 becomes 1 (everything else, NaN included, passes)
RT_HD V4 clamp1(V4 v) {
    return rtm::v4(v.x > 1.0f ? 1.0f : v.x, v.y > 1.0f ? 1.0f : v.y, v.z > 1.0f ? 1.0f : v.z, v.w > 1.0f ? 1.0f : v.w);
}

// 2^-k when n = 2^k (x * 2^-k is the same correctly rounded value as x / 2^k), else 0: divide
RT_HD float mean_recip(int n) { return (n & (n - 1)) == 0 ? 1.0f / (float)n : 0.0f; }
// mean = sum / n (raytracer.cu's per-sample colour, build-defined spp average)
RT_HD float mean(float x, float recip, float n) { return recip != 0.0f ? x * recip : x / n; }
RT_HD V4 mean4(V4 s, float recip, float n) {
    return rtm::v4(mean(s.x, recip, n), mean(s.y, recip, n), mean(s.z, recip, n), mean(s.w, recip, n));
}

// Color(float r, g, b, a) truncation to uint8 and to_encoding (color.h:41-42, color.cu:23-26)
RT_HD uint32_t pack(V4 m) {
    return ((uint32_t)(uint8_t)((float)255 * m.x) << 24) + ((uint32_t)(uint8_t)((float)255 * m.y) << 16) +
           ((uint32_t)(uint8_t)((float)255 * m.z) << 8) + (uint32_t)(uint8_t)((float)255 * m.w);
}

// One more sample r into a pixel's running sums: the raw sum and the sum of clamped samples.
RT_HD void fold(V4& sum_r, V4& sum_c, V4 r) {
    const V4 c = clamp1(r);
    sum_r = rtm::v4(sum_r.x + r.x, sum_r.y + r.y, sum_r.z + r.z, sum_r.w + r.w);
    sum_c = rtm::v4(sum_c.x + c.x, sum_c.y + c.y, sum_c.z + c.z, sum_c.w + c.w);
}

// The frame of n samples from the sums.
RT_HD uint32_t resolve_rgba(V4 sum_c, int n) { return pack(mean4(sum_c, mean_recip(n), (float)n)); }
RT_HD V4 resolve_radiance(V4 sum_r, int n) { return mean4(sum_r, mean_recip(n), (float)n); }

}  // namespace rta
