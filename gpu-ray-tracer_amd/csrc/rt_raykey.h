// rt_raykey.h — the coherence key of a ray query (rt_query, RT_QUERY_ORDER_SORTED): one 64-bit
// key per ray as traced, a pure function of the ray and a box, so that rays sorted by key travel
// in waves whose lanes visit the same subtrees.  Host and device evaluate the same code and
// agree bit for bit under the build's float rules (-ffp-contract=off, correctly rounded
// division): the float steps are + - x /, comparisons and float -> int conversion only; the
// rest is integer bit work.  No HIP call; tests/query_order_host.cpp runs it on the host.
//
//   bit 63                     the ray is rejected (ray_traceable false): it sorts last
//   bits [32, 32 + 3 B)        the origin's cell in the box, B = RAYKEY_ORIGIN_BITS per axis,
//                              Morton-interleaved (x lowest); origins outside clamp to the edge cells
//   bits [0, 32)               the unit direction on the octahedral square, 16 bits per axis,
//                              Morton-interleaved
// A rejected ray's key is RAYKEY_REJECTED: bit 63 and bit RAYKEY_BITS - 1, the bit above the
// origin field, so a sort over the low RAYKEY_BITS bits alone already puts it last.
// With one shared origin (camera rays) the order is a z-order over the screen; with scattered
// origins space comes first and direction second.
#pragma once

#include "rt_math.h"

// Measured choice (tools/query_bench.py cases c and d at 4, 6, 8 and 10): 4 was
// the only rung at which the ambient-occlusion fans gained from the sort (1.18 ms against 1.99
// in caller order; 2.30 / 2.48 / 2.44 at 6 / 8 / 10), and its shorter key sorts fastest.
#ifndef RAYKEY_ORIGIN_BITS
#define RAYKEY_ORIGIN_BITS 4
#endif

namespace rtk {

using rtm::Ray;
using rtm::V3;

constexpr int ORIGIN_BITS = RAYKEY_ORIGIN_BITS;
static_assert(ORIGIN_BITS >= 1 && ORIGIN_BITS <= 10, "3 B origin bits + 32 direction bits + the rejected bit fit 63 bits");
constexpr int DIR_BITS = 16;
constexpr int RAYKEY_BITS = 2 * DIR_BITS + 3 * ORIGIN_BITS + 1;   // the bits a sort has to look at
constexpr uint64_t RAYKEY_REJECTED = (1ull << 63) | (1ull << (RAYKEY_BITS - 1));

struct KeyBox { V3 mn, mx; };   // the quantisation box of the origins (rt_query_last's bounds6)

RT_HD bool finite3(V3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// query_kernel's test of a ray as traced (make_ray's or camera_at's result): every component
// finite and the direction not the zero vector (rmath::Ray: a direction shorter than 1e-5, or too
// long for its length to be finite, normalises to zero).  False: the ray reports a miss and
// takes no part in its wave.
RT_HD bool ray_traceable(const Ray& r) {
    return finite3(r.o) && finite3(r.d) && (r.d.x != 0.0f || r.d.y != 0.0f || r.d.z != 0.0f);
}
// The ray a caller's origin / direction is traced as, and whether it is traced at all.
RT_HD bool caller_ray(V3 o, V3 d, Ray& r) {
    r = rtm::make_ray(o, d);                                   // Ray ctor (geometry.h:216)
    return finite3(d) && ray_traceable(r);
}

// x in [lo, lo + ext) -> its cell of 2^bits, clamped to the edge cells (a degenerate or
// non-finite extent: cell 0)
RT_HD uint32_t quantize(float x, float lo, float ext, int bits) {
    const float cells = (float)(1u << bits);
    if (!(ext > 0.0f)) return 0u;
    const float f = (x - lo) / ext * cells;
    if (!(f >= 0.0f)) return 0u;
    if (f >= cells) return (1u << bits) - 1u;
    return (uint32_t)(int)f;
}
RT_HD uint64_t spread2(uint64_t v) {                           // bit j (j < 16) -> bit 2j
    v &= 0xffffull;
    v = (v | (v << 8)) & 0x00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0full;
    v = (v | (v << 2)) & 0x33333333ull;
    v = (v | (v << 1)) & 0x55555555ull;
    return v;
}
RT_HD float absf(float x) { return x < 0.0f ? -x : x; }

// Octahedral map of a nonzero direction to [0, 1]^2: project on |x| + |y| + |z| = 1, fold the
// lower half (z < 0) outwards over the diagonals.  Neighbouring directions stay neighbours
// except across the fold's outer edges.
RT_HD void oct_square(V3 d, float& u, float& v) {
    const float s = absf(d.x) + absf(d.y) + absf(d.z);
    float px = d.x / s, py = d.y / s;
    if (d.z < 0.0f) {
        const float fx = 1.0f - absf(py), fy = 1.0f - absf(px);
        px = px < 0.0f ? -fx : fx;
        py = py < 0.0f ? -fy : fy;
    }
    u = px * 0.5f + 0.5f;
    v = py * 0.5f + 0.5f;
}
RT_HD uint32_t dir_code(V3 d) {
    float u, v;
    oct_square(d, u, v);
    return (uint32_t)(spread2(quantize(u, 0.0f, 1.0f, DIR_BITS)) | (spread2(quantize(v, 0.0f, 1.0f, DIR_BITS)) << 1));
}
RT_HD uint64_t origin_code(V3 o, const KeyBox& b) {
    const uint64_t cx = quantize(o.x, b.mn.x, b.mx.x - b.mn.x, ORIGIN_BITS);
    const uint64_t cy = quantize(o.y, b.mn.y, b.mx.y - b.mn.y, ORIGIN_BITS);
    const uint64_t cz = quantize(o.z, b.mn.z, b.mx.z - b.mn.z, ORIGIN_BITS);
    return rtm::spread3(cx) | (rtm::spread3(cy) << 1) | (rtm::spread3(cz) << 2);
}
// ok: the ray is traced (caller_ray's / ray_traceable's result for r)
RT_HD uint64_t ray_key(const Ray& r, bool ok, const KeyBox& b) {
    if (!ok) return RAYKEY_REJECTED;
    return (origin_code(r.o, b) << (2 * DIR_BITS)) | (uint64_t)dir_code(r.d);
}
RT_HD uint64_t ray_key(const Ray& r, const KeyBox& b) { return ray_key(r, ray_traceable(r), b); }

}  // namespace rtk
