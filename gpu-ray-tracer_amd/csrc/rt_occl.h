// rt_occl.h — the per-pixel arithmetic of the ambient-occlusion pass (rt_occlusion), shared by
// occl_surface_kernel / occlusion_kernel / occl_rays_kernel (rt_kernels.hip) and the host test
// (tests/occl_host.cpp): one definition of the surface point, the facing, the tangent frame, the
// raw direction of a sample and the resolve, as rt_accum.h is for rt_accumulate's fold.  Every
// float step below is a single float32 + - x / (the build has no contraction), in the order
// written; host and device agree bit for bit.  The direction table's generation is host only.
// Further down: the interleaved pattern's entry index and the filtered resolve's accept test and
// resolve (occlusion_il_kernel, occl_rays_il_kernel, occl_filter_kernel; tests/occl_filter_host.cpp).
//
//   p  = o + t d                      per component: t x d, then + o  (rtm::at)
//   n  = the hit's normal, each component negated when dot(n, d) > 0 (rtm::dot: ((0 + x x) + y y) + z z)
//   s  = copysignf(1, n.z)
//   a  = -1 / (s + n.z)               (s + n.z) is in [1, 2] or [-2, -1]: n.z = -1 gives a = 1/2, finite
//   b  = (n.x x n.y) x a
//   t1 = (1 + ((s x n.x) x n.x) x a,  s x b,              -(s x n.x))
//   t2 = (b,                          s + (n.y x n.y) x a, -n.y)
//   sample k's raw direction = (x_k t1 + y_k t2) + z_k n, per component ((x_k x t1.c) + (y_k x t2.c)) + z_k x n.c
//   sample k's origin        = p + bias n, per component (bias x n.c) + p.c
//   visibility = 1 - (float)count / (float)n           (correctly rounded division, then the subtraction)
#pragma once

#include <stdint.h>

#include "rt_accum.h"

namespace rto {

using rtm::V3;
using rtm::V4;

constexpr int AO_MAX_SAMPLES = 1024;       // RT_AO_MAX_SAMPLES (rt_amd.h): the direction table's length

struct Frame { V3 p, n, t1, t2; };

RT_HD V3 surface_point(V3 o, V3 d, float t) { return o + t * d; }
RT_HD V3 faced(V3 n, V3 d) { return rtm::dot(n, d) > 0.0f ? rtm::v3(-n.x, -n.y, -n.z) : n; }
RT_HD void tangent_frame(V3 n, V3& t1, V3& t2) {
    const float s = copysignf(1.0f, n.z);
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    t1 = rtm::v3(1.0f + ((s * n.x) * n.x) * a, s * b, -(s * n.x));
    t2 = rtm::v3(b, s + (n.y * n.y) * a, -n.y);
}
RT_HD Frame make_frame(V3 p, V3 n) {
    Frame f;
    f.p = p; f.n = n;
    tangent_frame(n, f.t1, f.t2);
    return f;
}
RT_HD V3 ray_origin(const Frame& f, float bias) { return f.p + bias * f.n; }
RT_HD V3 raw_direction(const Frame& f, V3 dk) { return (dk.x * f.t1 + dk.y * f.t2) + dk.z * f.n; }

RT_HD float visibility(int count, int n) { return 1.0f - (float)count / (float)n; }
// visibility as an opaque grey through Color's truncation (rta::pack)
RT_HD uint32_t grey(float vis) { return rta::pack(rtm::v4(vis, vis, vis, 1.0f)); }

// The interleaved pattern (RT_AO_PATTERN_INTERLEAVED): pixel (x, y) has class c = (x & 3) + 4 (y & 3)
// and its sample k uses table entry 16 k + c; everything after the entry is the shared pattern's.
// Any 4 x 4 window of pixels holds each class once, so after n samples it has used entries
// 0 ... 16 n - 1, each exactly once.
constexpr int AO_CLASSES = 16;
constexpr int AO_INTERLEAVED_MAX_SAMPLES = AO_MAX_SAMPLES / AO_CLASSES;
RT_HD int pixel_class(int x, int y) { return (x & 3) + 4 * (y & 3); }
RT_HD int interleaved_entry(int k, int c) { return AO_CLASSES * k + c; }

// The filtered resolve (rt_occlusion_set_filter): centre C = (pc, nc), tap Q = (pq, nq), both
// surface records.  A tap is accepted when it is live, its normal is within normal_min of the
// centre's and it lies within plane_tol of the centre's tangent plane:
//   dot(nc, nq) >= normal_min   and   |dot(nc, e)| <= plane_tol,   e = pq - pc per component
// (rtm::dot's order, one rounding each; a NaN accepts nothing).  The centre tap itself is accepted
// by the caller without the test.  S: the integer sum of the m accepted taps' counts, n: samples held.
constexpr int AO_FILTER_LO = 2, AO_FILTER_HI = 1;             // taps dx, dy in [-AO_FILTER_LO, AO_FILTER_HI]
RT_HD bool filter_accept(V3 pc, V3 nc, V3 pq, V3 nq, bool live_q, float normal_min, float plane_tol) {
    if (!live_q) return false;
    if (!(rtm::dot(nc, nq) >= normal_min)) return false;
    const V3 e = pq - pc;
    return fabsf(rtm::dot(nc, e)) <= plane_tol;
}
RT_HD float filtered_visibility(int S, int m, int n) { return 1.0f - (float)S / (float)(m * n); }

// History across camera moves (rt_occlusion_set_history): a new pixel with the live record (p, n)
// looks its surface point up in the frame of the previous camera C (DCamera's fields), the
// inverse of camera_at:
//   v  = p - C.pos per component;   a = dot(v, C.f), sx = dot(v, C.r), sy = dot(v, C.u)
//   gx = (C.near_ x sx) / a,  gy = (C.near_ x sy) / a             (no history unless a > 0)
//   cx = gx x C.unit + 0.5f x C.W,  cy = 0.5f x C.H - gy x C.unit
//   fx = floorf(cx + 0.5f), fy = floorf(cy + 0.5f)                (sample 0's ray of pixel x passes through cx = x)
// and the source pixel is ((int)fx, (int)fy) when 0 <= fx < C.W and 0 <= fy < C.H, compared in
// float before any conversion: a NaN rejects.  The caller accepts the source with filter_accept
// (the new pixel is the centre).
template <class CAM>
RT_HD bool reproject(V3 p, const CAM& C, int& qx, int& qy) {
    const V3 v = p - C.pos;
    const float a = rtm::dot(v, C.f), sx = rtm::dot(v, C.r), sy = rtm::dot(v, C.u);
    if (!(a > 0.0f)) return false;
    const float gx = (C.near_ * sx) / a, gy = (C.near_ * sy) / a;
    const float cx = gx * C.unit + 0.5f * C.W, cy = 0.5f * C.H - gy * C.unit;
    const float fx = floorf(cx + 0.5f), fy = floorf(cy + 0.5f);
    if (!(fx >= 0.0f && fx < C.W && fy >= 0.0f && fy < C.H)) return false;
    qx = (int)fx; qy = (int)fy;
    return true;
}
// The seed a pixel takes from its accepted source: c of the source's T = n_h + n samples were
// occluded.  Up to max_history samples are carried as they are; more are scaled down to
// max_history, the count rounded to nearest (int32, truncating divisions; c x max_history < 2^22).
RT_HD void history_seed(int c, int T, int max_history, int& c_h, int& n_h) {
    if (T <= max_history) { c_h = c; n_h = T; }
    else { n_h = max_history; c_h = (c * max_history + T / 2) / T; }
}
// The filtered resolve with per-pixel totals: S as above, N the integer sum of the accepted taps' n_h + n.
RT_HD float filtered_visibility_total(int S, int N) { return 1.0f - (float)S / (float)N; }

// Host only.  Entry k of the direction table: point k of the R2 sequence (rt::spp_offset's constants, in
// double; k = 0 -> the pole) taken to the unit disk by (u, v) -> sqrt(u) (cos 2 pi v, sin 2 pi v)
// and lifted to the hemisphere, z = sqrt(max(0, 1 - x^2 - y^2)): cosine-weighted.  Double
// throughout, each component rounded to float32 once.
inline void ao_direction(int k, float out3[3]) {
    const double a1 = 0.7548776662466927, a2 = 0.5698402909980532;
    double u = (double)k * a1, v = (double)k * a2;
    u -= floor(u); v -= floor(v);
    const double r = sqrt(u), phi = 6.283185307179586476925286766559 * v;
    const double x = r * cos(phi), y = r * sin(phi);
    const double zz = 1.0 - x * x - y * y;
    out3[0] = (float)x; out3[1] = (float)y; out3[2] = (float)sqrt(zz > 0.0 ? zz : 0.0);
}

}  // namespace rto
