// Host check of the axis-specialised leaf step (gpu-ray-tracer_amd/csrc/rt_math.h:
// axis_plane_pass<AX>, axis_inplane_reject<AX>), compiled with the kernels' float rules, against
// the form it replaced in cast_local (rt_kernels.hip): the same arithmetic with every component
// picked by a run-time axis index (comp()).
//  1. N random (ray, TriAx record) pairs per axis: the plane time's bits, the window test
//     lo <= tt < t_best and the in-plane reject agree.  One in eight directions has a zero or
//     sub-threshold component (inv = NaN: the reference rejects), records sit around the ray's
//     crossing point so that both outcomes of the reject occur, and points are placed on the
//     window's edges (e == 0, e == win, |pa - a_ax| == off) as far as float arithmetic allows.
//  2. the edge values of the window test for every pair: inv = NaN never passes; lo == tt passes;
//     t_best == tt does not (the strict <).
//   leaf_loop_host N -> prints "pairs passes rejects nan_inv mismatches edge_errors"; exit status 1 on any error
#include "rt_math.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
using namespace rtm;
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// cast_local's earlier form, restated: a run-time axis index and selects
static float comp(V3 v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }
static bool plane_pass_comp(const TriAx& x, int ax, V3 o, V3 inv, float lo, float t_best, float& tt) {
    tt = axis_plane_t(x.a_ax, comp(o, ax), comp(inv, ax));
    return tt >= lo && tt < t_best;
}
static bool reject_comp(const TriAx& x, int ax, const Ray& mr, float tt) {
    const int au = ax == 2 ? 0 : ax + 1, av = ax == 0 ? 2 : ax - 1;
    const float pu = comp(mr.o, au) + tt * comp(mr.d, au), pv = comp(mr.o, av) + tt * comp(mr.d, av);
    const float pa = comp(mr.o, ax) + tt * comp(mr.d, ax);
    const float e = fmaxf(fmaxf(x.ulo - pu, pu - x.uhi), fmaxf(x.vlo - pv, pv - x.vhi));
    return e > 0.0f && e <= x.win && fabsf(pa - x.a_ax) <= x.off;
}
static float axis_inv(float d) { return fabsf(d) < THRESH ? std::numeric_limits<float>::quiet_NaN() : rcp_cr(d); }

struct Tally { long pairs = 0, passes = 0, rejects = 0, nan_inv = 0, mismatch = 0, edge_err = 0; };

template <int AX> static void one(const TriAx& x, const Ray& mr, V3 inv, float lo, float t_best, Tally& T) {
    float tt, tt_c;
    const bool p = axis_plane_pass<AX>(x, mr.o, inv, lo, t_best, tt);
    const bool p_c = plane_pass_comp(x, AX, mr.o, inv, lo, t_best, tt_c);
    T.pairs++;
    if (p != p_c || bits(tt) != bits(tt_c)) T.mismatch++;
    const bool r = axis_inplane_reject<AX>(x, mr, tt), r_c = reject_comp(x, AX, mr, tt_c);
    if (tt == tt && r != r_c) T.mismatch++;
    if (tt != tt && (r || r_c)) T.mismatch++;                // a NaN time rejects nothing (and passes nothing)
    T.passes += p;
    T.rejects += p && r;
    if (tt != tt) {
        T.nan_inv++;
        if (p) T.edge_err++;
        return;
    }
    // the window's ends: lo == tt is inside, t_best == tt is not
    float e0, e1;
    if (!axis_plane_pass<AX>(x, mr.o, inv, tt, INFINITY, e0) || bits(e0) != bits(tt)) T.edge_err++;
    if (axis_plane_pass<AX>(x, mr.o, inv, -INFINITY, tt, e1) || bits(e1) != bits(tt)) T.edge_err++;
    if (axis_plane_pass<AX>(x, mr.o, inv, tt, tt, e1)) T.edge_err++;
    if (!axis_plane_pass<AX>(x, mr.o, inv, tt, nextafterf(tt, INFINITY), e1)) T.edge_err++;
    if (axis_plane_pass<AX>(x, mr.o, inv, nextafterf(tt, INFINITY), INFINITY, e1)) T.edge_err++;
}

template <int AX> static void sweep(long n, Tally& T) {
    constexpr int AU = AX == 2 ? 0 : AX + 1, AV = AX == 0 ? 2 : AX - 1;
    std::mt19937_64 g(20240611 + AX);
    std::normal_distribution<float> N(0.0f, 1.0f);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    for (long i = 0; i < n; i++) {
        V3 raw = v3(N(g), N(g), N(g));
        auto set = [&](long k, float s) { (k == 0 ? raw.x : k == 1 ? raw.y : raw.z) = s; };
        if (i % 8 == 0) set((i / 8) % 3, (i % 16 == 0) ? 0.0f : 3e-6f * N(g));     // |d_a| < 1e-5: inv = NaN
        if (i % 24 == 3) set((i / 24) % 3, -0.0f);
        const Ray mr = make_ray(v3(4.0f * N(g), 4.0f * N(g), 4.0f * N(g)), raw);
        if (!(dot(mr.d, mr.d) > 0.5f)) continue;
        const V3 inv = v3(axis_inv(mr.d.x), axis_inv(mr.d.y), axis_inv(mr.d.z));
        TriAx x;
        x.code = AX | 8;
        x.a_ax = 4.0f * N(g);
        float tt = axis_plane_t(x.a_ax, pick<AX>(mr.o), pick<AX>(inv));
        if (!(tt == tt)) tt = 1.0f;
        // a record of extent D about a point near the crossing: the excess e falls on both sides
        // of 0 and of win
        const float D = exp2f(6.0f * U(g) - 4.0f), m = 1e-4f * D;
        const float pu = pick<AU>(mr.o) + tt * pick<AU>(mr.d), pv = pick<AV>(mr.o) + tt * pick<AV>(mr.d);
        const float pa = pick<AX>(mr.o) + tt * pick<AX>(mr.d);
        const float cu = pu + D * N(g) * (i % 5 == 0 ? 1000.0f : 1.0f), cv = pv + D * N(g);
        x.ulo = cu - 0.5f * D - m; x.uhi = cu + 0.5f * D + m;
        x.vlo = cv - 0.5f * D - m; x.vhi = cv + 0.5f * D + m;
        x.win = 1e3f * D; x.off = m;
        switch (i % 7) {                                      // the window's edges
            case 1: x.uhi = pu; x.vlo = pv - D; x.vhi = pv + D; x.ulo = pu - D; break;      // e == 0: not rejected
            case 2: x.uhi = nextafterf(pu, -INFINITY); x.vlo = pv - D; x.vhi = pv + D; x.ulo = pu - D; break;
            case 3: x.win = fmaxf(fmaxf(x.ulo - pu, pu - x.uhi), fmaxf(x.vlo - pv, pv - x.vhi)); break;   // e == win
            case 4: x.off = fabsf(pa - x.a_ax); break;        // |pa - a_ax| == off: still rejected
            case 5: x.off = nextafterf(fabsf(pa - x.a_ax), -INFINITY); break;
            default: break;
        }
        const float lo = fmaxf(THRESH, i % 3 ? -INFINITY : tt - fabsf(N(g)));
        const float t_best = i % 4 ? tt + fabsf(N(g)) : INFINITY;
        one<AX>(x, mr, inv, lo, (i % 11 == 0) ? tt - 0.25f : t_best, T);
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
    Tally T;
    sweep<0>(n, T);
    sweep<1>(n, T);
    sweep<2>(n, T);
    std::printf("%ld %ld %ld %ld %ld %ld\n", T.pairs, T.passes, T.rejects, T.nan_inv, T.mismatch, T.edge_err);
    return (T.mismatch || T.edge_err) ? 1 : 0;
}
