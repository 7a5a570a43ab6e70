// Host check of the unit-length fast path (gpu-ray-tracer_amd/csrc/rt_math.h: unit_window,
// unit_head, unit_len_rcp, normalized_unit, qrot_identity_unit), compiled with the kernels' float rules.
//  1. every float s in [1 - 2^-13, 1 + 2^-13]: unit_window(s) exactly on |s - 1| <= 2^-14, and
//     inside it unit_len_rcp == (sqrtf(s), 1.0f / sqrtf(s)) bit for bit;
//  2. the first floats outside the window on both sides, zeros, denormals, infinities, NaNs and
//     negative numbers: not in the window;
//  3. N random directions through make_ray's normalisation and dir_pre's four stages (rt_kernels.hip:
//     qrot_identity, len / normalized, qrot_identity, len / normalized): the first squared length
//     passes the chain's vote (unit_head), every later one lies in the window, and the unit chain
//     returns the generic chain's bits; the same for heads scaled across unit_head's window and
//     for hit_normal's order of the stages.
//   unitlen_host N -> prints "swept in_window window_errors value_errors special_errors
//                             dirs stages_outside chain_mismatches"; exit status 1 on any error
#include "rt_math.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
using namespace rtm;
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static bool same(V3 a, V3 b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

int main(int argc, char** argv) {
    const long n_dirs = argc > 1 ? std::atol(argv[1]) : 1000000;
    long swept = 0, in_window = 0, window_err = 0, value_err = 0, special_err = 0;
    const double W = 0x1p-14;
    for (uint32_t u = bits(1.0f - 0x1p-13f); u <= bits(1.0f + 0x1p-13f); u++) {
        const float s = from_bits(u);
        swept++;
        const double dev = (double)s - 1.0;
        const bool want = (dev < 0 ? -dev : dev) <= W;
        if (unit_window(s) != want) window_err++;
        if (!want) continue;
        in_window++;
        float L, r;
        unit_len_rcp(s, L, r);
        const float l_ref = sqrtf(s), r_ref = 1.0f / l_ref;
        if (bits(L) != bits(l_ref) || bits(r) != bits(r_ref)) value_err++;
        if (bits(L) != bits(sqrt_cr(s)) || bits(r) != bits(rcp_cr(sqrt_cr(s)))) value_err++;
    }
    const float inf = std::numeric_limits<float>::infinity();
    const float outside[] = {
        nextafterf(1.0f - 0x1p-14f, 0.0f), nextafterf(1.0f + 0x1p-14f, 2.0f),
        0.0f, -0.0f, from_bits(1u), from_bits(0x007fffffu), from_bits(0x80000001u), std::numeric_limits<float>::min(),
        inf, -inf, std::numeric_limits<float>::quiet_NaN(), from_bits(0x7f800001u), from_bits(0xffc00000u),
        -1.0f, from_bits(bits(-1.0f) + 3u), 0.5f, 2.0f, 1e-5f, std::numeric_limits<float>::max(),
    };
    for (float s : outside) if (unit_window(s)) special_err++;
    if (!unit_window(1.0f) || !unit_window(1.0f - 0x1p-14f) || !unit_window(1.0f + 0x1p-14f)) special_err++;

    if (!unit_head(1.0f) || !unit_head(1.0f - 0x1p-16f) || !unit_head(1.0f + 0x1p-16f) ||
        unit_head(nextafterf(1.0f - 0x1p-16f, 0.0f)) || unit_head(nextafterf(1.0f + 0x1p-16f, 2.0f)))
        special_err++;
    for (float s : outside) if (unit_head(s)) special_err++;

    // 3. the claim that the fast path is the common path, and that one vote on a chain's head
    // (unit_head) covers its later stages
    std::mt19937_64 g(20240607);
    std::normal_distribution<float> N(0.0f, 1.0f);
    std::uniform_real_distribution<float> E(-10.0f, 20.0f);
    long dirs = 0, stages_outside = 0, mismatch = 0;
    // the chain of dir_pre from a head d: generic against unit forms
    auto chain = [&](V3 d, bool traced) {
        const V3 ld = qrot_identity(d);
        const float dir_len = len(ld);
        const V3 lrd = normalized(ld);
        const V3 md = qrot_identity(lrd);
        const float scale = len(md);
        const V3 mrd = normalized(md);
        if (traced && !unit_head(dot(d, d))) stages_outside++;            // a traced direction passes the vote
        if (!unit_head(dot(d, d))) return;
        const float later[3] = {dot(ld, ld), dot(lrd, lrd), dot(md, md)};
        for (float s : later) if (!unit_window(s)) stages_outside++;
        float u_len, u_scale;
        const V3 uld = qrot_identity_unit(d);
        const V3 ulrd = normalized_unit(uld, u_len);
        const V3 umd = qrot_identity_unit(ulrd);
        const V3 umrd = normalized_unit(umd, u_scale);
        if (!same(umrd, mrd) || bits(u_len) != bits(dir_len) || bits(u_scale) != bits(scale) || !same(uld, ld) ||
            !same(ulrd, lrd) || !same(umd, md))
            mismatch++;
        // hit_normal's order of the same stages: normalized, rotation, normalized, rotation
        const V3 hn = qrot_identity(normalized(qrot_identity(normalized(d))));
        float l;
        const V3 un = qrot_identity_unit(normalized_unit(qrot_identity_unit(normalized_unit(d, l)), l));
        if (!same(hn, un)) mismatch++;
    };
    for (long i = 0; i < n_dirs; i++) {
        V3 raw = v3(N(g), N(g), N(g));
        if (i % 7 == 0) raw.x = 0.0f;                        // axis-aligned and planar directions
        if (i % 11 == 0) raw.y = -0.0f;
        if (i % 13 == 0) raw.z = raw.z * 1e-6f;
        const float mag = exp2f(E(g));                       // any length before the Ray ctor
        raw = mag * raw;
        const V3 d = make_ray(v3(0.0f, 0.0f, 0.0f), raw).d;
        if (!(dot(d, d) > 0.5f)) continue;                   // (|raw| <= 1e-5: the Ray ctor gives the zero vector)
        dirs++;
        chain(d, true);
        // heads spread over the vote's window and past both of its edges
        if (i % 4 == 0) chain((1.0f + (float)((i / 4) % 801 - 400) * 0x1p-24f) * d, false);
    }
    std::printf("%ld %ld %ld %ld %ld %ld %ld %ld\n", swept, in_window, window_err, value_err, special_err, dirs,
                stages_outside, mismatch);
    return (window_err || value_err || special_err || stages_outside || mismatch) ? 1 : 0;
}
