// batch_stage_host — batch_plan (csrc/rt_plan.h: the layout of a batch of caller rays given with host
// pointers in an entry's staging), a pure host function, on the command line for
// tests/test_batch_stage_host.py.  The part lists are rt_query's and rt_shade's (rt_query.cpp,
// rt_shade.cpp): bytes per ray, inputs first.
//
//   batch_stage_host entry n mask   ->   in_bytes total, then a line "output present bytes off" per part
//
// entry: query | shade; mask: bit k set = part k of the entry's list is present.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device.h"

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: batch_stage_host query|shade n mask\n"); return 2; }
    const bool shade = !std::strcmp(argv[1], "shade");
    const size_t n = (size_t)std::atoll(argv[2]);
    const unsigned mask = (unsigned)std::strtoul(argv[3], nullptr, 0);
    static char there;                                      // a present part's non-null pointer; never dereferenced
    const char* src[16] = {};                               // the parameter fields the parts are made from
    char* dst[16] = {};
    int k = 0;
    auto in = [&](size_t per_ray) { src[k] = (mask >> k) & 1 ? &there : nullptr; k++; return rtd::in_part(src[k - 1], per_ray * n); };
    auto out = [&](size_t per_ray) { dst[k] = (mask >> k) & 1 ? &there : nullptr; k++; return rtd::out_part(dst[k - 1], per_ray * n); };
    std::vector<rtd::BatchPart> parts;
    if (shade) parts = {in(12), in(12), in(8), out(16), out(4), out(24)};                  // origin dir pixel | radiance rgba rays_out
    else parts = {in(12), in(12), in(4), in(8), out(4), out(4), out(4), out(8), out(12), out(1), out(24)};
    //            origin  dir     tmax   pixel | t       inst    tri     uv      normal   hit     rays_out
    const rtd::BatchPlan P = rtd::batch_plan(parts.data(), parts.size());
    std::printf("%zu %zu\n", P.in_bytes, P.total);
    for (const rtd::BatchPart& p : parts) std::printf("%d %d %zu %zu\n", (int)p.output, (int)p.present, p.bytes, p.off);
    return 0;
}
