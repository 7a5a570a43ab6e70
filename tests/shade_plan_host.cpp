// shade_plan_host — shade_plan (csrc/rt_plan.h: which shade kernel a batch of rt_shade gets, and its
// grid), a pure host function, on the command line for tests/test_shade_host.py.  The frame-stack
// bucket comes from shade_shortcuts of a host scene with one material, refractive or not, at the
// given depth, as rt_shade forms it.
//
//   shade_plan_host n use_bvh n_leaf ftree refractive depth tex   ->   tree ns_bucket tex block blocks ns
#include <cstdio>
#include <cstdlib>

#include "rt_device.h"

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: shade_plan_host n use_bvh n_leaf ftree refractive depth tex\n"); return 2; }
    rtd::SceneView S{};
    S.use_bvh = std::atoi(argv[2]); S.n_leaf = std::atoi(argv[3]); S.ftree = std::atoi(argv[4]);
    rt::Scene h;
    rt::DMat m{};
    m.refractive = std::atoi(argv[5]) != 0;
    h.d_mats.push_back(m);
    h.depth = std::atoi(argv[6]);
    const rtd::ShadeShortcuts sc = rtd::shade_shortcuts(h, false, false, -1);
    const rtd::ShadeKey k = rtd::shade_plan(std::atoll(argv[1]), S, sc.ns, std::atoi(argv[7]) != 0);
    std::printf("%d %d %d %d %d %d\n", k.tree, k.ns_bucket, (int)k.tex, k.block, k.blocks, sc.ns);
    return 0;
}
