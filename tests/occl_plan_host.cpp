// occl_plan_host — occlusion_plan (csrc/rt_plan.h: the ambient-occlusion pass's tree form, lane
// mapping and grid), a pure host function, on the command line for tests/test_occlusion_plan_host.py.
//
//   occl_plan_host W H use_bvh n_leaf ftree map   ->   tree map n_waves block blocks default_map
#include <cstdio>
#include <cstdlib>

#include "rt_device.h"

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: occl_plan_host W H use_bvh n_leaf ftree map\n"); return 2; }
    rtd::SceneView S{};
    S.use_bvh = std::atoi(argv[3]); S.n_leaf = std::atoi(argv[4]); S.ftree = std::atoi(argv[5]);
    const rtd::OcclPlan p = rtd::occlusion_plan(std::atoi(argv[1]), std::atoi(argv[2]), S, std::atoi(argv[6]));
    std::printf("%d %d %d %d %d %d\n", p.tree, p.map, p.n_waves, p.block, p.blocks, (int)rtd::RT_OCCL_MAP_DEFAULT);
    return 0;
}
