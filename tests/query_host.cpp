// Host driver of tests/test_query_host.py: query_plan (csrc/rt_plan.h), which query kernel and
// launch a batch of rays gets (rt_query), is pure host arithmetic, so it is printed here on a
// machine without a GPU.  Host pass only; nothing calls HIP.
//   query_host plan n_rays n_inst n_real depth use_bvh any_hit counted n_cu form
//       one SceneView of those counts, as upload and view_of (rt_runtime.cpp) set them: n_leaf
//       padded from n_inst, ftree = ordered_tree_usable(n_real, depth); form < 0: by batch size
//   query_host sweep n_inst n_real depth use_bvh n_cu
//       the same fields for a ladder of batch sizes, each with form -1, 0 and 1, one line each
//       (first field: n_rays, second: form)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_device.h"

using namespace rtd;

static SceneView view(int n_inst, int n_real, int depth, int use_bvh) {
    SceneView S{};
    S.n_inst = n_inst; S.n_real = n_real; S.use_bvh = use_bvh;
    S.ftree = ordered_tree_usable(n_real, depth) ? 1 : 0;
    S.n_leaf = 0;                                              // padded(): 1 << ceil(log2(n)), 0 for none
    if (n_inst > 0) { S.n_leaf = 1; while (S.n_leaf < n_inst) S.n_leaf <<= 1; }
    S.prune_abs = -1.0f;                                       // rt_query: the camera-ray shortcuts off
    return S;
}

static void print(const QueryKey& k) {
    printf("tree %d lds %d any_hit %d counted %d persistent %d block %d blocks %d shm %zu\n", k.tree, (int)k.lds,
           (int)k.any_hit, (int)k.counted, (int)k.persistent, k.block, k.blocks, k.shm);
}

int main(int argc, char** argv) {
    auto arg = [&](int i) { return i < argc ? atoll(argv[i]) : 0ll; };
    if (argc == 11 && !strcmp(argv[1], "plan")) {
        const SceneView S = view((int)arg(3), (int)arg(4), (int)arg(5), (int)arg(6));
        print(query_plan(arg(2), S, arg(7) != 0, arg(8) != 0, (int)arg(9), (int)arg(10)));
    } else if (argc == 7 && !strcmp(argv[1], "sweep")) {
        const SceneView S = view((int)arg(2), (int)arg(3), (int)arg(4), (int)arg(5));
        static const long long ns[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 16383, 16384, 16385, 65536, 100000,
                                       262144, 262145, 1000000, 2073600, 16777216, 3000000000ll};
        for (long long n : ns)
            for (int form = -1; form <= 1; form++) {
                printf("n_rays %lld form %d ", n, form);
                print(query_plan(n, S, false, false, (int)arg(6), form));
            }
    } else {
        fprintf(stderr, "usage: query_host plan ... | sweep ...\n");
        return 2;
    }
    return 0;
}
