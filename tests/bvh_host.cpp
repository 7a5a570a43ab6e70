// bvh_host.cpp — the ordered tree's node search (csrc/rt_bvh.h: fnode_split, the code the build
// kernels and the host's ordered_tree_shape share) and the build's form choice, on the host.
//   bvh_host split FILE   FILE: one key set per line, "nr k0 k1 ... k(nr-1)" (sorted, decimal
//                         u64).  Prints "first last gamma" of nodes 0 .. nr-2, one per line,
//                         set after set.
//   bvh_host form N N_INST   prints bvh_form for N padded leaves and N_INST instances.
// Built by tests/test_bvh_host.py with the kernels' compiler, host pass only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device.h"

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "form")) {
        printf("%d\n", rtb::bvh_form(atoi(argv[2]), atoi(argv[3]), rtd::BVH_WG_LEAVES));
        return 0;
    }
    if (argc != 3 || strcmp(argv[1], "split")) return 2;
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    int nr;
    std::vector<unsigned long long> k;
    while (fscanf(f, "%d", &nr) == 1) {
        k.resize(nr);
        for (int i = 0; i < nr; i++)
            if (fscanf(f, "%llu", &k[i]) != 1) return 3;
        for (int i = 0; i + 1 < nr; i++) {
            int first, last, gamma;
            rtb::fnode_split(k.data(), nr, i, first, last, gamma);
            printf("%d %d %d\n", first, last, gamma);
        }
    }
    fclose(f);
    return 0;
}
