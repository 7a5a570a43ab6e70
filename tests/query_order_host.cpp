// Host driver of tests/test_query_order_host.py and tests/test_gpu_query_order.py: the coherence
// key of a ray query (csrc/rt_raykey.h) and query_order_plan (csrc/rt_plan.h) are pure host
// arithmetic, so they are printed here on a machine without a GPU.  Host pass only; nothing calls HIP.
//   query_order_host info
//       origin_bits, key_bits and the rejected key
//   query_order_host plan n_rays mode counted
//       sort, key_bits, keys_bytes, idx_bytes, scratch_bytes
//   query_order_host keys in.bin out.bin
//       in.bin: n x 12 float32 (a ray as traced: origin, unit direction; then a box: min3, max3);
//       out.bin: n x uint64 keys
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device.h"

using namespace rtd;

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "info")) {
        printf("origin_bits %d key_bits %d rejected %llu\n", rtk::ORIGIN_BITS, rtk::RAYKEY_BITS,
               (unsigned long long)rtk::RAYKEY_REJECTED);
    } else if (argc == 5 && !strcmp(argv[1], "plan")) {
        const QueryOrderPlan p = query_order_plan(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0);
        printf("sort %d key_bits %d keys_bytes %zu idx_bytes %zu scratch_bytes %zu\n", (int)p.sort, p.key_bits, p.keys_bytes,
               p.idx_bytes, p.scratch_bytes);
    } else if (argc == 4 && !strcmp(argv[1], "keys")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) { perror(argv[2]); return 1; }
        std::vector<float> in;
        float row[12];
        while (fread(row, sizeof row, 1, f) == 1) in.insert(in.end(), row, row + 12);
        fclose(f);
        std::vector<unsigned long long> keys(in.size() / 12);
        for (size_t i = 0; i < keys.size(); i++) {
            const float* a = &in[12 * i];
            const rtm::Ray r{rtm::v3(a[0], a[1], a[2]), rtm::v3(a[3], a[4], a[5])};
            keys[i] = rtk::ray_key(r, rtk::KeyBox{rtm::v3(a[6], a[7], a[8]), rtm::v3(a[9], a[10], a[11])});
        }
        f = fopen(argv[3], "wb");
        if (!f) { perror(argv[3]); return 1; }
        fwrite(keys.data(), sizeof(unsigned long long), keys.size(), f);
        fclose(f);
    } else {
        fprintf(stderr, "usage: query_order_host info | plan n_rays mode counted | keys in.bin out.bin\n");
        return 2;
    }
    return 0;
}
