// Host driver of tests/test_shadow_hints_host.py: the occluder hint table's packing (csrc/rt_plan.h:
// hint_key, hint_code and its inverses, hint_node_ok, the table's size) is pure arithmetic.
//   shadow_hints_host key INST TRI LIGHT     -> the entry index
//   shadow_hints_host code NODE SIDE         -> code node side
//   shadow_hints_host ok CODE N_REAL         -> 0 / 1
//   shadow_hints_host size N_INST            -> entries bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_device.h"

using namespace rtd;

int main(int argc, char** argv) {
    auto arg = [&](int i) { return i < argc ? atoll(argv[i]) : 0ll; };
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "key")) printf("%d\n", hint_key((int)arg(2), (int)arg(3)) + ((int)arg(4) & 3));
    else if (!strcmp(argv[1], "code")) {
        const int c = hint_code((int)arg(2), (int)arg(3));
        printf("%d %d %d\n", c, hint_node(c), hint_side(c));
    } else if (!strcmp(argv[1], "ok")) printf("%d\n", hint_node_ok((int)arg(2), (int)arg(3)) ? 1 : 0);
    else if (!strcmp(argv[1], "size")) printf("%zu %zu\n", hint_table_ints((int)arg(2)), hint_bytes((int)arg(2)));
    else return 2;
    return 0;
}
