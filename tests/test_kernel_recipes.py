"""The recipe table of tests/kernel_recipes.py on the host: every recipe's product scene is built
without a device, its counts (rt_scene_info), its frame-stack depth (as shade_shortcuts derives it)
and its launch options go through `plan_host key` (trace_variant_key, csrc/rt_plan.h), and the
answer must be the kernel the recipe is filed under.  With the table's keys equal to the 47 kernels
of the build, tests/test_gpu_kernel_matrix.py is complete before anyone has a GPU."""
import pytest

import kernel_recipes as kr
from test_plan_host import KERNELS, plan  # noqa: F401  (the plan_host fixture)


@pytest.fixture(scope="module")
def host_scenes(rt, tmp_path_factory):
    tmp, cache = tmp_path_factory.mktemp("recipes"), {}

    def get(name):
        if name not in cache:
            cache[name] = kr.build_scene(name, (64, 48), rt, None, tmp)[0]
        return cache[name]
    return get


def test_one_recipe_per_kernel():
    assert len(KERNELS) == 47
    assert set(kr.RECIPES) == KERNELS                          # none missing, none extra
    assert len({kr.kernel_id(k) for k in kr.RECIPES}) == 47


@pytest.mark.parametrize("key", sorted(kr.RECIPES), ids=kr.kernel_id)
def test_recipe_reaches_its_kernel(plan, host_scenes, key):  # noqa: F811
    r = kr.RECIPES[key]
    s = host_scenes(r.scene)
    family, refractive, rot = kr.parse(r.scene)
    # the scene is the case its name says
    n = s.info()["n_instances"]
    if family == "one":
        assert n == 1
    elif family in ("two", "tess"):
        assert n == 2 and s.info()["n_tris"] == (768 if family == "tess" else 36)
    elif family == "chain":
        assert 513 <= n <= 743 and not kr.scene_ftree(s)        # 1024 padded leaves; the ordered tree is too deep
    elif family == "mid":
        assert 744 <= n <= 1024, n                            # 80 n - 64 > 59392; 1024 padded leaves
    else:
        assert 2100 <= n <= 4096, n
    assert (kr.scene_ns(s, r.depth) > 0) == refractive
    assert kr.scene_ns(s, r.depth) == (0 if key[0] == 0 else r.depth)
    assert bool(kr.plan_key_args(s, r)[3]) == (not rot)       # tri_ax
    assert kr.scene_ftree(s) == (0 if family in ("one", "chain") else 1)
    got = kr.plan_key(plan, s, r)
    assert (got["ns_bucket"], got["lds"], got["mode"]) == key, (r, got)
    # M_PROF frames come from rt_frame_work and only from it
    assert bool(key[2] & kr.M_PROF) == r.prof
