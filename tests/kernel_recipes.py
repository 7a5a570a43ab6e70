"""One recipe per trace kernel: for every trace_kernel<NS, LDS, MODE> of the build (test_plan_host.KERNELS),
a scene and launch options whose frame runs that kernel.  TEST INFRASTRUCTURE (may use the oracle).

tests/test_kernel_recipes.py proves the table on the host (every recipe's scene counts, through
`plan_host key`, give the recipe's own key; the 47 keys are the 47 kernels);
tests/test_gpu_kernel_matrix.py renders every recipe, asserts the kernel the launch used
(Scene.last_trace) and compares the frame with the oracle.

The scenes, and what makes each the case it is (rt_plan.h: lds_bytes, park_fields, trace_variant_key;
a persistent block parks 25 fields x 4 B x 1024 lanes = 102400 B for NS = 0, 29 fields = 118784 B
otherwise, beside the scene image, within PARK_LDS_LIMIT = 161792 B; LDS_LIMIT = 153600 B):

  one    one cube.  n_real < 2, so there is no ordered tree (ftree = 0): the heap image (80 B) with
         the parking area, MODE 4 (M_PARK).
  two    two cubes (3 cube meshes, 36 triangles).  Ordered tree (64 B) + instance records (32 B)
         + the shading cache (36 x 128 B triangles and a few records) + parking: the parked fast
         kernels MODE 180, 116 (rt_frame_work), 420 (use_bvh = 0), 56 / 24 (textured).
  tess   two instances of an axis-aligned cube whose 12 triangles are each split into 64
         (8 x 8 quads per face, 768 triangles): shade_bytes >= 768 x 128 = 98304 B does not fit
         beside the parking area (161792 - 102400 = 59392 B), so M_SHADE is off: MODE 52.  Long
         runs of coplanar neighbours for tri_axis_records' shared-plane flag.
  mid    a cube field generated from world8_stress_tex.json, grid_size 10: 744 < n < 1024
         instances.  Ordered tree + instances = 80 n - 64 B > 59392 B (n > 743): no room for the
         whole parking area, so MODE 692 / 700 (partial parking, tree 64 (n - 1) + shade + 57344 B),
         MODE 16 with RT_NO_PART or a refractive material (n > 538: 80 n - 64 > 161792 - 118784),
         and the heap image a16(52 x 1024) + 16 n > 59392 B for the unparked heap kernels
         MODE 0 (use_bvh = 0, one instance rotated: the unspecialised brute-force loop), 1, 2, 3.
  chain  521 cubes whose ordered tree is deeper than the fast traversal's 31-entry stack, so
         ordered_tree_shape turns it off (ftree = 0 with more than one instance): 37 small cubes
         whose Morton keys share successively longer prefixes (chain_positions; depth 36) over a
         22 x 22 floor.  1024 padded leaves: the heap image 53248 + 16 n = 61584 B leaves no room
         to park, so use_bvh = 1 runs MODE 0 through the heap traversal.  The refractive MODE 0
         recipes use it: the oracle's brute-force frame of the 876-cube field at depth 4 takes a
         minute (every ray tests every triangle), its BVH frame of this scene well under a second.
  big    the same field at grid_size 16: n > 2048 instances, 4096 padded leaves.  The heap image
         (52 x 4096 B) and the ordered tree (80 n - 64 B, n >= 1921) both exceed LDS_LIMIT: LDS = 0.

Variants: `_r` one refractive material (Kt in (0, 1), eta 1.3; with Kr and Ka so that every
bounce shows): ns = max(depth, 1), NS 2 at depth 2 and NS 9 at depth 3 or 4 (rt_env_set); all-opaque
scenes have ns = 0.  `_rot` one instance turned 45 degrees about y: S.tri_ax = nullptr, the kernels
without M_AXIS / M_SHADE / M_BRUTE.

Depths outside 2 to 4 (0 and 1 in the NS 2 bucket, 5 to 9 with the NS 9 stack full), several refractive
media of different eta and Kt, and total internal reflection: tests/integrator_cases.py and
tests/test_gpu_integrator.py, over the kernels a small scene reaches (M180, M420, M116, M2).
"""
import json
import os
import sys
from collections import namedtuple

import numpy as np

from conftest import ROOT, scene_path
from test_plan_host import KERNELS, NG

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_atlas  # noqa: E402

M_MULTI, M_STATS, M_PARK, M_TEX, M_FT, M_AXIS, M_PROF, M_SHADE, M_BRUTE, M_PART = (1 << i for i in range(10))

# scene: a scene name (family[_r][_rot], build_scene); depth: rt_env_set before the frame; no_part: RT_NO_PART in the
# environment; prof: the frame is rt_frame_work's
Recipe = namedtuple("Recipe", "scene spp stats tex use_bvh depth no_part prof")


def _r(scene, depth, spp=8, stats=False, tex=False, use_bvh=True, no_part=False, prof=False):
    return Recipe(scene, spp, stats, tex, use_bvh, depth, no_part, prof)


def _recipes():
    t = {}
    # the frame-stack buckets: all-opaque (ns = 0), refractive at depth 2 (ns = 2) and at depth 4 (ns = 4 -> NG)
    for ns, sfx, d in ((0, "", 3), (2, "_r", 2), (NG, "_r", 4)):
        t[ns, 1, 0] = _r("chain" + sfx, d)                              # the heap kernel, nothing parked
        t[ns, 1, M_PARK] = _r("one" + sfx, d)
        t[ns, 1, M_FT | M_PARK] = _r("two" + sfx + "_rot", d)
        t[ns, 1, M_FT | M_PARK | M_AXIS] = _r("tess" + sfx, d)
        t[ns, 1, M_FT | M_PARK | M_AXIS | M_PROF] = _r("two" + sfx, d, prof=True)
        t[ns, 1, M_FT | M_PARK | M_AXIS | M_SHADE] = _r("two" + sfx, d)
        t[ns, 1, M_BRUTE | M_PARK | M_SHADE | M_AXIS] = _r("two" + sfx, d, use_bvh=False)
        t[ns, 0, 0] = _r("big" + sfx, d)
    t[0, 1, 0] = _r("mid_rot", 3, spp=2, use_bvh=False)                 # opaque: MODE 0's brute-force loop instead
    # M_FT alone: the tree in LDS, nothing parked.  Opaque: partial parking switched off
    t[0, 1, M_FT] = _r("mid", 3, no_part=True)
    t[2, 1, M_FT] = _r("mid_r", 2)
    t[NG, 1, M_FT] = _r("mid_r", 4)
    # partial parking (NS = 0 only), plain and textured
    t[0, 1, M_PARK | M_FT | M_AXIS | M_SHADE | M_PART] = _r("mid", 3)
    t[0, 1, M_PARK | M_FT | M_AXIS | M_SHADE | M_PART | M_TEX] = _r("mid", 3, tex=True)
    # textured fast kernels (NS 2 and NG only), with and without the axis path
    for ns, d in ((2, 2), (NG, 4)):
        t[ns, 1, M_TEX | M_FT] = _r("two_r_rot", d, tex=True)
        t[ns, 1, M_TEX | M_FT | M_AXIS] = _r("two_r", d, tex=True)
    # the generic kernels (NG only): counted, multi-round and textured, heap image in LDS or not
    # (65 spp at depth 3, still the NG bucket: the oracle's rays double with every level)
    for lds, plain, texd in ((1, "mid_r", "two_r"), (0, "big_r", "big_r")):
        t[NG, lds, M_MULTI] = _r(plain, 3, spp=65)
        t[NG, lds, M_STATS] = _r(plain, 4, stats=True)
        t[NG, lds, M_MULTI | M_STATS] = _r(plain, 3, spp=65, stats=True)
        t[NG, lds, M_TEX] = _r(texd, 4, tex=True, use_bvh=bool(1 - lds))   # (two cubes: brute force, no ordered tree)
        t[NG, lds, M_TEX | M_MULTI] = _r(texd, 3, spp=65, tex=True)
        t[NG, lds, M_TEX | M_STATS] = _r(texd, 4, tex=True, stats=True)
        t[NG, lds, M_TEX | M_MULTI | M_STATS] = _r(texd, 3, spp=65, tex=True, stats=True)
    return t


RECIPES = _recipes()
assert set(RECIPES) == KERNELS, (sorted(set(RECIPES) - KERNELS), sorted(KERNELS - set(RECIPES)))


def kernel_id(key):
    return "NS%d-LDS%d-M%d" % key


def frame_size(recipe):
    """64 x 48 at up to 8 spp, 32 x 24 at 65."""
    return (64, 48) if recipe.spp <= 8 else (32, 24)


# ---- scenes -------------------------------------------------------------------------------
ROT45 = (0.0, 0.38268343, 0.0, 0.92387953)      # 45 degrees about y
DOWN45 = (0.3826834, 0.0, 0.0, 0.9238795)        # 45 degrees about x: forward (0, 0, 1) turns down
FIELD_GRID = {"mid": 10, "big": 16}
ATLAS_TILES = ((0, 0, 64), (128, 128, 64), (64, 64, 64))
# Every scene has three lights and specular materials, the last light shining down and towards the
# cameras (they look along +z): its highlight on the top faces is in view, so the state a kernel
# keeps across the earlier lights' shadow queries (the hit's unit normal, the sums) shows in the frame.
TOWARDS_CAMERA = ((0.2, -1.0, -1.0), (0.6, 0.6, 0.7, 1.0))


def _materials(rt, refractive):
    m = rt.material
    first = (m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.2, 0.6, 1), Ks=(0.3, 0.3, 0.3, 1), Kt=(0.5, 0.6, 0.7, 1),
               Kr=(0.4, 0.4, 0.4, 1), alpha=4.0, eta=1.3) if refractive
             else m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.6, 0.3, 0.1, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0))
    return [first,
            m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.5, 0.2, 1), Ks=(0.8, 0.8, 0.8, 1), alpha=6.0),
            m(Ka=(0.05, 0.05, 0.05, 1), Kd=(0.3, 0.3, 0.3, 1), Ks=(0.5, 0.5, 0.5, 1), Kr=(0.7, 0.7, 0.7, 1), alpha=8.0)]


def _tess_cube(b, scale, mat, n=8):
    """build_cube's 12 triangles (rt_scene.cpp, same corners and winding), each split into n x n."""
    c = {k: scale * np.array(v, np.float32) for k, v in dict(
        A=(-.5, .5, -.5), B=(.5, .5, -.5), C=(-.5, -.5, -.5), D=(.5, -.5, -.5),
        E=(-.5, .5, .5), F=(.5, .5, .5), G=(-.5, -.5, .5), H=(.5, -.5, .5)).items()}
    mesh = b.create_mesh()
    for tri in ("DAB", "CAD", "AEB", "EFB", "DBH", "BFH", "CGA", "AGE", "GHE", "EHF", "GCD", "DHG"):
        p0, p1, p2 = (c[k] for k in tri)

        def v(i, j):
            return p0 + (p1 - p0) * np.float32(i / n) + (p2 - p0) * np.float32(j / n)   # multiples of scale / n: exact
        for i in range(n):
            for j in range(n - i):
                small = [(v(i, j), v(i + 1, j), v(i, j + 1))]
                if i + j < n - 1:
                    small.append((v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)))
                for s in small:
                    b.add_triangle(mesh, *[b.add_vertex(*[float(x) for x in p]) for p in s], mat)
    return mesh


def _finish(b, size, depth):
    b.add_point_light((0.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
    b.add_directional_light((0.3, -1.0, 0.8), (0.9, 0.8, 0.7, 1.0))
    b.add_directional_light(*TOWARDS_CAMERA)
    b.finish(size[0], size[1], 60.0, 100.0, cam_pos=(0.1, 4.5, -4.2), cam_quat=DOWN45,
             dist_atten=(0.1, 0.05, 0.01), ambience=(0.3, 0.3, 0.3, 1.0), depth=depth)


def _built(b, rt, family, refractive, size):
    mats = _materials(rt, refractive)
    if family == "tess":
        meshes = [_tess_cube(b, 1.0, mats[0])]
        places = [(0, (-0.7, 0.0, 0.0)), (0, (0.9, 0.5, 1.4))]
    else:
        meshes = [b.build_cube(1.0, mt, tile=tile) for mt, tile in zip(mats, ATLAS_TILES)]
        places = [(0, (-0.7, 0.0, 0.0)), (2, (0.9, 0.5, 1.4))][:1 if family == "one" else 2]
    for mesh, pos in places:
        b.set_trans(b.add_trans(meshes[mesh]), pos=pos)
    _finish(b, size, 3)


def chain_positions(n=40):
    """Cube centres whose Morton keys (z_order, rt_math.h: the raw float bits of x, y, z interleaved, x first)
    share successively longer prefixes: all coordinates in [64, 128), so sign and exponent agree,
    and centre k sets one more of the interleaved mantissa bits (x has 13 of them in the key, y and z
    12 each: 37 in all), the next one left clear.  The ordered tree over them is a chain: depth n - 1.
    The mantissa bits below the key's (10 of x: up to 2^-7 here) hold a different offset per centre and
    axis, so that no two cubes share a face plane."""
    pos, bits = [], [0, 0, 0]
    used = [13, 12, 12]
    for k in range(n):
        axis, lvl = k % 3, k // 3
        if lvl >= used[axis]:
            break
        pos.append([64.0 * (1.0 + b / 2.0 ** 13) + ((37 * k + 101 * a) % 1000) * 2.0 ** -17 for a, b in enumerate(bits)])
        bits[axis] |= 1 << (12 - lvl)
    return np.array(pos, np.float32)


def morton_keys(centres):
    """z_order (rt_math.h) of float32 centres: x bit 31 - k at key bit 63 - 3 k (k < 22), y at 62 - 3 k, z at
    61 - 3 k (k < 21).  Sorted, as Python ints."""
    keys = []
    for x, y, z in np.ascontiguousarray(centres, np.float32).view(np.uint32).tolist():
        key = 0
        for k in range(22):
            key |= ((x >> (31 - k)) & 1) << (63 - 3 * k)
            if k < 21:
                key |= ((y >> (31 - k)) & 1) << (62 - 3 * k) | ((z >> (31 - k)) & 1) << (61 - 3 * k)
        keys.append(key)
    return sorted(keys)


def radix_tree_depth(keys):
    """Internal nodes on the longest root-leaf path of the radix tree over sorted keys (equal keys: told
    apart by index, a balanced subtree -- fnode_delta, rt_bvh.h)."""
    if len(keys) < 2:
        return 0
    if keys[0] == keys[-1]:
        return int(np.ceil(np.log2(len(keys))))
    top = (keys[0] ^ keys[-1]).bit_length() - 1
    split = next(i for i in range(1, len(keys)) if (keys[i] >> top) & 1)
    return 1 + max(radix_tree_depth(keys[:split]), radix_tree_depth(keys[split:]))


FT_MAX_DEPTH = 31      # rt_runtime.cpp: the fast traversal's stack


def scene_ftree(s):
    """SceneView::ftree as view_of sets it: at least two leaves and an ordered tree no deeper than the
    fast traversal's stack.  (Cube instances without rotation: the box centre is the instance position.)"""
    pos = s.export("instances")[:, 4:7]
    return int(len(pos) >= 2 and radix_tree_depth(morton_keys(pos)) <= FT_MAX_DEPTH)


def _chain(b, rt, refractive, size):
    mats = _materials(rt, refractive)
    small = b.build_cube(0.25, mats[0], tile=ATLAS_TILES[0])
    floor = [b.build_cube(1.0, mt, tile=tile) for mt, tile in zip(mats[1:], ATLAS_TILES[1:])]
    chain = chain_positions()
    for p in chain:
        b.set_trans(b.add_trans(small), pos=[float(x) for x in p])
    for i in range(22):
        for j in range(22):
            b.set_trans(b.add_trans(floor[(i + j) % 2]), pos=(117.0 + i, 126.0, 120.0 + j))
    c = [float(x) for x in chain[-1]]
    b.add_point_light((c[0] - 3.0, c[1] + 8.0, c[2] - 4.0), (1.0, 1.0, 1.0, 1.0))
    b.add_directional_light((0.3, -1.0, 0.8), (0.9, 0.8, 0.7, 1.0))
    b.add_directional_light(*TOWARDS_CAMERA)
    b.finish(size[0], size[1], 60.0, 100.0, cam_pos=(c[0] - 0.5, c[1] - 0.5, c[2] - 4.0),
             dist_atten=(0.1, 0.05, 0.01), ambience=(0.3, 0.3, 0.3, 1.0), depth=3)


def _field_json(tmp_dir, family, refractive):
    d = json.load(open(scene_path("world8_stress_tex")))
    d["grid_size"] = FIELD_GRID[family]
    for c in d["cubes"][:-1]:
        c.update(Ks=[80, 80, 80, 255], alpha=4.0)
    (dv, dc) = TOWARDS_CAMERA
    d["lights"]["directional"].append({"dir": list(dv), "col": [round(255 * x) for x in dc]})
    if refractive:       # the top layer: rays refract into the stack below it
        d["cubes"][-1].update(Kt=[0.5, 0.6, 0.7, 1], eta=1.3)
    p = os.path.join(str(tmp_dir), "%s%s.json" % (family, "_r" if refractive else ""))
    with open(p, "w") as f:
        json.dump(d, f)
    return p


def parse(name):
    parts = name.split("_")
    return parts[0], "r" in parts[1:], "rot" in parts[1:]


def rotated_instance(s):
    """The instance the `_rot` scenes turn: the top cube of the column nearest the origin (in view)."""
    inst = s.export("instances")
    d = np.hypot(inst[:, 4], inst[:, 6])
    col = np.flatnonzero(d == d.min())
    return int(col[np.argmax(inst[col, 5])])


def build_scene(name, size, rt, oracle, tmp_dir):
    """(product scene, oracle scene) named `name` (a family above, `_r`, `_rot`) at `size`; oracle None: the product scene alone
    (host only: scenes load without a device)."""
    family, refractive, rot = parse(name)
    if family in FIELD_GRID:
        path = _field_json(tmp_dir, family, refractive)
        s = rt.Scene.load_json(path, *size)
        o = oracle.load(path, *size) if oracle else None
    else:
        if oracle:
            from twin import Twin
            b = Twin(rt, oracle)
            s, o = b.gpu, b.orc
        else:
            b = s = rt.Scene.create()
            o = None
        if family == "chain":
            _chain(b, rt, refractive, size)
        else:
            _built(b, rt, family, refractive, size)
    atlas = make_atlas.atlas()
    s.set_atlas(atlas)
    if o:
        o.set_atlas(atlas)
    if rot:
        k = rotated_instance(s)
        s.set_trans(k, quat=ROT45)
        if o:
            o.set_trans(k, quat=ROT45)
    return s, o


def second_camera(name, s):
    """A pose inside or beside the scene from which part of the frame hits and part misses."""
    family, _, _ = parse(name)
    if family in FIELD_GRID:
        # above the middle of the field with the scene's own orientation, as test_gpu_large.py looks at its fields
        return (0.0, float(s.camera()[0][1]), -0.25 * FIELD_GRID[family]), tuple(float(x) for x in s.camera()[1])
    if family == "chain":      # above the end of the chain, looking 20 degrees down at it and over the floor's far edge
        c = [float(x) for x in chain_positions()[-1]]
        return (c[0] - 0.3, c[1] + 1.5, c[2] - 4.0), (0.1736482, 0.0, 0.0, 0.9848078)
    return (2.6, 1.0, -1.5), (0.0, -0.3826834, 0.0, 0.9238795)


# ---- the plan's inputs, from a host scene ----------------------------------------------------
def scene_ns(s, depth):
    """shade_shortcuts' ns (rt_plan.h): 0 without a refractive material (any Kt channel > 0), else max(depth, 1)."""
    opaque = not (s.export("materials")[:, 16:20] > 0).any()
    return 0 if opaque else max(depth, 1)


def plan_key_args(s, recipe):
    """`plan_host key`'s arguments for `recipe` on product scene `s`, as upload and view_of (rt_runtime.cpp)
    set them: n_real = n_inst (every instance box is proper), ftree (scene_ftree), tri_ax and a
    non-negative pruning slack when every rotation is the identity."""
    i = s.info()
    n = i["n_instances"]
    ident = bool((s.export("instances")[:, 0:4] == np.array([0, 0, 0, 1], np.float32)).all())
    return [n, n, scene_ftree(s), int(ident and i["n_tris"] > 0), int(recipe.use_bvh), i["n_tris"], i["n_mats"], i["n_lights"],
            i["n_meshes"], 0.5 if ident else -1.0, recipe.spp, int(recipe.tex), int(recipe.stats), int(recipe.prof),
            scene_ns(s, recipe.depth), int(recipe.no_part), 0]


def plan_key(plan, s, recipe):
    f = [int(v) for v in plan("key", *plan_key_args(s, recipe)).split()]
    return dict(zip(("ns_bucket", "lds", "mode", "shm", "part_k", "sky", "sky_brute"), f))
