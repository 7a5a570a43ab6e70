"""Scenes and expected records for the per-frame BVH build's tests (test_bvh_host.py on the CPU,
test_gpu_bvh_build.py on the device).  TEST INFRASTRUCTURE.

Scenes are built over twin.Twin (product and oracle get the same builder calls) or on the oracle
alone.  The expected arrays -- the heap's child-pair boxes, the leaf -> instance map and the
ordered radix tree of the fast kernels -- come from the oracle's BVH (OracleScene.bvh(): the
reference's boxes in storage order and its `ordering`) and numpy; no product code is involved.

Layout of the expectations (what Scene.export("bvh_*") must return):
  pairs      [n, 12] float32: heap node k (1 <= k < 2n) is storage box 2n-1-k; its component c of
             (mn.xyz, mx.xyz) sits at [k >> 1, (k & 1) + 2 c].  A degenerate box, and node 0, is
             mn = +inf, mx = -inf.
  leaf_inst  [n] int32: leaf_inst[k - n] = ordering[2n-1-k].
  fnode      [n_real - 1, 16]: the ordered tree over the real leaves, storage [0, n_real), defined
             top-down: position p carries the augmented key (key_p << 32) | p; a node over
             [first, last] splits at the highest differing bit of its end keys, gamma being the last
             position with that bit clear; the node of [first, gamma] has index gamma, the node of
             [gamma+1, last] index gamma+1, the root 0.  Record i: child A = [gamma+1, last], child
             B = [first, gamma]; 12 floats interleaved as in pairs, then int32 {A, B, 0, 0} with a
             one-leaf child as -1 - ordering[p].
"""
import bisect

import numpy as np

INF = np.float32(np.inf)
PLACEMENTS = ("lattice", "one_point", "scattered")
RULES = ("seventh", "all", "all_but_one")

# (n_inst, placement, degenerate rule): the smallest sizes on each side of every switch of the build
CASES = ([(n, "lattice", "seventh") for n in (1, 2, 3, 33, 64, 65, 1000, 1024, 1025, 2048, 2049, 8192, 8193, 20000)]
         + [(n, "one_point", "seventh") for n in (3, 65, 1025, 2049, 8193)]
         + [(n, "scattered", "seventh") for n in (65, 1025, 8193)]
         + [(n, "lattice", r) for r in ("all", "all_but_one") for n in (3, 70)])
MOVING = (70, 8193)              # lattice, every 7th degenerate, three frame slots
RAY_SCENES = (70, 1100, 2100)    # lattice, every 7th degenerate, 96 x 64


def case_id(c):
    return "%d-%s-%s" % c


def padded(n_inst):
    n = 1
    while n < n_inst:
        n *= 2
    return n


def expected_form(n_inst):
    """The build a scene of n_inst instances must take (rt_amd.h, RT_EXPORT_BVH_INFO)."""
    n = padded(n_inst)
    if n > 8192:
        return 4                                   # grid-wide
    if n > 2048:
        return 3                                   # one workgroup, tree in HBM
    return 1 if n >= 64 and 64 * ((n_inst + 63) // 64) <= 1024 else 2


def degenerate_mask(n_inst, rule):
    i = np.arange(n_inst)
    if rule == "seventh":
        return (i % 7 == 0) | (i == n_inst - 1)
    if rule == "all":
        return np.ones(n_inst, bool)
    assert rule == "all_but_one"
    return i != n_inst // 2


def lattice_side(n_real):
    """Cells per axis of the lattice: about three real instances per cell, so most keys are tied
    while the cells still give many distinct keys."""
    return max(1, int(round((n_real / 3.0) ** (1.0 / 3.0))))


def layout(n_inst, placement, rule):
    """Deterministic instance table of a case: mesh (0: unit cube, 1: cube of scale 2, 2: empty mesh),
    position and unit quaternion per instance, and the lattice side."""
    rng = np.random.default_rng([n_inst, PLACEMENTS.index(placement), RULES.index(rule)])
    deg = degenerate_mask(n_inst, rule)
    mesh = np.where(rng.random(n_inst) < 0.3, 1, 0)
    quat = np.tile(np.array([0, 0, 0, 1], np.float32), (n_inst, 1))
    side = lattice_side(int((~deg).sum()))
    if placement == "lattice":
        pos = (2.0 * (rng.integers(0, side, (n_inst, 3)) - side // 2)).astype(np.float32)
        real = np.flatnonzero(~deg)
        for j, i in enumerate(real):                 # exact duplicates: same mesh, same pose
            if j and i % 5 == 2:
                src = real[rng.integers(0, j)]
                mesh[i], pos[i] = mesh[src], pos[src]
    elif placement == "one_point":
        pos = np.tile(np.array([2.0, -4.0, 6.0], np.float32), (n_inst, 1))
    else:
        assert placement == "scattered"
        pos = rng.uniform(-40.0, 40.0, (n_inst, 3)).astype(np.float32)
        q = rng.normal(size=(n_inst, 4))
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        quat[1::2] = q[1::2]
    mesh[deg] = 2
    return {"mesh": mesh, "pos": pos, "quat": quat, "side": side, "degenerate": deg}


def _mat(Kd, Kr=(0, 0, 0, 0)):
    return np.array([0, 0, 0, 0, .1, .1, .1, 1] + list(Kd) + [0] * 8 + list(Kr) + [0.0, 1.0], np.float32)


def build(b, n_inst, placement="lattice", rule="seventh", width=8, height=8, lit=False):
    """The case's scene through the SceneBuilder calls of `b` (a Twin, an OracleScene or a product
    Scene).  lit: one point light and reflective materials at depth 2 (the ray tests); the camera
    looks at the lattice from outside it either way.  Returns the layout."""
    L = layout(n_inst, placement, rule)
    kr = (.4, .4, .4, 1) if lit else (0, 0, 0, 0)
    meshes = [b.build_cube(1.0, _mat((.8, .3, .2, 1), kr)), b.build_cube(2.0, _mat((.2, .4, .8, 1), kr)), b.create_mesh()]
    for i in range(n_inst):
        t = b.add_trans(meshes[L["mesh"][i]])
        b.set_trans(t, pos=L["pos"][i], quat=L["quat"][i])
    if lit:
        b.add_point_light((3.0, 2.0 * L["side"] + 4.0, -2.0 * L["side"] - 3.0), (1.0, 0.95, 0.9, 1.0))
    dist = L["side"] + (L["side"] + 1.5) / 0.4
    b.finish(width, height, 0.5, 20.0, cam_pos=(0.3, 0.2, -dist), ambience=(0.2, 0.2, 0.2, 1.0), depth=2 if lit else 0)
    return L


def move_tenth(b, L, frame):
    """Before frame `frame`: a tenth of the instances move onto other instances' centres (new tied
    keys), by set_trans on `b`; the layout follows."""
    n = L["pos"].shape[0]
    rng = np.random.default_rng([n, 1000 + frame])
    movers = rng.choice(n, max(1, n // 10), replace=False)
    for t, src in zip(movers, rng.integers(0, n, movers.size)):
        L["pos"][t] = L["pos"][src]
        b.set_trans(int(t), pos=L["pos"][t])


def coincident_hit_share(L, hit_inst):
    """(share of the hit pixels whose instance has the mesh and pose of another instance, share of
    the pixels that hit anything)."""
    rows = np.concatenate([L["mesh"][:, None].astype(np.float32), L["pos"], L["quat"]], axis=1)
    _, inv, cnt = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    twin = cnt[inv.ravel()] > 1
    hit = hit_inst[hit_inst >= 0]
    return (float(twin[hit].mean()) if hit.size else 0.0), float((hit_inst >= 0).mean())


def ordered_tree(keys):
    """The top-down definition: for sorted `keys` (ints) the list of (index, first, last, gamma) of
    every internal node, parents before children."""
    nr = len(keys)
    aug = [(int(k) << 32) | p for p, k in enumerate(keys)]
    nodes = []
    todo = [(0, 0, nr - 1)] if nr >= 2 else []
    while todo:
        i, first, last = todo.pop()
        bit = (aug[first] ^ aug[last]).bit_length() - 1
        gamma = bisect.bisect_left(aug, ((aug[first] >> bit) | 1) << bit, first, last + 1) - 1
        nodes.append((i, first, last, gamma))
        if gamma > first:
            todo.append((gamma, first, gamma))
        if last > gamma + 1:
            todo.append((gamma + 1, gamma + 1, last))
    return nodes


class Expected:
    """The records the device must hold for the oracle scene's current poses."""

    def __init__(self, oracle, orc_scene):
        boxes, order = orc_scene.bvh()
        n = order.shape[0]
        nd = boxes[:, 6] != 0
        self.n_leaf, self.n_inst, self.order = n, orc_scene.n_instances, order
        self.n_real = int(nd[:n].sum())
        # the real leaves are storage [0, n_real), exactly the leaves with nd = 1
        assert nd[:self.n_real].all() and not nd[self.n_real:n].any()
        stored = np.where(nd[:, None], boxes[:, :6], np.array([INF] * 3 + [-INF] * 3, np.float32)).astype(np.float32)
        node = np.concatenate([np.array([[INF] * 3 + [-INF] * 3], np.float32), stored[::-1]])   # heap node k = row k
        self.pairs = np.ascontiguousarray(node.reshape(n, 2, 6).transpose(0, 2, 1)).reshape(n, 12)
        self.leaf_inst = np.ascontiguousarray(order[::-1])
        # Morton keys of the real leaves: gen_morton's argument, the negated box centre
        lb = boxes[:self.n_real, :6]
        centre = np.float32(0.5) * (lb[:, :3] + lb[:, 3:6])
        self.keys = oracle.kat("zorder", -centre) if self.n_real else np.zeros(0, np.uint64)
        assert (self.keys[1:] >= self.keys[:-1]).all()
        self.nodes = ordered_tree([int(k) for k in self.keys])
        nr = self.n_real
        self.fnode = np.zeros((max(nr - 1, 0), 16), np.float32)
        refs = self.fnode.view(np.int32)[:, 12:]
        depth = {0: 1}
        rng_box = {}                                 # node index -> box of its range (exact min / max)

        def child_box(lo, hi, idx):
            return lb[lo] if lo == hi else rng_box[idx]
        for i, first, last, gamma in reversed(self.nodes):      # children before parents
            a, b = child_box(gamma + 1, last, gamma + 1), child_box(first, gamma, gamma)
            self.fnode[i, 0:12:2], self.fnode[i, 1:12:2] = a, b
            rng_box[i] = np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])])
            refs[i, 0] = -1 - order[last] if gamma + 1 == last else gamma + 1
            refs[i, 1] = -1 - order[first] if gamma == first else gamma
        for i, first, last, gamma in self.nodes:                 # parents before children
            for c, lo, hi in ((gamma + 1, gamma + 1, last), (gamma, first, gamma)):
                if lo != hi:
                    depth[c] = depth[i] + 1
        self.fdepth = max(depth.values()) if nr >= 2 else 0
        self.ftree = int(nr >= 2 and self.fdepth <= 31)

    def tied_share(self):
        """Share of the real leaves whose key another real leaf has too."""
        if not self.n_real:
            return 0.0
        _, inv, cnt = np.unique(self.keys, return_inverse=True, return_counts=True)
        return float((cnt[inv] > 1).mean())

    def dfs_leaves(self):
        """Storage positions of the leaves in the order a child-A-first walk of fnode meets them."""
        if self.n_real < 2:
            return list(range(self.n_real))
        where = {int(inst): p for p, inst in enumerate(self.order[:self.n_real])}
        refs = self.fnode.view(np.int32)[:, 12:14]
        out, todo = [], [0]
        while todo:
            r = todo.pop()
            if r < 0:
                out.append(where[-1 - r])
            else:
                todo += [int(refs[r, 1]), int(refs[r, 0])]       # A is popped first
        return out


def check_export(scene, exp, ctx=""):
    """The product scene's exported tree against the expectations; returns the info dict.  Heap
    boxes, leaf map and the ordered tree's references bit for bit; the ordered tree's boxes as
    float values (-0 equals +0: the device groups a range's min / max differently from numpy)."""
    info = scene.export("bvh_info")
    assert info["form"] == expected_form(exp.n_inst), (ctx, info)
    for k in ("n_leaf", "n_inst", "n_real", "fdepth", "ftree"):
        assert info[k] == getattr(exp, k), (ctx, k, info, getattr(exp, k))
    pairs, leaf, fnode = scene.export("bvh_pairs"), scene.export("bvh_leaf_inst"), scene.export("bvh_fnode")
    bad = np.flatnonzero(leaf != exp.leaf_inst)
    assert bad.size == 0, (ctx, "leaf_inst", bad.size, bad[:4], leaf[bad[:4]], exp.leaf_inst[bad[:4]])
    bad = np.flatnonzero((pairs.view(np.uint32) != exp.pairs.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (ctx, "pairs", bad.size, bad[:4])
    assert fnode.shape == exp.fnode.shape, (ctx, fnode.shape)
    bad = np.flatnonzero((fnode.view(np.int32)[:, 12:] != exp.fnode.view(np.int32)[:, 12:]).any(axis=1))
    assert bad.size == 0, (ctx, "fnode refs", bad.size, bad[:4])
    bad = np.flatnonzero((fnode[:, :12] != exp.fnode[:, :12]).any(axis=1))
    assert bad.size == 0, (ctx, "fnode boxes", bad.size, bad[:4])
    return info
