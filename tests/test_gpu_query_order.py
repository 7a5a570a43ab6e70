"""The coherence order of ray queries on the GPU (rt_query_set_order, RT_QUERY_ORDER_SORTED; Scene.query's
reorder=): a sorted batch gives every ray the result the same call gives in caller order, bit for bit and
at the ray's own index, over every batch shape, kernel form and pointer side; rt_query_last reports the
sort; the device's keys are the host program's; counted queries and one-wave batches stay in caller
order; the mode is scene state and touches nothing but rt_query.

The reference in every case is the same call with RT_QUERY_ORDER_CALLER.  Default scene: world8_stress
at 96 x 64 (6144 rays) from the value check's camera."""
import numpy as np
import pytest

import query_cases as qc
import query_order_lib as ql
from conftest import scene_path
from kernel_recipes import build_scene

pytestmark = pytest.mark.gpu
ALL = ("t", "inst", "tri", "uv", "normal", "hit", "rays_out")
QT_ORDERED, QT_HEAP, QT_BRUTE = 0, 1, 2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, keys=ALL, ctx=""):
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(want[k])), (ctx, k, int((bits(got[k]) != bits(want[k])).reshape(len(want[k]), -1).any(axis=1).sum()))


def both(s, ctx, want=ALL, sorts=True, **kw):
    """The query in caller order and sorted (reorder=True): equal in every bit; returns the caller-order result.
    sorts: whether the sorted call has to have sorted (n > 64, uncounted)."""
    a = s.query(want=want, **kw)
    last = s.query_last()
    assert (last["sorted"], last["ordered"]) == (0, 0), ctx
    b = s.query(want=want, reorder=True, **kw)
    last = s.query_last()
    assert (last["sorted"], last["ordered"]) == (int(sorts), int(sorts)), (ctx, last)
    assert_same(b, a, keys=want, ctx=ctx)
    return a


class W8:
    pass


@pytest.fixture(scope="module")
def w8(gpu):
    c = W8()
    W, H = qc.VALUES_SIZE
    c.s = gpu.Scene.load_json(scene_path(qc.VALUES_SCENE), W, H)
    c.s.set_camera(*qc.VALUES_CAMERA)
    c.pix = qc.all_pixels(W, H)
    c.rays = c.s.query(pixels=c.pix, want=("rays_out",))["rays_out"]
    c.n = len(c.pix)
    c.perm = np.random.default_rng(qc.PERM_SEED).permutation(c.n)
    c.o_p, c.d_p = c.rays[c.perm, 0:3].copy(), c.rays[c.perm, 3:6].copy()
    c.ref = c.s.query(origins=c.o_p, dirs=c.d_p, want=ALL)             # caller order, the whole permuted frame
    assert (c.ref["hit"] != 0).sum() > 1000 and (c.ref["hit"] == 0).sum() > 100
    return c


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ql.HostProgram(tmp_path_factory.mktemp("qorder_gpu"))


# ---- 1. bit equality, sorted against caller order ----------------------------------------------------------
def test_permuted_frame(w8):
    a = both(w8.s, "permuted", origins=w8.o_p, dirs=w8.d_p)
    assert_same(a, w8.ref)
    m = w8.n - qc.DROPPED
    assert m % 64 != 0
    both(w8.s, "permuted, rays dropped", origins=w8.o_p[:m], dirs=w8.d_p[:m])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_short_batches(w8, n):
    a = both(w8.s, "n = %d" % n, sorts=n > 64, origins=w8.o_p[:n], dirs=w8.d_p[:n])
    assert_same(a, {k: w8.ref[k][:n] for k in ALL}, ctx="n = %d against the frame's" % n)


def test_permuted_pixel_list(w8):
    a = both(w8.s, "pixel mode", pixels=w8.pix[w8.perm])
    assert np.array_equal(bits(a["rays_out"]), bits(w8.rays[w8.perm]))


def _tmax_for(t):
    k = np.arange(len(t)) % 4
    return np.select([k == 0, k == 1, k == 2], [np.float32(0.5) * t, t, np.nextafter(t, np.float32(np.inf))],
                     np.float32(np.inf)).astype(np.float32), k


def test_tmax_and_any_hit(w8):
    tmax, k = _tmax_for(w8.ref["t"])
    expect = (w8.ref["inst"] >= 0) & (k >= 2)                          # a hit exactly when t < tmax
    assert (expect & (k == 2)).sum() > 300 and ((w8.ref["inst"] >= 0) & (k == 1)).sum() > 300
    a = both(w8.s, "tmax", origins=w8.o_p, dirs=w8.d_p, tmax=tmax)
    assert np.array_equal(a["hit"] != 0, expect)
    for kw in (dict(tmax=tmax), {}):
        h = both(w8.s, "any_hit", want=("hit", "rays_out"), origins=w8.o_p, dirs=w8.d_p, any_hit=True, **kw)
        assert np.array_equal(h["hit"] != 0, expect if kw else w8.ref["hit"] != 0)
        assert w8.s.query_last()["any_hit"] == 1


def test_brute_force(w8):
    a = both(w8.s, "use_bvh = 0", origins=w8.o_p, dirs=w8.d_p, use_bvh=False)
    assert w8.s.query_last()["tree"] == QT_BRUTE
    assert np.array_equal(a["hit"], w8.ref["hit"])


@pytest.mark.parametrize("form", ["small", "persistent"])
def test_both_forms(w8, monkeypatch, form):
    monkeypatch.setenv("RT_QUERY_FORM", form)
    for kw in ({}, dict(use_bvh=False), dict(any_hit=True)):
        want = ("hit",) if kw.get("any_hit") else ALL
        both(w8.s, "%s %s" % (form, kw), want=want, origins=w8.o_p, dirs=w8.d_p, **kw)
        last = w8.s.query_last()
        assert last["persistent"] == int(form == "persistent") and last["ordered"] == 1
        assert last["lds"] == int(form == "persistent")                # (world8_stress's image fits LDS)


def test_device_pointers(w8, gpu):
    import torch
    n = w8.n - qc.DROPPED
    dt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}
    o_d, d_d = torch.from_numpy(w8.o_p[:n]).cuda(), torch.from_numpy(w8.d_p[:n]).cuda()
    got = []
    for reorder in (False, True):
        out = {k: torch.full((n, c) if c > 1 else (n,), 77, dtype=dt[t], device="cuda") for k, (c, t) in gpu.QUERY_OUTPUTS.items()}
        torch.cuda.synchronize()
        w8.s.query_device(n, origin_ptr=o_d.data_ptr(), dir_ptr=d_d.data_ptr(), reorder=reorder,
                          **{k + "_ptr": v.data_ptr() for k, v in out.items()})
        assert w8.s.query_last()["sorted"] == int(reorder)
        got.append({k: v.cpu().numpy() for k, v in out.items()})
    assert_same(got[1], got[0], ctx="device pointers")
    assert_same(got[0], {k: w8.ref[k][:n] for k in ALL}, ctx="device pointers against host pointers")
    # pixel mode and tmax from device memory
    px_d, tm_d = torch.from_numpy(w8.pix[w8.perm]).cuda(), torch.from_numpy(_tmax_for(w8.ref["t"])[0]).cuda()
    hits = []
    for reorder in (False, True):
        hit = torch.full((w8.n,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        w8.s.query_device(w8.n, pixel_ptr=px_d.data_ptr(), tmax_ptr=tm_d.data_ptr(), any_hit=True, hit_ptr=hit.data_ptr(), reorder=reorder)
        hits.append(hit.cpu().numpy())
    assert np.array_equal(hits[0], hits[1]) and 0 < hits[0].sum() < w8.n and hits[0].max() == 1


def test_one_instance_scene_takes_the_heap_walk(gpu, tmp_path):
    size = (64, 48)
    s, _ = build_scene("one", size, gpu, None, tmp_path)
    pix = qc.all_pixels(*size)
    perm = np.random.default_rng(qc.PERM_SEED).permutation(len(pix))
    rays = s.query(pixels=pix, want=("rays_out",))["rays_out"][perm]
    a = both(s, "one instance", origins=rays[:, 0:3], dirs=rays[:, 3:6])
    assert s.query_last()["tree"] == QT_HEAP
    assert 50 < (a["hit"] != 0).sum() < len(pix)
    both(s, "one instance, occlusion", want=("hit",), origins=rays[:, 0:3], dirs=rays[:, 3:6], any_hit=True)


def test_rotated_instances(gpu, oracle):
    from test_gpu_query import _rotated12
    size = (64, 48)
    s, _ = _rotated12(gpu, oracle, size)
    pix = qc.all_pixels(*size)
    perm = np.random.default_rng(qc.PERM_SEED).permutation(len(pix))
    rays = s.query(pixels=pix, want=("rays_out",))["rays_out"][perm]
    a = both(s, "rotated", origins=rays[:, 0:3], dirs=rays[:, 3:6])
    assert s.query_last()["tree"] == QT_ORDERED
    assert 200 < (a["hit"] != 0).sum() < len(pix)
    # scattered origins: from the hit points back along the normals' hemisphere
    h = a["hit"] != 0
    p = (a["rays_out"][h, 0:3] + a["t"][h, None] * a["rays_out"][h, 3:6] + np.float32(1e-3) * a["normal"][h]).astype(np.float32)
    d = (a["normal"][h] + np.float32(0.5) * np.random.default_rng(3).normal(size=(h.sum(), 3))).astype(np.float32)
    both(s, "rotated, from the hit points", origins=p, dirs=d)


def _hostile(w8):
    """The permuted frame with 1% of its rays replaced by rejected rays and 5% by exact duplicates of other rays."""
    rng = np.random.default_rng(11)
    o, d = w8.o_p.copy(), w8.d_p.copy()
    slots = rng.permutation(w8.n)
    n_rej, n_dup = w8.n // 100, w8.n // 20
    rej, dup = slots[:n_rej], slots[n_rej:n_rej + n_dup]
    src = slots[n_rej + n_dup:][rng.integers(0, w8.n - n_rej - n_dup, n_dup)]
    o[dup], d[dup] = o[src], d[src]
    bad = ql.REJECTED_RAYS[np.arange(n_rej) % len(ql.REJECTED_RAYS)]
    o[rej], d[rej] = bad[:, 0:3], bad[:, 3:6]
    return o, d, rej, dup, src


def test_rejected_rays_and_duplicates(w8):
    o, d, rej, dup, src = _hostile(w8)
    a = both(w8.s, "rejected and duplicate rays", origins=o, dirs=d)
    assert not a["hit"][rej].any() and np.isposinf(a["t"][rej]).all() and (a["inst"][rej] == -1).all()
    assert_same({k: a[k][dup] for k in ALL}, {k: a[k][src] for k in ALL}, ctx="duplicates")
    keep = np.ones(w8.n, bool)
    keep[rej] = keep[dup] = False
    assert_same({k: a[k][keep] for k in ALL}, {k: w8.ref[k][keep] for k in ALL}, ctx="the untouched rays")
    both(w8.s, "rejected and duplicate rays, occlusion", want=("hit",), origins=o, dirs=d, any_hit=True)


# ---- 2. rt_query_last -------------------------------------------------------------------------------------------
def test_query_last_reports_the_sort(w8, gpu, host):
    o, d, rej, dup, src = _hostile(w8)
    r = w8.s.query(origins=o, dirs=d, want=("rays_out", "hit"), reorder=True)
    last = w8.s.query_last(want_order=True)
    assert (last["ordered"], last["sorted"], last["tree"], last["counted"], last["any_hit"]) == (1, 1, QT_ORDERED, 0, 0)
    assert last["blocks"] == -(-w8.n // 256) and last["persistent"] == 0
    order = last["order"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(w8.n))            # a permutation of 0..n-1
    box = last["bounds"]
    assert np.isfinite(box).all() and (box[3:6] > box[0:3]).all()
    inst = w8.s.export("instances")[:, 4:7]
    assert (box[0:3] <= inst.min(axis=0)).all() and (box[3:6] >= inst.max(axis=0)).all()
    keys = host.keys(r["rays_out"][order], box)
    assert (keys[1:] >= keys[:-1]).all()                               # non-decreasing host keys
    tie = keys[1:] == keys[:-1]
    assert tie.sum() >= len(dup) // 2                                  # (the duplicates tie, at least)
    assert (order[1:][tie] > order[:-1][tie]).all()                    # equal keys in index order
    rejected = (keys & ql.REJECTED_BIT) != 0
    assert rejected.sum() == len(rej) and rejected[-len(rej):].all()   # rejected rays last
    assert set(order[-len(rej):].tolist()) == set(rej.tolist())
    # the size check of the order's destination
    buf = np.zeros(w8.n, np.uint32)
    rtamd = gpu
    assert rtamd.lib().rt_query_last(w8.s._h, None, None, buf.ctypes.data, w8.n - 1) == rtamd.RT_ERR_ARG
    assert rtamd.lib().rt_query_last(w8.s._h, None, None, buf.ctypes.data, w8.n) == rtamd.RT_OK
    assert np.array_equal(buf, last["order"])
    # one wave, or a counted call: not sorted, the unordered kernel
    w8.s.set_query_order(rtamd.RT_QUERY_ORDER_SORTED)
    try:
        w8.s.query(origins=o[:64], dirs=d[:64])
        last = w8.s.query_last(want_order=True)
        assert (last["ordered"], last["sorted"], last["order"]) == (0, 0, None) and not last["bounds"].any()
        w8.s.query(origins=o, dirs=d, stats=True)
        last = w8.s.query_last()
        assert (last["ordered"], last["sorted"], last["counted"], last["tree"]) == (0, 0, 1, QT_HEAP)
        w8.s.query(origins=o[:65], dirs=d[:65])
        assert w8.s.query_last()["sorted"] == 1
    finally:
        w8.s.set_query_order(rtamd.RT_QUERY_ORDER_CALLER)


# ---- 3. the device's keys ----------------------------------------------------------------------------------------
def test_device_keys_equal_the_host_programs(w8, gpu, host):
    box = ql.scene_box(w8.s.arrays())
    eo, ed = ql.edge_rays(box)
    rays = np.concatenate([w8.rays, ql.as_traced(eo, ed)])
    boxes = np.tile(box, (len(rays), 1)).astype(np.float32)
    boxes[-7:] = np.float32([[0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [-1, -1, -1, 1, 1, 1], [0, 0, 0, 1e30, 1e-30, 1],
                             [-np.inf, 0, 0, np.inf, 1, 1], [np.nan] * 6, [-3e38, -3e38, -3e38, 3e38, 3e38, 3e38]])
    dev = gpu.kat_device("ray_key", rays, boxes)
    want = host.keys(rays, boxes)
    assert np.array_equal(dev, want), int((dev != want).sum())
    assert ((want & ql.REJECTED_BIT) != 0).sum() == len(ql.REJECTED_RAYS)
    assert len(np.unique(want)) > 4000                                  # (the frame's rays spread over the direction codes)


# ---- 4. counted queries -------------------------------------------------------------------------------------------
def test_counted_query_is_the_caller_orders(w8):
    a = w8.s.query(origins=w8.o_p, dirs=w8.d_p, want=ALL, stats=True)
    b = w8.s.query(origins=w8.o_p, dirs=w8.d_p, want=ALL, stats=True, reorder=True)
    assert_same(b, a, ctx="counted")
    for k in ("rays", "nodes", "leaves", "tri_tests"):
        assert a["stats"][k] == b["stats"][k] and a["stats"][k] > 0, k
    assert a["stats"]["rays"] == w8.n


# ---- 5. the mode is scene state ---------------------------------------------------------------------------------
def test_mode_is_scene_state(gpu, w8):
    W, H = qc.VALUES_SIZE
    s = gpu.Scene.load_json(scene_path(qc.VALUES_SCENE), W, H)
    other = gpu.Scene.load_json(scene_path(qc.VALUES_SCENE), W, H)
    for x in (s, other):
        x.set_camera(*qc.VALUES_CAMERA)
    first = s.render(spp=1, want=("rgba",), stats=False)["rgba"]
    lt = s.last_trace()
    q = dict(origins=w8.o_p, dirs=w8.d_p, want=ALL)
    s.set_query_order(gpu.RT_QUERY_ORDER_SORTED)
    for _ in range(2):                                                  # it persists across calls
        assert_same(s.query(**q), w8.ref, ctx="sorted by the scene's mode")
        assert s.query_last()["sorted"] == 1
    assert_same(s.query(reorder=True, **q), w8.ref)                     # reorder= in sorted mode: sorted, and the mode stays
    assert s.query_last()["sorted"] == 1
    s.query(**q)
    assert s.query_last()["sorted"] == 1
    other.query(**q)                                                    # a second scene is unaffected
    assert other.query_last()["sorted"] == 0
    assert s.last_trace() == lt                                         # no trace kernel was launched
    fr = s.render(spp=1, want=("rgba",), stats=False)["rgba"]
    assert fr.tobytes() == first.tobytes() and s.last_trace() == lt     # the frame after sorted queries
    s.set_query_order(gpu.RT_QUERY_ORDER_CALLER)
    s.query(**q)
    assert s.query_last()["sorted"] == 0
    s.query(reorder=True, **q)                                          # reorder= restores caller order
    assert s.query_last()["sorted"] == 1
    s.query(**q)
    assert s.query_last()["sorted"] == 0
    with pytest.raises(gpu.RtError) as e:
        s.set_query_order(2)
    assert e.value.code == gpu.RT_ERR_ARG
    # instances that move take the keys' box with them
    s.query(reorder=True, **q)
    b0 = s.query_last()["bounds"].copy()
    far = int(np.argmax(s.export("instances")[:, 4]))
    pos = s.export("instances")[far, 4:7].copy()
    pos[0] += 5.0
    s.set_trans(far, pos=pos)
    other.set_trans(far, pos=pos)
    a, b = other.query(**q), s.query(reorder=True, **q)
    assert_same(b, a, ctx="after a move")
    b1 = s.query_last()["bounds"]
    assert abs(b1[3] - (b0[3] + 5.0)) <= 1e-5 and np.array_equal(b1[[0, 1, 2, 4, 5]], b0[[0, 1, 2, 4, 5]])


# ---- 6. a split scene ---------------------------------------------------------------------------------------------
def test_split_scene_answers_like_the_unsplit(gpu, w8):
    W, H = qc.VALUES_SIZE
    s = gpu.Scene.load_json(scene_path(qc.VALUES_SCENE), W, H)
    s.set_camera(*qc.VALUES_CAMERA)
    s.set_devices([0], 3)                                               # three virtual ranks on one GPU
    frame = s.render(spp=1)["rgba"]
    got = s.query(origins=w8.o_p, dirs=w8.d_p, want=ALL, reorder=True)
    assert s.query_last()["sorted"] == 1
    assert_same(got, w8.ref, ctx="split scene")
    assert np.array_equal(s.render(spp=1)["rgba"], frame)
