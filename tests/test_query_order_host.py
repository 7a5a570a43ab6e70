"""The coherence order of ray queries (rt_query_set_order, RT_QUERY_ORDER_SORTED) on a machine without
a GPU: the entries are exported and listed and check their arguments before they need a device; the
ray key (csrc/rt_raykey.h) and query_order_plan (csrc/rt_plan.h), printed by
tests/query_order_host.cpp; and the coherence the key's order buys, measured with the oracle."""
import ctypes

import numpy as np
import pytest

import query_cases as qc
import query_order_lib as ql
from conftest import scene_path


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ql.HostProgram(tmp_path_factory.mktemp("qorder"))


@pytest.fixture(scope="module")
def world1(rt):
    return rt.Scene.load_json(scene_path("world1"), 16, 16)


# ---- the C ABI ---------------------------------------------------------------------------------
def test_order_symbols_exported_and_listed(rt):
    L = ctypes.CDLL(rt.LIB_PATH)
    for name in ("rt_query_set_order", "rt_query_last"):
        assert hasattr(L, name), name
        assert name in rt.SYMBOLS
    assert rt.lib().rt_abi_version() == 5                      # additive: the version stays
    assert (rt.RT_QUERY_ORDER_CALLER, rt.RT_QUERY_ORDER_SORTED) == (0, 1)


def test_set_order_checks_the_mode(rt, world1):
    f = rt.lib().rt_query_set_order
    try:
        assert f(world1._h, 1) == rt.RT_OK
        assert f(world1._h, 0) == rt.RT_OK
        for bad in (-1, 2):
            assert f(world1._h, bad) == rt.RT_ERR_ARG, bad
            assert rt.lib().rt_last_error()
        assert f(None, 0) == rt.RT_ERR_ARG
    finally:
        f(world1._h, 0)


def _device_opts(rt, n):
    """Device-pointer options with fake, non-null pointers: never dereferenced before the device is needed."""
    o = rt.QueryOpts()
    rt.lib().rt_query_opts_default(ctypes.byref(o))
    o.n, o.host = n, 0
    o.origin, o.dir, o.t = 0x1000, 0x2000, 0x3000
    return o


def test_sorted_mode_caps_the_batch_at_32_bit_indices(rt):
    s = rt.Scene.load_json(scene_path("world1"), 16, 16)
    s.set_query_order(rt.RT_QUERY_ORDER_SORTED)
    for n in (1 << 31, (1 << 31) + 5, 1 << 40):
        assert rt.lib().rt_query(s._h, ctypes.byref(_device_opts(rt, n)), None) == rt.RT_ERR_LIMIT, n
        assert b"2^31" in rt.lib().rt_last_error()
    # a bad argument is still a bad argument first
    o = _device_opts(rt, 1 << 31)
    o.t = None
    assert rt.lib().rt_query(s._h, ctypes.byref(o), None) == rt.RT_ERR_ARG
    # caller order has no such cap: the call goes on to need a device
    s.set_query_order(rt.RT_QUERY_ORDER_CALLER)
    if rt.device_count() == 0:
        assert rt.lib().rt_query(s._h, ctypes.byref(_device_opts(rt, 1 << 31)), None) == rt.RT_ERR_NODEV


def test_query_last_before_any_query(rt):
    s = rt.Scene.load_json(scene_path("world1"), 16, 16)
    v, b = np.zeros(8, np.int32), np.zeros(6, np.float32)
    # (with a device the scene is warmed at creation: by a frame, not by a query)
    assert rt.lib().rt_query_last(s._h, v.ctypes.data, b.ctypes.data, None, 0) == rt.RT_ERR_STATE
    with pytest.raises(rt.RtError) as e:
        s.query_last()
    assert e.value.code == rt.RT_ERR_STATE


def test_sorted_mode_without_gpu_fails_loudly(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is present")
    s = rt.Scene.load_json(scene_path("world1"), 16, 16)
    s.set_query_order(rt.RT_QUERY_ORDER_SORTED)
    n = 200
    with pytest.raises(rt.RtError) as e:
        s.query(origins=np.zeros((n, 3), np.float32), dirs=np.tile(np.float32([0, 0, 1]), (n, 1)))
    assert e.value.code == rt.RT_ERR_NODEV
    with pytest.raises(rt.RtError) as e:
        s.query(pixels=[(1, 2)] * n, reorder=True)
    assert e.value.code == rt.RT_ERR_NODEV
    assert s._query_order == rt.RT_QUERY_ORDER_SORTED            # reorder= put the scene's own mode back
    s.set_query_order(rt.RT_QUERY_ORDER_CALLER)
    with pytest.raises(rt.RtError) as e:
        s.query(pixels=[(1, 2)] * n, reorder=True)
    assert e.value.code == rt.RT_ERR_NODEV and s._query_order == rt.RT_QUERY_ORDER_CALLER
    assert rt.lib().rt_query_last(s._h, None, None, None, 0) == rt.RT_ERR_STATE   # nothing was launched


# ---- the key -------------------------------------------------------------------------------------
BOX = np.float32([-4.0, -1.0, -2.5, 6.0, 3.0, 9.5])


def fields(host, keys):
    """(rejected, origin Morton code, direction code) of keys."""
    ob = np.uint64(3 * host.info["origin_bits"])
    rej = (keys >> np.uint64(63)) != 0
    return rej, (keys >> np.uint64(32)) & ((np.uint64(1) << ob) - np.uint64(1)), keys & np.uint64(0xffffffff)


def demorton3(code, bits):
    out = np.zeros((len(code), 3), np.int64)
    for j in range(bits):
        for a in range(3):
            out[:, a] |= ((code >> np.uint64(3 * j + a)) & np.uint64(1)).astype(np.int64) << j
    return out


def test_key_layout(host):
    B = host.info["origin_bits"]
    assert 1 <= B <= 10
    assert host.info["key_bits"] == 32 + 3 * B + 1
    assert host.info["rejected"] == (1 << 63) | (1 << (32 + 3 * B))


def test_rejected_rays_carry_bit_63_and_sort_last(host):
    rays = ql.as_traced(ql.REJECTED_RAYS[:, 0:3], ql.REJECTED_RAYS[:, 3:6])
    keys = host.keys(rays, BOX)
    assert (keys == np.uint64(host.info["rejected"])).all(), [hex(int(k)) for k in keys]
    o, d = ql.edge_rays(BOX)
    k_all = host.keys(ql.as_traced(o, d), BOX)
    rej = fields(host, k_all)[0]
    assert rej.sum() == len(ql.REJECTED_RAYS) and (~rej).sum() > 40
    assert k_all[~rej].max() < k_all[rej].min()
    # ... also under a sort that looks at the low key_bits bits alone
    low = k_all & ((np.uint64(1) << np.uint64(host.info["key_bits"])) - np.uint64(1))
    assert low[~rej].max() < low[rej].min()
    # a degenerate or non-finite box rejects nothing and breaks nothing: cell 0 on that axis
    for box in ([0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [-np.inf, 0, 0, np.inf, 1, 1], [np.nan] * 6):
        k = host.keys(ql.as_traced(o, d), np.float32(box))
        assert np.array_equal(fields(host, k)[0], rej), box


def test_origins_clamp_to_the_box_and_order_before_the_direction(host):
    B = host.info["origin_bits"]
    N = 1 << B
    mn, ext = BOX[0:3].astype(np.float64), (BOX[3:6] - BOX[0:3]).astype(np.float64)
    rng = np.random.default_rng(5)
    # outside: clamped to the edge cells
    d = np.float32([0.1, -0.7, 0.4])
    far = np.float32([[-1e6, 0, 0], [1e6, 0, 0], [0, -50, 0], [0, 1e30, 0], [0, 0, -3], [0, 0, 3e38], [-9, -9, -9], [99, 99, 99]])
    cells = demorton3(fields(host, host.keys(ql.as_traced(far, np.tile(d, (len(far), 1))), BOX))[1], B)
    inside = np.clip(np.floor((far.astype(np.float64) - mn) / ext * N), 0, N - 1).astype(np.int64)
    assert np.array_equal(cells, inside), (cells, inside)
    assert cells[0, 0] == 0 and cells[1, 0] == N - 1 and cells[3, 1] == N - 1 and cells[5, 2] == N - 1
    assert (cells[6] == 0).all() and (cells[7] == N - 1).all()
    # inside: the cell of the origin, away from cell borders
    frac = (rng.integers(0, N, size=(500, 3)) + rng.uniform(0.05, 0.95, size=(500, 3))) / N
    o = (mn + frac * ext).astype(np.float32)
    dirs = rng.normal(size=(500, 3)).astype(np.float32)
    keys = host.keys(ql.as_traced(o, dirs), BOX)
    rej, oc, dc = fields(host, keys)
    assert not rej.any()
    assert np.array_equal(demorton3(oc, B), np.floor(frac * N).astype(np.int64))
    # monotone in the origin cell before the direction: a larger cell code is a larger key whatever the directions
    order = np.argsort(keys, kind="stable")
    assert (np.diff(oc[order].astype(np.int64)) >= 0).all()
    a, b = rng.integers(0, 500, 2000), rng.integers(0, 500, 2000)
    m = oc[a] != oc[b]
    assert np.array_equal(keys[a][m] < keys[b][m], oc[a][m] < oc[b][m])
    # within one cell the direction decides
    same = np.tile(o[:1], (500, 1))
    k2 = host.keys(ql.as_traced(same, dirs), BOX)
    assert len(set(fields(host, k2)[1].tolist())) == 1
    assert np.array_equal(np.argsort(k2, kind="stable"), np.argsort(fields(host, k2)[2], kind="stable"))


def test_equal_rays_equal_keys_and_directions_are_distinct(host):
    o, d = ql.edge_rays(BOX)
    rays = ql.as_traced(o, d)
    assert np.array_equal(host.keys(rays, BOX), host.keys(rays.copy(), BOX))
    twice = np.concatenate([rays, rays])
    k = host.keys(twice, BOX)
    assert np.array_equal(k[:len(rays)], k[len(rays):])
    c = 0.5 * (BOX[0:3] + BOX[3:6])
    for dirs in (ql.OCTANTS, ql.AXES, np.concatenate([ql.OCTANTS, ql.AXES])):
        keys = host.keys(ql.as_traced(np.tile(c, (len(dirs), 1)), dirs), BOX)
        rej, oc, dc = fields(host, keys)
        assert not rej.any()
        assert len(set(dc.tolist())) == len(dirs), [hex(int(x)) for x in dc]
        assert len(set(oc.tolist())) == 1
    # the direction's length does not matter beyond the normalisation's rounding: the same 16-bit cells or their neighbours
    k1 = fields(host, host.keys(ql.as_traced(np.tile(c, (8, 1)), ql.OCTANTS), BOX))[2]
    k2 = fields(host, host.keys(ql.as_traced(np.tile(c, (8, 1)), 1000 * ql.OCTANTS), BOX))[2]
    assert np.array_equal(k1 >> np.uint64(8), k2 >> np.uint64(8))


# ---- the plan -------------------------------------------------------------------------------------
def test_order_plan(host):
    none = dict(sort=0, key_bits=0, keys_bytes=0, idx_bytes=0, scratch_bytes=0)
    for n in (1, 63, 64):
        assert host.plan(n, 1, 0) == none, n                        # one wave anyway
    for n in (65, 6144, 1920 * 1080, (1 << 31) - 1):
        assert host.plan(n, 0, 0) == none                           # caller order
        assert host.plan(n, 1, 1) == none                           # a counted query is not sorted
        p = host.plan(n, 1, 0)
        a256 = lambda b: (b + 255) // 256 * 256                      # noqa: E731
        assert p == dict(sort=1, key_bits=host.info["key_bits"], keys_bytes=a256(8 * n), idx_bytes=a256(4 * n),
                         scratch_bytes=2 * a256(8 * n) + 2 * a256(4 * n)), n


# ---- coherence --------------------------------------------------------------------------------------
def chunk_metric(inst):
    """m: the mean number of distinct hit instances per 64-ray chunk over the hit rays -- the rays of a
    sequence that hit, in the sequence's order, cut into chunks of 64 (the last one may be short)."""
    seq = inst[inst >= 0]
    return float(np.mean([len(np.unique(seq[i:i + 64])) for i in range(0, len(seq), 64)]))


def test_sorted_order_is_nearer_to_the_frames_than_to_the_shuffled(rt, oracle, host):
    """world8_stress at 96 x 64 from the value check's camera; the hit instance of every pixel is the
    oracle's.  Pixel order, the PERM_SEED permutation, and the permuted rays in the stable order of
    their host keys: m_sorted^2 <= m_pixel m_permuted.
    Measured: 4.09 against 7.18 and 31.93."""
    W, H = qc.VALUES_SIZE
    s = rt.Scene.load_json(scene_path(qc.VALUES_SCENE), W, H)
    o = oracle.load(scene_path(qc.VALUES_SCENE), W, H)
    s.set_camera(*qc.VALUES_CAMERA)
    o.set_camera(*s.camera())
    inst = oracle.render(o, spp=1, want=("hit_inst", "hit_tri"))["hit_inst"].ravel()
    rays = qc.camera_rays(s.export("camera"), qc.all_pixels(W, H))
    perm = np.random.default_rng(qc.PERM_SEED).permutation(W * H)
    keys = host.keys(rays[perm], ql.scene_box(s.arrays()))
    assert not fields(host, keys)[0].any()
    order = perm[np.argsort(keys, kind="stable")]
    assert np.array_equal(np.sort(order), np.arange(W * H))
    m_pixel, m_perm, m_sorted = chunk_metric(inst), chunk_metric(inst[perm]), chunk_metric(inst[order])
    print("distinct hit instances per 64-ray chunk: pixel order %.3f, permuted %.3f, sorted by key %.3f" % (m_pixel, m_perm, m_sorted))
    assert m_pixel < m_perm
    assert m_sorted ** 2 <= m_pixel * m_perm, (m_sorted, m_pixel, m_perm)
