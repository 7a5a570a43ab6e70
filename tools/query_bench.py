"""Ray-query throughput (rt_query): rays/s for the primary rays of a frame, world8_stress at 1920x1080
by default, with device buffers, median of `calls` synchronous calls after warm-up:
  a  the frame's rays in pixel order (origin / dir mode; also the pixel mode itself)
  b  the same rays under a fixed permutation (incoherent packets)
  c  occlusion (any_hit): from every primary hit point towards the point light, tmax = its distance
  d  ambient-occlusion fans (any_hit): 4 seeded directions in the normal's hemisphere per hit point, tmax = 2
each with the BVH kept (rebuild_bvh = 0: the query alone) and rebuilt per call (the default), and each
in caller order and sorted (RT_QUERY_ORDER_SORTED, reorder=True), the two modes alternated call by call
in one run, plus the sorted call stopped after its sort (key kernel + radix sort alone).  Then
the latency of Scene.pick, the small / persistent crossover (both forms forced through
RT_QUERY_FORM over a ladder of batch sizes: the frame's last m rays in pixel order, then m
permuted rays; BVH kept) and, as context, the trace
stage's own primary-query rate: rt_frame_work's lanes_primary over the lone trace kernel time at 1 spp
(that kernel also shades).  One JSON line per result.
Usage: python tools/query_bench.py [scene] [W] [H] [calls]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-ray-tracer_amd"))
import rtamd  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "world8_stress"
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080)
calls = max(20, int(sys.argv[4])) if len(sys.argv) > 4 else 30
rtamd.set_device(0)
s = rtamd.Scene.load_json(os.path.join(ROOT, "scenes", scene + ".json"), W, H)
n = W * H


def out(**kw):
    print(json.dumps(dict(scene=scene, W=W, H=H, **kw)), flush=True)


def median_ms(fn, reps=calls, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()                                                   # rt_query returns when the results are complete
        ts.append(time.perf_counter() - t)
    return sorted(ts)[len(ts) // 2] * 1e3


dev = "cuda"
y, x = np.mgrid[0:H, 0:W]
pix = torch.from_numpy(np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)).to(dev)
t_d = torch.empty(n, dtype=torch.float32, device=dev)
inst_d = torch.empty(n, dtype=torch.int32, device=dev)
tri_d = torch.empty(n, dtype=torch.int32, device=dev)
hit_d = torch.empty(n, dtype=torch.uint8, device=dev)
rays_d = torch.empty((n, 6), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
s.query_device(n, pixel_ptr=pix.data_ptr(), t_ptr=t_d.data_ptr(), inst_ptr=inst_d.data_ptr(), rays_out_ptr=rays_d.data_ptr())
o_a, d_a = rays_d[:, 0:3].contiguous(), rays_d[:, 3:6].contiguous()
perm = torch.from_numpy(np.random.default_rng(20240607).permutation(n)).to(dev)
o_b, d_b = o_a[perm].contiguous(), d_a[perm].contiguous()
# c: shadow-like segments from the primary hit points to the first point light
lights = s.export("lights")
point = lights[lights[:, 3] == 0]
hitm = inst_d >= 0
n_c = int(hitm.sum())
if len(point) and n_c:
    L = torch.from_numpy(point[0, 0:3].copy()).to(dev)
    p = (o_a + t_d[:, None] * d_a)[hitm].contiguous()
    d_c = (L[None, :] - p).contiguous()
    tmax_c = torch.linalg.norm(d_c, dim=1).contiguous()
torch.cuda.synchronize()


def closest(o_t, d_t, m, rebuild):
    return lambda **kw: s.query_device(m, origin_ptr=o_t.data_ptr(), dir_ptr=d_t.data_ptr(), t_ptr=t_d.data_ptr(),
                                       inst_ptr=inst_d.data_ptr(), tri_ptr=tri_d.data_ptr(), rebuild_bvh=rebuild, **kw)


# d: ambient-occlusion fans -- from every primary hit point (lifted 1e-3 along the hit normal, off
# its own triangle) FAN directions in the hemisphere of the normal, from a seeded generator;
# any_hit with tmax = 2 units; a hit point's FAN rays are consecutive, as a caller generates them
FAN, FAN_SEED, FAN_TMAX = 4, 20240608, 2.0
n_d = 0
if n_c:
    nrm_d = torch.empty((n, 3), dtype=torch.float32, device=dev)
    s.query_device(n, origin_ptr=o_a.data_ptr(), dir_ptr=d_a.data_ptr(), t_ptr=t_d.data_ptr(), inst_ptr=inst_d.data_ptr(),
                   normal_ptr=nrm_d.data_ptr())
    nh = nrm_d[hitm]
    ph = ((o_a + t_d[:, None] * d_a)[hitm] + 1e-3 * nh)
    g = torch.Generator(device="cpu")
    g.manual_seed(FAN_SEED)
    v = torch.randn((n_c, FAN, 3), generator=g, dtype=torch.float32).to(dev)
    v = v / torch.linalg.norm(v, dim=2, keepdim=True)
    v = torch.where(((v * nh[:, None, :]).sum(dim=2, keepdim=True) < 0), -v, v)
    o_d = ph[:, None, :].expand(n_c, FAN, 3).reshape(-1, 3).contiguous()
    d_d = v.reshape(-1, 3).contiguous()
    n_d = n_c * FAN
    tmax_d = torch.full((n_d,), FAN_TMAX, dtype=torch.float32, device=dev)
    hit_dd = torch.empty(n_d, dtype=torch.uint8, device=dev)
    del v, nh, ph, nrm_d
torch.cuda.synchronize()

caller_only = bool(os.environ.get("QUERY_BENCH_CALLER_ONLY"))        # (a library without rt_query_set_order: A/B runs)


def paired_ms(fn, reps=calls, warm=3):
    """Median ms of fn() in caller order and of fn(reorder=True), the two alternated call by call in
    one run; then of the sorted call stopped after its sort (RT_QUERY_SORT_ONLY: key kernel + radix
    sort + the call's host path, no trace)."""
    if caller_only:
        return median_ms(fn, reps, warm), None, None
    ts = {False: [], True: []}
    for k in range(warm + reps):
        for reorder in (False, True):
            t = time.perf_counter()
            fn(reorder=reorder)
            if k >= warm:
                ts[reorder].append(time.perf_counter() - t)
    med = {r: sorted(v)[len(v) // 2] * 1e3 for r, v in ts.items()}
    os.environ["RT_QUERY_SORT_ONLY"] = "1"
    try:
        sort_only = median_ms(lambda: fn(reorder=True), reps, warm)
    finally:
        del os.environ["RT_QUERY_SORT_ONLY"]
    return med[False], med[True], sort_only


def report(case, rays, fn, rebuild, **extra):
    a, b, k = paired_ms(fn)
    row = dict(case=case, rays=rays, median_ms=round(a, 4), mrays_per_s=round(rays / a / 1e3, 1))
    if b is not None:
        row.update(sorted_median_ms=round(b, 4), sorted_mrays_per_s=round(rays / b / 1e3, 1), key_sort_only_ms=round(k, 4),
                   sorted_over_caller=round(b / a, 3))
    out(**row, rebuild_bvh=int(rebuild), calls=calls, **extra)


for rebuild in (False, True):
    report("a_pixel_mode", n, lambda **kw: s.query_device(n, pixel_ptr=pix.data_ptr(), t_ptr=t_d.data_ptr(), inst_ptr=inst_d.data_ptr(),
                                                          tri_ptr=tri_d.data_ptr(), rebuild_bvh=rebuild, **kw), rebuild)
    report("a_pixel_order", n, closest(o_a, d_a, n, rebuild), rebuild)
    report("b_permuted", n, closest(o_b, d_b, n, rebuild), rebuild)
    if len(point) and n_c:
        report("c_any_hit_to_light", n_c,
               lambda **kw: s.query_device(n_c, origin_ptr=p.data_ptr(), dir_ptr=d_c.data_ptr(), tmax_ptr=tmax_c.data_ptr(),
                                           any_hit=True, hit_ptr=hit_d.data_ptr(), rebuild_bvh=rebuild, **kw), rebuild)
        torch.cuda.synchronize()
        out(case="c_occluded", occluded=round(float(hit_d[:n_c].float().mean()), 4))
    if n_d:
        report("d_ao_fans", n_d,
               lambda **kw: s.query_device(n_d, origin_ptr=o_d.data_ptr(), dir_ptr=d_d.data_ptr(), tmax_ptr=tmax_d.data_ptr(),
                                           any_hit=True, hit_ptr=hit_dd.data_ptr(), rebuild_bvh=rebuild, **kw), rebuild,
               fan=FAN, tmax=FAN_TMAX)
        torch.cuda.synchronize()
        out(case="d_occluded", occluded=round(float(hit_dd.float().mean()), 4))
if os.environ.get("QUERY_BENCH_CASES_ONLY"):                          # (the RAYKEY_ORIGIN_BITS ladder: cases a-d alone)
    sys.exit(0)

# pick: one ray through the host path (pinned staging, one copy each way)
for rebuild in (False, True):
    ms = median_ms(lambda: s.query(pixels=[(W // 2, H // 2)], rebuild_bvh=rebuild), reps=max(calls, 100), warm=5)
    out(case="pick", rebuild_bvh=int(rebuild), median_us=round(ms * 1e3, 1), calls=max(calls, 100))

# the small / persistent crossover: the last m rays of the frame in pixel order (its bottom rows,
# where the rays hit; the top rows are sky, which costs nothing to trace) and m rays of the
# permuted list, BVH kept
for kind, o_t, d_t in (("coherent", o_a, d_a), ("permuted", o_b, d_b)):
    cross = None
    for m in (64, 256, 1024, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1048576, n):
        if m > n:
            continue
        o_m, d_m = o_t[n - m:], d_t[n - m:]
        row = {}
        for form in ("small", "persistent"):
            os.environ["RT_QUERY_FORM"] = form
            row[form] = median_ms(closest(o_m, d_m, m, False))
        del os.environ["RT_QUERY_FORM"]
        if cross is None and row["persistent"] < row["small"]:
            cross = m
        elif row["persistent"] >= row["small"]:
            cross = None                                       # (the first batch from which persistent stays faster)
        out(case="crossover", rays_kind=kind, rays=m, small_us=round(row["small"] * 1e3, 1),
            persistent_us=round(row["persistent"] * 1e3, 1))
    out(case="crossover_found", rays_kind=kind, persistent_faster_from=cross)

# context: the trace stage's own primary queries at 1 spp
w = s.frame_work(spp=1)
rgba = torch.empty(n, dtype=torch.int32, device=dev)
for _ in range(3):
    s.render_device(spp=1, rgba_ptr=rgba.data_ptr(), sync=True)
s.timing_collect()
for _ in range(calls):
    s.render_device(spp=1, rgba_ptr=rgba.data_ptr(), sync=True, timing=True)
tc = s.timing_collect()
trace_ms = tc["trace_ms_total"] / max(tc["frames"], 1)
out(case="trace_stage_context", lanes_primary=w["lanes_primary"], queries=w["queries"], lone_trace_ms=round(trace_ms, 4),
    primary_mrays_per_s=round(w["lanes_primary"] / trace_ms / 1e3, 1))
