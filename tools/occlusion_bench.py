"""The ambient-occlusion pass (rt_occlusion) against the unfused route on the same rays,
world8_stress at 1920x1080 by default, 16 samples, radius +inf and 2, device outputs, one JSON line
per result:
  - fused: one rt_occlusion call of 16 samples from a restart (the surface record, then the
    samples; the BVH built once);
  - unfused: per sample one rt_query(any_hit, tmax = radius) on that sample's exported rays
    (rt_occlusion_rays) held in device buffers, the BVH built by the first query only; the flags are
    not reduced (the caller's own reduction would come on top);
  - each the median of `calls` calls after warm-up, repeated five times: the medians, and the
    run-to-run spread (largest minus smallest of the five); the fused pass counts as faster when its
    median of medians is below the unfused route's by more than the unfused route's spread;
  - occlusion rays per second of both (rays = samples x pixels with a primary hit);
  - the fused pass under both lane mappings (RT_OCCL_MAP = row / tile);
  - the fused pass continuing an accumulation (16 more samples, no surface record).
Usage: python tools/occlusion_bench.py [scene] [W] [H] [calls] [samples]"""
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
calls = int(sys.argv[4]) if len(sys.argv) > 4 else 30
K = int(sys.argv[5]) if len(sys.argv) > 5 else 16
REPS, WARM = 5, 3
rtamd.set_device(0)
s = rtamd.Scene.load_json(os.path.join(ROOT, "scenes", scene + ".json"), W, H)
n_px = W * H


def out(**kw):
    print(json.dumps(dict(scene=scene, W=W, H=H, samples=K, **kw)), flush=True)


def medians(fn, reps=REPS):
    """`reps` medians (ms) of `calls` timed calls each, after WARM untimed ones."""
    for _ in range(WARM):
        fn()
    meds = []
    for _ in range(reps):
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        meds.append(sorted(ts)[len(ts) // 2] * 1e3)
    return meds


def summary(meds):
    return dict(medians_ms=[round(m, 4) for m in meds], median_ms=round(sorted(meds)[len(meds) // 2], 4),
                spread_ms=round(max(meds) - min(meds), 4))


vis = torch.empty((H, W), dtype=torch.float32, device="cuda")
occ = torch.empty((H, W), dtype=torch.int32, device="cuda")
flags = torch.empty(n_px, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()

for radius in (float("inf"), 2.0):
    rname = "inf" if radius == float("inf") else radius
    tmax = torch.full((n_px,), radius, dtype=torch.float32, device="cuda")

    def fused():
        return s.occlusion_device(samples=K, radius=radius, restart=True, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr())

    fused()
    count = occ.cpu().numpy().copy()
    # the exported rays of samples 0 .. K - 1, in device buffers
    origins, dirs = [], []
    for k in range(K):
        r = s._occlusion_rays(k).reshape(n_px, 6)
        if k == 0:
            n_hit = int((r[:, 3:6] != 0).any(axis=1).sum())
        origins.append(torch.from_numpy(np.ascontiguousarray(r[:, 0:3])).cuda())
        dirs.append(torch.from_numpy(np.ascontiguousarray(r[:, 3:6])).cuda())
    torch.cuda.synchronize()
    rays = K * n_hit

    def unfused():
        for k in range(K):
            s.query_device(n_px, origin_ptr=origins[k].data_ptr(), dir_ptr=dirs[k].data_ptr(), tmax_ptr=tmax.data_ptr(),
                           any_hit=True, rebuild_bvh=(k == 0), hit_ptr=flags.data_ptr())

    # the two routes answer the same question: the flags' sum over the samples is the count
    total = np.zeros(n_px, np.int32)
    for k in range(K):
        s.query_device(n_px, origin_ptr=origins[k].data_ptr(), dir_ptr=dirs[k].data_ptr(), tmax_ptr=tmax.data_ptr(),
                       any_hit=True, hit_ptr=flags.data_ptr())
        total += flags.cpu().numpy().astype(np.int32)
    assert np.array_equal(total, count.ravel()), int((total != count.ravel()).sum())

    f, u = summary(medians(fused)), summary(medians(unfused))
    faster = f["median_ms"] < u["median_ms"] - u["spread_ms"]
    out(what="fused vs unfused", radius=rname, hit_pixels=n_hit, occlusion_rays=rays, fused=f, unfused=u,
        fused_grays_per_s=round(rays / f["median_ms"] * 1e-6, 3), unfused_grays_per_s=round(rays / u["median_ms"] * 1e-6, 3),
        fused_is_faster=bool(faster), occluded_samples=int(count.sum()))

    for m in ("row", "tile"):
        os.environ["RT_OCCL_MAP"] = m
        fused()
        assert np.array_equal(occ.cpu().numpy(), count), m
        out(what="lane mapping", radius=rname, map=m, fused=summary(medians(fused)))
    del os.environ["RT_OCCL_MAP"]

    def more():
        if s.occlusion_info[0] + K > rtamd.RT_AO_MAX_SAMPLES:
            s.occlusion_reset()
            fused()
        return s.occlusion_device(samples=K, radius=radius, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr())

    fused()                                                        # 16 held; one block of calls stays under the limit
    out(what="continuing (no surface record)", radius=rname, fused=summary(medians(more, reps=1)))
    del origins, dirs
