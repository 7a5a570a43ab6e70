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
Then the interleaved pattern and the filtered resolve (section "filter"), same protocol:
  - the shared pattern, and the interleaved pattern under both of its lane mappings (RT_OCCL_MAP =
    tile / class): `class` counts as faster only when its median is below `tile`'s by more than the
    larger of the two spreads, at both radii;
  - a call with the filter on against the same call with it off (visibility and rgba written), and
    occl_filter_kernel's own time by start/stop events on its dispatch (rt_occlusion_filter_timing);
  - a quality table: the mean absolute difference of `visibility`, over the pixels with a primary
    hit, from the shared pattern's 1024-sample frame at the same radius, for shared n = 4, 16, 64,
    interleaved n = 4, interleaved n = 4 + filter, shared n = 4 + filter (a record, no threshold).
Then, on request only (section "history", or --history anywhere on the line), the
interactive setting of 3.9 under a moving camera: 32 poses, each the last one translated by
(0.05, 0, 0) through rt_camera_translate, 4 interleaved samples a pose through the filter, radius
+inf, device outputs.  History off (a restart a pose: what a library before the history does, and
the only leg such a library runs) and on (every pose after the first a move):
  - per pose the call's time, the median over `calls` repetitions of the whole path, and the
    median of those over the moving poses 2 .. 32;
  - occl_reproject_kernel's and the resolving kernel's own times by events on their dispatches
    (rt_occlusion_history_timing), medians over the moving poses of further repetitions;
  - the mean |visibility - the shared pattern's unfiltered 1024-sample frame at that pose| over
    the pixels with a primary hit, at poses 1, 2, 4, 8, 16 and 32 (a record, no threshold).
Usage: python tools/occlusion_bench.py [scene] [W] [H] [calls] [samples] [all|base|filter|history] [--history]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-ray-tracer_amd"))
import rtamd  # noqa: E402

HISTORY_FLAG = "--history" in sys.argv
argv = [a for a in sys.argv if a != "--history"]
scene = argv[1] if len(argv) > 1 else "world8_stress"
W, H = (int(argv[2]), int(argv[3])) if len(argv) > 3 else (1920, 1080)
calls = int(argv[4]) if len(argv) > 4 else 30
K = int(argv[5]) if len(argv) > 5 else 16
SECTIONS = "history" if HISTORY_FLAG else argv[6] if len(argv) > 6 else "all"
assert SECTIONS in ("all", "base", "filter", "history"), SECTIONS
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

for radius in (float("inf"), 2.0) if SECTIONS in ("all", "base") else ():
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

# ---- the interleaved pattern and the filtered resolve ----
rgba = torch.empty((H, W), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
decision = []
for radius in (float("inf"), 2.0) if SECTIONS in ("all", "filter") else ():
    rname = "inf" if radius == float("inf") else radius

    def call(samples=K):
        return s.occlusion_device(samples=samples, radius=radius, restart=True, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr(),
                                  rgba_ptr=rgba.data_ptr())

    def frame(samples):
        call(samples)
        return vis.cpu().numpy().copy()

    s.set_occlusion_pattern("shared")
    s.set_occlusion_filter(False)
    shared = summary(medians(call))
    out(what="pattern", radius=rname, pattern="shared", filter=False, outputs="visibility, occluded, rgba", fused=shared)
    s.set_occlusion_pattern("interleaved")
    res, count = {}, None
    for m in ("tile", "class"):
        os.environ["RT_OCCL_MAP"] = m
        call()
        assert s.occlusion_config["map"] == m
        c = occ.cpu().numpy().copy()
        assert count is None or np.array_equal(c, count), m       # no result depends on the map
        count = c
        res[m] = summary(medians(call))
        out(what="pattern", radius=rname, pattern="interleaved", map=m, filter=False, fused=res[m],
            per_sample_over_shared=round(res[m]["median_ms"] / shared["median_ms"], 3))
    del os.environ["RT_OCCL_MAP"]
    margin = max(res["tile"]["spread_ms"], res["class"]["spread_ms"])
    decision.append(res["class"]["median_ms"] < res["tile"]["median_ms"] - margin)
    out(what="interleaved map", radius=rname, class_is_faster=bool(decision[-1]), margin_ms=margin)

    # the filter: the whole call on / off (the build's default map), and the kernel alone
    for pattern in ("shared", "interleaved"):
        s.set_occlusion_pattern(pattern)
        s.set_occlusion_filter(False)
        off = summary(medians(call))
        s.set_occlusion_filter(True)
        on = summary(medians(call))
        s.filter_timing(True)
        ks = []
        for _ in range(REPS):
            t = []
            for _ in range(calls):
                call()
                t.append(s.filter_timing(True))
            ks.append(sorted(t)[len(t) // 2])
        s.filter_timing(False)
        s.set_occlusion_filter(False)
        out(what="filter", radius=rname, pattern=pattern, map=s.occlusion_config["map"], call_filter_off=off, call_filter_on=on,
            occl_filter_kernel=summary(ks))

    # quality: mean |visibility - the shared pattern's 1024-sample frame| over the hit pixels
    s.set_occlusion_pattern("shared")
    ref = frame(1024)
    hit = s.query(pixels=np.stack(np.mgrid[0:H, 0:W][::-1], axis=-1).reshape(-1, 2).astype(np.int32), want=("hit",))["hit"].reshape(H, W) != 0
    table = {}
    for name, pattern, n, filt in (("shared n=4", "shared", 4, False), ("shared n=16", "shared", 16, False), ("shared n=64", "shared", 64, False),
                                   ("interleaved n=4", "interleaved", 4, False), ("interleaved n=4 + filter", "interleaved", 4, True),
                                   ("shared n=4 + filter", "shared", 4, True)):
        s.set_occlusion_pattern(pattern)
        s.set_occlusion_filter(filt)
        v = frame(n)
        table[name] = round(float(np.abs(v[hit] - ref[hit]).mean()), 5)
        levels = len(np.unique(v[hit]))
        table[name + " (grey levels)"] = levels
    s.set_occlusion_pattern("shared")
    s.set_occlusion_filter(False)
    out(what="quality: mean |visibility - shared n=1024| over hit pixels", radius=rname, hit_pixels=int(hit.sum()), table=table)
if decision:
    out(what="interleaved map decision", class_becomes_default=bool(all(decision)), per_radius=[bool(d) for d in decision])


# ---- history across camera moves ----
def history_leg():
    POSES, STEP, N, MARKS = 32, (0.05, 0.0, 0.0), 4, (1, 2, 4, 8, 16, 32)
    has = hasattr(rtamd.lib(), "rt_occlusion_set_history")
    p0, q0 = s.camera()
    pixels = np.stack(np.mgrid[0:H, 0:W][::-1], axis=-1).reshape(-1, 2).astype(np.int32)

    def path():
        """The poses in order, the camera set for each."""
        s.set_camera(p0, q0)
        for i in range(1, POSES + 1):
            if i > 1:
                s.translate_camera(STEP)
            yield i

    s.set_occlusion_pattern("shared")
    s.set_occlusion_filter(False)
    refs, hits = {}, {}
    for i in path():
        if i in MARKS:
            s.occlusion_device(samples=1024, restart=True, visibility_ptr=vis.data_ptr())
            refs[i] = vis.cpu().numpy().copy()
            hits[i] = s.query(pixels=pixels, want=("hit",))["hit"].reshape(H, W) != 0
    s.set_occlusion_pattern("interleaved")
    s.set_occlusion_filter(True)
    for mode in ("off", "on") if has else ("off",):
        if has:
            s.set_occlusion_history(mode == "on")
        times = [[] for _ in range(POSES)]
        err = {}
        for r in range(WARM + calls):
            s.occlusion_reset()
            for i in path():
                t0 = time.perf_counter()
                s.occlusion_device(samples=N, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr(), rgba_ptr=rgba.data_ptr())
                dt = time.perf_counter() - t0
                if r >= WARM:
                    times[i - 1].append(dt * 1e3)
                if r == 0 and i in MARKS:
                    err[str(i)] = round(float(np.abs(vis.cpu().numpy()[hits[i]] - refs[i][hits[i]]).mean()), 5)
        per_pose = [round(sorted(t)[len(t) // 2], 4) for t in times]
        moving = sorted(per_pose[1:])
        kern = {}
        if mode == "on":
            rp, rs = [], []
            s.history_timing(True)
            for r in range(REPS):
                s.occlusion_reset()
                for i in path():
                    s.occlusion_device(samples=N, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr(), rgba_ptr=rgba.data_ptr())
                    if i > 1:
                        a, b = s.history_timing(True)
                        rp.append(a)
                        rs.append(b)
            s.history_timing(False)
            kern = dict(occl_reproject_kernel_ms=round(sorted(rp)[len(rp) // 2], 4), resolving_filter_kernel_ms=round(sorted(rs)[len(rs) // 2], 4),
                        moves=s.occlusion_history["moves"])
        else:
            s.filter_timing(True)
            fs = []
            for r in range(REPS):
                for i in path():
                    s.occlusion_device(samples=N, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr(), rgba_ptr=rgba.data_ptr())
                    fs.append(s.filter_timing(True))
            s.filter_timing(False)
            kern = dict(occl_filter_kernel_ms=round(sorted(fs)[len(fs) // 2], 4))
        print(json.dumps(dict(scene=scene, W=W, H=H, what="history", history=mode, poses=POSES, step=STEP, samples_per_pose=N,
                              pattern="interleaved", filter=True, radius="inf", repetitions=calls, call_ms_per_pose=per_pose,
                              call_ms_pose_1=per_pose[0], call_ms_moving_median=moving[len(moving) // 2],
                              call_ms_moving_min=moving[0], call_ms_moving_max=moving[-1],
                              mean_abs_error_vs_1024=err, **kern)), flush=True)
    if has:
        s.set_occlusion_history(False)
    s.set_occlusion_filter(False)
    s.set_occlusion_pattern("shared")
    s.set_camera(p0, q0)


if SECTIONS == "history":
    history_leg()
