"""Per-sample cost of progressive refinement (rt_accumulate), world8_stress at 1920x1080 by default,
device outputs, one JSON line per result:
  - one rt_accumulate sample (a 1-spp trace into the pass buffer, the fold and its resolve, BVH
    rebuilt per call as rt_render does) against one synchronous rt_render(spp = 1) into the same
    RGBA8 buffer, the two alternated call by call in one run: medians and the difference;
  - the same with both outputs (RGBA8 and radiance) requested from both;
  - the fold kernel alone (accum_fold_kernel over buffers of the canvas size, timed by the
    dispatches' own events), folding only and folding with the resolve, its bytes per pixel and
    the bandwidth that makes, as a fraction of the achievable HBM rate given on the command line
    (default 6.3 TB/s, MI355X);
  - adaptive mode: one uniform sample against one adaptive refinement sample (mask built), two
    blocks of alternated calls, the needed and traced tile counts, and the one-off edge and list
    kernels and the tiles fold alone.
Usage: python tools/accum_bench.py [scene] [W] [H] [calls] [hbm_TBps]"""
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-ray-tracer_amd"))
import rtamd  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "world8_stress"
W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080)
calls = max(20, int(sys.argv[4])) if len(sys.argv) > 4 else 40
hbm = float(sys.argv[5]) if len(sys.argv) > 5 else 6.3
rtamd.set_device(0)
s = rtamd.Scene.load_json(os.path.join(ROOT, "scenes", scene + ".json"), W, H)
n_px = W * H


def out(**kw):
    print(json.dumps(dict(scene=scene, W=W, H=H, **kw)), flush=True)


def med(ts):
    return sorted(ts)[len(ts) // 2] * 1e3


rgba = torch.empty((H, W), dtype=torch.int32, device="cuda")
rad = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()

for both in (False, True):
    rp = rad.data_ptr() if both else None
    acc = lambda: s.accumulate_device(rgba_ptr=rgba.data_ptr(), radiance_ptr=rp)          # noqa: E731
    ren = lambda: s.render_device(spp=1, rgba_ptr=rgba.data_ptr(), radiance_ptr=rp, sync=True)   # noqa: E731
    s.accumulate_reset()
    for _ in range(3):
        acc()
        ren()
    ta, tr = [], []
    for _ in range(calls):                                     # alternated: drift hits both alike
        t = time.perf_counter(); acc(); ta.append(time.perf_counter() - t)
        t = time.perf_counter(); ren(); tr.append(time.perf_counter() - t)
    out(what="sample", outputs="rgba+radiance" if both else "rgba", calls=calls, accumulate_ms=round(med(ta), 4),
        render_spp1_ms=round(med(tr), 4), extra_ms=round(med(ta) - med(tr), 4), samples_held=s.accumulated[0])

# the fold kernel alone
L = rtamd.lib()
L.rt_accum_fold_time.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
for resolve, nbytes in ((0, 16 + 32 + 32), (1, 16 + 32 + 32 + 4 + 16)):
    ms = ctypes.c_double()
    r = L.rt_accum_fold_time(s._h, 50, resolve, ctypes.byref(ms))
    assert r == 0, L.rt_last_error()
    tbps = n_px * nbytes / (ms.value * 1e-3) / 1e12
    out(what="fold_kernel", resolve=bool(resolve), kernel_ms=round(ms.value, 5), bytes_per_pixel=nbytes,
        TB_per_s=round(tbps, 3), hbm_achievable_TB_per_s=hbm, fraction=round(tbps / hbm, 3))

# adaptive mode (rt_accumulate_set_adaptive): one uniform sample against one adaptive refinement
# sample (default threshold, the mask already built), alternated call by call on two scenes of the
# same canvas, in two blocks: the spread between the blocks' uniform medians is the run's noise,
# and the adaptive sample has to beat the uniform one by more than that.
if hasattr(L, "rt_accumulate_set_adaptive"):
    u = s
    a = rtamd.Scene.load_json(os.path.join(ROOT, "scenes", scene + ".json"), W, H)
    a.set_accumulate_adaptive(True)
    rgba2 = torch.empty((H, W), dtype=torch.int32, device="cuda")
    uni = lambda: u.accumulate_device(rgba_ptr=rgba.data_ptr())      # noqa: E731
    ada = lambda: a.accumulate_device(rgba_ptr=rgba2.data_ptr())     # noqa: E731
    u.accumulate_reset()
    for _ in range(3):
        uni()
        ada()                                                  # sample 0 and the mask, then refinement samples
    tiles = a.accumulate_tiles()
    n_tiles = tiles["need"].size
    blocks = []
    for _ in range(2):
        tu, tad = [], []
        for _ in range(calls):
            t = time.perf_counter(); uni(); tu.append(time.perf_counter() - t)
            t = time.perf_counter(); ada(); tad.append(time.perf_counter() - t)
        blocks.append((med(tu), med(tad)))
    spread = abs(blocks[0][0] - blocks[1][0])
    um, am = min(b[0] for b in blocks), max(b[1] for b in blocks)   # the comparison least kind to adaptive
    out(what="adaptive_sample", outputs="rgba", calls=calls, threshold=round(tiles["threshold"], 6), tiles=n_tiles,
        needed=tiles["needed"], traced=tiles["traced"], uniform_ms=[round(b[0], 4) for b in blocks],
        adaptive_ms=[round(b[1], 4) for b in blocks], uniform_spread_ms=round(spread, 4), saved_ms=round(um - am, 4),
        faster_by_more_than_spread=bool(um - am > spread), samples_held=a.accumulated[0])
    L.rt_accum_adaptive_time.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    ms4 = (ctypes.c_double * 4)()
    r = L.rt_accum_adaptive_time(a._h, 50, ms4)
    assert r == 0, L.rt_last_error()
    out(what="adaptive_kernels", tiles=n_tiles, needed=tiles["needed"], edge_kernel_ms=round(ms4[0], 5),
        lists_kernel_ms=round(ms4[1], 5), fold_tiles_ms=round(ms4[2], 5), fold_tiles_resolve_ms=round(ms4[3], 5))
    # where a pass's time goes: events on the scene's stream around one refinement pass and one uniform pass
    L.rt_accum_pass_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    ms8 = (ctypes.c_double * 8)()
    r = L.rt_accum_pass_timeline(a._h, 30, ms8)
    assert r == 0, L.rt_last_error()
    for k, what in ((0, "pass_timeline_adaptive"), (4, "pass_timeline_uniform")):
        out(what=what, pre_trace_gap_ms=round(ms8[k], 5), trace_ms=round(ms8[k + 1], 5), fold_ms=round(ms8[k + 2], 5),
            marker_to_fold_end_ms=round(ms8[k + 3], 5),
            note="gap: marker before launch_trace to the first dispatch's start (adaptive: the counter image's copy; uniform: the "
                 "memset); trace: adaptive the trace kernel over the tile lists, uniform the sky pre-pass and the trace kernel")
