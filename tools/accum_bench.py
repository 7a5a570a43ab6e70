"""Per-sample cost of progressive refinement (rt_accumulate), world8_stress at 1920x1080 by default,
device outputs, one JSON line per result:
  - one rt_accumulate sample (a 1-spp trace into the pass buffer, the fold and its resolve, BVH
    rebuilt per call as rt_render does) against one synchronous rt_render(spp = 1) into the same
    RGBA8 buffer, the two alternated call by call in one run: medians and the difference;
  - the same with both outputs (RGBA8 and radiance) requested from both;
  - the fold kernel alone (accum_fold_kernel over buffers of the canvas size, timed by the
    dispatches' own events), folding only and folding with the resolve, its bytes per pixel and
    the bandwidth that makes, as a fraction of the achievable HBM rate given on the command line
    (default 6.3 TB/s, MI355X).
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
