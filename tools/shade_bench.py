"""rt_shade on a frame's worth of rays, world8_stress at 1920x1080 by default, device buffers, one
JSON line per result:
  - case 1: the frame's primary rays in pixel mode (sample 0);
  - case 2: the same rays as origin / dir (the rays_out of case 1);
  - case 3: the same rays under a fixed permutation, in caller order and with order = SORTED;
  - for context, the lone 1-spp rt_render of the same build (device outputs, radiance and rgba);
  - each the median of `calls` calls after warm-up, repeated five times: the medians, their median
    and the run-to-run spread (largest minus smallest of the five).
There is no earlier figure to hold these against and so no threshold: a record.
Usage: python tools/shade_bench.py [scene] [W] [H] [calls]"""
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
REPS, WARM, PERM_SEED = 5, 3, 20241021
rtamd.set_device(0)
s = rtamd.Scene.load_json(os.path.join(ROOT, "scenes", scene + ".json"), W, H)
n = W * H


def out(**kw):
    print(json.dumps(dict(scene=scene, W=W, H=H, rays=n, **kw)), flush=True)


def medians(fn):
    """REPS medians (ms) of `calls` timed calls each, after WARM untimed ones."""
    for _ in range(WARM):
        fn()
    meds = []
    for _ in range(REPS):
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        meds.append(sorted(ts)[len(ts) // 2] * 1e3)
    return meds


def summary(meds):
    m = sorted(meds)[len(meds) // 2]
    return dict(medians_ms=[round(x, 4) for x in meds], median_ms=round(m, 4), spread_ms=round(max(meds) - min(meds), 4),
                mrays_per_s=round(n / m * 1e-3, 1))


y, x = np.mgrid[0:H, 0:W]
pix = torch.from_numpy(np.stack([x.ravel(), y.ravel()], axis=1).astype(np.int32)).cuda()
rad = torch.empty((n, 4), dtype=torch.float32, device="cuda")
rgba = torch.empty(n, dtype=torch.int32, device="cuda")
rays = torch.empty((n, 6), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()

s.shade_device(n, pixel_ptr=pix.data_ptr(), radiance_ptr=rad.data_ptr(), rgba_ptr=rgba.data_ptr(), rays_out_ptr=rays.data_ptr())
frame = rgba.cpu().numpy().copy()
org, dirs = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous()
perm = torch.from_numpy(np.random.default_rng(PERM_SEED).permutation(n)).cuda()
org_p, dirs_p = org[perm].contiguous(), dirs[perm].contiguous()
torch.cuda.synchronize()


def pixels():
    s.shade_device(n, pixel_ptr=pix.data_ptr(), radiance_ptr=rad.data_ptr(), rgba_ptr=rgba.data_ptr())


def caller():
    s.shade_device(n, origin_ptr=org.data_ptr(), dir_ptr=dirs.data_ptr(), radiance_ptr=rad.data_ptr(), rgba_ptr=rgba.data_ptr())


def permuted(reorder):
    s.shade_device(n, origin_ptr=org_p.data_ptr(), dir_ptr=dirs_p.data_ptr(), reorder=reorder, radiance_ptr=rad.data_ptr(),
                   rgba_ptr=rgba.data_ptr())


def render():
    s.render_device(spp=1, compact=False, rgba_ptr=rgba.data_ptr(), radiance_ptr=rad.data_ptr(), sync=True)


render()
assert np.array_equal(rgba.cpu().numpy(), frame)                  # pixel mode is the frame
out(what="context: rt_render spp=1 alone", kernel=s.last_trace(), **summary(medians(render)))
out(what="case 1: pixel mode", **summary(medians(pixels)), kernel=s.shade_last())
out(what="case 2: origin / dir, pixel order", **summary(medians(caller)), kernel=s.shade_last())
out(what="case 3: permuted, caller order", **summary(medians(lambda: permuted(False))), kernel=s.shade_last())
keep = rgba.cpu().numpy().copy()
out(what="case 3: permuted, order = SORTED", **summary(medians(lambda: permuted(True))), kernel=s.shade_last())
assert np.array_equal(rgba.cpu().numpy(), keep)                   # the sorted batch is the caller-order batch
