"""Host time per camera render call: what device_render's plumbing costs where the kernel is next to nothing.  A 64 x 64, 1 spp
PIXEL render in the device form without stats (ort_render_image_device: the call enqueues and returns; the next call on the scene
waits for it), the same frame as an adaptive call that never checks (ort_render_adaptive_device, min_spp = max_spp = 8, four
planes), and a closest-hit query over 4096 rays in the same form (ort_raycast_device: the ray queries go through the same steps
around their launch).  Per leg: --warmup calls, then --reps windows of --calls calls each ending in one device synchronise, timed on the host
clock around the window (a call settles the one before it, so the figure holds that call's kernel too); then --calls calls each
followed by a synchronise, the clock around the call alone ("idle_us": what the host spends in a call that has nothing to wait
for).  One JSON line: per leg the microseconds per call of every window, their median, s = (max - min) / median, and the
quartiles of idle_us.  ORT_LIB=path/to/libort.so measures another build of the library with the same script (the binding is the
same): compare two builds by running them alternately, several times each, and hold the change's median against the spread of
the parent's own medians.
usage: python3 tools/render_call_bench.py [--scene c3_bunny_room] [--size 64] [--calls 300] [--reps 7] [--warmup 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXED = (8, 8, 0.3, 0.05, 3)   # min_spp, max_spp, tolerance, floor, check_every: no check ever fires


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3_bunny_room")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    import torch
    from offline_raytracer_amd import api
    if api.device_count() < 1:
        raise SystemExit("render_call_bench: no HIP device (a host time per call is measured against a real queue)")
    scene = api.Scene.load_scn(os.path.join(ROOT, "data", a.scene + ".scn")).commit().upload(0)
    dev = torch.device("cuda", 0)
    n = a.size * a.size
    rgb = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    spp, m2, fin = (torch.zeros(n, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.int32))
    rng = np.random.default_rng(2024)   # rays from the camera's place in all directions
    d = rng.normal(size=(4096, 3))
    rays = torch.from_numpy(np.concatenate([np.tile(scene.camera(a.size, a.size)[0], (4096, 1)), d / np.linalg.norm(d, axis=1, keepdims=True)],
                                           axis=1).astype("<f4")).to(dev)
    hits = torch.zeros(4096 * 24, dtype=torch.uint8, device=dev)
    plain = scene.params(a.size, a.size, 1, 2024, "pixel")
    adaptive = scene.params(a.size, a.size, 0, 2024, "pixel")
    legs = {
        "plain": lambda: scene.render_device(rgb.data_ptr(), plain),
        "adaptive": lambda: scene.render_adaptive_device(adaptive, *FIXED, rgb.data_ptr(), spp.data_ptr(), m2.data_ptr(), fin.data_ptr()),
        "raycast": lambda: scene.raycast_device(rays.data_ptr(), 4096, hits.data_ptr()),
    }
    out = {"lib": api.LIB_PATH, "scene": a.scene, "size": a.size, "calls": a.calls}
    for name, call in legs.items():
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6 / a.calls)
        med = sorted(us)[len(us) // 2]
        idle = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            idle.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
        idle.sort()
        out[name] = {"us_per_call": [round(x, 2) for x in us], "median": round(med, 2), "s": round((max(us) - min(us)) / med, 4),
                     "idle_us": [round(idle[len(idle) * q // 4], 2) for q in (1, 2, 3)]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
