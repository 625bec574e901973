"""What a batch of views buys: one ort_render_views_device call over V views against V back-to-back ort_render_image_device
calls, one GPU, same process, same work -- V copies of the scene's own camera, every view with the same seed, so that the
single-view call can do the identical work (and the frames are compared bit for bit before anything is timed).

Per scene and configuration V x (W x H), CHUNK policy, three legs:
  batch        one ort_render_views_device call (the VIEWS kernels: plain loop, four waves)
  seq_plain    V ort_render_image_device calls with ORT_EXCHANGE=0 ORT_WAVES5=0: the same kernel, launched V times
  seq_default  V ort_render_image_device calls with the launch policy left alone (ray exchange and five-waves unit allowed)
Each leg is timed end to end on the host, from before the first call to after one final device synchronisation; --warmup
rounds, then --reps timed rounds, the three legs alternating within a round so that clocks and cache state drift alike for all.
One JSON line per scene and configuration: the median ms of each leg, s = (max - min) / median of seq_plain's timings,
speedup = seq_plain / batch, ok = batch <= seq_plain * (1 + s), and vs_default = seq_default / batch.
usage: python3 tools/views_bench.py [--scenes c3_bunny_room,c2_analytic] [--configs 64x128,16x256,4x512] [--spp 64] [--chunk 16]
                                    [--warmup 2] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ORT_KNOBS_LIVE"] = "1"   # the legs differ in knobs: read them at every call

PLAIN = {"ORT_EXCHANGE": "0", "ORT_WAVES5": "0"}


def with_env(env, f):
    old = {k: os.environ.get(k) for k in PLAIN}
    for k in PLAIN:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return f()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3_bunny_room,c2_analytic")
    ap.add_argument("--configs", default="64x128,16x256,4x512", help="VxS: V views of S x S pixels")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()

    import torch
    from offline_raytracer_amd import api

    for name in a.scenes.split(","):
        scene = api.Scene.load_scn(os.path.join(ROOT, "data", name + ".scn")).commit().upload(0)
        for cfg in a.configs.split(","):
            V, S = (int(x) for x in cfg.split("x"))
            p = api.Scene.params(S, S, a.spp, a.seed, "chunk", chunk=a.chunk)
            cams = np.repeat(scene.camera(S, S)[None], V, axis=0)
            seeds = np.full(V, a.seed, "<u4")
            out_b = torch.zeros((V, S, S, 3), dtype=torch.float32, device="cuda")
            out_s = torch.zeros((V, S, S, 3), dtype=torch.float32, device="cuda")
            frame_bytes = S * S * 12

            def batch():
                scene.render_views_device(out_b.data_ptr(), p, cams, seeds)

            def sequence():
                for v in range(V):
                    scene.render_device(out_s.data_ptr() + v * frame_bytes, p)

            def timed(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            legs = [("batch", {}, batch), ("seq_plain", PLAIN, sequence), ("seq_default", {}, sequence)]
            ms = {k: [] for k, _, _ in legs}
            for r in range(a.warmup + a.reps):
                for k, env, f in legs:
                    t = with_env(env, lambda: timed(f))
                    if r >= a.warmup:
                        ms[k].append(t)
                if r == 0:   # the same work: every frame of the batch is the single view's frame
                    same = bool(torch.equal(out_b.view(torch.int32), out_s.view(torch.int32)))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            s = (max(ms["seq_plain"]) - min(ms["seq_plain"])) / med["seq_plain"]
            print(json.dumps({"scene": name, "views": V, "width": S, "height": S, "spp": a.spp, "chunk": a.chunk, "reps": a.reps,
                              "frames_identical": same,
                              "batch_ms": round(med["batch"], 3), "seq_plain_ms": round(med["seq_plain"], 3),
                              "seq_default_ms": round(med["seq_default"], 3), "s": round(s, 4),
                              "speedup": round(med["seq_plain"] / med["batch"], 4), "ok": med["batch"] <= med["seq_plain"] * (1 + s),
                              "vs_default": round(med["seq_default"] / med["batch"], 4),
                              "batch_all_ms": [round(x, 3) for x in ms["batch"]], "seq_plain_all_ms": [round(x, 3) for x in ms["seq_plain"]],
                              "seq_default_all_ms": [round(x, 3) for x in ms["seq_default"]]}), flush=True)
        scene.close()


if __name__ == "__main__":
    main()
