"""`python bench.py --gpus N` as ONE plain process (how the driver starts the 1-GPU line, and possibly the scaling
run): the parent starts N rank processes itself -- children, before anything touches a GPU -- relays rank 0's single
JSON line and fails if a rank fails.  Here on CPU with --rendezvous-only: the ranks meet over gloo and do not render
(the render path has no CPU fallback).  Reference counterpart: main() starting its own workers, macos_main.mm:565-598."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=180):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=timeout)


def test_plain_process_starts_its_own_ranks():
    r = _run(["--gpus", "2", "--rendezvous-only"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout  # ONE JSON line, whatever the ranks' libraries print
    js = json.loads(lines[0])
    assert js["rendezvous"] == "ok" and js["world"] == 2 and js["rank_sum"] == js["expected"] == 3.0


def test_three_ranks():
    r = _run(["--gpus", "3", "--rendezvous-only"])
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["world"] == 3 and js["rank_sum"] == 6.0


def test_a_dead_rank_fails_the_launch_promptly():
    t0 = time.time()
    r = _run(["--gpus", "2", "--rendezvous-only"], env={"ORT_BENCH_TEST_FAIL_RANK": "1"}, timeout=120)
    assert r.returncode != 0
    assert "rank 1 exited with code 3" in r.stderr
    assert time.time() - t0 < 60  # rank 0 is not left waiting in the rendezvous
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_torchrun_form_still_works():
    """the contract's N > 1 launch: python -m torch.distributed.run ... bench.py --gpus N"""
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    port = 29600 + os.getpid() % 300
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), BENCH, "--gpus", "2", "--rendezvous-only"], env=e, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    js = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1 and js[0]["world"] == 2


def test_steps_must_be_positive():
    r = _run(["--steps", "0"], timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_of_a_large_frame_is_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs above the size limit: the same seeded pixels every time, stored with their flat indices"""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 12 * 100)
    img = np.arange(30 * 20 * 3, dtype=np.float32).reshape(30, 20, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img)
    assert sorted(os.listdir(tmp_path / "a")) == ["image_sample.npy", "image_sample_pixel.npy"]
    sample = np.load(tmp_path / "a" / "image_sample.npy")
    pixel = np.load(tmp_path / "a" / "image_sample_pixel.npy")
    assert sample.dtype == np.float32 and pixel.dtype == np.float64 and len(sample) == len(pixel) == 50
    np.testing.assert_array_equal(sample, img.reshape(-1, 3)[pixel.astype(np.int64)])
    np.testing.assert_array_equal(pixel, np.load(tmp_path / "b" / "image_sample_pixel.npy"))
    bench.dump_outputs(str(tmp_path / "c"), img[:2])  # within the limit: the whole frame
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "image.npy"), img[:2])


@pytest.mark.gpu
def test_dump_outputs_is_the_rendered_frame(api, oracle, tmp_path):
    """a plain run times the steps and writes the last step's frame, which is the render call's image bit for bit; the
    roofline and the CPU baseline appear only with --full"""
    w, h, spp, seed = 64, 40, 8, 7
    size = ["--width", str(w), "--height", str(h), "--spp", str(spp), "--chunk", "4", "--seed", str(seed)]
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")] + size, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["steps"] == 2 and js["ms_per_step"] > 0 and js["metric"] == js["unit"] == "Mpaths/s"
    assert "roofline" not in js and "cpu_baseline" not in js
    got = np.load(tmp_path / "out" / "image.npy")
    assert got.dtype == np.float32 and got.shape == (h, w, 3)
    scene = api.Scene.load_scn(os.path.join(ROOT, "data", "c3_bunny_room.scn")).commit()
    ref, _ = oracle.OracleScene(scene.flatten(w, h)).render(w, h, spp, seed, "chunk", chunk=4, threads=8)
    assert_bits_equal(got, ref, "bench.py --dump-outputs vs the oracle")
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "1", "--full", "--cpu-sample-spp", "4"] + size, env={"ORT_CPU_BASELINE_CORES": "1"},
             timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["roofline"]["kernel_ms"] > 0 and js["cpu_baseline"]["value"] > 0
