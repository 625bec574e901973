"""SURVEY 8 row f4 on Linux: the reference's driver -- main()'s 1 024 tiles handed to a pool of worker threads through a work
queue (macos_main.mm:565-598, 602-662) -- as a developer tool, tools/host_sim: the kernel's own lane code (ort_lane.h) compiled
for the host, one simulated lane per thread, all workers on one job counter.  It is NOT a fallback of the product (the library
never loads or links it; the render call has no CPU path): here it is held against the pixels of the compiled reference
(golden fixtures) and against the oracle, bit for bit, single- and multi-threaded."""
import os
import subprocess

import numpy as np
import pytest

import host_sim_tool
from conftest import DATA, GOLDEN, assert_bits_equal


@pytest.fixture(scope="module")
def host_sim():
    return host_sim_tool.built("host_sim")


def _run(tool, scene, w, h, spp, seed, policy, chunk, out, threads, extra=None, base=None):
    """scene: the name of a scene under data/, or with base (its directory) the path of a .scn"""
    env = dict(os.environ, SIM_THREADS=str(threads))
    env.update(extra or {})
    scn, base = (scene, base) if base else (os.path.join(DATA, scene + ".scn"), DATA + "/")
    r = subprocess.run([tool, scn, base, str(w), str(h), str(spp), str(seed), policy, str(chunk), out],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    return np.fromfile(out, "<f4").reshape(h, w, 3)


def test_tile_queue_on_threads_reproduces_the_reference_schedule(host_sim, tmp_path):
    """main()'s own schedule (TILE32: 32x32 tiles, tile seeds drawn from the master series in row-major order) on 8 worker
    threads == on one == the compiled reference's pixels (tests/golden/renders_testscene.npz, made by oracle/_ref/ref_det)"""
    z = np.load(os.path.join(GOLDEN, "renders_testscene.npz"))
    want = z["tile32_64x64_2spp_c1_s12345"]
    one = _run(host_sim, "testscene", 64, 64, 2, 12345, "tile32", 0, str(tmp_path / "t1.f32"), 1)
    many = _run(host_sim, "testscene", 64, 64, 2, 12345, "tile32", 0, str(tmp_path / "t8.f32"), 8)
    assert_bits_equal(one, want, "one worker vs the reference")
    assert_bits_equal(many, want, "eight workers vs the reference")


@pytest.mark.parametrize("scene,w,h,spp,policy,chunk,extra", [
    ("c2_analytic", 93, 61, 6, "chunk", 2, {}),            # ragged edge blocks, all lobes
    ("c3_bunny_room", 96, 64, 4, "pixel", 0, {"SIM_DIFFUSE": "1"}),
    ("c3_bunny_room", 96, 64, 4, "chunk", 2, {"SIM_WIDE": "1"}),  # the 4-wide tree
])
def test_worker_pool_matches_the_oracle(host_sim, api, oracle, tmp_path, scene, w, h, spp, policy, chunk, extra):
    got = _run(host_sim, scene, w, h, spp, 77, policy, chunk, str(tmp_path / "o.f32"), 8, extra)
    sc = api.Scene.load_scn(os.path.join(DATA, scene + ".scn")).commit()
    ref, _ = oracle.OracleScene(sc.flatten(w, h)).render(w, h, spp, 77, policy, chunk=max(chunk, 1), threads=8)
    assert_bits_equal(got, ref, "%s %s on 8 workers vs the oracle" % (scene, policy))


@pytest.mark.parametrize("variant", ["mats_over", "lights_over", "ref_limits"])
def test_lane_code_reads_the_tables_from_their_arrays_past_the_caps(host_sim, api, oracle, manifest, tmp_path, variant):
    """host_sim runs the TABS = false lane code: materials through load_mat(sv.materials, m), light types through
    sv.light_is_sphere[li].  The scenes of tools/make_tablescene.py with 49 materials, 65 lights and 100 of each put most of
    what a path reads past index 48 / 64: the pixels are the compiled reference's (renders_tables_<variant>.npz) and, at a
    size with ragged 8x8 edge blocks, the oracle's.  (Shown to fail on a scratch copy of ort_lane.h: with the light lookup
    reading sv.light_is_sphere[li & 63] lights_over and ref_limits go red and every older test of this file and of
    test_host.py stays green; with load_mat reading material hit_mat & 47 all three variants go red.)"""
    import table_scenes
    scene, _, csg = table_scenes.build(api, variant, tmp_path)
    scn, base = str(tmp_path / (variant + ".scn")), str(tmp_path) + "/"
    z = np.load(os.path.join(GOLDEN, "renders_tables_%s.npz" % variant))
    for e in manifest["tablescenes"][variant]["renders"]:
        threads = 8 if e["policy"] in ("pixel", "chunk", "tile32") else 1
        got = _run(host_sim, scn, e["width"], e["height"], e["spp"], e["seed"], e["policy"], e["chunk"] if e["policy"] == "chunk" else 0,
                   str(tmp_path / "g.f32"), threads, base=base)
        assert_bits_equal(got, z[e["key"]], "%s %s vs the reference" % (variant, e["key"]))
    scene.commit()
    for w, h, spp, policy, chunk, extra in ((93, 61, 6, "chunk", 2, {}), (45, 35, 5, "pixel", 0, {"SIM_FORCE_FALLBACK": "0xf"})):
        got = _run(host_sim, scn, w, h, spp, 77, policy, chunk, str(tmp_path / "o.f32"), 8, extra, base=base)
        ref, _ = oracle.OracleScene(scene.flatten(w, h), with_reference_csg=csg).render(w, h, spp, 77, policy, chunk=max(chunk, 1), threads=8)
        assert_bits_equal(got, ref, "%s %s on 8 workers vs the oracle" % (variant, policy))
