"""The scenes at and past the caps of the kernels' LDS tables (tools/make_tablescene.py), for the CPU and the GPU tests: the
variants with their counts taken from the caps that csrc/ort_plan.h states (through tools/launch_plan, the same numbers
tests/test_launch_plan.py pins), and the conditions that make a wrong table index visible, checked on the oracle's output."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_tablescene  # noqa: E402

TOOL = os.path.join(ROOT, "tools", "launch_plan")
GOLDEN_VARIANTS = ["at_caps", "mats_over", "lights_over", "ref_limits"]   # what the reference loads: tests/golden/*_tables_<variant>.npz
OVER_MATS = ["mats_over", "mats_over_diffuse", "ref_limits", "beyond_ref"]
OVER_LIGHTS = ["lights_over", "ref_limits", "beyond_ref"]
W, H = 64, 48


def launch_plan_tool():
    src = [os.path.join(ROOT, "tools", "launch_plan.cpp"), os.path.join(ROOT, "include", "ort.h")]
    src += [os.path.join(ROOT, "offline_raytracer_amd", "csrc", h) for h in ("ort_plan.h", "ort_setup.h", "ort_scene.h")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(s) > os.path.getmtime(TOOL) for s in src):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or hipcc
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan", "CXX=" + cxx])
    return TOOL


_caps = {}


def caps():
    """{"materials": 48, "lights": 64, "pro_slots": 40} as ort_plan.h has them"""
    if not _caps:
        env = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        out = subprocess.run([launch_plan_tool(), "width=8", "height=8", "spp=1"], env=env, capture_output=True, text=True, timeout=60, check=True)
        _caps.update(json.loads(out.stdout)["tab_caps"])
    return _caps


def variants():
    c = caps()
    return make_tablescene.variants(c["materials"], c["lights"])


def build(api, variant, directory):
    """-> (uncommitted product scene, counts, with_reference_csg of the oracle scene that matches it)"""
    kw = variants()[variant]
    if variant == "beyond_ref":
        args, counts = make_tablescene.arrays(**kw)
        return api.Scene.from_arrays(**args), counts, False
    scn, counts = make_tablescene.write_scene(str(directory), stem=variant, **kw)
    return api.Scene.load_scn(scn), counts, True


def primary_rays(flat, w=W, h=H):
    """the rays through the pixel centres of a w x h frame"""
    cam = np.asarray(flat.camera, "<f4")
    ys, xs = np.mgrid[0:h, 0:w]
    fx = ((xs + 0.5) / w * 2 - 1).astype("<f4")
    fy = ((ys + 0.5) / h * 2 - 1).astype("<f4")
    d = (fx[..., None] * cam[1] + fy[..., None] * cam[2] - cam[3]).astype("<f4").reshape(-1, 3)
    return np.broadcast_to(cam[0], d.shape).copy(), d


def assert_conditions(variant, scene, osc, flat):
    """What makes a table read at a wrong index change pixels, from the oracle's closest hits of the primary rays and from the
    light list: no primary miss; past the material cap a quarter of the primary hits on materials from the cap on, the
    last material among them; past the light cap (by more than one light) a quarter of the lights from the cap on; every
    light from the cap on of the other type than the light one cap below; no power-of-two period up to the cap."""
    c = caps()
    kw = variants()[variant]
    si = scene.info()
    assert (si.material_count, si.light_count) == (kw["materials"], kw["lights"])
    o, d = primary_rays(flat)
    _, _, mat = osc.raycast(o, d)
    assert (mat != 0).all(), "%s: the room is closed" % variant
    assert (mat == si.material_count - 1).any(), "%s: the last material is seen" % variant
    n_mat, cap = si.material_count, c["materials"]
    for m in range(len(make_tablescene.WALLS) + 1, n_mat):   # a material read at a shifted, flipped or wrapped index is another one
        for j in {m - 1, m ^ 1, m % cap, m & (cap - 1)} - {m}:
            assert j >= n_mat or flat.materials[m].tobytes() != flat.materials[j].tobytes(), (variant, m, j)
    if variant in OVER_MATS:
        assert si.material_count > c["materials"]
        assert (mat >= c["materials"]).mean() >= 0.25, "%s: %.3f of the primary hits past the material cap" % (variant, (mat >= c["materials"]).mean())
    types = flat.lights["type"]
    assert set(types.tolist()) == {1, 2}
    if variant in OVER_LIGHTS:
        assert len(types) > c["lights"]
        assert (types[c["lights"]:] != types[:len(types) - c["lights"]]).all()
        if len(types) > c["lights"] + 1:
            assert len(types) - c["lights"] >= len(types) / 4
    if len(types) >= c["lights"]:
        p = 1
        while p <= c["lights"] and p < len(types):
            assert (types[p:] != types[:-p]).any(), "%s: the light types have period %d" % (variant, p)
            p *= 2
