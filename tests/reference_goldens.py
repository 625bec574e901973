"""The generated test scenes as the REFERENCE sees them (test infrastructure): the scene files behind the fixtures that
tests/golden/make_golden.py --only-generated writes (renders_deepscene.npz, raycast_deepscene.npz, renders_light_pick.npz,
renders_rooms.npz, chains_rooms.npz), their keys, and the oracle's planes to hold against them.  The generator, the CPU tests
(tests/test_oracle_golden.py) and the GPU tests (tests/test_gpu_reference_goldens.py) build the files from here, so all three
speak of the same bytes; manifest.json["generated"] holds each file's SHA-256.

The twins as FILES.  The tests of the light-group and feature renders patch a material array (light_groups_cases.dark_twin,
feature_cases.twin); the reference reads scene files.  A dark twin is the room's text with every `light` line but one reading
`light 0 0 0`: the loader gives emit all-zero bits there and keeps is_light.  The white twin is the room's text with every `brdf`
and `light` line reading `light 1 1 1`.  The `light` statement takes integers, so the albedo twin cannot be written."""
import hashlib
import os
import sys

import numpy as np

import deep_scenes
import light_groups_cases as lg
import render_adaptive_cases as rac
import test_gpu_light_pick as pick
from conftest import DATA, GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_deepscene  # noqa: E402

FILES = ("renders_deepscene.npz", "raycast_deepscene.npz", "renders_light_pick.npz", "renders_rooms.npz", "chains_rooms.npz")
CHAIN_SCENES = ("room_all_lobes", "glass_room")
CHAIN_SAMPLES = rac.MAX_SPP   # whole chains: 64 samples a pixel
# (policy, chunk) at deep_scenes.GPU_RENDER and at deep_scenes.RENDER, and of the grazing camera's scene at GPU_RENDER
DEEP_GPU = (("pixel", 0), ("chunk", 2))
DEEP_HOST = (("pixel", 0), ("chunk", 2), ("whole", 0), ("tile32", 0))
DEEP_GRAZE = (("pixel", 0),)


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def render_key(policy, w, h, spp, chunk, seed):
    return "%s_%dx%d_%dspp_c%d_s%d" % (policy, w, h, spp, max(chunk, 1), seed)


# ---- the deep scene ------------------------------------------------------------------------------------------------------------
def deep_files(directory):
    """writes deepscene.scn, its two PLY files and deepscene_graze.scn into directory -> (scn, graze_scn, layout)"""
    scn, layout = make_deepscene.write_scene(str(directory))
    return scn, deep_scenes.write_graze_scene(scn, layout, str(directory)), layout


def deep_renders():
    """[(which scene: "cone" or "graze", policy, w, h, spp, chunk, key)] of renders_deepscene.npz, seed deep_scenes.SEED"""
    out = []
    for cam, size, policies in (("cone", deep_scenes.GPU_RENDER, DEEP_GPU), ("cone", deep_scenes.RENDER, DEEP_HOST),
                                ("graze", deep_scenes.GPU_RENDER, DEEP_GRAZE)):
        w, h, spp, _ = size
        for policy, chunk in policies:
            out.append((cam, policy, w, h, spp, chunk, cam + "__" + render_key(policy, w, h, spp, chunk, deep_scenes.SEED)))
    return out


# ---- the light-pick rooms ------------------------------------------------------------------------------------------------------
def pick_rooms():
    """[(flavour, lights, key, the scene's text)] of tests/test_gpu_light_pick.py, as that module writes them"""
    return [(f, l, "%s_%s" % (f, l), pick.ROOM + pick.SPHERES[f] + pick.LIGHTS[l][0]) for f in pick.SPHERES for l in pick.LIGHTS]


# ---- the rooms of the light-group, feature, adaptive and sample-map renders -------------------------------------------------------
def room_text(name):
    assert name in lg.ROOMS
    return lg.ROOM + lg.SPHERES[name[len("room_"):]] + lg.THREE_LIGHTS


def dark_text(text, keep, lights=3):
    """a scene's text with every `light` line but the keep-th (in file order, which is the light materials' order) reading light 0 0 0"""
    out, k = [], 0
    for line in text.splitlines():
        if line.startswith("light "):
            if k != keep:
                line = "light 0 0 0"
            k += 1
        out.append(line)
    assert k == lights
    return "\n".join(out) + "\n"


def dark_twin_text(name, keep):
    """the room with every `light` line but the keep-th reading light 0 0 0"""
    return dark_text(room_text(name), keep)


def white_twin_text(name):
    """the room with every `brdf` and `light` line reading light 1 1 1: every material m >= 1 a light of emit (1, 1, 1)"""
    return "\n".join("light 1 1 1" if line.startswith(("brdf ", "light ")) else line for line in room_text(name).splitlines()) + "\n"


def room_variants(name):
    """[(variant, text)]: own, dark0..dark2, white"""
    return [("own", room_text(name))] + [("dark%d" % g, dark_twin_text(name, g)) for g in range(3)] + [("white", white_twin_text(name))]


def write_text(directory, stem, text):
    path = os.path.join(str(directory), stem + ".scn")
    with open(path, "w") as f:
        f.write(text)
    return path


def chain_scene(directory, name):
    """-> (scn, base_dir) of a scene of CHAIN_SCENES"""
    if name in lg.ROOMS:
        return write_text(directory, name, room_text(name)), str(directory) + "/"
    return os.path.join(DATA, name + ".scn"), DATA + "/"


def chains_from(z, name):
    """chains_rooms.npz -> {(x, y): (colours (CHAIN_SAMPLES, 3), states)} as render_adaptive_cases.chains gives them"""
    cols, states = z[name + "__colours"], z[name + "__states"]
    assert cols.shape == (rac.H, rac.W, CHAIN_SAMPLES, 3) and states.shape == (rac.H, rac.W, CHAIN_SAMPLES)
    return {(x, y): (cols[y, x], states[y, x]) for y in range(rac.H) for x in range(rac.W)}


# ---- the oracle's side ---------------------------------------------------------------------------------------------------------
def oracle_pixel_planes(oracle, osc, w, h, spp, seed, rr=0.8):
    """-> (the oracle's PIXEL render, its stats, the per-pixel final states of the one-pixel jobs that the render is)"""
    img, st = osc.render(w, h, spp, seed, "pixel", rr=rr, threads=1)
    states = np.zeros((h, w), "<u4")
    one = np.zeros((h, w, 3), "<f4")
    for y in range(h):
        for x in range(w):
            _, states[y, x] = osc.tiled_raytrace(one, x, y, x + 1, y + 1, oracle.job_seed(seed, y * w + x), spp, rr)
    assert (one.view("<u4") == img.view("<u4")).all()
    return img, st, states


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == 4 and want.dtype.itemsize == 4, "%s: %s vs %s" % (what, got.shape, want.shape)
    ne = got.view("<u4") != want.view("<u4")
    assert not ne.any(), "%s: %d of %d words differ; first at %s" % (what, int(ne.sum()), ne.size, tuple(np.argwhere(ne)[0]) if ne.any() else None)
