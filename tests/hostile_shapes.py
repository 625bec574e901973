"""Hostile shapes (test infrastructure, next to void_material.py and hostile_materials.py): spheres of radius -0.5, 0 and 1e-20,
boxes written with negative and zero extents, cylinders with a zero axis, a negative and a zero radius, meshes scaled by 0, -0.6
and 1e-20 or turned by the quaternion 0 0 0 0, lights made of such shapes, and single shapes of size 1e12, 1e6 and 1e8 that blow
the scene's box up.  The reference reads and renders all of them: tests/golden/make_golden.py --only-shapes writes its closest
hits, frames, final states, chains and scene-dumps (raycast_shapes.npz, renders_shapes.npz, chains_shapes.npz,
manifest.json["generated"]["shapes"]), and the CPU tests (tests/test_hostile_shapes_host.py) and the GPU tests
(tests/test_gpu_hostile_shapes.py) build the files and the rays from here.

The scenes, as texts (light_groups_cases' room and camera; every hostile shape under a `brdf` line of its own, so that `mat` in
a hit record names the shape):
  shapes_seen     all of HOSTILE between the room and light_groups_cases.THREE_LIGHTS, in front of the camera
  shapes_lights   the room, three diffuse spheres and six lights: a sphere of radius -0.9, a sphere of radius 0, a zero-axis
                  cylinder, cylinders of radius -0.3 and 0, and one ordinary sphere light
  shapes_far_<k>  the room, the all-lobes spheres, the three lights and ONE far or huge shape (FAR): each changes the quadric
                  slack of every other shape.  The mesh scaled by 1e8 is here and not in shapes_seen for that reason
  shapes_leaves   shapes_seen's shapes among seven slabs larger than any of them and a grid of small ordinary shapes: the slabs
                  fill the analytic prologue, so every hostile shape lies in a tree leaf
  <scene>_plain   the scene without its hostile shapes (shapes_lights: without its hostile lights)
  <scene>_dark<g> reference_goldens.dark_text's dark twins of shapes_seen (3) and shapes_lights (6)
and one scene of arrays (arrays_scene: what a file cannot express, held against the oracle alone).

Every line listed here made the reference end with status 0 within its time limit (make_golden.py checks that on every run);
none had to be left out.  The product refuses three further lines at commit -- `sphere 0.0e+39 ...` (a NaN centre), a radius of
1.0e+39 (inf) and one of 1.0e+20 --, which the reference renders: REFUSED, pinned by test_hostile_shapes_host.py.

Everything is compared with hostile_materials.same_words: bit for bit, NaN matching NaN.  No pixel, ray or point is skipped."""
import os
import re
import shutil
import zlib

import numpy as np

import hostile_materials as hm
import host_sim_tool as hs
import light_groups_cases as lg
import raycast_cases
import reference_goldens as rg
import void_material as vm
from conftest import DATA

W, H = lg.W, lg.H          # 24 x 16
BIG = (96, 64)
SPP = 16
SEED = 2024
RR = 0.8
RECT = lg.RECT
CHAIN_SAMPLES = rg.CHAIN_SAMPLES
FILES = ("raycast_shapes.npz", "renders_shapes.npz", "chains_shapes.npz")
MESH = "letterX.ply"
HEAD = vm.HEAD                                           # screen, camera, ambient
ROOM = "\n".join(lg.ROOM.splitlines()[3:]) + "\n"        # seven `brdf` lines, seven boxes: materials 1 .. 7
ROOM_MATERIALS = 7

# (name, kind, the shape's line), in file order; the shape's material is MAT[name]
HOSTILE = (
    ("sphere_neg", "sphere", "sphere 0.000000 0.000000 0.900000 -0.5"),
    ("sphere_zero", "sphere", "sphere 1.000000 1.000000 0.800000 0.0"),
    ("sphere_tiny", "sphere", "sphere -1.000000 0.800000 0.700000 1.0e-20"),
    ("box_inv1", "box", "box 1.000000 -1.000000 0.000000 -0.700000 0.700000 1.600000"),        # one inverted axis
    ("box_inv3", "box", "box 2.000000 2.000000 1.600000 -0.700000 -0.700000 -1.600000"),       # three
    ("box_flat", "box", "box 2.500000 0.000000 0.500000 0.700000 0.700000 0.000000"),          # flat
    ("cyl_axis0", "cylinder", "cylinder 1.800000 2.300000 0.300000 0.000000 0.000000 0.000000 0.25"),
    ("cyl_neg", "cylinder", "cylinder -0.500000 2.000000 0.300000 0.700000 -0.900000 1.100000 -0.25"),
    ("cyl_zero", "cylinder", "cylinder 0.500000 -2.000000 0.300000 0.700000 -0.900000 1.100000 0.0"),
    ("mesh_zero", "mesh", "mesh letterX.ply  1.600000 0.300000 1.100000 0.0  q 0.707107 0.707107 0 0"),
    ("mesh_neg", "mesh", "mesh letterX.ply  3.000000 -0.500000 1.100000 -0.6  q 0.707107 0.707107 0 0"),
    ("mesh_tiny", "mesh", "mesh letterX.ply  0.300000 1.600000 1.100000 1.0e-20  q 0.707107 0.707107 0 0"),
    ("mesh_q0", "mesh", "mesh letterX.ply  2.800000 1.800000 1.100000 0.6  q 0 0 0 0"),
    # an axis whose squared length underflows to 0 and a box written with no extent at all.  The cylinder's bounds in the
    # reference's octree are 0/0: with this line in the scene its walk finds the cylinder of radius 0 on 180 of 4 000 rays aimed
    # along that cylinder's axis, without it on 1 003 -- where the reference finds a shape and where it does not is what is pinned
    ("cyl_axis_tiny", "cylinder", "cylinder 2.600000 -1.600000 0.300000 0.000000 0.000000 1.0e-30 0.25"),
    ("box_point", "box", "box 0.500000 2.600000 0.600000 0.000000 0.000000 0.000000"),
)
NAMES = tuple(n for n, _, _ in HOSTILE)
KIND = {n: k for n, k, _ in HOSTILE}
KINDS_OF_SHAPE = ("sphere", "box", "cylinder", "mesh")
MAT = {n: ROOM_MATERIALS + 1 + i for i, n in enumerate(NAMES)}
# where rays are aimed: a centre, a half-extent about it and, for the cylinder without a radius, the half axis to spread along: the
# reference's cylinder test reports rays that all but meet the axis of a cylinder of radius 0, so that shape is hit by rays aimed
# that closely.  The spheres of radius 0 and 1e-20 and the meshes scaled to a point get rays that pass within 0.004 of them
AIM = {"sphere_neg": ((0, 0, 0.9), 0.5), "sphere_zero": ((1, 1, 0.8), 0.004), "sphere_tiny": ((-1, 0.8, 0.7), 0.004),
       "box_inv1": ((0.65, -0.65, 0.8), 0.8), "box_inv3": ((1.65, 1.65, 0.8), 0.8), "box_flat": ((2.85, 0.35, 0.5), 0.4),
       "cyl_axis0": ((1.8, 2.3, 0.3), 0.3), "cyl_neg": ((-0.15, 1.55, 0.85), 0.7), "cyl_zero": ((0.85, -2.45, 0.85), 0.002, (0.33, -0.43, 0.52)),
       "mesh_zero": ((1.6, 0.3, 1.1), 0.004), "mesh_neg": ((3.0, -0.5, 1.1), 0.6), "mesh_tiny": ((0.3, 1.6, 1.1), 0.004),
       "mesh_q0": ((2.8, 1.8, 1.1), 0.6), "cyl_axis_tiny": ((2.6, -1.6, 0.3), 0.3), "box_point": ((0.5, 2.6, 0.6), 0.004)}
# what the reference's closest-hit records say of the rays that start inside the room (asserted by test_hostile_shapes_host.py):
# a shape is named on at least 32 of them, or on none.  (raycast_cases' rays from 1e8 and further away are another matter: from
# there the float32 quadratic "hits" any sphere, and seven of them name the spheres of radius 0 and 1e-20.)
HIT = ("sphere_neg", "box_inv1", "box_inv3", "box_flat", "cyl_neg", "cyl_zero", "mesh_neg", "mesh_q0")   # NEVER: the other seven
NEVER = tuple(n for n in NAMES if n not in HIT)


def _brdf(i, lobes=False):
    """a diffuse material of its own colour per shape; with lobes every third one also has a specular lobe"""
    kd = (0.25 + 0.05 * (i % 11), 0.80 - 0.05 * (i % 9), 0.30 + 0.05 * (i % 7))
    ks = (0.5, 0.5, 0.5) if lobes and i % 3 == 1 else (0.0, 0.0, 0.0)
    return "brdf %.6f %.6f %.6f %.6f %.6f %.6f 10 0.000000 0.000000 0.000000 1.0" % (kd + ks)


# for the follow renders: the hostile shapes that rays do meet (HIT), turned into mirrors and glass -- Kd = 0, so a sample is
# followed THROUGH them and its bounce ray starts on a sphere of radius -0.5, an inverted or flat box, a cylinder of radius -0.25
# or 0, a mesh scaled by -0.6 or turned by a zero quaternion.  Every shape keeps a `brdf` line of its own: MAT stands
MIRROR = "brdf 0.000000 0.000000 0.000000 1.000000 1.000000 1.000000 20 0.000000 0.000000 0.000000 1.0"
GLASS = "brdf 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 10 1.000000 1.000000 1.000000 1.4"
FOLLOW_SPECULAR = {"sphere_neg": GLASS, "box_inv1": MIRROR, "box_inv3": GLASS, "box_flat": MIRROR, "cyl_neg": MIRROR, "cyl_zero": GLASS,
                   "mesh_neg": MIRROR, "mesh_q0": GLASS}
assert set(FOLLOW_SPECULAR) == set(HIT)


def hostile_block(lobes=True, specular=False):
    return "".join("%s\n%s\n" % (FOLLOW_SPECULAR[n] if specular and n in FOLLOW_SPECULAR else _brdf(i, lobes), line) for i, (n, _, line) in enumerate(HOSTILE))


# ---- shapes_lights ---------------------------------------------------------------------------------------------------------------
LIGHT_NAMES = ("light_sphere_neg", "light_sphere_zero", "light_cyl_axis0", "light_cyl_neg", "light_cyl_zero", "light_plain")
HOSTILE_LIGHTS = """light 3 3 2
sphere 0.000000 0.000000 2.800000 -0.9
light 2 1 1
sphere 3.000000 1.000000 2.000000 0.0
light 1 3 1
cylinder 2.000000 -1.000000 1.500000 0.000000 0.000000 0.000000 0.3
light 1 1 3
cylinder -1.200000 -1.200000 2.600000 2.400000 0.000000 0.000000 -0.3
light 3 1 1
cylinder -1.200000 1.200000 2.600000 2.400000 0.000000 0.000000 0.0
"""
PLAIN_LIGHT = """light 2 2 2
sphere 1.500000 -2.000000 3.000000 0.5
"""
N_LIGHTS = {"shapes_seen": 3, "shapes_lights": 6}

# ---- shapes_far -------------------------------------------------------------------------------------------------------------------
FAR = {
    "sphere_r": "sphere 0.000000 0.000000 0.900000 1.0e+12",
    "sphere_c": "sphere 1.0e+12 0.000000 0.900000 0.5",
    "box": "box 1.0e+6 0.000000 0.900000 0.500000 0.500000 0.500000",
    "mesh": "mesh letterX.ply  1.600000 0.300000 1.100000 1.0e+8  q 0.707107 0.707107 0 0",
}
FAR_SCENES = tuple("shapes_far_" + k for k in FAR)


# ---- shapes_leaves ---------------------------------------------------------------------------------------------------------------
def _leaves_fill():
    """seven slabs along the ceiling, each larger (in the half area of its box) than every hostile box, which with the room's
    seven boxes spend the analytic prologue's whole budget; and a 4 x 3 grid of small ordinary spheres, boxes and cylinders on
    the floor, so that the leaves which hold the hostile shapes hold ordinary ones too.  table_scenes' way of generating a room:
    a rule, no random draw"""
    out = ["brdf 0.500000 0.500000 0.600000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0"]
    for k in range(7):
        out.append("box %.6f %.6f 8.000000 2.200000 2.200000 0.050000" % (-2.5 + 2.4 * (k % 4), -2.5 + 2.4 * (k // 4)))
    out.append("brdf 0.700000 0.400000 0.300000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0")
    for j in range(3):
        for i in range(4):
            x, y = -2.4 + 1.7 * i + 0.15 * j, -2.6 + 2.3 * j
            k = (i + j) % 3
            if k == 0:
                out.append("sphere %.6f %.6f 0.150000 0.15" % (x, y))
            elif k == 1:
                out.append("box %.6f %.6f 0.000000 0.250000 0.250000 0.300000" % (x, y))
            else:
                out.append("cylinder %.6f %.6f 0.050000 0.200000 0.100000 0.350000 0.06" % (x, y))
    return "\n".join(out) + "\n"


# ---- the texts ---------------------------------------------------------------------------------------------------------------------
SCENES = ("shapes_seen", "shapes_lights") + FAR_SCENES + ("shapes_leaves",)
NO_NONFINITE = ("shapes_seen", "shapes_leaves") + FAR_SCENES   # no reference frame of these holds a non-finite word


def text(name, plain=False, specular=False):
    """the text of a scene of SCENES; plain: without its hostile shapes; specular (shapes_seen, shapes_leaves): FOLLOW_SPECULAR's
    shapes as mirrors and glass"""
    if name == "shapes_seen":
        return HEAD + ROOM + ("" if plain else hostile_block(specular=specular)) + lg.THREE_LIGHTS
    if name == "shapes_lights":
        return HEAD + ROOM + lg.SPHERES["diffuse"] + ("" if plain else HOSTILE_LIGHTS) + PLAIN_LIGHT
    if name in FAR_SCENES:
        far = "" if plain else _brdf(5) + "\n" + FAR[name[len("shapes_far_"):]] + "\n"
        return HEAD + ROOM + lg.SPHERES["all_lobes"] + far + lg.THREE_LIGHTS
    if name == "shapes_leaves":
        return HEAD + ROOM + ("" if plain else hostile_block(lobes=False, specular=specular)) + _leaves_fill() + lg.THREE_LIGHTS
    raise KeyError(name)


DARK = tuple("%s_dark%d" % (n, g) for n in N_LIGHTS for g in range(N_LIGHTS[n]))
PLAIN = tuple(n + "_plain" for n in SCENES)
STEMS = SCENES + PLAIN + DARK
# written at test time for the follow renders alone; the reference has no frame of them (every follow reference is the oracle's)
SPECULAR = ("shapes_seen_specular", "shapes_leaves_specular")


def scene_text(stem):
    if stem in SPECULAR:
        return text(stem[:-len("_specular")], specular=True)
    if stem in SCENES:
        return text(stem)
    if stem in PLAIN:
        return text(stem[:-len("_plain")], plain=True)
    m = re.match(r"(\w+)_dark(\d)$", stem)
    if m and m.group(1) in N_LIGHTS:
        return rg.dark_text(text(m.group(1)), int(m.group(2)), lights=N_LIGHTS[m.group(1)])
    raise KeyError(stem)


# (scene, policy, chunk, (w, h), whether the final states are kept) of renders_shapes.npz, all at SPP and SEED
POLICIES = (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))
RENDERS = ([(s, p, c, (W, H), p == "pixel") for s in SCENES for p, c in POLICIES] +
           [(s, p, c, BIG, False) for s in SCENES for p, c in POLICIES[:2]] +
           [(s, "pixel", 0, (W, H), False) for s in PLAIN + DARK])
CHAINS = ("shapes_seen", "shapes_lights", "shapes_leaves")


def key(scene, policy, chunk, size):
    return scene + "__" + rg.render_key(policy, size[0], size[1], SPP, chunk, SEED)


def write(directory, stem, txt=None):
    """-> (scn, base) of the scene's file in directory, the PLY file its `mesh` lines name next to it"""
    dst = os.path.join(str(directory), MESH)
    if not os.path.exists(dst):
        shutil.copyfile(os.path.join(DATA, MESH), dst)
    return rg.write_text(directory, stem, scene_text(stem) if txt is None else txt), str(directory) + "/"


same_words = hm.same_words
chains_from = hm.chains_from


class Case(hm.Case):
    """hostile_materials.Case of a stem of STEMS"""
    write_scene = staticmethod(write)


_cases = {}
_shared = {}


def case(api, oracle, name, tmp_path_factory, commit=""):
    """the case of a stem, once.  commit: a tag for a second commit of the same file (the caller has set the builder's knobs, as
    PROLOGUE_WIDE, in the environment); what the tests expect of it is what they expect of the first"""
    if name + commit not in _cases:
        _cases[name + commit] = Case(api, oracle, name, tmp_path_factory.mktemp("shapes_" + name))
    return _cases[name + commit]


# ---- where the hostile shapes are in the arrays, and in the tree -----------------------------------------------------------------------
def shape_index(flat):
    """{name: (kind, the index of the shape in its array of flat)}: the shape whose material is MAT[name]"""
    out = {}
    for n in NAMES:
        arr = {"sphere": flat.spheres["mat"], "box": flat.boxes["mat"], "cylinder": flat.cylinders["mat"],
               "mesh": np.array([m["mat"] for m in flat.meshes], "<u4")}[KIND[n]]
        at = np.flatnonzero(arr == MAT[n])
        assert len(at) == 1, n
        out[n] = (KIND[n], int(at[0]))
    return out


PROLOGUE_WIDE = {"ORT_ANALYTIC_PROLOGUE": "24"}   # a commit whose prologue takes every box and sphere of shapes_seen and one cylinder


def prologue_of(c, env=None):
    """tools/host_sim --tree-check on the case's file -> ({kind: the source indices the analytic prologue holds}, the check's own
    line as tree_shapes.tree_check reads it).  Every other shape lies in exactly one leaf: the check fails otherwise"""
    r = hs.run(hs.built("host_sim"), ["--tree-check", c.scn, c.base], env=env)
    m = re.search(r"^prologue: box([ \d]*) sphere([ \d]*) cylinder([ \d]*)$", r.stderr, re.M)
    assert r.stdout.startswith("tree-check ok:") and m, r.stdout + r.stderr
    words = r.stdout.split()
    return ({k: [int(x) for x in m.group(i + 1).split()] for i, k in enumerate(("box", "sphere", "cylinder"))},
            {words[i]: int(words[i + 1]) for i in range(2, words.index("max_leaf"), 2)})


def in_prologue(c, env=None):
    """-> {name: whether the hostile shape is a prologue shape of the commit} (a mesh's triangles never are)"""
    pro, _ = prologue_of(c, env)
    return {n: kind != "mesh" and i in pro[kind] for n, (kind, i) in shape_index(c.flat).items()}


# ---- rays -------------------------------------------------------------------------------------------------------------------------
N_AIMED = 1024         # per hostile shape
N_ANY = 1500
RAY_KINDS = NAMES + ("any", "edges")


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype("<f4")


def _inside(rng, n, near):
    if near:
        return np.stack([rng.uniform(-2.5, 6.5, n), rng.uniform(-2.5, 6.5, n), rng.uniform(0.05, 6.0, n)], axis=1)
    return np.stack([rng.uniform(-2.5, 14.5, n), rng.uniform(-2.5, 14.5, n), rng.uniform(0.05, 8.8, n)], axis=1)


def ray_sets(flat, cast_t):
    """(rays (n, 6) float32, kind (n,) index into RAY_KINDS) on shapes_seen: 1 024 rays at each hostile shape from origins inside
    the room (half of them near the table), 1 500 from inside the room in any direction, and raycast_cases.cases at scale 1
    (non-finite, zero, extreme and grazing rays; cast_t(rays) -> t places those that start on a surface: the reference's cast in
    make_golden.py, the oracle's in the tests -- the manifest's SHA-256 of the rays says they agree)"""
    rng = np.random.default_rng(zlib.crc32(b"hostile shapes rays"))
    parts = []
    for n in NAMES:
        centre, half = AIM[n][:2]
        o = np.where((np.arange(N_AIMED) % 2 == 0)[:, None], _inside(rng, N_AIMED, True), _inside(rng, N_AIMED, False))
        target = np.asarray(centre, np.float64) + rng.uniform(-1.0, 1.0, (N_AIMED, 3)) * half
        if len(AIM[n]) > 2:
            target = target + rng.uniform(-1.0, 1.0, (N_AIMED, 1)) * np.asarray(AIM[n][2], np.float64)
        parts.append(np.concatenate([o, _unit(target - o)], axis=1).astype("<f4"))
    parts.append(np.concatenate([_inside(rng, N_ANY, False), raycast_cases.unit_vectors(rng, N_ANY)], axis=1).astype("<f4"))
    edges, _ = raycast_cases.cases(flat, cast_t, seed=27, scale=1)
    parts.append(edges)
    rays = np.ascontiguousarray(np.concatenate(parts), "<f4")
    return rays, np.repeat(np.arange(len(parts)), [len(x) for x in parts]).astype(np.int32)


rays_sha256 = vm.rays_sha256


def rays_of(c):
    """ray_sets of the shapes_seen case, placed by the oracle's casts, once"""
    if "rays" not in _shared:
        osc = c.twin(None)
        _shared["rays"] = ray_sets(c.flat, lambda r: osc.raycast(r[:, 0:3], r[:, 3:6])[0])
    return _shared["rays"]


def exact_subset(kind):
    """the rays that go through the exact walk alone (every ray re-cast: three orders of magnitude slower): the first 120 at each
    hostile shape and the first 200 in any direction, 2 000 in all -> a mask over the set"""
    m = np.zeros(len(kind), bool)
    for k in range(len(NAMES)):
        m[np.flatnonzero(kind == k)[:120]] = True
    m[np.flatnonzero(kind == RAY_KINDS.index("any"))[:200]] = True
    assert m.sum() == 2000
    return m


def records(z, name):
    """raycast_shapes.npz -> (t, n, mat) of the reference's closest hits on shapes_seen or shapes_leaves, for the same rays"""
    pre = {"shapes_seen": "", "shapes_leaves": "leaves__"}[name]
    return z[pre + "t"], z[pre + "n"], z[pre + "mat"]


RAYCAST_SCENES = ("shapes_seen", "shapes_leaves")


def hostile_hit(mat):
    return np.isin(np.asarray(mat), list(MAT.values()))


def one_ulp_ladder(rays, t, mat):
    """occluded_cases.laddered over the reference's t: per ray the rungs of its ladder, among them tmax one ulp below, at and one
    ulp above the hit -> (rays, tmax, expected)"""
    import occluded_cases as oc
    rr, tm, want, _ = oc.laddered(rays, t, mat)
    return rr, tm, want


# ---- points lifted off the hostile shapes' hit points ---------------------------------------------------------------------------------
N_POINTS = 192


def point_set(rays, kind, t, n, mat):
    """192 points: the hit points o + t d of the rays from inside the room whose closest hit names a hostile shape, taken in turn over the shapes
    that are hit, lifted by 1e-3 along the record's normal turned towards the ray's origin -> (points (192, 6) float32: p and n,
    seeds (192,) uint32, the material each point stands on)"""
    rng = np.random.default_rng(zlib.crc32(b"hostile shapes points"))
    t, n, mat = np.asarray(t, "<f4"), np.asarray(n, "<f4"), np.asarray(mat)
    ok = (kind != RAY_KINDS.index("edges")) & np.isfinite(rays).all(axis=1) & (t < 1e3) & (t > 1e-2) & np.isfinite(n).all(axis=1) & (np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-3)
    per = [np.flatnonzero(ok & (mat == MAT[name])) for name in NAMES]
    per = [p for p in per if len(p)]
    take, k = [], 0
    while len(take) < N_POINTS:
        p = per[k % len(per)]
        if k // len(per) < len(p):
            take.append(p[k // len(per)])
        k += 1
        assert k < 100 * N_POINTS
    take = np.array(take)
    r, nn = rays[take], n[take]
    nn = np.where((np.sum(nn * r[:, 3:6], axis=1) > 0)[:, None], -nn, nn).astype("<f4")
    p = (r[:, 0:3] + t[take, None] * r[:, 3:6]).astype("<f4")
    p = (p + np.float32(1e-3) * nn).astype("<f4")
    seeds = rng.integers(1, 1 << 32, size=N_POINTS, dtype=np.uint64).astype("<u4")
    return np.ascontiguousarray(np.concatenate([p, nn], axis=1), "<f4"), seeds, mat[take]


def points_of(c, hits):
    """point_set of the shapes_seen case on the reference's records (raycast_shapes.npz), once"""
    if "points" not in _shared:
        rays, kind = rays_of(c)
        _shared["points"] = point_set(rays, kind, hits["t"], hits["n"], hits["mat"])
    return _shared["points"]


# ---- views ---------------------------------------------------------------------------------------------------------------------------
VIEW_SEEDS = vm.VIEW_SEEDS
FEATURE_SPP = vm.FEATURE_SPP
QUERY_SPP = vm.QUERY_SPP


def view_cameras(api, c):
    """three views: the scene's own camera, light_groups_cases' second pose, and the scene's own moved to the centre of the sphere
    of radius -0.5 (shapes_seen, shapes_leaves) or, in a scene without it, a step nearer the table"""
    cam = c.cam.copy()
    s = c.flat.spheres[c.flat.spheres["r"] == np.float32(-0.5)]
    cam[0] = s[0]["center"] if len(s) else cam[0] * np.float32(0.8)
    return np.stack([c.cam, lg.batch_cameras(api, c)[1], cam])


# ---- the renders that follow mirrors and glass (follow_cases.py) ---------------------------------------------------------------------
# shapes_seen and shapes_leaves, the scenes of the feature tests, give every hostile shape a material with a diffuse part: no sample
# is followed there (the oracle's count is 0 from every view), so the follow render must BE the first-hit render on them
# (identity 2 of include/ort.h).  Their SPECULAR twins, written at test time, make the hostile shapes that rays meet mirrors and
# glass: there the bounce rays START ON hostile shapes -- in the prologue (shapes_seen_specular) and in leaves
# (shapes_leaves_specular).  The far scenes keep the room's glass and mirror spheres next to one shape of size 1e6 to 1e12
FOLLOW_SCENES = ("shapes_seen", "shapes_leaves") + SPECULAR + FAR_SCENES
FOLLOWING = SPECULAR + FAR_SCENES
FOLLOW_SETTINGS = hm.FOLLOW_SETTINGS


def follow_world(api, c):
    """follow_cases' world of a case: the single frame from the scene's own camera on SEED, the batch view_cameras on VIEW_SEEDS"""
    import follow_cases as fw
    return fw.case_world(c, view_cameras(api, c), VIEW_SEEDS)


def follow_conditions(api, c):
    """printed and asserted from the oracle's side (follow_cases.chain; the scene's own frame at rr 0.5, cap 64).  A scene without
    a specular-only material follows nothing from any view (-> False: the caller asserts identity 2).  Otherwise at least 5 % of
    the samples are followed, some path bounces twice, at least 10 die at the roulette and none reaches the cap (-> True); on the
    SPECULAR twins samples are followed through a hostile sphere, a hostile box, a hostile cylinder and a hostile mesh, and at
    rr 0.8, cap 2 at least 5 samples are recorded at the cap on a specular-only surface"""
    import follow_cases as fw
    w = follow_world(api, c)
    ch = fw.chains(w, FEATURE_SPP, *FOLLOW_SETTINGS[0])
    spec = fw.specular_only(c.flat)
    through = {n: int(ch[0].followed_by_mat[MAT[n]]) for n in NAMES if MAT[n] < len(ch[0].followed_by_mat) and ch[0].followed_by_mat[MAT[n]]}
    print("%s: specular-only materials %s; followed share per frame %s, deaths %s, deepest b %s; the own frame's samples followed through hostile shapes: %s"
          % (c.name, np.flatnonzero(spec).tolist(), ["%.3f" % (k.followed / k.samples) for k in ch], [k.deaths for k in ch], [k.max_b for k in ch],
             through if c.name in SPECULAR else "-"))
    assert all(k.at_cap == 0 for k in ch)
    if not spec.any():
        assert all(k.followed == 0 and k.rays == k.samples for k in ch)
        return False
    assert ch[0].followed >= 0.05 * ch[0].samples and ch[0].deaths >= 10 and ch[0].max_b >= 2
    if c.name in SPECULAR:
        assert sorted(np.flatnonzero(spec).tolist()) == sorted(MAT[n] for n in FOLLOW_SPECULAR)
        for kind in KINDS_OF_SHAPE:
            assert any(KIND[n] == kind for n in through), (kind, through)
        assert fw.chains(w, FEATURE_SPP, *FOLLOW_SETTINGS[1])[0].capped_specular >= 5
    return True


# what the CPU and the GPU tests share, computed once and left unchanged: void_material's helpers, which key on the case's name
oracle_frame, pixel_planes, chains_of, first_hits = vm.oracle_frame, vm.pixel_planes, vm.chains_of, vm.first_hits
feature_expected, assert_features, ao_world, advance = vm.feature_expected, vm.assert_features, vm.ao_world, vm.advance


# ---- the scene of arrays: what a file cannot express ------------------------------------------------------------------------------------
ARRAYS = ("arrays_shapes",)


def arrays_scene(api):
    """void_material.arrays_scene's room, camera and lights with: a sphere of radius -0.0, one of a denormal radius (1e-40: r * r
    underflows to 0), a box with min == max on all three axes, a mesh whose index buffer repeats one vertex three times (in front
    of the letter's own triangles), and hostile shapes that carry material 0 -- a sphere of radius -0.5, a box with max < min and
    a zero-axis cylinder -- next to solid ones of the same kinds"""
    mats = np.zeros(7, api.MATERIAL_DTYPE)
    mats["ior"][:] = 1.0
    mats["diffuse"][1] = (0.7, 0.7, 0.7)
    mats["diffuse"][2] = (0.8, 0.3, 0.3)
    mats["diffuse"][3] = (0.3, 0.3, 0.8); mats["specular"][3] = (1, 1, 1, 20)
    mats["is_light"][4:6] = 1
    mats["emit"][4] = (4, 4, 3)
    mats["emit"][5] = (1, 2, 3)
    mats["diffuse"][6] = (0.2, 0.8, 0.2)
    boxes = [((-4, -4, -0.2), (4, 4, 0), 1), ((-4, -4, 5), (4, 4, 5.2), 1), ((-4.2, -4, -0.2), (-4, 4, 5.2), 6),
             ((1.1, -1.9, 0.6), (1.1, -1.9, 0.6), 2),                                     # min == max
             ((4, -4, -0.2), (4.2, 4, 5.2), 1), ((-4, -4.2, -0.2), (4, -4, 5.2), 3), ((-4, 4, -0.2), (4, 4.2, 5.2), 1),
             ((-1.4, 1.1, 0.9), (-2.0, 0.5, 0), 0),                                       # max < min, material 0
             ((0.3, 2.2, 0.7), (-0.3, 1.6, 0), 6)]                                        # max < min, solid
    box = np.zeros(len(boxes), api.BOX_DTYPE)
    for i, v in enumerate(boxes):
        box[i] = v
    spheres = [((0, 0, 4.2), 0.7, 4), ((0.3, 0.2, 0.6), 0.5, 2),
               ((1.6, 0.4, 1.4), -0.0, 6),                                                # -0.0
               ((1.4, -1.0, 0.45), 1e-40, 3),                                             # denormal
               ((-1.0, -1.3, 0.5), -0.5, 0),                                              # negative, material 0
               ((-0.5, -2.6, 0.4), -0.4, 2),                                              # negative, solid
               ((-2.5, -2.5, 3.0), 0.5, 5)]
    sph = np.zeros(len(spheres), api.SPHERE_DTYPE)
    for i, v in enumerate(spheres):
        sph[i] = v
    assert sph["r"][2].tobytes() == np.float32(-0.0).tobytes() and 0 < sph["r"][3] < np.finfo("<f4").tiny
    cyls = [((-2.5, 2.5, 0.3), (0.9, 0.4, 1.5), 0.25, 6), ((2.2, -0.6, 0.2), (0, 0, 0), 0.2, 0),   # zero axis, material 0
            ((-3.0, -1.0, 2.0), (1.5, 0.3, 0.2), -0.2, 1), ((0.2, -1.8, 0.3), (0, 0, 0), 0.3, 2)]  # negative radius; zero axis, solid
    cyl = np.zeros(len(cyls), api.CYLINDER_DTYPE)
    for i, v in enumerate(cyls):
        cyl[i] = v
    lights = np.array([(1, 0), (1, 6), (2, 0), (2, 2), (2, 3)], api.LIGHT_DTYPE)   # the loader's rule: every cylinder with a material
    v, ix = vm._letter(api)
    place = lambda at, s: (v * np.float32(s) + np.asarray(at, "<f4")).astype("<f4")
    repeated = np.concatenate([np.array([0, 0, 0, 5, 5, 5], ix.dtype), ix.reshape(-1)])   # two triangles of one vertex each, first
    meshes = [dict(vertices=place((2.5, -2.5, 0.1), 0.5), indices=repeated, mat=3), dict(vertices=place((1.2, 1.2, 0.1), -0.6), indices=ix, mat=0),
              dict(vertices=place((-2.8, 2.0, 0.1), 0.0), indices=ix, mat=6)]
    q = np.array([0.279589, 0.480987, 0.718247, 0.416981], "<f4")
    return api.Scene.from_arrays(mats, sph, box, cyl, lights, meshes, camera_p=(3.3, 2.0, 2.6), camera_quat_xyzw=q, camera_height_ratio=0.3, screen=(W, H))


class ArraysCase(vm.ArraysCase):
    def __init__(self, api, oracle, name):
        self.name, self.oracle, self.csg = name, oracle, False
        self.scene = arrays_scene(api).commit()
        self.flat = self.scene.flatten(W, H)
        self.lights = [int(m) for m in np.nonzero(self.flat.materials["is_light"])[0]]
        self.cam = np.asarray(self.flat.camera, "<f4").reshape(4, 3)
        self._twins = {}


def arrays_case(api, oracle, name="arrays_shapes"):
    if name not in _cases:
        _cases[name] = ArraysCase(api, oracle, name)
    return _cases[name]


def arrays_rays(c):
    """1 000 rays from inside the room in any direction and 1 000 from inside it aimed at the hostile shapes of the arrays"""
    k = ("arrays rays", c.name)
    if k not in _shared:
        rng = np.random.default_rng(zlib.crc32(b"hostile shapes arrays rays"))
        inside = lambda n: np.stack([rng.uniform(-3.8, 3.8, n), rng.uniform(-3.8, 3.8, n), rng.uniform(0.1, 4.8, n)], axis=1)
        anyway = np.concatenate([inside(1000), raycast_cases.unit_vectors(rng, 1000)], axis=1).astype("<f4")
        f = c.flat
        at = [f.spheres[i]["center"] for i in (2, 3, 4, 5)] + [(f.boxes[i]["min"] + f.boxes[i]["max"]) / 2 for i in (3, 7, 8)]
        at += [cy["base"] + cy["axis"] / 2 for cy in f.cylinders] + [(m["aabb_min"] + m["aabb_max"]) / 2 for m in f.meshes]
        o = inside(1000)
        target = np.array(at, np.float64)[rng.integers(0, len(at), 1000)] + rng.normal(size=(1000, 3)) * 0.2
        aimed = np.concatenate([o, _unit(target - o)], axis=1).astype("<f4")
        _shared[k] = np.ascontiguousarray(np.concatenate([anyway, aimed]), "<f4")
    return _shared[k]


# ---- the scenes the product refuses at commit --------------------------------------------------------------------------------------------
REFUSED_MESSAGE = "scene contains a non-finite or oversized primitive"
# (what, the line): the lexer reads 0.0e+39 as 0 * inf = NaN and 1.0e+39 as inf, as the reference's does
REFUSED = (("nan_centre", "sphere 0.0e+39 0.000000 0.900000 0.5"), ("inf_radius", "sphere 0.000000 0.000000 0.900000 1.0e+39"),
           ("radius_1e20", "sphere 0.000000 0.000000 0.900000 1.0e+20"))
ACCEPTED = (("radius_1e12", FAR["sphere_r"]),)


def refused_text(line):
    return HEAD + ROOM + lg.SPHERES["diffuse"] + _brdf(5) + "\n" + line + "\n" + lg.THREE_LIGHTS
