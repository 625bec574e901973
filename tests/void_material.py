"""Shapes that carry material 0, the no-hit material (test infrastructure, next to hostile_materials.py).  In a .scn file every
shape written before the first `brdf` or `light` line gets material 0 (ort_parse.cpp, the reference's parser.cpp alike), and
ort_scene_create accepts mat = 0 on any shape.  Such a VOID shape is real geometry -- it wins closest-hit contests, has a
distance, a normal and a place in both trees -- and every caller of the hit treats it as a miss: occlusion byte 0, an open
ambient-occlusion sample, a path that ends, a feature sample that does not count.

The scenes, as texts (light_groups_cases' room, all-lobes spheres and three lights):
  void_seen    void shapes in front of the camera: a sphere over the table, a box on the floor, an oblique cylinder, a PLY mesh,
               a sphere bit-identical to one of the room's solid spheres (file order decides the tie: the void one is first), and
               a sphere that encloses the second light
  void_hidden  the same kinds of shapes in the corner behind the camera (x > 8, y > 6): no camera sample sees them, paths meet
               them at bounces only -- the scene the REFERENCE can render (a primary void hit dereferences a null material there)
  <scene>_solid    one grey `brdf` line in front of the void shapes: same geometry, trees and test order, every shape solid
  <scene>_removed  the void shapes left out
  <scene>_dark<g>  reference_goldens.dark_text's dark twins
  all_void     void_seen without any `brdf` or `light` line: one material, no lights, every frame +0
and one scene of arrays (arrays_scene: what a file cannot order, held against the oracle alone).

tests/golden/make_golden.py --only-void writes the reference's closest hits on void_seen (raycast_void.npz) and its frames,
final states and chains of void_hidden (renders_void.npz, chains_void.npz); the CPU tests (tests/test_void_material_host.py) and
the GPU tests (tests/test_gpu_void_material.py) build the files and the rays from here.  Everything is compared bit for bit."""
import hashlib
import os
import shutil
import zlib

import numpy as np

import hostile_materials as hm
import light_groups_cases as lg
import raycast_cases
import reference_goldens as rg
from conftest import DATA

W, H = lg.W, lg.H          # 24 x 16
BIG = (96, 64)
SPP = 16
SEED = 2024
RR = 0.8
RECT = lg.RECT
CHAIN_SAMPLES = rg.CHAIN_SAMPLES
NO_PRIM = 0xFFFFFFFF
FILES = ("raycast_void.npz", "renders_void.npz", "chains_void.npz")
GREY = "brdf " + hm.GREY
MESH = "letterX.ply"
HEAD = "\n".join(lg.ROOM.splitlines()[:3]) + "\n"   # screen, camera, ambient
BODY = "\n".join(lg.ROOM.splitlines()[3:]) + "\n" + lg.SPHERES["all_lobes"] + lg.THREE_LIGHTS
CAMERA_P = (5.553228, 2.942755, 2.900874)

# the void shapes of each scene, in file order; each line is one shape
VOID = {
    "void_seen": """sphere 0.700000 -0.200000 1.500000 0.4
box 2.000000 -1.500000 0.000000 0.700000 0.700000 1.600000
cylinder 1.800000 2.300000 0.300000 0.700000 -0.900000 1.100000 0.25
mesh letterX.ply  1.600000 0.300000 1.100000 0.6  q 0.707107 0.707107 0 0
sphere 1.000000 1.000000 0.800000 0.3
sphere 3.000000 1.000000 2.000000 0.6
""",
    "void_hidden": """sphere 10.000000 8.000000 1.500000 1.2
box 9.000000 10.000000 0.000000 2.000000 2.000000 3.000000
cylinder 12.000000 7.000000 0.300000 0.700000 2.900000 2.100000 0.6
mesh letterX.ply  11.000000 11.000000 2.000000 2.0  q 0.707107 0.707107 0 0
sphere 13.000000 12.000000 1.000000 0.8
sphere 12.000000 9.000000 5.000000 1.5
""",
}
SCENES = tuple(VOID)
TWINS = ("solid", "removed")
COINCIDENT = "sphere 1.000000 1.000000 0.800000 0.3"   # void_seen's fifth void shape and the room's second solid sphere
assert COINCIDENT in VOID["void_seen"] and COINCIDENT in lg.SPHERES["all_lobes"]
ENCLOSED_LIGHT = 1   # void_seen's last void sphere encloses THREE_LIGHTS' second light


def text(name, twin=None):
    """the text of void_seen or void_hidden, or of its `solid` or `removed` twin"""
    assert name in SCENES and twin in (None,) + TWINS
    void = {None: VOID[name], "solid": GREY + "\n" + VOID[name], "removed": ""}[twin]
    return HEAD + void + BODY


def dark(name, keep):
    return rg.dark_text(text(name), keep)


def all_void():
    """void_seen with no `brdf` and no `light` line: every shape carries material 0"""
    return "\n".join(l for l in text("void_seen").splitlines() if not l.startswith(("brdf ", "light "))) + "\n"


def scene_text(stem):
    """stem: void_seen, void_hidden, <scene>_solid, <scene>_removed, <scene>_dark<g> or all_void"""
    if stem == "all_void":
        return all_void()
    for name in SCENES:
        if stem == name:
            return text(name)
        for t in TWINS:
            if stem == name + "_" + t:
                return text(name, t)
        for g in range(3):
            if stem == "%s_dark%d" % (name, g):
                return dark(name, g)
    raise KeyError(stem)


STEMS = tuple([n + s for n in SCENES for s in ("", "_solid", "_removed", "_dark0", "_dark1", "_dark2")] + ["all_void"])
# what the reference renders: void_hidden and its dark twins.  void_seen and all_void have primary void hits, which it cannot take
RENDERED = ("void_hidden",) + tuple("void_hidden_dark%d" % g for g in range(3))
RENDERS = ([("void_hidden", p, c, (W, H), p == "pixel") for p, c in (("pixel", 0), ("chunk", 4), ("whole", 0), ("tile32", 0))] +
           [("void_hidden", p, c, BIG, False) for p, c in (("pixel", 0), ("chunk", 4))] +
           [("void_hidden_dark%d" % g, "pixel", 0, (W, H), False) for g in range(3)])


def key(scene, policy, chunk, size):
    return scene + "__" + rg.render_key(policy, size[0], size[1], SPP, chunk, SEED)


def write(directory, stem, txt=None):
    """-> (scn, base) of the scene's file in directory, the PLY file its `mesh` line names next to it"""
    dst = os.path.join(str(directory), MESH)
    if not os.path.exists(dst):
        shutil.copyfile(os.path.join(DATA, MESH), dst)
    return rg.write_text(directory, stem, scene_text(stem) if txt is None else txt), str(directory) + "/"


def void_counts(name):
    """how many spheres, boxes, cylinders and meshes of a scene are void: they are the first of each array"""
    kinds = [l.split()[0] for l in VOID[name].splitlines()]
    return {k: kinds.count(k) for k in ("sphere", "box", "cylinder", "mesh")}


same_words = hm.same_words
chains_from = hm.chains_from


class Case(hm.Case):
    """hostile_materials.Case of a stem of STEMS"""
    write_scene = staticmethod(write)


_cases = {}
_shared = {}


def case(api, oracle, name, tmp_path_factory):
    if name not in _cases:
        _cases[name] = Case(api, oracle, name, tmp_path_factory.mktemp("void_" + name))
    return _cases[name]


# ---- the scene of arrays: what a file cannot order ------------------------------------------------------------------------------
ARRAYS = ("arrays_diffuse", "arrays_all_lobes")


def _letter(api):
    """data/letterX.ply's vertices and indices, read with the product's own loader"""
    k = "letter"
    if k not in _shared:
        t = HEAD + GREY + "\nmesh %s  0.000000 0.000000 0.000000 1.0  q 1 0 0 0\n" % MESH
        m = api.Scene.parse_scn(t, DATA + "/").flatten(W, H).meshes[0]
        _shared[k] = (m["vertices"].copy(), m["indices"].copy())
    return _shared[k]


def arrays_scene(api, flavour):
    """test_gpu_parity._degenerate_scene's room and camera (as hostile_materials.emission_scene has them) with void shapes in the
    middle and at the end of every array, a coincident void/solid pair in both orders for spheres and for boxes, and a void mesh
    between two solid ones.  flavour: arrays_diffuse (Ks = Kt = 0 everywhere) or arrays_all_lobes (a glass and a mirror sphere)"""
    assert flavour in ARRAYS
    mats = np.zeros(7, api.MATERIAL_DTYPE)
    mats["ior"][:] = 1.0
    mats["diffuse"][1] = (0.7, 0.7, 0.7)
    mats["diffuse"][2] = (0.8, 0.3, 0.3)
    mats["diffuse"][3] = (0.3, 0.3, 0.8)
    if flavour == "arrays_all_lobes":
        mats["diffuse"][2] = 0; mats["transmission"][2] = 1; mats["ior"][2] = 1.4
        mats["diffuse"][3] = 0; mats["specular"][3] = (1, 1, 1, 20)
    mats["is_light"][4:6] = 1
    mats["emit"][4] = (4, 4, 3)
    mats["emit"][5] = (1, 2, 3)
    mats["diffuse"][6] = (0.2, 0.8, 0.2)
    boxes = [((-4, -4, -0.2), (4, 4, 0), 1), ((-4, -4, 5), (4, 4, 5.2), 1), ((-4.2, -4, -0.2), (-4, 4, 5.2), 6),
             ((0.8, -2.2, 0), (1.4, -1.6, 1.2), 0),                                       # void, in the middle
             ((4, -4, -0.2), (4.2, 4, 5.2), 1), ((-4, -4.2, -0.2), (4, -4, 5.2), 3), ((-4, 4, -0.2), (4, 4.2, 5.2), 1),
             ((-2.0, 0.5, 0), (-1.4, 1.1, 0.9), 0), ((-2.0, 0.5, 0), (-1.4, 1.1, 0.9), 2),   # coincident: void first
             ((-0.3, 1.6, 0), (0.3, 2.2, 0.7), 6), ((-0.3, 1.6, 0), (0.3, 2.2, 0.7), 0),     # coincident: solid first
             ((2.0, 1.5, 0), (2.5, 2.0, 1.5), 0)]                                         # void, at the end
    box = np.zeros(len(boxes), api.BOX_DTYPE)
    for i, v in enumerate(boxes):
        box[i] = v
    spheres = [((0, 0, 4.2), 0.7, 4), ((0.3, 0.2, 0.6), 0.5, 2),
               ((1.6, 0.4, 1.4), 0.45, 0),                                                # void, in the middle
               ((1.4, -1.0, 0.45), 0.4, 3),
               ((-1.0, -1.3, 0.5), 0.45, 0), ((-1.0, -1.3, 0.5), 0.45, 6),                # coincident: void first
               ((-0.5, -2.6, 0.4), 0.4, 2), ((-0.5, -2.6, 0.4), 0.4, 0),                  # coincident: solid first
               ((-2.5, -2.5, 3.0), 0.5, 5),                                               # the second light ...
               ((-2.5, -2.5, 3.0), 0.8, 0)]                                               # ... enclosed by a void sphere, at the end
    sph = np.zeros(len(spheres), api.SPHERE_DTYPE)
    for i, v in enumerate(spheres):
        sph[i] = v
    cyls = [((-2.5, 2.5, 0.3), (0.9, 0.4, 1.5), 0.25, 6), ((2.2, -0.6, 0.2), (0.5, 0.7, 1.6), 0.2, 0),
            ((-3.0, -1.0, 2.0), (1.5, 0.3, 0.2), 0.2, 1), ((0.2, -1.8, 0.3), (-0.6, 0.5, 1.3), 0.2, 0)]
    cyl = np.zeros(len(cyls), api.CYLINDER_DTYPE)
    for i, v in enumerate(cyls):
        cyl[i] = v
    # the loader's rule for files: light spheres, and every cylinder with a material
    lights = np.array([(1, 0), (1, 8), (2, 0), (2, 2)], api.LIGHT_DTYPE)
    v, ix = _letter(api)
    place = lambda at, s: (v * np.float32(s) + np.asarray(at, "<f4")).astype("<f4")
    meshes = [dict(vertices=place((2.5, -2.5, 0.1), 0.5), indices=ix, mat=3), dict(vertices=place((1.2, 1.2, 0.1), 0.6), indices=ix, mat=0),
              dict(vertices=place((-2.8, 2.0, 0.1), 0.5), indices=ix, mat=6)]
    q = np.array([0.279589, 0.480987, 0.718247, 0.416981], "<f4")
    return api.Scene.from_arrays(mats, sph, box, cyl, lights, meshes, camera_p=(3.3, 2.0, 2.6), camera_quat_xyzw=q, camera_height_ratio=0.3, screen=(W, H))


ARRAY_PAIRS = {"spheres": ((4, 5), (7, 6)), "boxes": ((7, 8), (10, 9))}   # (void, solid) indices: void first, solid first


class ArraysCase:
    """arrays_scene committed, its flattened arrays and the oracle's scene (no reference CSG)"""

    def __init__(self, api, oracle, name):
        self.name, self.oracle, self.csg = name, oracle, False
        self.scene = arrays_scene(api, name).commit()
        self.flat = self.scene.flatten(W, H)
        self.lights = [int(m) for m in np.nonzero(self.flat.materials["is_light"])[0]]
        self.cam = np.asarray(self.flat.camera, "<f4").reshape(4, 3)
        self._twins = {}

    twin, table, per_light = hm.Case.twin, hm.Case.table, hm.Case.per_light

    def camera(self, size=None):
        size = tuple(size) if size else (W, H)
        return self.cam if size == (W, H) else np.asarray(self.scene.flatten(*size).camera, "<f4").reshape(4, 3)


def arrays_case(api, oracle, name):
    if name not in _cases:
        _cases[name] = ArraysCase(api, oracle, name)
    return _cases[name]


PAIR_RAYS = 64


def pair_rays(c, kind, order):
    """64 rays at a coincident pair of arrays_scene (kind: "spheres" or "boxes"; order 0: the void shape first in the array,
    1: the solid one first) from a point 1.2 towards the camera, with nothing in between -> (rays (64, 6), the solid shape's material)"""
    arr = getattr(c.flat, kind)
    v, s = ARRAY_PAIRS[kind][order]
    assert arr[v]["mat"] == 0 and arr[s]["mat"] != 0 and arr[v].tobytes()[:-4] == arr[s].tobytes()[:-4] and (v < s) == (order == 0)
    rng = np.random.default_rng(zlib.crc32(("void pair %s %d" % (kind, order)).encode()))
    centre = arr[v]["center"] if kind == "spheres" else (arr[v]["min"] + arr[v]["max"]) / 2 + np.float32((0, 0, 0.2))
    to_cam = np.asarray(c.cam[0], np.float64) - centre
    o = np.tile((centre + 1.2 * to_cam / np.linalg.norm(to_cam)).astype("<f4"), (PAIR_RAYS, 1))
    d = centre + rng.normal(size=(PAIR_RAYS, 3)).astype("<f4") * np.float32(0.1 if kind == "spheres" else 0.06) - o
    return np.concatenate([o, _unit(d)], axis=1).astype("<f4"), int(arr[s]["mat"])


def arrays_rays(c):
    """the rays of the closest-hit and occlusion queries on arrays_scene: the four coincident pairs' 64 rays each, 1 000 rays from
    inside the room in any direction, and 500 from inside it aimed at the shapes that carry material 0 -> (rays, kind: 0 pair, 1
    any, 2 aimed)"""
    k = ("arrays rays", c.name)
    if k not in _shared:
        rng = np.random.default_rng(zlib.crc32(b"void arrays rays"))
        pairs = np.concatenate([pair_rays(c, kind, order)[0] for kind in ("spheres", "boxes") for order in (0, 1)])
        inside = lambda n: np.stack([rng.uniform(-3.8, 3.8, n), rng.uniform(-3.8, 3.8, n), rng.uniform(0.1, 4.8, n)], axis=1)
        anyway = np.concatenate([inside(1000), raycast_cases.unit_vectors(rng, 1000)], axis=1).astype("<f4")
        f = c.flat
        at = [s["center"] for s in f.spheres[f.spheres["mat"] == 0]] + [(b["min"] + b["max"]) / 2 for b in f.boxes[f.boxes["mat"] == 0]]
        at += [cy["base"] + cy["axis"] / 2 for cy in f.cylinders[f.cylinders["mat"] == 0]]
        at += [(m["aabb_min"] + m["aabb_max"]) / 2 for m in f.meshes if m["mat"] == 0]
        o = inside(500)
        target = np.array(at, np.float64)[rng.integers(0, len(at), 500)] + rng.normal(size=(500, 3)) * 0.15
        aimed = np.concatenate([o, _unit(target - o)], axis=1).astype("<f4")
        rays = np.ascontiguousarray(np.concatenate([pairs, anyway, aimed]), "<f4")
        _shared[k] = (rays, np.repeat(np.arange(3), [len(pairs), 1000, 500]))
    return _shared[k]


# ---- ray sets on void_seen ----------------------------------------------------------------------------------------------------------
N_GOLDEN, N_AIMED, N_SURFACE, N_PAIR = 4000, 2000, 500, 500
KINDS = ("golden", "aimed", "surface", "pair", "hostile")


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype("<f4")


def _targets(rng, flat, n, counts):
    """n points in and around the first counts[kind] shapes of each array (the void ones) and inside the void meshes' boxes"""
    pts = []
    for s in flat.spheres[:counts["sphere"]]:
        pts.append((s["center"], np.full(3, s["r"])))
    for b in flat.boxes[:counts["box"]]:
        pts.append(((b["min"] + b["max"]) / 2, (b["max"] - b["min"]) / 2))
    for c in flat.cylinders[:counts["cylinder"]]:
        pts.append((c["base"] + c["axis"] / 2, np.abs(c["axis"]) / 2 + c["r"]))
    for m in flat.meshes[:counts["mesh"]]:
        pts.append(((m["aabb_min"] + m["aabb_max"]) / 2, (m["aabb_max"] - m["aabb_min"]) / 2))
    which = rng.integers(0, len(pts), n)
    c = np.array([pts[k][0] for k in which], np.float64)
    e = np.array([pts[k][1] for k in which], np.float64)
    return c + rng.uniform(-0.7, 0.7, (n, 3)) * e


def ray_sets(flat, cast, parents=None):
    """(rays (n, 6) float32, kind (n,) index into KINDS) on void_seen; cast(rays) -> (t, mat) is the first cast that places the rays
    that start on a surface (the reference's in make_golden.py, the oracle's in the tests: the manifest's SHA-256 says they agree).
    golden: test_gpu_raycast.golden_like's distribution; aimed: from origins inside the room at the void shapes; surface: from a
    void surface -- the hit point o + t d of a ray whose closest hit carries material 0 --, new directions; pair: aimed at the
    coincident spheres; hostile: raycast_cases.cases at scale 1.  parents: a list that gets (the 500 rays whose hit points the
    surface rays start from, their t, their mat)"""
    rng = np.random.default_rng(zlib.crc32(b"void rays"))
    counts = void_counts("void_seen")
    golden = raycast_cases.golden_like(rng, N_GOLDEN)
    inside = lambda n: np.stack([rng.uniform(-2.5, 14.5, n), rng.uniform(-2.5, 14.5, n), rng.uniform(0.05, 8.8, n)], axis=1)
    near = lambda n: np.stack([rng.uniform(-2.5, 6.5, n), rng.uniform(-2.5, 6.5, n), rng.uniform(0.05, 6.0, n)], axis=1)
    o = np.where((np.arange(N_AIMED) % 2 == 0)[:, None], near(N_AIMED), inside(N_AIMED))
    aimed = np.concatenate([o, _unit(_targets(rng, flat, N_AIMED, counts) - o)], axis=1).astype("<f4")
    # from a void surface: the hit points of rays whose closest hit is void, new directions
    o2 = near(4 * N_SURFACE)
    first = np.concatenate([o2, _unit(_targets(rng, flat, 4 * N_SURFACE, counts) - o2)], axis=1).astype("<f4")
    t, mat = cast(first)
    t, mat = np.asarray(t, "<f4"), np.asarray(mat)
    hit = np.flatnonzero((t < raycast_cases.FLT_MAX) & (mat == 0))[:N_SURFACE]
    assert len(hit) == N_SURFACE
    if parents is not None:
        parents.append((first[hit], t[hit], mat[hit]))
    p = (first[hit, 0:3] + t[hit, None] * first[hit, 3:6]).astype("<f4")
    surface = np.concatenate([p, raycast_cases.unit_vectors(rng, N_SURFACE)], axis=1).astype("<f4")
    s = flat.spheres[counts["sphere"] - 2]   # the coincident void sphere (the enclosing one is the last void sphere)
    o3 = near(N_PAIR)
    pair = np.concatenate([o3, _unit(s["center"] + rng.normal(size=(N_PAIR, 3)) * 0.5 * s["r"] - o3)], axis=1).astype("<f4")
    hostile, _ = raycast_cases.cases(flat, lambda r: cast(r)[0], seed=26, scale=1)
    parts = [golden, aimed, surface, pair, hostile]
    rays = np.ascontiguousarray(np.concatenate(parts), "<f4")
    return rays, np.repeat(np.arange(len(parts)), [len(x) for x in parts]).astype(np.int32)


def exact_subset(kind):
    """the 2 000 rays that go through the exact walk alone (every ray re-cast: three orders of magnitude slower): the first 1 000
    golden, 500 aimed, 250 surface and 250 pair rays -> a mask over the set"""
    m = np.zeros(len(kind), bool)
    for k, n in (("golden", 1000), ("aimed", 500), ("surface", 250), ("pair", 250)):
        m[np.flatnonzero(kind == KINDS.index(k))[:n]] = True
    assert m.sum() == 2000
    return m


def rays_sha256(rays):
    return hashlib.sha256(np.ascontiguousarray(rays, "<f4").tobytes()).hexdigest()


def oracle_cast(osc):
    """-> cast(rays) -> (t, mat) of the oracle's closest hits"""
    def cast(r):
        t, _, mat = osc.raycast(r[:, 0:3], r[:, 3:6])
        return t, mat
    return cast


def rays_of(c):
    """ray_sets of a void_seen case, placed by the oracle's casts, once"""
    if "rays" not in _shared:
        parents = []
        _shared["rays"] = ray_sets(c.flat, oracle_cast(c.twin(None)), parents)
        _shared["parents"] = parents[0]
    return _shared["rays"]


def surface_parents(c):
    """(rays, t, mat) of the 500 rays whose hit points rays_of's surface rays start from"""
    rays_of(c)
    return _shared["parents"]


def occlusion_ladder(rays, t, mat, t_removed):
    """occluded_cases.laddered over the reference's t, and for every ray whose closest hit is void three more rungs: prev, at and
    next of the `removed` twin's distance for that ray (where a solid surface lies behind the void shape, or FLT_MAX), all
    expected 0 -> (rays, tmax, expected)"""
    import occluded_cases as oc
    rr, tm, want, _ = oc.laddered(rays, t, mat)
    void = np.flatnonzero((np.asarray(mat) == 0) & (np.asarray(t, "<f4") < oc.FLT_MAX))
    tr = np.asarray(t_removed, "<f4")[void]
    with np.errstate(over="ignore"):
        extra = np.stack([np.nextafter(tr, -oc.INF), tr, np.nextafter(tr, oc.INF)], axis=1).astype("<f4")
    return (np.concatenate([rr, np.repeat(np.ascontiguousarray(rays, "<f4")[void], 3, axis=0)]), np.concatenate([tm, extra.reshape(-1)]),
            np.concatenate([want, np.zeros(3 * len(void), bool)]))


# ---- points for ambient occlusion and irradiance -----------------------------------------------------------------------------------
N_POINTS = 256


def point_set(flat, cast_full):
    """256 points on the floor, the table and the walls of void_seen, lifted by 1e-3 n; the first half stands within 0.1 x the
    scene's diagonal (ao_cases' radius R, the largest finite rung below 0.4 x the diagonal) of a void shape: rays from around the
    void shapes down and outwards find the surface (cast_full(rays) -> t, n, mat), the second half's rays start anywhere.
    -> (points (256, 6) float32: p and n, seeds (256,) uint32)"""
    rng = np.random.default_rng(zlib.crc32(b"void points"))
    counts = void_counts("void_seen")
    out = []
    for near in (True, False):
        got = np.zeros((0, 6), "<f4")
        while len(got) < N_POINTS // 2:
            n = 512
            if near:
                o = _targets(rng, flat, n, counts) + rng.normal(size=(n, 3)) * 0.3
            else:
                o = np.stack([rng.uniform(-2.5, 14.5, n), rng.uniform(-2.5, 14.5, n), rng.uniform(0.05, 8.8, n)], axis=1)
            d = raycast_cases.unit_vectors(rng, n)
            if near:
                d[: n // 2, 2] = -np.abs(d[: n // 2, 2])
            r = np.concatenate([o, d], axis=1).astype("<f4")
            t, nrm, mat = cast_full(r)
            ok = (np.asarray(mat) != 0) & (np.asarray(t) < 1e3) & (np.asarray(t) > 1e-2)
            if near:
                ok &= np.asarray(t) < 2.0
            p = (r[ok, 0:3] + np.asarray(t, "<f4")[ok, None] * r[ok, 3:6]).astype("<f4")
            nn = np.asarray(nrm, "<f4")[ok]
            nn = np.where((np.sum(nn * r[ok, 3:6], axis=1) > 0)[:, None], -nn, nn).astype("<f4")   # towards the side the ray came from
            p = (p + np.float32(1e-3) * nn).astype("<f4")
            got = np.concatenate([got, np.concatenate([p, nn], axis=1)])
        out.append(got[: N_POINTS // 2])
    seeds = rng.integers(1, 1 << 32, size=N_POINTS, dtype=np.uint64).astype("<u4")
    return np.ascontiguousarray(np.concatenate(out), "<f4"), seeds


def void_distance(flat, p, name="void_seen"):
    """the distance from each point of p (n, 3) to the nearest void shape's bounding box"""
    counts = void_counts(name)
    boxes = [(s["center"] - s["r"], s["center"] + s["r"]) for s in flat.spheres[:counts["sphere"]]]
    boxes += [(b["min"], b["max"]) for b in flat.boxes[:counts["box"]]]
    boxes += [(np.minimum(c["base"], c["base"] + c["axis"]) - c["r"], np.maximum(c["base"], c["base"] + c["axis"]) + c["r"]) for c in flat.cylinders[:counts["cylinder"]]]
    boxes += [(m["aabb_min"], m["aabb_max"]) for m in flat.meshes[:counts["mesh"]]]
    p = np.asarray(p, np.float64)
    return np.min([np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0), axis=1) for lo, hi in boxes], axis=0)


def points_of(c):
    if "points" not in _shared:
        osc = c.twin(None)
        _shared["points"] = point_set(c.flat, lambda r: osc.raycast(r[:, 0:3], r[:, 3:6]))
    return _shared["points"]


# ---- what the CPU and the GPU tests share: computed once, left unchanged ---------------------------------------------------------------
VIEW_SEEDS = (SEED, 7, 99)
FEATURE_SPP = 5
QUERY_SPP = 4


def inside_camera(api, c):
    """the scene's own view moved to the centre of the scene's first void sphere (in the room: the one over the table): every sample's first hit is
    that sphere, from within"""
    s = c.flat.spheres[np.flatnonzero(c.flat.spheres["mat"] == 0)[0]]
    cam = c.cam.copy()
    cam[0] = s["center"]
    return cam


def view_cameras(api, c):
    """three views: the scene's own camera, light_groups_cases' second pose, and one standing inside the first void sphere"""
    return np.stack([c.cam, lg.batch_cameras(api, c)[1], inside_camera(api, c)])


# ---- the renders that follow mirrors and glass (follow_cases.py) ---------------------------------------------------------------------
# a view for them on void_seen: close to the room's glass sphere (0, 0, 0.9), which fills most of the frame, from the side
# opposite the void sphere over the table and the void box -- the refracted rays leave the glass towards them, so followed samples
# END on void shapes at b >= 1, which no view of view_cameras gives (the oracle's count there is 0).  p, x_axis, y_axis, z_axis
# as hostile_materials.UP_CAM is written
GLASS_CAM = np.array([[-0.634, -1.023, 1.074], [0.499, -0.309, 0.0], [-0.029, -0.048, -0.387], [-0.522, -0.841, 0.143]], "<f4")
FOLLOW_SETTINGS = hm.FOLLOW_SETTINGS
FOLLOW_SEEDS = VIEW_SEEDS + (0xDEADBEEF,)


def follow_world(api, c):
    """follow_cases' world of a case: the single frame from the scene's own camera on SEED; the batch is view_cameras (the third
    stands inside a void sphere: every sample ends on it at b == 0) and GLASS_CAM"""
    import follow_cases as fw
    return fw.case_world(c, np.concatenate([view_cameras(api, c), GLASS_CAM[None]]), FOLLOW_SEEDS)


def follow_conditions(api, c):
    """what the follow frames of a case must exercise, from the oracle's side (follow_cases.chain), printed and asserted.
    void_seen: the scene's own camera ends at least 50 samples on void shapes, GLASS_CAM at least 5 of them at b >= 1 -- a bounce
    ray that ends on a void shape records nothing and, as sample 0, leaves ids {0, that shape}.  void_hidden: no camera sample
    sees a void shape from the scene's own camera, and a few followed ones end on one (non-zero, below 1 % of the samples).
    all_void: every sample of every frame ends on a void shape at b == 0 or misses"""
    import follow_cases as fw
    w = follow_world(api, c)
    per = {s: fw.chains(w, FEATURE_SPP, *s) for s in FOLLOW_SETTINGS}
    for (rr, cap), ch in per.items():
        print("%s rr %g cap %d: per frame (own, own, pose 1, inside, GLASS_CAM) followed %s, void ends %s, of them at b >= 1 %s, sample 0's %s"
              % (c.name, rr, cap, [k.followed for k in ch], [k.void_ends for k in ch], [k.void_bounce_ends for k in ch], [int(k.void0.sum()) for k in ch]))
    own, glass = per[FOLLOW_SETTINGS[0]][0], per[FOLLOW_SETTINGS[0]][4]
    if c.name == "void_seen":
        assert own.void_ends >= 50 and int(own.void0.sum()) >= 50
        assert glass.void_bounce_ends >= 5 and int((glass.void0_bounces >= 1).sum()) >= 5
        assert glass.followed >= 0.10 * glass.samples
    elif c.name == "void_hidden":
        for s in FOLLOW_SETTINGS:
            k = per[s][0]
            assert 0 < k.void_ends == k.void_bounce_ends < 0.01 * k.samples
        assert own.followed >= 0.10 * own.samples
    else:
        assert all(k.followed == 0 and k.rays == k.samples and not k.hits.any() for ch in per.values() for k in ch)
    assert all((k.void0.all() and k.void_ends == k.samples) for k in (per[s][3] for s in FOLLOW_SETTINGS))   # inside the void sphere


def accumulate_primary_void_pixels(call, c, what, passes=(2, 3)):
    """accumulating passes over the whole frame of void_seen: a pixel whose every camera sample ends on a void shape has sum +0,
    m2 +0, out_rgb +0, count = the samples asked for, and its state advanced by the camera draws alone -- the state
    feature_cases.camera_rays leaves after that many samples.  `call`: accumulate_cases.host_call's or library_call's.  Such
    pixels exist (asserted: at least 50 of 384) -> their number"""
    import accumulate_cases as acs
    n = sum(passes)
    f = first_hits(c, (W, H), spp=n)
    void = ((f.mat == 0) & (f.t.view("<u4") != raycast_cases.FLT_MAX.view("<u4"))).all(axis=1)
    assert void.sum() >= 50, void.sum()
    got = acs.Planes()
    for k in passes:
        call(got, None, k)
    ys, xs = f.ys[void], f.xs[void]
    for a, name in ((got.sum, "sum_rgb"), (got.m2, "m2"), (got.rgb, "out_rgb")):
        assert not np.ascontiguousarray(a[0][ys, xs]).view("<u4").any(), "%s: %s of a pixel whose samples all end on a void shape" % (what, name)
    assert (got.count[0] == n).all() and (got.states[0][ys, xs] == f.after[void, n - 1]).all(), what
    assert (got.states[0][ys, xs] != f.after[void, passes[0] - 1]).all()
    return int(void.sum())


def advance(oracle, seed, steps):
    """the stream's state `steps` draws after seed (0 is taken as 1): radiance_cases.step, the oracle's xorshift restated there"""
    import radiance_cases as rc
    s = int(seed) or 1
    for _ in range(steps):
        s = rc.step(s)
    return s


def first_hits(c, size, seed=SEED, spp=1, cam=None):
    """feature_cases.frame of the scene's own camera: per pixel and sample the oracle's closest hit of the camera ray"""
    import feature_cases as fc
    w, h = size
    cam = c.camera(size) if cam is None else cam
    k = ("first", c.name, size, seed, spp, np.asarray(cam, "<f4").tobytes())
    if k not in _shared:
        _shared[k] = fc.frame(c.oracle, c.twin(None), c.flat, cam, w, h, seed, spp)
    return _shared[k]


def oracle_frame(c, size, policy, chunk, cam=None, seed=SEED, spp=SPP, rect=None):
    w, h = size
    cam = c.camera(size) if cam is None else np.asarray(cam, "<f4").reshape(4, 3)
    k = ("frame", c.name, size, policy, chunk, cam.tobytes(), seed, spp, rect)
    if k not in _shared:
        osc = c.twin(None)
        osc.set_camera(cam)
        _shared[k] = osc.render(w, h, spp, seed, policy, chunk=max(chunk, 1), rect=rect, rr=RR, threads=8)[0]
        osc.set_camera(c.cam)
    return _shared[k]


def pixel_planes(c, spp=SPP, seed=SEED):
    """-> (the oracle's PIXEL frame at 24 x 16, the final states), once"""
    k = ("pixel", c.name, spp, seed)
    if k not in _shared:
        osc = c.twin(None)
        osc.set_camera(c.cam)
        img, _, states = rg.oracle_pixel_planes(c.oracle, osc, W, H, spp, seed, RR)
        _shared[k] = (img, states)
    return _shared[k]


def chains_of(c):
    """render_adaptive_cases.chains of a case without goldens: 64 one-sample calls a pixel, once"""
    import render_adaptive_cases as rac
    k = ("chains", c.name)
    if k not in _shared:
        osc = c.twin(None)
        osc.set_camera(c.cam)
        _shared[k] = rac.chains(osc, W, H, SEED, RR)
    return _shared[k]


def void_only_text(name="void_seen"):
    """the void shapes of a scene alone, under one grey `brdf`: a cast in it tells whether a ray meets a void shape at all"""
    return HEAD + GREY + "\n" + VOID[name]


def ao_world(c, pts):
    """ao_cases.World of a case on pts = points_of(the void_seen case), which its twins share: the oracle's table of 8 samples a point and ao_cases.radius_array's radii (R = 0.1 x the
    scene's diagonal for most; +inf, NaN, 0, -1, FLT_MAX, 0.4 x the diagonal; the points' own hit distances and their neighbours)"""
    import ao_cases as ao
    import irradiance_cases as ic
    import radiance_cases as rc
    k = ("ao", c.name)
    if k not in _shared:
        points, seeds = pts
        w = ao.World()
        w.name, w.scene, w.flat, w.osc = c.name, c.scene, c.flat, c.twin(None)
        assert ic.in_domain(points).all()
        w.pts = ic.Points(points, seeds, np.ones(len(points), bool), np.zeros(len(points), bool))
        w.base = len(points)
        w.d, w.t, w.mat, w.after = ao.sample_table(c.oracle, w.osc, w.pts)
        w.lo, w.hi = rc.origin_box(c.flat)
        w.diag = float(np.linalg.norm(np.asarray(w.hi, np.float64) - np.asarray(w.lo, np.float64)))
        w.R = np.float32(0.1 * w.diag)
        w.radii, w.own = ao.radius_array("void_seen", w)
        _shared[k] = w
    return _shared[k]


def feature_expected(c, cam, seed, spp=FEATURE_SPP, size=None):
    """-> (feature_cases.expected's planes, the frame): a void first hit does not count in hits and adds nothing to albedo, normal
    or depth -- feature_cases.expected sums over mat != 0 -- and ids[..., 0] of sample 0 holds material 0.  ids[..., 1], the shape,
    is not the oracle's to say: assert_features takes it from the closest-hit query on sample 0's ray"""
    import feature_cases as fc
    w, h = size if size else (W, H)
    k = ("features", c.name, np.asarray(cam, "<f4").tobytes(), seed, spp, (w, h))
    if k not in _shared:
        f = fc.frame(c.oracle, c.twin(None), c.flat, cam, w, h, int(seed), spp)
        _shared[k] = (fc.expected(f, spp), f)
    return _shared[k]


def assert_features(got, want, f, prims, what):
    """every plane in every bit; ids[..., 1] is prims (h, w): the `prim` the closest-hit query gives for sample 0's ray of each
    pixel, NO_PRIM exactly where that sample misses -- so a void first hit has material 0 WITH a shape"""
    import feature_cases as fc
    for k in fc.PLANES:
        if k == "ids":
            continue
        same_words(got[k], want[k], "%s %s" % (what, k))
    ids = np.ascontiguousarray(got["ids"])
    assert (ids[..., 0] == want["ids"][..., 0]).all(), what + " ids: materials"
    p = np.asarray(prims, "<u4").reshape(f.h, f.w)
    bad = ids[..., 1] != p
    assert not bad.any(), "%s ids: %d shapes differ from the closest-hit query's; first %r" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    missed = (f.t[:, 0].view("<u4") == raycast_cases.FLT_MAX.view("<u4"))
    assert ((p[f.ys, f.xs] == NO_PRIM) == missed).all(), what + " ids: NO_PRIM exactly on a miss"
    return int(((f.mat[:, 0] == 0) & ~missed).sum())
