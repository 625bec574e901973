"""Light-group renders (ort_render_light_groups, ort_render_views_light_groups and their device forms) against the oracle as it
stands: the reference, the scenes and the guard values (test infrastructure, next to feature_cases.py).

THE DARK TWIN is the reference.  A second OracleScene from the same flattened scene with only the materials changed: every light
material outside the group keeps is_light and gets emit = +0.  Geometry, tree and light list are untouched, so every path takes the
same turns and draws the same numbers; the dark lights add +-0, or a NaN that the bounce guard drops, to a sum that started at +0,
which never changes it.  The twin's own PIXEL render at the same seed, spp and rr IS the group's frame, in every bit; the oracle's
render of the scene itself is out_rgb, and the states its one-pixel jobs return are final_states.  Nothing of the call is
restated."""
import os

import numpy as np

import host_sim_tool as hs
from conftest import DATA

F = np.float32
W, H = 24, 16          # 3 x 2 blocks of 8 x 8: partial in both directions
RECT = (3, 2, 21, 13)
SPPS = (16, 1)
SEED = 2024
RR = 0.8
NO_GROUP = 0xFF
MAX_GROUPS = 8
GUARD_F, GUARD_STATE = F(-7.0), 0xDDDDDDDD   # what host_sim's planes start with, and the GPU tests' too

# tests/test_gpu_light_pick.py's room and its two flavours of spheres on the table, as they stand there
ROOM = """screen 400 300
camera 5.553228 2.942755 2.900874 b 0.2 q 0.416981 0.279589 0.480987 0.718247
ambient 0.125000 0.125000 0.125000
brdf 0.600000 0.600000 0.600000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 -0.100000 18.000000 18.000000 0.100000
brdf 0.600000 0.600000 0.600000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 8.900000 18.000000 18.000000 0.100000
brdf 0.200000 0.900000 0.200000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 -0.100000 0.100000 18.000000 9.000000
brdf 0.900000 0.200000 0.900000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box 15.000000 -3.000000 -0.100000 0.100000 18.000000 9.000000
brdf 0.200000 0.200000 0.900000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 -3.000000 -0.100000 18.000000 0.100000 9.000000
brdf 0.900000 0.900000 0.200000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
box -3.000000 15.000000 -0.100000 18.000000 0.100000 9.000000
brdf 0.595000 0.560000 0.210000 0.000000 0.000000 0.000000 200 0.000000 0.000000 0.000000 1.0
box -1.200000 -1.200000 0.390000 2.400000 2.400000 0.020000
"""
SPHERES = {
    "all_lobes": """brdf 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 10 1.000000 1.000000 1.000000 1.4
sphere 0.000000 0.000000 0.900000 0.5
brdf 0.000000 0.000000 0.000000 0.200000 0.000000 0.000000 10 1.000000 0.000000 0.000000 1.2
sphere 1.000000 1.000000 0.800000 0.3
brdf 0.000000 0.000000 0.000000 1.000000 1.000000 1.000000 20 0.000000 0.000000 0.000000 1.0
sphere -1.000000 0.800000 0.700000 0.3
""",
    "diffuse": """brdf 0.800000 0.300000 0.300000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
sphere 0.000000 0.000000 0.900000 0.5
brdf 0.300000 0.800000 0.300000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
sphere 1.000000 1.000000 0.800000 0.3
brdf 0.300000 0.300000 0.800000 0.000000 0.000000 0.000000 10 0.000000 0.000000 0.000000 1.0
sphere -1.000000 0.800000 0.700000 0.3
""",
}
# three lights of three colours: a large sphere over the table, a small sphere to the side, a cylinder along the table's edge
THREE_LIGHTS = """light 3 3 2
sphere 0.000000 0.000000 2.800000 0.9
light 2 1 1
sphere 3.000000 1.000000 2.000000 0.4
light 1 1 3
cylinder -1.200000 -1.200000 2.600000 2.400000 0.000000 0.000000 0.3
"""
ROOMS = ("room_all_lobes", "room_diffuse")
DATA_SCENES = ("c2_analytic", "testscene", "c4_dwarf_room")
TABLE_SCENE = "table_ref_limits"   # tests/table_scenes.py's ref_limits: 100 materials, lights 7, 30, 53 and 76 -- two past the 48 of the LDS table
SCENES = ROOMS + DATA_SCENES + (TABLE_SCENE,)


class _Flat:
    pass


def dark_twin(oracle, flat, keep, csg=True):
    """the OracleScene of flat whose light materials outside keep have emit = +0 (is_light stays); keep = None: flat's own"""
    t = _Flat()
    t.__dict__.update(flat.__dict__)
    if keep is not None:
        mats = flat.materials.copy()
        for m in np.nonzero(flat.materials["is_light"])[0]:
            if int(m) not in keep:
                mats["emit"][m] = F(0.0)
        assert (mats["is_light"] == flat.materials["is_light"]).all()
        t.materials = mats
    return oracle.OracleScene(t, with_reference_csg=csg)


class SceneRef:
    """what tools/host_sim loads of a scene that is no Case: host_light_groups' and host_sample_map's c"""

    def __init__(self, scn, base):
        self.scn, self.base = scn, base

    def hs_args(self):
        return [self.scn, self.base]


class Case:
    """One scene: the product's committed scene, its flattened arrays, its light materials, and the oracle's frames of it and of
    its dark twins, each computed once and handed out read-only"""

    def __init__(self, api, oracle, name, directory):
        self.name, self.oracle = name, oracle
        self.csg = True
        if name in ROOMS:
            self.scn = os.path.join(str(directory), name + ".scn")
            with open(self.scn, "w") as f:
                f.write(ROOM + SPHERES[name[len("room_"):]] + THREE_LIGHTS)
            self.base = str(directory) + "/"
            self.scene = api.Scene.load_scn(self.scn)
        elif name == TABLE_SCENE:
            import table_scenes
            self.scene, _, self.csg = table_scenes.build(api, "ref_limits", directory)
            self.scn, self.base = os.path.join(str(directory), "ref_limits.scn"), str(directory) + "/"
            assert os.path.exists(self.scn)
        else:
            self.scn, self.base = os.path.join(DATA, name + ".scn"), DATA + "/"
            self.scene = api.Scene.load_scn(self.scn)
        self.scene.commit()
        self.flat = self.scene.flatten(W, H)
        self.lights = [int(m) for m in np.nonzero(self.flat.materials["is_light"])[0]]
        self.cam = np.asarray(self.flat.camera, "<f4").reshape(4, 3)
        self._twins, self._frames, self._cams = {}, {}, {}

    def hs_args(self):
        return [self.scn, self.base]

    # ---- group tables ------------------------------------------------------------------------------------------------
    def table(self, groups, filler=0x5A):
        """{material: group} -> a byte per material: the lights named their group, other lights NO_GROUP, every material that
        is no light a filler the call must not read"""
        t = np.full(len(self.flat.materials), filler, np.uint8)
        t[self.lights] = NO_GROUP
        for m, g in groups.items():
            assert m in self.lights
            t[m] = g
        return t

    def per_light(self):
        """one group per light material, in material order"""
        return {m: g for g, m in enumerate(self.lights)}

    # ---- the oracle's frames -----------------------------------------------------------------------------------------
    def twin(self, keep):
        """the OracleScene whose light materials outside keep have emit = +0; keep = None: the scene itself"""
        key = None if keep is None else frozenset(keep)
        if key not in self._twins:
            self._twins[key] = dark_twin(self.oracle, self.flat, key, self.csg)
        return self._twins[key]

    def camera(self, size=None):
        """the scene's own camera for a frame of size (w, h): the module's 24 x 16 by default"""
        size = tuple(size) if size else (W, H)
        if size not in self._cams:
            self._cams[size] = self.cam if size == (W, H) else np.asarray(self.scene.flatten(*size).camera, "<f4").reshape(4, 3)
        return self._cams[size]

    def frame(self, keep, spp, seed=SEED, cam=None, rect=None, size=None):
        """the PIXEL render (h, w, 3) of twin(keep) from cam (the scene's own by default); pixels outside rect are +0.  size:
        (w, h), the module's 24 x 16 by default"""
        w, h = size if size else (W, H)
        cam = self.camera(size) if cam is None else np.asarray(cam, "<f4").reshape(4, 3)
        key = (None if keep is None else frozenset(keep), spp, seed, cam.tobytes(), rect, (w, h))
        if key not in self._frames:
            osc = self.twin(keep)
            osc.set_camera(cam)
            img, _ = osc.render(w, h, spp, seed, "pixel", rect=rect, rr=RR, threads=8)
            img.setflags(write=False)
            self._frames[key] = img
        return self._frames[key]

    def states(self, spp, seed=SEED, cam=None, rect=None, size=None):
        """the final states (h, w) of the scene's own one-pixel jobs, which are its PIXEL render's pixels; outside rect 0"""
        w, h = size if size else (W, H)
        cam = self.camera(size) if cam is None else np.asarray(cam, "<f4").reshape(4, 3)
        key = ("states", spp, seed, cam.tobytes(), rect, (w, h))
        if key not in self._frames:
            img = self.frame(None, spp, seed, cam, rect, size)
            osc = self.twin(None)
            osc.set_camera(cam)
            x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
            st = np.zeros((h, w), "<u4")
            one = np.zeros((h, w, 3), "<f4")
            for y in range(y0, y1):
                for x in range(x0, x1):
                    _, st[y, x] = osc.tiled_raytrace(one, x, y, x + 1, y + 1, self.oracle.job_seed(seed, y * w + x), spp, RR)
            assert (one.view("<u4") == img.view("<u4")).all()   # the PIXEL render is these jobs
            st.setflags(write=False)
            self._frames[key] = st
        return self._frames[key]

    def expected(self, groups, G, spp, seed=SEED, cam=None, rect=None, size=None):
        """{material: group}, G -> the (G, h, w, 3) frames the call must give inside rect: frame g is the twin's that keeps group g"""
        return np.stack([self.frame([m for m, k in groups.items() if k == g], spp, seed, cam, rect, size) for g in range(G)])


_cases = {}


def case(api, oracle, name, tmp_path_factory):
    if name not in _cases:
        _cases[name] = Case(api, oracle, name, tmp_path_factory.mktemp("light_groups_" + name))
    return _cases[name]


BATCH_SEEDS = (SEED, 7, 99)


def batch_cameras(api, c, size=None):
    """three views for a batch of the rooms: the scene's own camera, one a step nearer the table and turned a little, and the
    scene's own again (on another seed: BATCH_SEEDS); for frames of size (w, h), the module's 24 x 16 by default"""
    w, h = size if size else (W, H)
    own = c.camera(size)
    q = np.array([0.416981, 0.279589, 0.480987, 0.718247]) + np.array([0.02, -0.015, 0.01, 0.0])
    other = api.camera_from_pose(own[0] * F(0.9), q / np.linalg.norm(q), 0.2, w, h)
    return np.stack([own, other, own])


# ---- outside the rect ------------------------------------------------------------------------------------------------------
def inside(rect, size=None):
    w, h = size if size else (W, H)
    m = np.zeros((h, w), bool)
    x0, y0, x1, y1 = rect if rect else (0, 0, w, h)
    m[y0:y1, x0:x1] = True
    return m


def assert_plane(got, want, rect, guard, what):
    """got (..., H, W[, 3]) equals want bit for bit inside rect and still holds guard outside it"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    m = inside(rect)
    g, w = got.view("<u4"), want.view("<u4")
    if got.ndim >= 3 and got.shape[-1] == 3 and got.shape[-3:-1] == (H, W):
        gi, wi, go = g[..., m, :], w[..., m, :], g[..., ~m, :]
    else:
        gi, wi, go = g[..., m], w[..., m], g[..., ~m]
    bad = gi != wi
    assert not bad.any(), "%s: %d of %d words inside the rect differ; first %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
    gw = np.array(guard, got.dtype).reshape(1).view("<u4")[0]
    assert (go == gw).all(), "%s: %d words outside the rect were written" % (what, int((go != gw).sum()))


# ---- tools/host_sim --light-groups -----------------------------------------------------------------------------------------
def host_light_groups(tool, d, c, table, G, spp, seed=SEED, rect=None, cams=None, seeds=None, want_rgb=True, want_states=True, **kw):
    """-> (frames (V, G, H, W, 3), rgb (V, H, W, 3) or None, states (V, H, W) or None); cams None: the single-frame form (V = 1)"""
    d = str(d)
    np.ascontiguousarray(table, np.uint8).tofile(os.path.join(d, "groups.u8"))
    if cams is not None:
        np.ascontiguousarray(cams, "<f4").tofile(os.path.join(d, "cams.f32"))
        np.ascontiguousarray(seeds, "<u4").tofile(os.path.join(d, "vseeds.u32"))
    V = 1 if cams is None else len(cams)
    x0, y0, x1, y1 = rect if rect else (0, 0, W, H)
    outs = [os.path.join(d, n) for n in ("lg.f32", "rgb.f32", "states.u32")]
    for o in outs:
        if os.path.exists(o):
            os.remove(o)
    args = ["--light-groups"] + c.hs_args() + [os.path.join(d, "cams.f32") if cams is not None else "-",
                                                os.path.join(d, "vseeds.u32") if cams is not None else seed,
                                                W, H, x0, y0, x1, y1, spp, repr(float(RR)), os.path.join(d, "groups.u8"), G,
                                                outs[0], outs[1] if want_rgb else "-", outs[2] if want_states else "-"]
    hs.run(tool, args, **kw)
    return (np.fromfile(outs[0], "<f4").reshape(V, G, H, W, 3),
            np.fromfile(outs[1], "<f4").reshape(V, H, W, 3) if want_rgb else None,
            np.fromfile(outs[2], "<u4").reshape(V, H, W) if want_states else None)
