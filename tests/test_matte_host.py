"""ID-matte renders (ort_render_matte, ort_render_views_matte and their device forms) and ort_matte_mask, host side: the input set
shown to earn its keep from the reference alone, the C ABI surface and its errors in the order include/ort.h gives them, the launch
plan, the lane code run on host threads (tools/host_sim --matte), plain and under ASan + UBSan, against the reference of
tests/matte_cases.py word for word, the identities of include/ort.h, and the mask's pixel function (tools/mattemask_sim), plain and
sanitized, against numpy on hostile slots."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import feature_cases as fc
import host_sim_tool as hs
import matte_cases as mc
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_matte", "ort_render_matte_device", "ort_render_views_matte", "ort_render_views_matte_device", "ort_matte_mask",
         "ort_matte_mask_device"}
MODES = ("material", "object", "prim")


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    return lambda name: mc.world(api, oracle, load_scene, tmp_path_factory, name)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


def _built(target):
    """tools/<target> (mattemask_sim or its _san twin), made when missing or older than its sources"""
    tool = os.path.join(hs.TOOLS, target)
    src = [os.path.join(hs.TOOLS, "mattemask_sim.cpp"), os.path.join(hs.TOOLS, "Makefile"), os.path.join(hs.CSRC, "ort_mattemask.h")]
    if not os.path.exists(tool) or any(os.path.getmtime(s) > os.path.getmtime(tool) for s in src):
        r = subprocess.run(["make", "-s", "-B", "-C", hs.TOOLS, target], capture_output=True, text=True)
        assert r.returncode == 0, "make %s failed (exit %d)\n%s" % (target, r.returncode, (r.stdout + r.stderr)[-4000:])
    return tool


# ---- 1. the inputs earn their keep: from the reference alone ---------------------------------------------------------------------------
def test_inputs_earn_their_keep(world):
    """over the four frames of the open scene, BY_MATERIAL, spp 5, full frame: pixels that lose samples to `other` at K 1 and 2,
    pixels whose kept ids are not the K largest, pixels whose final order is not the order of first appearance, pixels with a tie"""
    w = world("open")
    sets = mc.sample_ids(w, None, "material")
    count = {"other1": 0, "other2": 0, "not_largest2": 0, "reordered8": 0, "tie8": 0}
    for ids, rec in sets:
        hist = mc.histogram(ids[:, :5], rec[:, :5])
        _, _, o1, _, _ = mc.slots(ids[:, :5], rec[:, :5], 1)
        i2, c2, o2, _, _ = mc.slots(ids[:, :5], rec[:, :5], 2)
        i8, c8, _, _, f8 = mc.slots(ids[:, :5], rec[:, :5], 8)
        count["other1"] += int((o1 > 0).sum())
        count["other2"] += int((o2 > 0).sum())
        for p, h in enumerate(hist):
            kept = {int(x) for x in i2[p] if x != mc.EMPTY}
            left = [c for x, c in h.items() if x not in kept]
            # no choice of ties makes the kept ids the two largest: an id left out was seen more often than one that was kept
            count["not_largest2"] += bool(left) and max(left) > min(h[x] for x in kept)
            count["reordered8"] += bool((i8[p] != f8[p]).any())
            used = c8[p][i8[p] != mc.EMPTY]
            count["tie8"] += len(set(used.tolist())) < len(used)
    print(count)
    assert count["other1"] >= 100 and count["other2"] >= 5 and count["not_largest2"] >= 3 and count["reordered8"] >= 50 and count["tie8"] >= 5, count


def test_object_and_prim_inputs_earn_their_keep(host_sim, world, tmp_path):
    """over the three scenes BY_OBJECT ids name meshes, boxes, cylinders and spheres; BY_PRIM in the bunny room at spp 5 has pixels
    with more than two distinct triangles.  Not from the scene's own camera, nor from feature_cases' three views: the bunny stands
    in their focal plane (two triangles a pixel at the most, printed).  matte_cases.world adds a view for this: the last frame"""
    kinds = set()
    for name in mc.SCENES:
        w = world(name)
        for ids, rec in mc.sample_ids(w, mc.host_prims(host_sim, tmp_path, w), "object"):
            kinds |= set((ids[rec] >> 28).tolist())
            table = mc.object_table(w.flat)
            assert set(ids[rec].tolist()) <= set(table)
    assert kinds == {mc.HIT_MESH, 2, 3, 4}, kinds
    w = world("c3_bunny_room")
    most = []
    for ids, rec in mc.sample_ids(w, mc.host_prims(host_sim, tmp_path, w), "prim"):
        most.append(max(len({int(x) for x, r in zip(row, keep) if r and (x >> 28) == 0}) for row, keep in zip(ids[:, :5], rec[:, :5])))
    print("most distinct triangles in a pixel, per frame:", most)
    assert len(most) == 5 and most[-1] > 2


def test_object_ids_lists_every_object(api, world):
    for name in mc.SCENES:
        w = world(name)
        ids, mats = w.scene.object_ids()
        assert dict(zip(ids.tolist(), mats.tolist())) == mc.object_table(w.flat) and len(set(ids.tolist())) == len(ids)


# ---- 2. the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names and NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert ctypes.sizeof(api.MattePlanes) == 40 and ctypes.sizeof(api.Matte) == 8
    assert (api.MATTE_EMPTY, api.HIT_MESH, api.MAX_MATTE_SLOTS, api.MAX_MATTE_SELECT) == (0xFFFFFFFF, 1, 8, 256)
    section = hdr[hdr.index("ID-matte renders"):hdr.index("int ort_render_matte(")]
    for word in ("While other == 0 the slots are the pixel's exact histogram.", "Where other > 0 the kept ids are the first K to",
                 "appear, not the K largest.", "A lane cannot know the largest without holding them all.", "The caller sees which pixels are affected",
                 "and renders again with a larger K.", "#define ORT_MATTE_EMPTY 0xffffffffu", "#define ORT_HIT_MESH 1", "#define ORT_MAX_MATTE_SLOTS 8u",
                 "sum(counts) + other == hits", "count descending, with ties broken by ascending id", "m NULL; by above 2; slots 0 or above"):
        assert word in section, word


def _caller(api, views_form, device_form):
    """call(handle, params, m, planes[, views, count]) through one of the four entry points"""
    L = api.lib()
    cam = api.View()

    def call(handle, p, m, planes, views="own", count=1, stats=None):
        fp = ctypes.byref(planes) if planes is not None else None
        pm = ctypes.byref(m) if m is not None else None
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_matte_device(handle, pp, v, count, pm, fp, None, stats)
            return L.ort_render_views_matte(handle, pp, v, count, pm, fp, stats)
        if device_form:
            return L.ort_render_matte_device(handle, pp, pm, fp, None, stats)
        return L.ort_render_matte(handle, pp, pm, fp, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """ort_render_views_features' order -- INVALID (the null planes struct, null views, the view cap, null scene or params, the params,
    spp above 1 << 24, a misaligned plane) --, then this call's own: m NULL, by above 2, slots 0 or above 8, ids or counts NULL; then
    UNSUPPORTED (policy, shard, packed, a camera outside the box), then the scene's state: STATE before NO_DEVICE.  On a
    committed-but-not-uploaded scene and on an uncommitted one, so every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(8 * 8 * 4 * 8) for _ in range(5)]
    ptr = dict(zip(("ids", "counts", "other", "hits", "final_states"), (k[1] for k in keep)))
    full, good = api.MattePlanes(**ptr), api.Matte(1, 8)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    bad_p, bad_m = _params(api, width=0), api.Matte(3, 0)
    # nulls first: before bad params and a bad m
    assert call(s.handle, bad_p, bad_m, None) == api.ERR_INVALID
    assert b"planes" in L.ort_last_error()
    if views_form:
        assert call(s.handle, bad_p, bad_m, full, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, bad_p, bad_m, full, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), good, full) == api.ERR_INVALID
    assert call(s.handle, None, good, full) == api.ERR_INVALID
    # the params, as the render call judges them, before the planes' alignment and before m
    odd = api.MattePlanes(**{**ptr, "hits": ptr["hits"] + 2})
    for p, word in ((bad_p, b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, spp=0), b"spp"), (_params(api, policy=7), b"policy"), (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, None, odd) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    # spp above 1 << 24 and the alignment, before m and before what the call does not do
    chunky = _params(api, policy="chunk", spp=(1 << 24) + 1, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, None, odd) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    chunky.spp = 1 << 24
    for name in ptr:
        assert call(s.handle, chunky, None, api.MattePlanes(**{**ptr, name: ptr[name] + (1 if name == "ids" else 2)})) == api.ERR_INVALID, name
        assert b"4-byte aligned" in L.ort_last_error()
    # then m, by, slots, the required planes: in that order, each before the next
    no_ids = api.MattePlanes(**{**ptr, "ids": None})
    assert call(s.handle, chunky, None, no_ids) == api.ERR_INVALID
    assert b"null m" in L.ort_last_error()
    for by in (3, 0xFFFFFFFF):
        assert call(s.handle, chunky, api.Matte(by, 0), no_ids) == api.ERR_INVALID
        assert b"by must be" in L.ort_last_error()
    for slots in (0, 9, 0xFFFFFFFF):
        assert call(s.handle, chunky, api.Matte(2, slots), no_ids) == api.ERR_INVALID
        assert b"slots must be" in L.ort_last_error()
    for name in ("ids", "counts"):
        assert call(s.handle, chunky, good, api.MattePlanes(**{**ptr, name: None})) == api.ERR_INVALID
        assert b"ids or counts" in L.ort_last_error()
    # what the call does not do: any policy but PIXEL, shards, a packed plane
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), good, full) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), good, full) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), good, full) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), good, full, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it: the two required planes alone, every mode, the limits
    for by in (0, 1, 2):
        for slots in (1, 8):
            assert call(s.handle, _params(api, spp=1, chunk=5, rr=-3.0), api.Matte(by, slots), api.MattePlanes(ids=ptr["ids"], counts=ptr["counts"])) == state
    assert call(s.handle, _params(api, spp=1 << 24, rr=float("nan")), good, full) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), api.Matte(7, 0), api.MattePlanes(), count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


@pytest.mark.parametrize("device_form", [False, True])
def test_mask_errors_come_in_order(api, device_form):
    """ort_matte_mask without a device: frame_count 0 is OK whatever else; then nulls, alignment, slots, the frame's size, spp, the
    selection's length, EMPTY in it, each before the next; good arguments reach the device: NO_DEVICE on a machine without one"""
    L = api.lib()
    keep = [_aligned(4 * 4 * 8 * 4) for _ in range(3)]
    ids, counts, out = (k[1] for k in keep)
    sel = np.array([3, 3, 5], "<u4")
    bad_sel = np.array([3, mc.EMPTY], "<u4")

    def call(ids=ids, counts=counts, slots=8, spp=4, select=sel.ctypes.data, n=3, w=4, h=4, frames=1, out=out, device=0):
        if device_form:
            return L.ort_matte_mask_device(device, ids, counts, slots, spp, select, n, w, h, frames, out, None)
        return L.ort_matte_mask(device, ids, counts, slots, spp, select, n, w, h, frames, out)
    assert call(ids=None, counts=None, slots=0, spp=0, select=None, n=0, w=0, out=None, frames=0, device=99) == api.OK
    for null in ("ids", "counts", "select", "out"):
        assert call(**{null: None}, slots=0, w=0) == api.ERR_INVALID
        assert b"null" in L.ort_last_error()
    for odd in ("ids", "counts", "out"):
        assert call(**{odd: keep[0][1] + 2}, slots=0, w=0) == api.ERR_INVALID
        assert b"aligned" in L.ort_last_error()
    for slots in (0, 9):
        assert call(slots=slots, w=0, spp=0) == api.ERR_INVALID
        assert b"slots" in L.ort_last_error()
    for size in (dict(w=0), dict(h=-1), dict(w=1 << 15, h=1 << 14, frames=1)):
        assert call(spp=0, **size) == api.ERR_INVALID
        assert b"frame size" in L.ort_last_error()
    for spp in (0, (1 << 24) + 1):
        assert call(spp=spp, n=0) == api.ERR_INVALID
        assert b"spp" in L.ort_last_error()
    for n in (0, 257):
        assert call(n=n, select=bad_sel.ctypes.data) == api.ERR_INVALID
        assert b"select_count" in L.ort_last_error()
    assert call(select=bad_sel.ctypes.data, n=2, device=99) == api.ERR_INVALID
    assert b"ORT_MATTE_EMPTY" in L.ort_last_error()
    if api.device_count() < 1:
        assert call() == api.ERR_NO_DEVICE
    assert call(device=99) == api.ERR_NO_DEVICE


def test_python_shapes(api):
    s = _scene(api)
    with pytest.raises(api.OrtError) as e:
        s.render_matte(8, 6, 4, 3)
    assert e.value.code == api.ERR_NO_DEVICE
    for kw in (dict(by="colour"), dict(want=("hits", "hits")), dict(want=("ids",)), dict(want=("depth",))):
        with pytest.raises(ValueError):
            s.render_matte(8, 6, 4, 3, **kw)
    for slots in (0, 9):
        with pytest.raises(api.OrtError) as e:
            s.render_matte(8, 6, 4, 3, slots=slots)
        assert e.value.code == api.ERR_INVALID
    good = mc.guard_planes((6, 8), 2, ("ids", "counts", "hits"))
    for bad in ({"ids": good["ids"], "counts": good["counts"]}, {**good, "ids": good["ids"].astype("<i4")}, {**good, "counts": good["counts"][:, ::2]},
                {**good, "ids": np.zeros((6, 8, 8), "<u4")}, {**good, "other": np.zeros((6, 8), "<u4")}):
        with pytest.raises(ValueError):
            s.render_matte(8, 6, 4, 3, slots=2, want=("hits",), out=bad)
    cams = np.stack([s.camera(8, 6)] * 2)
    with pytest.raises(ValueError):
        s.render_views_matte(cams, [1], 8, 6, 4)
    with pytest.raises(api.OrtError) as e:
        s.render_views_matte(cams, [1, 2], 8, 6, 4)
    assert e.value.code == api.ERR_NO_DEVICE
    planes, st = s.render_views_matte(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, slots=3, want=("other", "hits", "states"))
    assert planes["ids"].shape == planes["counts"].shape == (0, 6, 8, 3) and planes["other"].shape == planes["states"].shape == (0, 6, 8)
    assert all(a.dtype == np.dtype("<u4") for a in planes.values()) and st["rays"] == 0
    p = s.params(8, 6, 4, 1, "pixel")
    with pytest.raises(ValueError):
        s.render_matte_device(p, colour=64)
    for call in (lambda: s.render_matte_device(p, ids=64, counts=128), lambda: s.render_views_matte_device(p, cams, [1, 2], ids=64, counts=128, hits=256)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        api.matte_mask(np.zeros((4, 4, 2), "<u4"), np.zeros((4, 4, 3), "<u4"), 4, [1])
    with pytest.raises(api.OrtError) as e:
        api.matte_mask(np.zeros((4, 4, 2), "<u4"), np.zeros((4, 4, 2), "<u4"), 4, [])
    assert e.value.code == api.ERR_INVALID


# ---- 3. the launch plan ---------------------------------------------------------------------------------------------------------------------
def test_launch_plan_matte_is_features():
    """plan_matte is plan_features and matte_view is features_view: query=matte prints query=features' lines, apart from the name"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")
    e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
    for env, args in (({}, ["width=1920", "height=1080", "x1=1920", "y1=1080", "materials=8", "fill=1", "spp=16"]),
                      ({}, ["width=24", "height=16", "x0=3", "y0=2", "x1=21", "y1=13", "views=3", "counters=1", "fill=1", "spp=5"]),
                      ({"ORT_JOB_BATCH": "7", "ORT_BATCH_TAIL": "1"}, ["width=1024", "height=768", "x1=1024", "y1=768", "materials=60", "fill=1"])):
        out = [subprocess.check_output([tool, "query=" + q] + args, env={**e, **env}).decode().splitlines() for q in ("matte", "features")]
        assert len(out[0]) > 10 and '"query": "matte"' in out[0][0]
        assert [l.replace('"query": "matte"', '"query": "features"') for l in out[0]] == out[1]
    assert subprocess.run([tool, "query=matte", "width=8", "height=8", "x1=9", "y1=8"], capture_output=True).returncode == 2


# ---- 4. the lane code on host threads -------------------------------------------------------------------------------------------------
def _single(got):
    return {k: v[0] for k, v in got.items()}


@pytest.mark.parametrize("by", MODES)
@pytest.mark.parametrize("name", mc.SCENES)
def test_host_sim_is_the_reference(host_sim, world, tmp_path, name, by):
    """all five planes, every word: the single frame and the batch of three views, K in {1, 2, 8}, spp 1 and 5, the tables in LDS form
    and from their arrays, one thread and eight"""
    w = world(name)
    prims = mc.host_prims(host_sim, tmp_path, w)
    for k in mc.KS:
        for spp in mc.SPPS:
            env, threads = ({"SIM_TABS": "1"}, 1) if (k == 2) == (spp == 5) else ({}, 8)
            one, batch = mc.expected_set(w, prims, by, spp, k)
            got, r = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, spp, by, k, seed=mc.SEED, base=w.base, env=env, threads=threads)
            mc.same_bits(_single(got), one, "%s %s K %d spp %d single" % (name, by, k, spp))
            assert hs.counters(r)["rays"] == mc.W * mc.H * spp and hs.counters(r)["paths"] == 0
            gotb, _ = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, spp, by, k, cams=w.mcams, seeds=w.mseeds, base=w.base, env=env, threads=8)
            mc.same_bits(gotb, batch, "%s %s K %d spp %d batch" % (name, by, k, spp))
            mc.check_order(gotb["ids"], gotb["counts"], gotb["other"], gotb["hits"])


@pytest.mark.parametrize("by", MODES)
def test_host_sim_rect_guards_planes_alone_and_forced_walk(host_sim, world, tmp_path, by):
    """the rect (3, 2, 21, 13) cuts blocks on all four sides: its pixels are the reference's in every plane, those outside keep their
    guard words (identity 6); other, hits and the states asked for or not change no word elsewhere (identity 5); the forced exact
    walk changes no word"""
    w = world("open")
    prims = mc.host_prims(host_sim, tmp_path, w)
    inside = np.zeros((mc.H, mc.W), bool)
    inside[mc.RECT[1]:mc.RECT[3], mc.RECT[0]:mc.RECT[2]] = True
    for k in (2, 8):
        _, batch = mc.expected_set(w, prims, by, 5, k, mc.RECT, mc.GUARDS)
        got, _ = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, mc.RECT, 5, by, k, cams=w.mcams, seeds=w.mseeds, base=w.base, threads=8)
        mc.same_bits(got, batch, "rect, batch, K %d" % k)
        for p in mc.PLANES:
            assert (got[p][:, ~inside] == mc.GUARDS[p]).all(), p
        for want in (("ids", "counts"), ("ids", "counts", "other"), ("ids", "counts", "hits"), ("ids", "counts", "states")):
            alone, _ = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, mc.RECT, 5, by, k, cams=w.mcams, seeds=w.mseeds, want=want, base=w.base, threads=8)
            assert set(alone) == set(want)
            mc.same_bits(alone, got, "planes %r alone" % (want,))
        forced, r = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, mc.RECT, 5, by, k, cams=w.mcams, seeds=w.mseeds, base=w.base, threads=8,
                                env={"SIM_FORCE_FALLBACK": "0xf"})
        assert hs.counters(r)["fallback"] > 0
        mc.same_bits(forced, got, "forced walk")


@pytest.mark.parametrize("name", mc.SCENES)
def test_identities_on_host_sim(host_sim, world, tmp_path, name):
    """(1) sum(counts) + other == hits, and hits and the states are --features' planes; (2) at spp 1 slot 0 is --features' ids.mat
    (BY_MATERIAL) or ids.prim (BY_PRIM) where it hit and EMPTY where it did not; (3) where other == 0 under both modes, the BY_OBJECT
    counts folded through object -> material are the BY_MATERIAL counts"""
    w = world(name)
    feat5, _ = fc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, 5, cams=w.mcams, seeds=w.mseeds, want=("hits", "states"), base=w.base, threads=8)
    feat1, _ = fc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, 1, cams=w.mcams, seeds=w.mseeds, want=("hits", "ids"), base=w.base, threads=8)
    got = {}
    for by in MODES:
        for k in (2, 8):
            g, _ = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, 5, by, k, cams=w.mcams, seeds=w.mseeds, base=w.base, threads=8)
            mc.check_order(g["ids"], g["counts"], g["other"], g["hits"])
            assert (g["hits"] == feat5["hits"]).all() and (g["states"] == feat5["states"]).all()
            got[by, k] = g
        one, _ = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, 1, by, 2, cams=w.mcams, seeds=w.mseeds, base=w.base, threads=8)
        hit = feat1["hits"] == 1
        assert hit.any() and ((one["ids"][..., 0] == mc.EMPTY) == ~hit).all() and (one["ids"][..., 1] == mc.EMPTY).all()
        if by == "material":
            assert (one["ids"][..., 0][hit] == feat1["ids"][..., 0][hit]).all()
        elif by == "prim":
            assert (one["ids"][..., 0][hit] == feat1["ids"][..., 1][hit]).all()
        else:
            assert (one["ids"][..., 0][hit] == mc.object_of_prim(w.flat, feat1["ids"][..., 1][hit])).all()
    table = mc.object_table(w.flat)
    folded = 0
    for k in (2, 8):
        o, m = got["object", k], got["material", k]
        exact = (o["other"] == 0) & (m["other"] == 0)
        for oi, oc, mi, mcnt in zip(o["ids"][exact], o["counts"][exact], m["ids"][exact], m["counts"][exact]):
            h = {}
            for x, c in zip(oi, oc):
                if x != mc.EMPTY:
                    h[table[int(x)]] = h.get(table[int(x)], 0) + int(c)
            assert h == {int(x): int(c) for x, c in zip(mi, mcnt) if x != mc.EMPTY}
            folded += len(h) < int((oi != mc.EMPTY).sum())
    assert folded > 0 or name != "open"   # on the open scene some pixel sees two objects of one material


# ---- 5. under the sanitizers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.SCENES)
def test_host_sim_under_sanitizers(world, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): every mode, K 1, 2 and 8, the batch at spp 5, a rect
    that cuts blocks, planes left out: ends clean, with the reference's planes"""
    san = hs.built("host_sim_san")
    w = world(name)
    prims = mc.host_prims(hs.built("host_sim"), tmp_path, w)
    for by, k, env in (("material", 1, {}), ("object", 2, {"SIM_TABS": "1"}), ("prim", 8, {})):
        one, batch = mc.expected_set(w, prims, by, 5, k)
        got, _ = mc.host_sim(san, tmp_path, w.scn, mc.W, mc.H, None, 5, by, k, seed=mc.SEED, base=w.base, env=env, threads=2)
        mc.same_bits(_single(got), one, "sanitized %s %s single" % (name, by))
        got, _ = mc.host_sim(san, tmp_path, w.scn, mc.W, mc.H, None, 5, by, k, cams=w.mcams, seeds=w.mseeds, want=("ids", "counts", "other"), base=w.base, threads=2)
        mc.same_bits(got, batch, "sanitized %s %s batch" % (name, by))
        _, rect = mc.expected_set(w, prims, by, 5, k, mc.RECT, mc.GUARDS)
        got, _ = mc.host_sim(san, tmp_path, w.scn, mc.W, mc.H, mc.RECT, 5, by, k, cams=w.mcams, seeds=w.mseeds, base=w.base, threads=2)
        mc.same_bits(got, rect, "sanitized %s %s rect" % (name, by))


# ---- 6. the mask's pixel function -----------------------------------------------------------------------------------------------------
def _mask_sim(tool, d, ids, counts, spp, select, check=True):
    d = str(d)
    ids.tofile(os.path.join(d, "k_ids.u32"))
    counts.tofile(os.path.join(d, "k_counts.u32"))
    np.asarray(select, "<u4").tofile(os.path.join(d, "k_select.u32"))
    f, h, w, k = ids.shape
    r = subprocess.run([tool] + [str(a) for a in (w, h, f, k, spp)] + [os.path.join(d, n) for n in ("k_ids.u32", "k_counts.u32", "k_select.u32", "k_mask.f32")],
                       capture_output=True, text=True, timeout=120)
    if check:
        assert r.returncode == 0, r.stderr[-1500:]
        return np.fromfile(os.path.join(d, "k_mask.f32"), "<f4").reshape(f, h, w)
    return r


@pytest.mark.parametrize("target", ["mattemask_sim", "mattemask_sim_san"])
def test_mask_sim_is_numpy(tmp_path, target):
    """the mask's pixel function on the host, plain and under ASan + UBSan, against numpy's one line, on hostile slots (all EMPTY,
    ids twice in a pixel, counts that sum above spp and wrap, 0xFFFFFFFF counts), selections with duplicates, of one id, of 256,
    of ids no slot holds; the arguments judged as the call judges them"""
    tool = _built(target)
    rng = np.random.default_rng(11)
    for k, shape in ((1, (1, 5, 7)), (2, (2, 9, 11)), (8, (3, 16, 24))):
        ids, counts = mc.hostile_slots(rng, shape, k)
        assert (ids == mc.EMPTY).all(axis=-1).any() and (counts == 0xFFFFFFFF).any()
        for spp, select in ((1, [3]), (5, [3, 3, 7, 3, 0]), (1 << 24, list(range(256))), (7, [500, 600]), (16, [11, 0, 5, 0xFFFFFFFE])):
            got = _mask_sim(tool, tmp_path, ids, counts, spp, select)
            want = mc.mask(ids, counts, spp, select)
            assert (got.view("<u4") == want.view("<u4")).all(), (k, spp, select)
    ids, counts = mc.hostile_slots(rng, (1, 4, 4), 2)
    for spp, select in ((0, [1]), ((1 << 24) + 1, [1]), (4, []), (4, list(range(257))), (4, [1, mc.EMPTY])):
        assert _mask_sim(tool, tmp_path, ids, counts, spp, select, check=False).returncode == 2


def test_mask_of_a_render_is_coverage(host_sim, world, tmp_path):
    """on the slots of a render (the open scene BY_MATERIAL, K 8, spp 5, exact everywhere): the mask of every material seen is hits / spp,
    and the masks of the materials one by one are each material's share"""
    w = world("open")
    got, _ = mc.host_sim(host_sim, tmp_path, w.scn, mc.W, mc.H, None, 5, "material", 8, cams=w.mcams, seeds=w.mseeds, base=w.base, threads=8)
    assert (got["other"] == 0).all()
    tool = _built("mattemask_sim")
    seen = sorted(set(got["ids"].reshape(-1).tolist()) - {mc.EMPTY})
    every = _mask_sim(tool, tmp_path, got["ids"], got["counts"], 5, seen + seen[:1])
    assert (every.view("<u4") == (got["hits"].astype("<f4") / np.float32(5)).astype("<f4").view("<u4")).all()
    total = np.zeros(every.shape, np.int64)
    for m in seen:
        one = _mask_sim(tool, tmp_path, got["ids"], got["counts"], 5, [m])
        total += np.rint(one * 5).astype(np.int64)
    assert (total == got["hits"]).all() and len(seen) >= 4
