"""Light-group renders (ort_render_light_groups, ort_render_views_light_groups and their device forms), host side: the helper that
turns the oracle into their reference (tests/light_groups_cases.py: the dark twin) pinned against the oracle's own PIXEL render,
the scenes shown not to be vacuous, the C ABI surface and its errors in the order include/ort.h gives them, the launch plan, and
the lane code with the group sums run on host threads (tools/host_sim --light-groups), plain and under ASan + UBSan, against the
twins bit for bit."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import host_sim_tool as hs
import light_groups_cases as lg
from conftest import DATA, ROOT
from host_cases import aligned as _aligned, params as _params, scene as _scene

NAMES = {"ort_render_light_groups", "ort_render_light_groups_device", "ort_render_views_light_groups", "ort_render_views_light_groups_device"}


@pytest.fixture()
def case(api, oracle, tmp_path_factory):
    return lambda name: lg.case(api, oracle, name, tmp_path_factory)


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


def _bits(a):
    return np.ascontiguousarray(a).view("<u4")


# ---- 1. the helper against the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lg.SCENES)
def test_every_light_in_one_group_is_the_pixel_render(case, name):
    """the twin that keeps every light changes no material: its frame is the oracle's PIXEL render of the scene, at both sample
    counts, whole frame and rect"""
    c = case(name)
    assert len(c.lights) >= 2 and 0 not in c.lights
    for spp in lg.SPPS:
        for rect in (None, lg.RECT):
            assert (_bits(c.frame(c.lights, spp, rect=rect)) == _bits(c.frame(None, spp, rect=rect))).all()
            assert (_bits(c.frame([], spp, rect=rect)) == 0).all()   # no light kept: +0 everywhere


@pytest.mark.parametrize("name", lg.ROOMS + lg.DATA_SCENES)
def test_per_light_twins_differ(case, name):
    """at 16 spp every light's own frame differs from the full render and from every other light's"""
    c = case(name)
    frames = [c.frame([m], 16) for m in c.lights]
    full = c.frame(None, 16)
    for i, f in enumerate(frames):
        assert (_bits(f) != _bits(full)).any(), c.lights[i]
        for j in range(i):
            assert (_bits(f) != _bits(frames[j])).any(), (c.lights[i], c.lights[j])


def test_the_rooms_are_the_three_light_room(case):
    for name in lg.ROOMS:
        c = case(name)
        assert len(c.flat.materials) == 14 and c.lights == [11, 12, 13]
        assert c.flat.lights["type"].tolist() == [1, 1, 2]
    assert (case("room_diffuse").flat.materials["specular"][1:, :3] == 0).all() and (case("room_all_lobes").flat.materials["specular"][1:, :3] != 0).any()


# ---- 2. not vacuous, as conditions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,each,two", [("room_all_lobes", 0.15, 0.10), ("room_diffuse", 0.15, 0.10), ("c2_analytic", 0.04, 0.10),
                                           ("testscene", 0.04, 0.10), ("c4_dwarf_room", 0.04, 0.10)])
def test_frames_are_not_vacuous(case, name, each, two):
    """from the oracle alone at 24 x 16 x 16 spp, seed 2024, rr 0.8, the scene's own camera, one group per light material: every
    group's frame is non-zero on at least `each` of the pixels, and at least `two` of the pixels are non-zero in two or more"""
    assert (lg.W, lg.H, lg.SEED, lg.RR, lg.SPPS[0]) == (24, 16, 2024, 0.8, 16)
    c = case(name)
    lit = np.stack([(c.frame([m], 16) != 0).any(axis=2) for m in c.lights])
    shares = lit.reshape(len(c.lights), -1).mean(axis=1)
    several = (lit.sum(axis=0) >= 2).mean()
    print("%s: lit share per light %s, by two or more %.3f" % (name, " / ".join("%.3f" % s for s in shares), several))
    assert (shares >= each).all() and several >= two


def test_table_scene_reads_entries_past_the_lds_cap(case):
    """the table scene: more materials than the LDS table holds, two light materials at indices from the cap on, and their group's
    frame is not black: a table entry read at a wrapped or clamped index changes pixels"""
    import table_scenes
    c = case(lg.TABLE_SCENE)
    cap = table_scenes.caps()["materials"]
    past = [m for m in c.lights if m >= cap]
    assert len(c.flat.materials) > cap and len(past) >= 2 and len(past) < len(c.lights)
    for rect in (None, lg.RECT):
        assert (c.frame(past, 16, rect=rect) != 0).any()
    for m in past:   # a wrapped index names no light: the filler, which is no group
        assert m % cap not in c.lights and m - cap not in c.lights


@pytest.mark.parametrize("name", lg.ROOMS)
def test_the_groups_do_not_add_up_bit_for_bit(case, name):
    """identity 5's reason to exist: the per-light frames, added in float32 in either order, are not the full frame on every pixel
    -- though they are to rounding"""
    c = case(name)
    f = [c.frame([m], 16) for m in c.lights]
    full = c.frame(None, 16)
    s = ((f[0] + f[1]).astype("<f4") + f[2]).astype("<f4")
    assert (_bits(s) != _bits(full)).any(axis=2).any()
    assert np.abs(s - full).max() <= 1e-5 * max(1.0, float(np.abs(full).max()))


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert (api.MAX_LIGHT_GROUPS, api.NO_LIGHT_GROUP) == (8, 0xFF)
    assert "#define ORT_MAX_LIGHT_GROUPS 8u" in hdr and "#define ORT_NO_LIGHT_GROUP   0xffu" in hdr
    section = hdr[hdr.index("light-group renders"):hdr.index("int ort_render_light_groups(")]
    for word in ("in ort_render_views_adaptive's order with the groups where ad stands", "ORT_ERR_INVALID", "ORT_ERR_UNSUPPORTED", "ORT_ERR_STATE",
                 "ORT_ERR_NO_DEVICE", "job_seed(seed, y*W + x)", "C_g = C_g + e", "C_g / (float)spp", "((v*G + g) * height*width*3)",
                 "left untouched in every plane", "Five identities", "emit = +0", "never read"):
        assert word in section, word
    order = [section.rindex(k) for k in ("ORT_ERR_INVALID (", "ORT_ERR_UNSUPPORTED (policy", "ORT_ERR_STATE (", "ORT_ERR_NO_DEVICE (")]
    assert order == sorted(order)


def _caller(api, views_form, device_form):
    """call(handle, params, groups, out_groups, out_rgb, states[, views, count]) through one of the four entry points; groups:
    None, an api.LightGroups, or (table bytes, G)"""
    L = api.lib()
    cam = api.View()
    keep = []

    def call(handle, p, groups, out, rgb, states, views="own", count=1, stats=None):
        if isinstance(groups, tuple):
            table = np.ascontiguousarray(groups[0], np.uint8)
            keep.append(table)
            groups = api.LightGroups(table.ctypes.data, len(table), groups[1])
        gp = ctypes.byref(groups) if groups is not None else None
        pp = ctypes.byref(p) if p is not None else None
        if views_form:
            v = ctypes.addressof(cam) if isinstance(views, str) else views
            if device_form:
                return L.ort_render_views_light_groups_device(handle, pp, gp, v, count, out, rgb, states, None, stats)
            return L.ort_render_views_light_groups(handle, pp, gp, v, count, out, rgb, states, stats)
        if device_form:
            return L.ort_render_light_groups_device(handle, pp, gp, out, rgb, states, None, stats)
        return L.ort_render_light_groups(handle, pp, gp, out, rgb, states, stats)
    return call, cam


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("views_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_errors_come_in_order(api, views_form, device_form, committed):
    """INVALID (nulls, the view cap, the params, spp above 1 << 24, then the groups clause by clause and the planes' alignment),
    UNSUPPORTED (policy, shard, packed, a camera outside the box), then the scene's state: STATE before NO_DEVICE.  On a
    committed-but-not-uploaded scene and on an uncommitted one, so every error comes before any device work"""
    s = _scene(api, committed)
    L = api.lib()
    call, view = _caller(api, views_form, device_form)
    cam = s.camera(8, 8)
    for k, name in enumerate(("p", "x_axis", "y_axis", "z_axis")):
        setattr(view.camera, name, api.V3(*[float(c) for c in cam[k]]))
    keep = [_aligned(4 * 8 * 8 * 12), _aligned(8 * 8 * 12), _aligned(256)]
    out, rgb, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    n = s.info().material_count
    lights = s.light_materials()
    assert n == 17 and lights == [13, 14, 15, 16]
    good_table = np.full(n, 0x5A, np.uint8)   # the entry of a material that is no light may hold any byte
    good_table[lights] = [0, 1, 0xFF, 3]
    GOOD = (good_table, 4)
    bad_groups = (good_table, 0)
    nan = float("nan")
    # nulls first: before bad params and bad groups
    assert call(s.handle, _params(api, width=0), bad_groups, None, rgb, fin) == api.ERR_INVALID
    assert b"group frames" in L.ort_last_error()
    if views_form:
        assert call(s.handle, _params(api, width=0), bad_groups, out, rgb, fin, views=None) == api.ERR_INVALID
        assert b"views" in L.ort_last_error()
        assert call(s.handle, _params(api, width=0), bad_groups, out, rgb, fin, count=api.MAX_VIEWS + 1) == api.ERR_INVALID
        assert b"ORT_MAX_VIEWS" in L.ort_last_error()
    assert call(None, _params(api), GOOD, out, rgb, fin) == api.ERR_INVALID
    assert call(s.handle, None, GOOD, out, rgb, fin) == api.ERR_INVALID
    # the params, as the render call judges them, before the groups; chunk is ignored
    for p, word in ((_params(api, width=0), b"image size"), (_params(api, rect=(4, 4, 4, 8)), b"rect"), (_params(api, rect=(0, 0, 9, 8)), b"rect"),
                    (_params(api, spp=0), b"spp"), (_params(api, rr=-0.5), b"rr"), (_params(api, rr=nan), b"rr"), (_params(api, policy=7), b"policy"),
                    (_params(api, shard=(3, 2)), b"shard index")):
        assert call(s.handle, p, bad_groups, out, rgb, fin) == api.ERR_INVALID, word
        assert word in L.ort_last_error(), (word, L.ort_last_error())
    assert call(s.handle, _params(api, width=70000, height=1), bad_groups, out, rgb, fin) == api.ERR_UNSUPPORTED   # as the render call: 16-bit coordinates
    assert call(s.handle, _params(api, spp=(1 << 24) + 1), bad_groups, out, rgb, fin) == api.ERR_INVALID
    assert b"1 << 24" in L.ort_last_error()
    # the groups, clause by clause, before what the call does not do
    chunky = _params(api, policy="chunk", spp=7, chunk=3, shard=(0, 2), packed=True)
    assert call(s.handle, chunky, None, out, rgb, fin) == api.ERR_INVALID
    assert b"null groups" in L.ort_last_error()
    assert call(s.handle, chunky, api.LightGroups(None, n, 4), out, rgb, fin) == api.ERR_INVALID
    assert b"group_of_material" in L.ort_last_error()
    for count in (n - 1, n + 1, 0):
        assert call(s.handle, chunky, (np.resize(good_table, max(count, 1)), 4) if count else api.LightGroups(good_table.ctypes.data, 0, 4), out, rgb, fin) == api.ERR_INVALID
        assert b"material_count" in L.ort_last_error()
    for G in (0, api.MAX_LIGHT_GROUPS + 1, 0xFFFFFFFF):
        assert call(s.handle, chunky, (good_table, G), out, rgb, fin) == api.ERR_INVALID
        assert b"group_count" in L.ort_last_error()
    for m, g, G in ((13, 4, 4), (16, 8, 8), (15, 0xFE, 8), (14, 1, 1)):
        t = good_table.copy()
        t[lights] = 0
        t[m] = g
        assert call(s.handle, chunky, (t, G), out, rgb, fin) == api.ERR_INVALID, (m, g, G)
        assert b"light material %d" % m in L.ort_last_error()
    for planes in ((out + 2, rgb, fin), (out, rgb + 1, fin), (out, rgb, fin + 2)):
        assert call(s.handle, chunky, GOOD, *planes) == api.ERR_INVALID
        assert b"4-byte aligned" in L.ort_last_error()
    # what the call does not do: any policy but PIXEL, shards, a packed framebuffer
    for policy in ("tile32", "whole", "chunk"):
        assert call(s.handle, _params(api, policy=policy, shard=(0, 2) if policy == "chunk" else (0, 1)), GOOD, out, rgb, fin) == api.ERR_UNSUPPORTED
        assert b"PIXEL" in L.ort_last_error()
    assert call(s.handle, _params(api, shard=(1, 2), packed=True), GOOD, out, rgb, fin) == api.ERR_UNSUPPORTED
    assert b"shard" in L.ort_last_error()
    assert call(s.handle, _params(api, packed=True), GOOD, out, rgb, fin) == api.ERR_UNSUPPORTED
    assert b"packed" in L.ort_last_error()
    if views_form:   # a camera outside the box, naming the view
        two = (api.View * 2)(view, view)
        two[1].camera.p = api.V3(1e6, 0.0, 0.0)
        assert call(s.handle, _params(api), GOOD, out, rgb, fin, views=ctypes.addressof(two), count=2) == api.ERR_UNSUPPORTED
        assert b"view 1" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it: the optional planes NULL, the limits, any byte where no light is
    assert call(s.handle, _params(api, spp=1 << 24, chunk=5, rr=7.5), GOOD, out, None, None) == state
    for filler in (0, 7, 8, 0xFE, 0xFF):
        t = np.full(n, filler, np.uint8)
        t[lights] = [7, 0xFF, 0, 7]
        assert call(s.handle, _params(api), (t, 8), out, rgb, fin) == state
    assert call(s.handle, _params(api), (np.where(good_table == 0x5A, 0x5A, 0).astype(np.uint8), 1), out, rgb, fin) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_empty_batch_is_ok(api, device_form):
    """view_count == 0: ORT_OK without a launch, whatever the other arguments"""
    call, _ = _caller(api, True, device_form)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, None, None, None, views=None, count=0) == api.OK
        assert call(s.handle, _params(api, width=0, policy="whole"), (np.zeros(3, np.uint8), 0), None, None, None, count=0) == api.OK
    assert call(None, None, None, None, None, None, views=None, count=0) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, None, None, None, views=None, count=0, stats=ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_shapes(api):
    s = _scene(api)
    lights = s.light_materials()
    assert lights == [13, 14, 15, 16]
    per_light = {m: g for g, m in enumerate(lights)}
    with pytest.raises(api.OrtError) as e:
        s.render_light_groups(8, 6, 4, 3, per_light, want_states=True)
    assert e.value.code == api.ERR_NO_DEVICE
    # the dict form, the sequence form, and what G defaults to
    lgs, table, G = s._light_groups(per_light, None)
    assert G == 4 and table.tolist() == [0xFF] * 13 + [0, 1, 2, 3] and (lgs.material_count, lgs.group_count) == (17, 4)
    assert s._light_groups({13: 2}, None)[2] == 3 and s._light_groups({13: 2}, 8)[2] == 8 and s._light_groups({}, None)[2] == 1
    seq = [9] * 13 + [1, 1, 0xFF, 0]
    assert s._light_groups(seq, None)[1].tolist() == seq and s._light_groups(seq, None)[2] == 2
    for bad in ([0] * 16, np.zeros((17, 1), np.uint8), {17: 0}, {-1: 0}):
        with pytest.raises(ValueError):
            s.render_light_groups(8, 6, 4, 3, bad)
    with pytest.raises(api.OrtError) as e:
        s.render_light_groups(8, 6, 4, 3, {13: 5}, group_count=4)
    assert e.value.code == api.ERR_INVALID
    planes = [np.zeros((4, 6, 8, 3), "<f4"), np.zeros((6, 8, 3), "<f4"), np.zeros((6, 8), "<u4")]
    for bad in (planes[:2], [planes[0], planes[1], planes[2].astype("<i8")], [planes[0][:, :, ::2], planes[1], planes[2]],
                [np.zeros((3, 6, 8, 3), "<f4"), planes[1], planes[2]]):
        with pytest.raises(ValueError):
            s.render_light_groups(8, 6, 4, 3, per_light, want_states=True, out=bad)
    cams = np.stack([s.camera(8, 6)] * 2)
    for bad_cams, bad_seeds in ((cams[:, :3], [1, 2]), (cams, [1]), (cams[0], [1, 2])):
        with pytest.raises(ValueError):
            s.render_views_light_groups(bad_cams, bad_seeds, 8, 6, 4, per_light)
    with pytest.raises(ValueError):
        s.render_views_light_groups(cams, [1, 2], 8, 6, 4, per_light, want_states=True, out=planes)   # one frame's planes for two views
    with pytest.raises(api.OrtError) as e:
        s.render_views_light_groups(cams, [1, 2], 8, 6, 4, per_light)
    assert e.value.code == api.ERR_NO_DEVICE
    fr, rgb, states, st = s.render_views_light_groups(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, per_light, want_states=True)
    assert fr.shape == (0, 4, 6, 8, 3) and rgb.shape == (0, 6, 8, 3) and states.shape == (0, 6, 8) and st["paths"] == 0
    fr, st = s.render_views_light_groups(np.zeros((0, 4, 3), "<f4"), [], 8, 6, 4, per_light, want_rgb=False)
    assert fr.shape == (0, 4, 6, 8, 3) and fr.dtype == np.dtype("<f4")
    p = s.params(8, 6, 4, 1, "pixel")
    for call in (lambda: s.render_light_groups_device(p, per_light, 64), lambda: s.render_views_light_groups_device(p, cams, [1, 2], per_light, 64)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE


# ---- 4. the launch plan -----------------------------------------------------------------------------------------------------------
def test_launch_plan_names_the_groups_kernels():
    """plan_pixel_jobs, RK_GROUPS: the plain loop over implicit one-pixel jobs of a batch of views, both BSDF flavours with counters,
    whatever the knobs say; its variant is groups<...> and is built; the plans of the other calls name what they named"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "launch_plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tool = os.path.join(ROOT, "tools", "launch_plan")

    def plan(env=None, **kw):
        e = {k: v for k, v in os.environ.items() if not k.startswith("ORT_")}
        e.update(env or {})
        return json.loads(subprocess.check_output([tool] + ["%s=%s" % kv for kv in kw.items()], env=e))
    frame = dict(policy="pixel", width=1920, height=1080, x1=1920, y1=1080, materials=8, lights=2, diffuse_only=1, sah_cost=0.5, spp=16)
    forced = {"ORT_EXCHANGE": "1", "ORT_WAVES5": "1", "ORT_WIDE": "1", "ORT_MODE": "wavefront", "ORT_DEBUG_UTIL": "1"}
    for env in ({}, forced):
        for counters in (0, 1):
            pl = plan(env, groups=1, variant=1, counters=counters, has_wide=1, **frame)
            assert pl["groups"] == 1 and pl["views"] == 1 and pl["view_count"] == 1 and pl["implicit"] == 1 and pl["mode"] == 1
            assert not (pl["exchange"] or pl["five"] or pl["wide"] or pl["wavefront"] or pl["util"])
            assert pl["variant"] == "groups<%d, 1, 1, 1, 0>" % counters and pl["built"] == 1
            assert pl["job_count"] == pl["view_jobs"] == 240 * 135 * 64 and pl["grid"] == pl["max_blocks"] == 1024
            assert pl["partial_bytes"] == pl["stash_bytes"] == pl["drain_bytes"] == 0
            same = plan(env, adaptive=1, counters=counters, has_wide=1, **frame)   # the adaptive render's launch in every other field
            assert {k: v for k, v in pl.items() if k not in ("groups", "variant", "built")} == {k: v for k, v in same.items() if k != "adaptive"}
    pl = plan({"ORT_KERNEL": "general", "ORT_LDS_TABLES": "0"}, groups=1, variant=1, views=3, x0=5, y0=9, **{**frame, "x1": 20, "y1": 17, "width": 27, "height": 19})
    assert pl["variant"] == "groups<0, 0, 0, 1, 0>" and pl["built"] == 1 and pl["view_count"] == 3
    assert pl["view_jobs"] == 3 * 2 * 64 and pl["job_count"] == 3 * pl["view_jobs"] and pl["grid"] == 5
    assert plan(groups=1, variant=1, **{**frame, "materials": 60})["variant"] == "groups<0, 1, 0, 1, 0>"
    # the other calls' plans name what they named
    assert plan(variant=1, **frame)["variant"].startswith(("loop<", "exchange<", "five<"))
    assert plan(variant=1, adaptive=1, **frame)["variant"] == "adaptive<0, 1, 1, 1, 0>"
    assert plan(variant=1, views=3, **frame)["variant"] == "loop_views<0, 1, 1, 1, 0>"
    for bad in (["groups=1", "policy=chunk"], ["groups=1", "adaptive=1", "policy=pixel"], ["groups=1", "policy=pixel", "shard_count=2"]):
        assert subprocess.run([tool, "width=8", "height=8", "x1=8", "y1=8"] + bad, capture_output=True).returncode == 2
    sweep = json.loads(subprocess.check_output([tool, "sweep=1"], env={k: v for k, v in os.environ.items() if not k.startswith("ORT_")}))
    assert sweep["plans"] > 0 and (sweep["unbuilt"], sweep["first"]) == (0, [])


# ---- 5. the lane code on host threads ---------------------------------------------------------------------------------------
def _check(c, got, groups, G, spp, rect, what, seed=lg.SEED, cams=None, seeds=None):
    frames, rgb, states = got
    V = len(frames)
    for v in range(V):
        cam, sd = (None, seed) if cams is None else (cams[v], int(seeds[v]))
        lg.assert_plane(frames[v], c.expected(groups, G, spp, sd, cam, rect), rect, lg.GUARD_F, "%s: view %d, group frames" % (what, v))
        if rgb is not None:
            lg.assert_plane(rgb[v], c.frame(None, spp, sd, cam, rect), rect, lg.GUARD_F, "%s: view %d, rgb" % (what, v))
        if states is not None:
            lg.assert_plane(states[v], c.states(spp, sd, cam, rect), rect, lg.GUARD_STATE, "%s: view %d, states" % (what, v))


@pytest.mark.parametrize("name", lg.SCENES)
def test_host_sim_is_the_twins(host_sim, case, tmp_path, name):
    """every scene, one group per light (the table scene: its lights past the cap sharing the last group), 16 spp and 1, the rect:
    every plane bit for bit, guards outside the rect intact; the tables in LDS form and from their arrays, both BSDF flavours
    where the scene allows, one thread and eight"""
    c = case(name)
    groups = c.per_light() if name != lg.TABLE_SCENE else {m: min(g, 2) for g, m in enumerate(c.lights)}
    G = max(groups.values()) + 1
    envs = [{}, {"SIM_TABS": "1"}] if name != lg.TABLE_SCENE else [{}]
    if name == "room_diffuse":
        envs = [{"SIM_DIFFUSE": "1"}, {"SIM_DIFFUSE": "1", "SIM_TABS": "1"}, {}]
    for spp in lg.SPPS:
        for k, env in enumerate(envs):
            for threads in ((8, 1) if k == 0 and spp == 16 else (8,)):
                got = lg.host_light_groups(host_sim, tmp_path, c, c.table(groups), G, spp, rect=lg.RECT, env=env, threads=threads)
                _check(c, got, groups, G, spp, lg.RECT, "%s %d spp %r, %d threads" % (name, spp, env, threads))
    # the whole frame, and the counters' paths: a path per sample
    r = hs.run(host_sim, ["--light-groups"] + c.hs_args() + ["-", lg.SEED, lg.W, lg.H, 0, 0, lg.W, lg.H, 16, repr(lg.RR), str(tmp_path / "groups.u8"), G,
                                                              str(tmp_path / "lg.f32"), "-", "-"], threads=8)
    assert hs.counters(r)["paths"] == lg.W * lg.H * 16
    lg.assert_plane(np.fromfile(str(tmp_path / "lg.f32"), "<f4").reshape(G, lg.H, lg.W, 3), c.expected(groups, G, 16), None, lg.GUARD_F, name + ": whole frame")


@pytest.mark.parametrize("name", ["room_all_lobes", "testscene"])
def test_host_sim_group_tables(host_sim, case, tmp_path, name):
    """identity 3 on the host: G = 1, G = 8 with empty groups, a light in no group, two lights sharing a group (against the twin
    that keeps both), the other lights regrouped, the optional planes not passed -- a group's frame depends only on which lights
    are in it"""
    c = case(name)
    a, b, rest = c.lights[0], c.lights[1], c.lights[2:]
    tables = {
        "G = 1, every light": ({m: 0 for m in c.lights}, 1),
        "G = 1, one light in no group": ({m: 0 for m in c.lights[1:]}, 1),
        "G = 8, empty groups": ({a: 6, b: 2, **{m: 7 for m in rest}}, 8),
        "two lights share a group": ({a: 1, b: 1, **{m: 0 for m in rest}}, 2),
        "only the last light, in group 2 of 3": ({c.lights[-1]: 2}, 3),
    }
    for what, (groups, G) in tables.items():
        for want_rgb, want_states in ((True, True), (False, False)):
            got = lg.host_light_groups(host_sim, tmp_path, c, c.table(groups), G, 16, rect=lg.RECT, want_rgb=want_rgb, want_states=want_states, threads=8)
            _check(c, got, groups, G, 16, lg.RECT, "%s: %s" % (name, what))
    # the fillers of the materials that are no light are not read
    for filler in (0, 3, 0xFF):
        got = lg.host_light_groups(host_sim, tmp_path, c, c.table(c.per_light(), filler), len(c.lights), 1, threads=8)
        _check(c, got, c.per_light(), len(c.lights), 1, None, "%s: filler %d" % (name, filler))


@pytest.mark.parametrize("name", lg.ROOMS)
def test_host_sim_batch_of_views(host_sim, api, case, tmp_path, name):
    """three views on three seeds, two of them the same camera: frames (v, .) are the single frame's for that camera and seed"""
    c = case(name)
    cams, seeds = lg.batch_cameras(api, c), lg.BATCH_SEEDS
    assert (cams[0] == cams[2]).all() and (cams[0] != cams[1]).any() and len(set(seeds)) == 3
    groups = c.per_light()
    for spp, rect in ((16, lg.RECT), (1, None)):
        got = lg.host_light_groups(host_sim, tmp_path, c, c.table(groups), 3, spp, rect=rect, cams=cams, seeds=seeds, threads=8)
        _check(c, got, groups, 3, spp, rect, "%s: batch, %d spp" % (name, spp), cams=cams, seeds=seeds)
        assert (_bits(got[0][0]) != _bits(got[0][2])).any() and (_bits(got[0][0]) != _bits(got[0][1])).any()
    one = lg.host_light_groups(host_sim, tmp_path, c, c.table(groups), 3, 16, rect=lg.RECT, cams=cams[1:2], seeds=seeds[1:2], threads=8)
    _check(c, one, groups, 3, 16, lg.RECT, name + ": batch of one", cams=cams[1:2], seeds=seeds[1:2])


# ---- 6. under the sanitizers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_all_lobes", "c2_analytic"])
def test_host_sim_under_sanitizers(case, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): ends clean, with the twins' planes; the planes are
    exactly as long as the frames, so a write past a plane's end is a write past the block"""
    san = hs.built("host_sim_san")
    c = case(name)
    groups = c.per_light()
    G = len(c.lights)
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
    for extra, spp, rect in (({}, 16, lg.RECT), ({"SIM_TABS": "1"}, 1, None)):
        got = lg.host_light_groups(san, tmp_path, c, c.table(groups), G, spp, rect=rect, env=dict(env, **extra), threads=2)
        _check(c, got, groups, G, spp, rect, "%s sanitized %r" % (name, extra))
    got = lg.host_light_groups(san, tmp_path, c, c.table({c.lights[0]: 7}), 8, 1, rect=lg.RECT, want_rgb=False, want_states=False,
                               env=env, threads=2)
    _check(c, got, {c.lights[0]: 7}, 8, 1, lg.RECT, name + " sanitized, G = 8")
