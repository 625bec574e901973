"""Irradiance queries (ort_irradiance, ort_irradiance_adaptive and their device forms), host side: the point sets shown not to
be vacuous from the oracle alone, the C ABI surface and its errors in the order include/ort.h gives them, the hemisphere draw
as the kernels compose it (unit op 20) against the oracle's composition, and the lane code run on host threads
(tools/host_sim --irradiance, --irradiance-adaptive) against identity I2 (rr = 0: the oracle's closed form) and identity I1
(rr = 0.8: a chain of the existing --radiance mode at spp = 1), all bits (tests/irradiance_cases.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adaptive_cases as ac
import host_sim_tool as hs
import irradiance_cases as ic
import radiance_cases as rc
import ref_io
from adaptive_cases import Adaptive
from conftest import DATA
from host_cases import aligned as _aligned, scene as _scene

NAMES = {"ort_irradiance", "ort_irradiance_device", "ort_irradiance_adaptive", "ort_irradiance_adaptive_device"}
SCENES = {"testscene": 128, "c2_analytic": 128, "c3_bunny_room": 64}
CHAIN = 17   # samples per point of the composed chain: the adaptive sets' largest max_spp
_worlds = {}


class World:
    pass


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


@pytest.fixture()
def world(api, oracle, load_scene):
    """name -> scene, oracle scene, points and the oracle's closed form of 8 samples per point at rr = 0; computed once"""
    def get(name):
        if name not in _worlds:
            w = World()
            w.name, w.scene = name, load_scene(name)
            w.flat = w.scene.flatten(1, 1)
            w.osc = oracle.OracleScene(w.flat)
            w.pts = ic.point_set(name, w.flat, w.osc, SCENES[name])
            w.closed = ic.chain_closed_form(oracle, w.osc, w.flat, w.pts, 8)
            w.chain = None
            _worlds[name] = w
        return _worlds[name]
    return get


def composed_chain(w, oracle, host_sim, tmp_path):
    """identity I1 on the CPU: CHAIN chained calls of host_sim --radiance at spp = 1, rr = 0.8; computed once per scene"""
    if w.chain is None:
        w.chain = ic.chain_by_radiance(oracle, w.pts, CHAIN, lambda rays, seeds: hs.radiance(host_sim, tmp_path, w.name, rays, seeds, 1, ic.RR, threads=8))
    return w.chain


# ---- 1. the point sets, from the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_point_sets_are_not_vacuous(world, oracle, name):
    """rr = 0, spp = 8: at least a tenth of the points inside the domain are not black, at least a tenth have both a sample that
    adds light and one that does not; and every kind of point the set promises is there"""
    w = world(name)
    p = w.pts
    lit, mixed = ic.lit_shares(w.closed)
    print("%s: lit %.3f, mixed %.3f of %d points inside the domain" % (name, lit, mixed, p.ok.sum()))
    assert lit >= 0.10 and mixed >= 0.10
    assert (~p.ok).sum() == 8 and p.far.sum() == 8 and p.ok[p.far].all()
    lo, hi = rc.origin_box(w.flat)
    assert ((p.points[p.far, 0:3] < lo) | (p.points[p.far, 0:3] > hi)).any(axis=1).all()
    inside = p.ok & ~p.far
    assert ((p.points[inside, 0:3] >= lo) & (p.points[inside, 0:3] <= hi)).all()
    n = p.points[p.ok, 3:6]
    for z in ic.LOBE_Z:
        assert (n[:, 2] == np.float32(z)).any(), z
    assert ((n[:, 2] == 1) & (n[:, 0] == 0) & (n[:, 1] == 0)).any() and ((n[:, 2] == -1) & (n[:, 0] == 0) & (n[:, 1] == 0)).any()
    l2 = ic.len2(n)
    assert (l2 < np.float32(0.99901)).any() and (l2 > np.float32(1.00099)).any()
    bad = p.points[~p.ok]
    with np.errstate(all="ignore"):
        bl = ic.len2(bad[:, 3:6])
    assert np.isnan(bad[:, 0:3]).any() and np.isinf(bad[:, 0:3]).any() and np.isnan(bad[:, 3:6]).any()
    assert (bl == 0).any() and ((bl > 0.2) & (bl < 0.3)).any() and ((bl > 3.9) & (bl < 4.1)).any()
    assert (p.seeds == 0).sum() == 1 and (p.seeds == 0xFFFFFFFF).sum() == 1 and p.ok[p.seeds == 0].all()
    one = np.flatnonzero(p.seeds == rc.unstep(0xFFFFFFFF))
    assert len(one) == 1 and p.ok[one[0]] and ic.draws(oracle, p.seeds[one])[0][0] == np.float32(1.0)


def test_lobe_normals_stand_at_the_domains_edges():
    n = ic.lobe_normals()
    l2 = ic.len2(n)
    assert ((l2 >= np.float32(0.999)) & (l2 <= np.float32(1.001))).all()
    assert float(l2[6]) - 0.999 < 3e-7 and 1.001 - float(l2[7]) < 3e-7   # within a few float32 steps of the bounds
    assert (np.abs(np.abs(n[2:6, 2]) - 1) < 3e-4).all() and (np.abs(ic.len2(n[:6]) - 1) < 1e-6).all()


# ---- 2. the C ABI -----------------------------------------------------------------------------------------------------------------
def test_irradiance_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert "pi * out_rgb" in hdr and "kd * out_rgb" in hdr
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands


def _caller(api, device_form, adaptive):
    L = api.lib()

    def call(handle, pts, seeds, n, spp, rr, out, states, flags=0, stats=None):
        if device_form:
            return L.ort_irradiance_device(handle, pts, seeds, n, spp, rr, out, states, flags, None, stats)
        return L.ort_irradiance(handle, pts, seeds, n, spp, rr, out, states, flags, stats)

    def call_ad(handle, pts, seeds, n, ad, rr, out, spp, m2, states, flags=0, stats=None):
        adp = ctypes.byref(api.Adaptive(*ad)) if ad is not None else None
        if device_form:
            return L.ort_irradiance_adaptive_device(handle, pts, seeds, n, adp, rr, out, spp, m2, states, flags, None, stats)
        return L.ort_irradiance_adaptive(handle, pts, seeds, n, adp, rr, out, spp, m2, states, flags, stats)
    return call_ad if adaptive else call


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_irradiance_errors_come_in_order(api, device_form, committed):
    """ort_radiance's order: INVALID (nulls, misaligned pointers, spp == 0, rr outside [0, 1)), then STATE before NO_DEVICE"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form, False)
    keep = [_aligned(4 * 24), _aligned(16), _aligned(48), _aligned(16)]
    pts, seeds, out, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, pts, seeds, 4, 1, 0.8, out, fin) == api.ERR_INVALID
    assert call(s.handle, None, seeds, 4, 1, 0.8, out, fin) == api.ERR_INVALID
    assert b"points" in L.ort_last_error()
    assert call(s.handle, pts, None, 4, 1, 0.8, out, fin) == api.ERR_INVALID
    assert call(s.handle, pts, seeds, 4, 1, 0.8, None, fin) == api.ERR_INVALID
    for r, sd, o, f in ((pts + 4, seeds, out, fin), (pts, seeds + 2, out, fin), (pts, seeds, out + 1, fin), (pts, seeds, out, fin + 2),
                        (pts + 2, seeds, out, None)):
        assert call(s.handle, r, sd, 4, 0, 2.0, o, f) == api.ERR_INVALID      # a misaligned pointer comes before spp and rr
        assert b"aligned" in L.ort_last_error()
    assert call(s.handle, pts, seeds, 4, 0, 2.0, out, fin) == api.ERR_INVALID
    assert b"spp" in L.ort_last_error()                                         # ... and spp before rr
    for rr in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert call(s.handle, pts, seeds, 4, 1, rr, out, fin) == api.ERR_INVALID, rr
        assert b"rr" in L.ort_last_error()
    assert call(s.handle, pts + 8, seeds + 4, 4, 3, 0.0, out + 4, None) == state
    assert call(s.handle, pts, seeds, 4, 1, 0.999, out, fin, api.RENDER_COUNTERS) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_irradiance_adaptive_errors_come_in_order(api, device_form, committed):
    """ort_radiance_adaptive's order: pointers, then ad, then rr, then the scene's state"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form, True)
    keep = [_aligned(4 * 24), _aligned(16), _aligned(48), _aligned(16), _aligned(16), _aligned(16)]
    pts, seeds, out, spp, m2, fin = (k[1] for k in keep)
    good = tuple(ic.MAIN)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, pts, seeds, 4, good, 0.8, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, None, seeds, 4, good, 0.8, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, pts, None, 4, good, 0.8, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, pts, seeds, 4, good, 0.8, None, spp, m2, fin) == api.ERR_INVALID
    for r, sd, o, sp, m, f in ((pts + 4, seeds, out, spp, m2, fin), (pts, seeds, out, spp + 2, m2, fin), (pts, seeds, out, spp, m2 + 1, fin),
                               (pts, seeds, out, spp, m2, fin + 2), (pts + 2, seeds, out, None, None, None)):
        assert call(s.handle, r, sd, 4, None, 0.8, o, sp, m, f) == api.ERR_INVALID     # a misaligned pointer comes before ad
        assert b"aligned" in L.ort_last_error()
    assert call(s.handle, pts, seeds, 4, None, 2.0, out, spp, m2, fin) == api.ERR_INVALID
    assert b"ad" in L.ort_last_error() and b"rr" not in L.ort_last_error()
    for bad, word in (((1, 16, 4, 0.3, 0.05), b"min_spp"), ((8, 7, 4, 0.3, 0.05), b"max_spp"), ((4, (1 << 24) + 1, 4, 0.3, 0.05), b"1 << 24"),
                      ((4, 16, 0, 0.3, 0.05), b"check_every"), ((4, 16, 4, float("nan"), 0.05), b"tolerance"), ((4, 16, 4, 0.3, -1.0), b"floor")):
        assert call(s.handle, pts, seeds, 4, bad, 2.0, out, spp, m2, fin) == api.ERR_INVALID, bad   # ... and ad before rr
        assert word in L.ort_last_error(), (bad, L.ort_last_error())
    assert call(s.handle, pts, seeds, 4, good, 1.0, out, spp, m2, fin) == api.ERR_INVALID
    assert b"rr" in L.ort_last_error()
    assert call(s.handle, pts + 8, seeds + 4, 4, (2, 2, 1, 0.0, 0.0), 0.0, out + 4, None, None, None) == state
    assert call(s.handle, pts, seeds, 4, good, 0.999, out, spp, m2, fin, api.RENDER_COUNTERS) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_irradiance_empty_batch_is_ok(api, device_form):
    """count == 0: ORT_OK without a launch, with nulls, whatever the other arguments"""
    call, call_ad = _caller(api, device_form, False), _caller(api, device_form, True)
    keep_r, p = _aligned(24)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, 0, 0, 2.0, None, None) == api.OK
        assert call(s.handle, p + 1, p + 1, 0, 1, 0.8, p + 1, p + 1) == api.OK
        assert call_ad(s.handle, None, None, 0, None, 2.0, None, None, None, None) == api.OK
        assert call_ad(s.handle, p + 1, p + 1, 0, (0, 0, 0, -1.0, -1.0), 0.8, p + 1, p + 1, p + 1, p + 1) == api.OK
    assert call(None, None, None, 0, 1, 0.8, None, None) == api.OK
    assert call_ad(None, None, None, 0, tuple(ic.MAIN), 0.8, None, None, None, None) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, 0, 1, 0.8, None, None, 0, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_irradiance_shapes(api):
    s = _scene(api)
    pts = np.zeros((3, 6), "<f4")
    for bad in (np.zeros((3, 5), "<f4"), np.zeros(6, "<f4")):
        with pytest.raises(ValueError):
            s.irradiance(bad, np.ones(len(bad), "<u4"), 1)
        with pytest.raises(ValueError):
            s.irradiance_adaptive(bad, np.ones(len(bad), "<u4"), 4, 16, 0.3)
    with pytest.raises(ValueError):
        s.irradiance(pts, np.ones(2, "<u4"), 1)
    with pytest.raises(api.OrtError) as e:
        s.irradiance(pts, np.ones(3, "<u4"), 2, want_states=True)
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.irradiance(pts, np.ones(3, "<u4"), 0)
    assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.OrtError) as e:
        s.irradiance_adaptive(pts, np.ones(3, "<u4"), 4, 16, 0.3)
    assert e.value.code == api.ERR_NO_DEVICE
    rgb, states, st = s.irradiance(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, want_states=True)
    assert rgb.shape == (0, 3) and rgb.dtype == np.dtype("<f4") and states.shape == (0,) and st["paths"] == 0
    assert len(s.irradiance_adaptive(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, 16, 0.3)) == 4
    for call in (lambda: s.irradiance_device(64, 64, 4, 1, 0.8, 64), lambda: s.irradiance_adaptive_device(64, 64, 4, 4, 16, 0.3, 0.05, 4, 0.8, 64)):
        with pytest.raises(api.OrtError) as e:
            call()
        assert e.value.code == api.ERR_NO_DEVICE


# ---- 3. the hemisphere draw as the kernels compose it ---------------------------------------------------------------------------
def op20_inputs(world):
    """the normals and seeds of the point sets' in-domain points, and 256 random ones"""
    rng = np.random.default_rng(20)
    normals = [rc._units(rng, 256)]
    seeds = [rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype("<u4")]
    for name in ("testscene", "c2_analytic"):
        p = world(name).pts
        normals.append(p.points[p.ok, 3:6])
        seeds.append(p.seeds[p.ok])
    return np.concatenate(seeds), np.concatenate(normals).astype("<f4")


def test_host_op20_is_the_oracles_composition(host_sim, world, oracle, tmp_path):
    seeds, normals = op20_inputs(world)
    assert (seeds == 0).any() and (seeds == 0xFFFFFFFF).any() and (normals[:, 2] == 1).any()
    ref_io.make_unit_records(20, ic.op20_rows(seeds, normals)).tofile(str(tmp_path / "in.bin"))
    hs.run(host_sim, ["--unit", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = ref_io.read_unit_output(str(tmp_path / "out.bin"))
    want = ic.op20_expected(oracle, seeds, normals)
    ic.assert_op20(got, want, "op 20 on the host")
    c1 = np.flatnonzero(seeds == rc.unstep(0xFFFFFFFF))   # c = 1: the direction is the normal itself (up to normalize)
    assert len(c1) and np.abs(want[c1, 0:3] - normals[c1] / np.linalg.norm(normals[c1], axis=1, keepdims=True)).max() < 1e-6


# ---- 4. the lane code on host threads -------------------------------------------------------------------------------------------
ENVS = {"testscene": [{}, {"SIM_TABS": "1"}], "c2_analytic": [{}, {"SIM_TABS": "1"}],
        "c3_bunny_room": [{"SIM_DIFFUSE": "1"}, {"SIM_TABS": "1", "SIM_DIFFUSE": "1"}, {}]}


@pytest.mark.parametrize("name", list(SCENES))
def test_host_sim_without_bounces_is_the_oracles_closed_form(host_sim, world, tmp_path, name):
    """identity I2, rr = 0, spp 1 and 8: colours and final states, both BSDF flavours, tables from LDS form and from their arrays;
    the far points took the exact walk where the tree holds quadrics; the counters' paths"""
    w = world(name)
    p = w.pts
    for spp in (1, 8):
        want = ic.expected_from(w.closed, p, spp)
        for env in ENVS[name]:
            rgb, fin, r = ic.host_sim(host_sim, tmp_path, name, p.points, p.seeds, spp, 0.0, env=env, threads=8)
            rc.assert_same(rgb, fin, *want, "%s rr 0 spp %d %r" % (name, spp, env))
            c = hs.counters(r)
            assert c["paths"] == spp * int(p.ok.sum())
            if name == "c2_analytic":
                assert c["fallback"] >= spp * int(p.far.sum())


@pytest.mark.parametrize("name", list(SCENES))
def test_host_sim_is_a_chain_of_radiance_samples(host_sim, world, oracle, tmp_path, name):
    """identity I1, rr = 0.8, spp 1 and 8: the --irradiance mode against spp chained calls of the --radiance mode at spp = 1"""
    w = world(name)
    p = w.pts
    chain = composed_chain(w, oracle, host_sim, tmp_path)
    assert sum((cols[:8] != 0).any() for cols, _ in chain.values()) >= len(chain) // 10
    for spp in (1, 8):
        want = ic.expected_from(chain, p, spp)
        for k, env in enumerate(ENVS[name]):
            if k and spp == 1:
                continue
            rgb, fin, _ = ic.host_sim(host_sim, tmp_path, name, p.points, p.seeds, spp, ic.RR, env=env, threads=8 if k == 0 else 3)
            rc.assert_same(rgb, fin, *want, "%s rr 0.8 spp %d %r" % (name, spp, env))
    # one thread, the points in another order: a point's answer is its own
    perm = np.random.default_rng(4).permutation(len(p.points))
    rgb, fin, _ = ic.host_sim(host_sim, tmp_path, name, p.points[perm], p.seeds[perm], 8, ic.RR, env=ENVS[name][0], threads=1)
    want = ic.expected_from(chain, p, 8)
    rc.assert_same(rgb, fin, want[0][perm], want[1][perm], name + " permuted")


@pytest.mark.parametrize("name", ["testscene", "c2_analytic"])
def test_adaptive_classes_are_present(host_sim, world, oracle, tmp_path, name):
    """on the composed chain, under both parameter sets: stopped at min_spp, strictly between, ran to max_spp -- each at least
    5 % of the points inside the domain"""
    w = world(name)
    chain = composed_chain(w, oracle, host_sim, tmp_path)
    assert ic.MAIN[:3] == (4, 16, 4) and ic.EVERY[:3] == (2, 17, 1) and ic.RR == 0.8
    for ad in ic.SETS:
        rgb, spp, m2, fin = ic.expected_adaptive(chain, w.pts, ad)
        at_min, between, at_max, lit = ac.classes(spp, rgb, w.pts.ok, ad)
        print("%s %r: at min %.3f, between %.3f, at max %.3f; early and lit %.3f" % (name, ad, at_min, between, at_max, lit))
        assert at_min >= 0.05 and between >= 0.05 and at_max >= 0.05


@pytest.mark.parametrize("name", list(SCENES))
def test_host_sim_adaptive_is_the_rule_over_the_chain(host_sim, world, oracle, tmp_path, name):
    """--irradiance-adaptive under two parameter sets: all four outputs equal adaptive_cases.cut over the composed chain; with
    min == max == n the --irradiance mode's bits at spp = n; the counters' paths are the samples taken"""
    w = world(name)
    p = w.pts
    chain = composed_chain(w, oracle, host_sim, tmp_path)
    for k, env in enumerate(ENVS[name]):
        for ad in ic.SETS:
            got, r = ic.host_sim_adaptive(host_sim, tmp_path, name, p.points, p.seeds, ad, ic.RR, env=env, threads=8 if k == 0 else 2)
            want = ic.expected_adaptive(chain, p, ad)
            ac.assert_same(got, want, "%s %r %r" % (name, ad, env))
            assert hs.counters(r)["paths"] == int(want[1].sum())
    for n in (2, 5):
        rgb, fin, _ = ic.host_sim(host_sim, tmp_path, name, p.points, p.seeds, n, ic.RR, threads=4)
        got, _ = ic.host_sim_adaptive(host_sim, tmp_path, name, p.points, p.seeds, Adaptive(n, n, 1, 0.3, 0.05), ic.RR, threads=4)
        rc.assert_same(got[0], got[3], rgb, fin, "%s min = max = %d" % (name, n))
        assert (got[1][p.ok] == n).all() and (got[1][~p.ok] == 0).all() and (got[2][~p.ok] == 0).all()


# ---- 5. under the sanitizers ------------------------------------------------------------------------------------------------------
def test_host_sim_irradiance_under_sanitizers(world, oracle, tmp_path):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly) on 64 points: ends clean, with the closed form's
    answers at rr = 0 and, under the stopping rule, the uniform mode's at min == max"""
    san = hs.built("host_sim_san")
    w = world("c2_analytic")
    p = w.pts.take(np.arange(64))
    closed = {i: w.closed[i] for i in range(64) if i in w.closed}
    for env in ({}, {"SIM_TABS": "1"}):
        rgb, fin, _ = ic.host_sim(san, tmp_path, "c2_analytic", p.points, p.seeds, 8, 0.0, env=env, threads=2)
        rc.assert_same(rgb, fin, *ic.expected_from(closed, p, 8), "sanitized %r" % env)
        got, _ = ic.host_sim_adaptive(san, tmp_path, "c2_analytic", p.points, p.seeds, Adaptive(8, 8, 1, 0.3, 0.05), 0.0, env=env, threads=2)
        rc.assert_same(got[0], got[3], rgb, fin, "sanitized, min = max = 8 %r" % env)
