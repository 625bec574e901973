"""Adaptive radiance queries (ort_radiance_adaptive / ort_radiance_adaptive_device), host side: the helper that turns the oracle
into their reference (tests/adaptive_cases.py) pinned against the oracle's own radiance reference, the case sets shown not to be
vacuous, the C ABI surface and its errors in the order include/ort.h gives them, and the lane code with the stopping rule run on
host threads (tools/host_sim --radiance-adaptive), plain and under ASan + UBSan, against that reference bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adaptive_cases as ac
import host_sim_tool as hs
import radiance_cases as rc
import table_scenes
from adaptive_cases import Adaptive
from conftest import DATA
from host_cases import aligned as _aligned, scene as _scene

NAMES = {"ort_radiance_adaptive", "ort_radiance_adaptive_device"}
N_RAYS = 128
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, load_scene, tmp_path_factory):
    """name -> scene, oracle scene, rays and the oracle's chains of 64 samples per ray at rr 0.8; computed once"""
    def get(name):
        if name not in _worlds:
            w = World()
            if name.startswith("tables_"):
                d = tmp_path_factory.mktemp("ad_" + name)
                scene, _, csg = table_scenes.build(api, name[len("tables_"):], d)
                w.scene, w.scn, w.base = scene.commit(), str(d / (name[len("tables_"):] + ".scn")), str(d) + "/"
            else:
                w.scene, w.scn, w.base, csg = load_scene(name), name, None, True
            flat = w.scene.flatten(1, 1)
            w.osc = oracle.OracleScene(flat, with_reference_csg=csg)
            w.cases = ac.cases_for(name, flat, w.osc, N_RAYS)
            w.chain = ac.chains(w.osc, w.cases, 64, ac.RR)
            _worlds[name] = w
        return _worlds[name]
    return get


@pytest.fixture(scope="module")
def host_sim():
    return hs.built("host_sim")


# ---- 1. the helper against the oracle alone ---------------------------------------------------------------------------------
def test_helper_without_checks_is_the_radiance_reference(world):
    """min == max == n: no check runs, and the expectation is radiance_cases.expected at spp = n, every ray taking n samples"""
    w = world("c2_analytic")
    idx = np.flatnonzero(w.cases.ok)
    for n in (2, 8, 17):
        rgb, spp, m2, fin = ac.expected_from(w.chain, w.cases, Adaptive(n, n, 3, 0.3, 0.05))
        want_rgb, want_fin = rc.expected(w.osc, w.cases.cams[idx], w.cases.seeds[idx], n, ac.RR)
        rc.assert_same(rgb[idx], fin[idx], want_rgb, want_fin, "min = max = %d" % n)
        assert (spp[idx] == n).all() and (spp[~w.cases.ok] == 0).all() and (m2[~w.cases.ok] == 0).all()
        assert np.isnan(rgb[~w.cases.ok]).all() and (fin[~w.cases.ok] == w.cases.seeds[~w.cases.ok]).all()
        assert (m2[idx] >= 0).all() and ((m2[idx] > 0) == (rgb[idx] != 0).any(axis=1)).all()


def test_helper_prefix_property(world):
    """what is expected at max_spp = 32 for a ray that stops by 12 is the expectation at max_spp = 16; and the rule restated:
    a ray stops where the estimated standard error, computed in float64 from the outputs, meets the threshold"""
    w = world("c2_analytic")
    a32 = ac.expected_from(w.chain, w.cases, Adaptive(4, 32, 4, 0.3, 0.05))
    a16 = ac.expected_from(w.chain, w.cases, Adaptive(4, 16, 4, 0.3, 0.05))
    early = w.cases.ok & (a32[1] <= 12)
    assert early.sum() >= 10 and (a32[1][early] == 12).any()
    for x, y in zip(a32, a16):
        assert x[early].tobytes() == y[early].tobytes()
    late = w.cases.ok & (a32[1] > 16)
    assert late.any() and (a16[1][late] == 16).all()
    # the estimate rebuilt from the outputs (include/ort.h): stopped rays are within the tolerance, up to rounding
    rgb, n, q = a32[0][early].astype(np.float64), a32[1][early].astype(np.float64), a32[2][early].astype(np.float64)
    m = rgb @ np.array([0.2126, 0.7152, 0.0722])
    se = np.sqrt(np.maximum(0, q / n - m * m) / (n - 1))
    assert (se <= 0.3 * np.maximum(np.abs(m), 0.05) * (1 + 1e-4)).all()


# ---- 2. the case sets are not vacuous ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room"])
def test_case_sets_are_not_vacuous(world, name):
    """from the oracle alone, under the GPU tests' main parameter set: each of the three classes (stopped at min_spp, strictly
    between, ran to max_spp) holds at least a tenth of the rays inside the domain; at least a tenth of those that stopped early
    are not black"""
    w = world(name)
    assert ac.MAIN[:3] == (4, 64, 4) and ac.RR == 0.8
    rgb, spp, m2, fin = ac.expected_from(w.chain, w.cases, ac.MAIN)
    at_min, between, at_max, lit = ac.classes(spp, rgb, w.cases.ok, ac.MAIN)
    print("%s: at min %.3f, between %.3f, at max %.3f; early and lit %.3f" % (name, at_min, between, at_max, lit))
    assert at_min >= 0.10 and between >= 0.10 and at_max >= 0.10 and lit >= 0.10
    assert (~w.cases.ok).sum() == 8 and (w.cases.seeds == 0).sum() <= 1


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------
def test_adaptive_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands
    assert ctypes.sizeof(api.Adaptive) == 20


def _caller(api, device_form):
    L = api.lib()

    def call(handle, rays, seeds, n, ad, rr, out, spp, m2, states, flags=0, stats=None):
        adp = ctypes.byref(api.Adaptive(*ad)) if ad is not None else None
        if device_form:
            return L.ort_radiance_adaptive_device(handle, rays, seeds, n, adp, rr, out, spp, m2, states, flags, None, stats)
        return L.ort_radiance_adaptive(handle, rays, seeds, n, adp, rr, out, spp, m2, states, flags, stats)
    return call


GOOD = tuple(ac.MAIN)   # any valid set: the errors do not depend on it


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_adaptive_errors_come_in_order(api, device_form, committed):
    """INVALID (nulls, misaligned pointers, the stopping rule's parameters, rr) on a committed-but-not-uploaded scene and on an
    uncommitted one; then the scene's state: STATE before NO_DEVICE"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form)
    keep = [_aligned(4 * 24), _aligned(16), _aligned(48), _aligned(16), _aligned(16), _aligned(16)]
    rays, seeds, out, spp, m2, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, rays, seeds, 4, GOOD, 0.8, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, None, seeds, 4, GOOD, 0.8, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, rays, None, 4, GOOD, 0.8, out, spp, m2, fin) == api.ERR_INVALID
    assert call(s.handle, rays, seeds, 4, GOOD, 0.8, None, spp, m2, fin) == api.ERR_INVALID
    for r, sd, o, sp, m, f in ((rays + 4, seeds, out, spp, m2, fin), (rays, seeds + 2, out, spp, m2, fin), (rays, seeds, out + 1, spp, m2, fin),
                               (rays, seeds, out, spp + 2, m2, fin), (rays, seeds, out, spp, m2 + 1, fin), (rays, seeds, out, spp, m2, fin + 2),
                               (rays + 2, seeds, out, None, None, None)):
        assert call(s.handle, r, sd, 4, None, 0.8, o, sp, m, f) == api.ERR_INVALID     # a misaligned pointer comes before ad
        assert b"aligned" in L.ort_last_error()
    assert call(s.handle, rays, seeds, 4, None, 2.0, out, spp, m2, fin) == api.ERR_INVALID
    assert b"ad" in L.ort_last_error() and b"rr" not in L.ort_last_error()
    nan, inf = float("nan"), float("inf")
    for bad, word in (((1, 64, 4, 0.3, 0.05), b"min_spp"), ((0, 64, 4, 0.3, 0.05), b"min_spp"), ((8, 7, 4, 0.3, 0.05), b"max_spp"),
                      ((4, (1 << 24) + 1, 4, 0.3, 0.05), b"1 << 24"), ((4, 64, 0, 0.3, 0.05), b"check_every"),
                      ((4, 64, 4, nan, 0.05), b"tolerance"), ((4, 64, 4, inf, 0.05), b"tolerance"), ((4, 64, 4, -0.5, 0.05), b"tolerance"),
                      ((4, 64, 4, 0.3, nan), b"floor"), ((4, 64, 4, 0.3, inf), b"floor"), ((4, 64, 4, 0.3, -1.0), b"floor")):
        assert call(s.handle, rays, seeds, 4, bad, 2.0, out, spp, m2, fin) == api.ERR_INVALID, bad   # ... and ad before rr
        assert word in L.ort_last_error(), (bad, L.ort_last_error())
    for rr in (1.0, 1.5, -0.25, nan, inf):
        assert call(s.handle, rays, seeds, 4, GOOD, rr, out, spp, m2, fin) == api.ERR_INVALID, rr
        assert b"rr" in L.ort_last_error()
    # all of these come before the scene's state; good arguments reach it, the limits of the parameters included
    assert call(s.handle, rays + 8, seeds + 4, 4, (2, 2, 1, 0.0, 0.0), 0.0, out + 4, None, None, None) == state
    assert call(s.handle, rays, seeds, 4, (2, 1 << 24, 0xFFFFFFFF, 1e30, 3e38), 0.999, out, spp, m2, fin, api.RENDER_COUNTERS) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_adaptive_empty_batch_is_ok(api, device_form):
    """count == 0: ORT_OK without a launch, whatever the other arguments"""
    call = _caller(api, device_form)
    keep_r, rays = _aligned(24)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, 0, None, 2.0, None, None, None, None) == api.OK
        assert call(s.handle, rays + 1, rays + 1, 0, (0, 0, 0, -1.0, -1.0), 0.8, rays + 1, rays + 1, rays + 1, rays + 1) == api.OK
    assert call(None, None, None, 0, GOOD, 0.8, None, None, None, None) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, 0, GOOD, 0.8, None, None, None, None, 0, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_adaptive_shapes(api):
    s = _scene(api)
    for bad in (np.zeros((3, 5), "<f4"), np.zeros(6, "<f4"), np.zeros((2, 3, 6), "<f4")):
        with pytest.raises(ValueError):
            s.radiance_adaptive(bad, np.ones(len(bad), "<u4"), 4, 64, 0.3)
    rays = np.zeros((3, 6), "<f4")
    for bad in (np.ones(2, "<u4"), np.ones((3, 1), "<u4"), 5):
        with pytest.raises(ValueError):
            s.radiance_adaptive(rays, bad, 4, 64, 0.3)
    with pytest.raises(ValueError):
        s.radiance_adaptive(rays, np.ones(3, "<u4"), -1, 64, 0.3)
    with pytest.raises(ValueError):
        s.radiance_adaptive(rays, np.ones(3, "<u4"), 4, 1 << 32, 0.3)
    with pytest.raises(api.OrtError) as e:
        s.radiance_adaptive(rays, np.ones(3, "<u4"), 4, 64, 0.3, want_states=True)
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.radiance_adaptive(rays, np.ones(3, "<u4"), 1, 64, 0.3)
    assert e.value.code == api.ERR_INVALID
    rgb, spp, m2, states, st = s.radiance_adaptive(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, 64, 0.3, want_states=True)
    assert rgb.shape == (0, 3) and rgb.dtype == np.dtype("<f4") and spp.shape == (0,) and spp.dtype == np.dtype("<u4")
    assert m2.shape == (0,) and m2.dtype == np.dtype("<f4") and states.shape == (0,) and st["paths"] == 0
    assert len(s.radiance_adaptive(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, 64, 0.3)) == 4
    with pytest.raises(api.OrtError) as e:
        s.radiance_adaptive_device(64, 64, 4, 4, 64, 0.3, 0.05, 4, 0.8, 64)
    assert e.value.code == api.ERR_NO_DEVICE


# ---- 4. the lane code on host threads ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,envs", [("c2_analytic", [{}, {"SIM_TABS": "1"}]),
                                       ("c3_bunny_room", [{"SIM_DIFFUSE": "1"}, {"SIM_TABS": "1", "SIM_DIFFUSE": "1"}, {}]),
                                       ("tables_mats_over", [{}])])
def test_host_sim_adaptive_is_the_oracles(host_sim, world, tmp_path, name, envs):
    """all four outputs, all bits (NaN by position): both BSDF flavours, the tables in LDS form and from their arrays; one thread
    and several; a check_every so large that the next check's count passes 2^32"""
    w = world(name)
    c = w.cases
    once = Adaptive(4, 64, 0xFFFFFFFC, 0.3, 0.05)
    want = {ad: ac.expected_from(w.chain, c, ad) for ad in ac.SETS + (once,)}
    assert ((want[once][1] == 4) | (want[once][1] == 64) | ~c.ok).all() and (want[once][1] == 64).any()
    for k, env in enumerate(envs):
        for ad, threads in ((ac.MAIN, 8), (ac.EVERY, 1), (ac.FIXED, 3), (once, 8)):
            if k and ad is not ac.MAIN:
                continue
            got = ac.host_sim(host_sim, tmp_path, w.scn, c.rays, c.seeds, ad, ac.RR, w.base, env=env, threads=threads)
            ac.assert_same(got, want[ad], "%s %r %r, %d threads" % (name, ad, env, threads))
    paths = hs.counters(hs.run(host_sim, ac.host_sim_args(str(tmp_path), w.scn, c.rays, c.seeds, ac.MAIN, ac.RR, w.base)[0]))["paths"]
    assert paths == int(want[ac.MAIN][1].sum())   # the counters' paths: the samples taken


@pytest.mark.parametrize("name", ["c2_analytic", "c3_bunny_room"])
def test_host_sim_identities_against_the_radiance_mode(host_sim, world, tmp_path, name):
    """min == max == n: the --radiance mode's colours and states at spp = n; a tolerance whose thr * thr is +inf (1e30, floor 1):
    every ray with finite Q stops at min_spp with that mode's results at spp = min_spp"""
    w = world(name)
    c = w.cases
    for n in (2, 5):
        rgb, fin = hs.radiance(host_sim, tmp_path, w.scn, c.rays, c.seeds, n, ac.RR, w.base, threads=4)
        got = ac.host_sim(host_sim, tmp_path, w.scn, c.rays, c.seeds, Adaptive(n, n, 1, 0.3, 0.05), ac.RR, w.base, threads=4)
        rc.assert_same(got[0], got[3], rgb, fin, "%s min = max = %d" % (name, n))
        assert (got[1][c.ok] == n).all() and (got[1][~c.ok] == 0).all()
    rgb, fin = hs.radiance(host_sim, tmp_path, w.scn, c.rays, c.seeds, 4, ac.RR, w.base, threads=4)
    got = ac.host_sim(host_sim, tmp_path, w.scn, c.rays, c.seeds, ac.HUGE, ac.RR, w.base, threads=4)
    assert np.isfinite(got[2]).all()
    rc.assert_same(got[0], got[3], rgb, fin, name + " huge tolerance")
    assert (got[1][c.ok] == 4).all()


# ---- 5. under the sanitizers --------------------------------------------------------------------------------------------------
def test_host_sim_adaptive_under_sanitizers(world, tmp_path):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly) on 64 rays: ends clean, with the oracle's answers"""
    san = hs.built("host_sim_san")
    w = world("c2_analytic")
    c = w.cases.take(np.arange(64))
    chain = {i: w.chain[i] for i in range(64) if i in w.chain}
    for env in ({}, {"SIM_TABS": "1"}):
        got = ac.host_sim(san, tmp_path, w.scn, c.rays, c.seeds, ac.MAIN, ac.RR, w.base, env=env, threads=2)
        ac.assert_same(got, ac.expected_from(chain, c, ac.MAIN), "sanitized %r" % env)
