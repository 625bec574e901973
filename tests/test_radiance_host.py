"""Radiance queries (ort_radiance / ort_radiance_device), host side: the helper that turns the oracle into their reference
(tests/radiance_cases.py) pinned against the oracle itself, the C ABI surface, and the argument and state errors in the order
include/ort.h gives them -- all reported before any device work, so they are the same on a machine without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import radiance_cases as rc
from conftest import DATA, assert_bits_equal
from host_cases import aligned as _aligned, scene as _scene

NAMES = {"ort_radiance", "ort_radiance_device"}


# ---- the helper -------------------------------------------------------------------------------------------------------------
def test_unstep_inverts_the_oracles_step(oracle):
    for seed in (1, 2, 0x80000000, 0xFFFFFFFF, 2024, 0x9E3779B9):
        tab = np.frombuffer(oracle.rng_table(seed, 64)[: 64 * 8], "<u4").reshape(64, 2)[:, 0]   # the state after each rng_01
        prev = seed
        for s in tab:
            assert rc.step(prev) == int(s)
            assert rc.unstep(int(s)) == prev
            prev = int(s)
    rng = np.random.default_rng(1)
    for x in rng.integers(0, 1 << 32, 2000):
        assert rc.unstep(rc.step(int(x))) == int(x) and rc.step(rc.unstep(int(x))) == int(x)


@pytest.fixture(scope="module")
def room(api, oracle, load_scene):
    scene = load_scene("c2_analytic")
    flat = scene.flatten(1, 1)
    return flat, oracle.OracleScene(flat)


def test_one_call_of_three_samples_is_three_chained_calls(room):
    """the oracle's pixel of a pinhole camera at spp = 3 == three spp = 1 calls chained through the returned state, their
    colours summed in float32 in sample order and divided by float32(3) (mean_of), final state included: how expected()
    combines samples is how the oracle does.  What expected() changes is only where each sample's stream starts: two steps
    back, over the aperture draw a radiance query does not make"""
    flat, osc = room
    rng = np.random.default_rng(11)
    lo, hi = rc.origin_box(flat)
    cams = np.concatenate([rc.inside(rng, lo, hi, 40), rc.axis_aligned(rng, lo, hi, 12)])
    seeds = rng.integers(1, 1 << 32, len(cams), dtype=np.uint64).astype("<u4")
    lit = 0
    for i, (p, z) in enumerate(cams):
        osc.set_camera(rc.camera_of(p, z))
        whole = np.zeros((1, 1, 3), "<f4")
        _, end = osc.tiled_raytrace(whole, 0, 0, 1, 1, int(seeds[i]), 3, 0.8)
        cols, s = np.zeros((3, 3), "<f4"), int(seeds[i])
        img = np.zeros((1, 1, 3), "<f4")
        for k in range(3):
            _, s = osc.tiled_raytrace(img, 0, 0, 1, 1, s, 1, 0.8)
            cols[k] = img[0, 0]
        assert_bits_equal(rc.mean_of(cols), whole[0, 0], "ray %d" % i)
        assert s == end
        lit += bool(whole.any())
        # and a link of expected()'s chain is such a call started two steps early
        start = rc.step(rc.step(int(seeds[i])))
        one, fin = rc.expected(osc, cams[i:i + 1], np.array([start], "<u4"), 1, 0.8)
        osc.set_camera(rc.camera_of(p, z))
        _, s1 = osc.tiled_raytrace(img, 0, 0, 1, 1, int(seeds[i]), 1, 0.8)
        assert_bits_equal(one[0], img[0, 0], "ray %d, first link" % i)
        assert fin[0] == s1
    assert lit >= len(cams) // 10


def test_pinhole_is_the_oracles_primary_ray(room):
    """rr = 0: no path bounces, so the value is the emission of what oracle.raycast(o, d) hits if that is a light, else 0; and
    the final state is the seed (light or miss: no roulette draw) or one step on"""
    flat, osc = room
    rng = np.random.default_rng(5)
    lo, hi = rc.origin_box(flat)
    cams = np.concatenate([rc.inside(rng, lo, hi, 150), rc.axis_aligned(rng, lo, hi, 24), rc.outside(rng, lo, hi, 24),
                           rc.probes(rng, osc, lo, hi, 24)])
    od = [rc.pinhole(p, z) for p, z in cams]
    o, d = np.array([a for a, _ in od]), np.array([b for _, b in od])
    l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype("<f4")
    assert ((l2 >= np.float32(0.999)) & (l2 <= np.float32(1.001))).all() and np.isfinite(o).all()
    seeds = rng.integers(1, 1 << 32, len(cams), dtype=np.uint64).astype("<u4")
    rgb, fin = rc.expected(osc, cams, seeds, 1, 0.0)
    t, _, mat = osc.raycast(o, d)
    lights = 0
    for i in range(len(cams)):
        m = flat.materials[mat[i]]
        ends = mat[i] == 0 or m["is_light"]
        want = m["emit"] if (mat[i] != 0 and m["is_light"]) else np.zeros(3, "<f4")
        assert_bits_equal(rgb[i], want, "ray %d (material %d)" % (i, mat[i]))
        assert fin[i] == (int(seeds[i]) if ends else rc.step(int(seeds[i])))
        lights += bool(mat[i] != 0 and m["is_light"])
    assert lights >= 3 and (mat != 0).sum() > len(cams) // 2


def test_mixed_cases_meet_their_conditions_on_a_room(room):
    flat, osc = room
    cases = rc.mixed("c2_analytic", flat, osc, 96)
    assert cases.ok.sum() == 88 and (cases.rays[cases.ok, 3:6] == 0).any()
    want = rc.expected_of(osc, cases, (1, 3), 0.8)
    rgb, fin = want[1]
    assert np.isnan(rgb[~cases.ok]).all() and (fin[~cases.ok] == cases.seeds[~cases.ok]).all()
    assert not np.isnan(rgb[cases.ok]).any()
    assert (want[3][0][cases.ok] != 0).any(axis=1).mean() >= 0.10
    assert rc.survives_primary(cases.seeds, fin)[cases.ok].mean() >= 0.25


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_radiance_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands


def test_job_seeds_are_the_oracles(api, oracle):
    for master in (0, 1, 2024, 0xFFFFFFFF, 0x9E3779B9):
        got = api.job_seeds(master, 300)
        assert got.dtype == np.dtype("<u4") and got.shape == (300,)
        assert got.tolist() == [oracle.job_seed(master, i) for i in range(300)]
    assert len(api.job_seeds(7, 0)) == 0


def _caller(api, device_form):
    L = api.lib()

    def call(handle, rays, seeds, n, spp, rr, out, states, flags=0, stats=None):
        if device_form:
            return L.ort_radiance_device(handle, rays, seeds, n, spp, rr, out, states, flags, None, stats)
        return L.ort_radiance(handle, rays, seeds, n, spp, rr, out, states, flags, stats)
    return call


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_radiance_errors_come_in_order(api, device_form, committed):
    """INVALID (nulls, misaligned pointers, spp == 0, rr outside [0, 1)) on a committed-but-not-uploaded scene and on an
    uncommitted one; then the scene's state: STATE before NO_DEVICE"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form)
    keep_r, rays = _aligned(4 * 24)
    keep_s, seeds = _aligned(4 * 4)
    keep_o, out = _aligned(4 * 12)
    keep_f, fin = _aligned(4 * 4)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, rays, seeds, 4, 1, 0.8, out, fin) == api.ERR_INVALID
    assert call(s.handle, None, seeds, 4, 1, 0.8, out, fin) == api.ERR_INVALID
    assert call(s.handle, rays, None, 4, 1, 0.8, out, fin) == api.ERR_INVALID
    assert call(s.handle, rays, seeds, 4, 1, 0.8, None, fin) == api.ERR_INVALID
    for r, sd, o, f in ((rays + 4, seeds, out, fin), (rays, seeds + 2, out, fin), (rays, seeds, out + 1, fin), (rays, seeds, out, fin + 2),
                        (rays + 2, seeds, out, None)):
        assert call(s.handle, r, sd, 4, 1, 0.8, o, f) == api.ERR_INVALID
        assert b"aligned" in L.ort_last_error()
    assert call(s.handle, rays, seeds, 4, 0, 0.8, out, fin) == api.ERR_INVALID
    assert b"spp" in L.ort_last_error()
    for rr in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert call(s.handle, rays, seeds, 4, 1, rr, out, fin) == api.ERR_INVALID, rr
        assert b"rr" in L.ort_last_error()
    # a null scene, a bad spp and a bad rr all come before the scene's state; good arguments reach it
    assert call(s.handle, rays + 8, seeds + 4, 4, 3, 0.0, out + 4, None) == state
    assert call(s.handle, rays, seeds, 4, 1, 0.999, out, fin, api.RENDER_COUNTERS) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_radiance_empty_batch_is_ok(api, device_form):
    """count == 0: ORT_OK without a launch, whatever the other arguments"""
    call = _caller(api, device_form)
    keep_r, rays = _aligned(24)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, 0, 0, 2.0, None, None) == api.OK
        assert call(s.handle, rays + 1, rays + 1, 0, 1, 0.8, rays + 1, rays + 1) == api.OK
    assert call(None, None, None, 0, 1, 0.8, None, None) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, 0, 1, 0.8, None, None, 0, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_radiance_shapes(api):
    s = _scene(api)
    for bad in (np.zeros((3, 5), "<f4"), np.zeros(6, "<f4"), np.zeros((2, 3, 6), "<f4")):
        with pytest.raises(ValueError):
            s.radiance(bad, np.ones(len(bad), "<u4"), 1)
    rays = np.zeros((3, 6), "<f4")
    for bad in (np.ones(2, "<u4"), np.ones((3, 1), "<u4"), 5):
        with pytest.raises(ValueError):
            s.radiance(rays, bad, 1)
    with pytest.raises(api.OrtError) as e:
        s.radiance(rays, np.ones(3, "<u4"), 2, want_states=True)
    assert e.value.code == api.ERR_NO_DEVICE
    with pytest.raises(api.OrtError) as e:
        s.radiance(rays, np.ones(3, "<u4"), 0)
    assert e.value.code == api.ERR_INVALID
    rgb, states, st = s.radiance(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, want_states=True)
    assert rgb.shape == (0, 3) and rgb.dtype == np.dtype("<f4") and states.shape == (0,) and st["paths"] == 0
    rgb, st = s.radiance(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4)
    assert rgb.shape == (0, 3)
    with pytest.raises(api.OrtError) as e:
        s.radiance_device(64, 64, 4, 1, 0.8, 64)
    assert e.value.code == api.ERR_NO_DEVICE
