"""SH light-probe queries (ort_probe_sh, ort_probe_sh_device), host side: the C ABI surface and its errors in the order
include/ort.h gives them, the point sets shown not to be vacuous, the sphere draw and the basis as the kernels compose them (unit
ops 21 and 22 through the lane code compiled for the host) against the oracle's composition and numpy, the lane code run on host
threads (tools/host_sim --probe-sh, plain and under the sanitizers) against identity I2 (rr = 0: the oracle's closed form) and
identity I1 (rr = 0.8: a chain of the existing --radiance mode at spp = 1), all bits (tests/probe_cases.py), and api.sh_basis and
api.sh_irradiance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import host_sim_tool as hs
import irradiance_cases as ic
import probe_cases as pc
import radiance_cases as rc
import ref_io
from conftest import DATA
from host_cases import aligned as _aligned, scene as _scene

NAMES = {"ort_probe_sh", "ort_probe_sh_device"}
SCENES = dict(pc.SCENES, c3_bunny_room=64)   # the bunny room: the diffuse flavour of the lane code, and a mesh
ENVS = {"testscene": [{}, {"SIM_TABS": "1"}], "c2_analytic": [{}, {"SIM_TABS": "1"}],
        "c3_bunny_room": [{"SIM_DIFFUSE": "1"}, {"SIM_TABS": "1", "SIM_DIFFUSE": "1"}]}
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
            w.pts = pc.point_set(name, w.flat, w.osc, SCENES[name])
            w.closed = pc.chain_closed_form(oracle, w.osc, w.flat, w.pts, pc.SPP)
            w.chain = None
            _worlds[name] = w
        return _worlds[name]
    return get


def composed_chain(w, oracle, host_sim, tmp_path):
    """identity I1 on the CPU: 8 chained calls of host_sim --radiance at spp = 1, rr = 0.8; computed once per scene"""
    if w.chain is None:
        w.chain = pc.chain_by_radiance(oracle, w.pts, pc.SPP, lambda rays, seeds: hs.radiance(host_sim, tmp_path, w.name, rays, seeds, 1, pc.RR, threads=8))
    return w.chain


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------------
def test_probe_entry_points_have_c_linkage(api):
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAMES <= names
    assert NAMES <= set(api.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(DATA), "include", "ort.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert "#define ORT_SH_COEFFS 9u" in hdr and "4 pi * out_sh" in hdr and api.SH_COEFFS == 9
    assert api.lib().ort_abi_version() == 3   # additive: the ABI version stands


def _caller(api, device_form):
    L = api.lib()

    def call(handle, pts, seeds, n, spp, rr, sh, rgb, states, flags=0, stats=None):
        if device_form:
            return L.ort_probe_sh_device(handle, pts, seeds, n, spp, rr, sh, rgb, states, flags, None, stats)
        return L.ort_probe_sh(handle, pts, seeds, n, spp, rr, sh, rgb, states, flags, stats)
    return call


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("committed", [True, False])
def test_probe_errors_come_in_order(api, device_form, committed):
    """ort_irradiance's order with out_sh as the required output: INVALID (nulls, misaligned pointers, spp == 0, rr outside
    [0, 1)), then STATE before NO_DEVICE; out_rgb and final_states may be NULL"""
    s = _scene(api, committed)
    L = api.lib()
    call = _caller(api, device_form)
    keep = [_aligned(4 * 24), _aligned(16), _aligned(4 * 108), _aligned(48), _aligned(16)]
    pts, seeds, sh, rgb, fin = (k[1] for k in keep)
    state = api.ERR_NO_DEVICE if committed else api.ERR_STATE
    assert call(None, pts, seeds, 4, 1, 0.8, sh, rgb, fin) == api.ERR_INVALID
    assert call(s.handle, None, seeds, 4, 1, 0.8, sh, rgb, fin) == api.ERR_INVALID
    assert b"points" in L.ort_last_error()
    assert call(s.handle, pts, None, 4, 1, 0.8, sh, rgb, fin) == api.ERR_INVALID
    assert call(s.handle, pts, seeds, 4, 1, 0.8, None, rgb, fin) == api.ERR_INVALID
    assert b"out_sh" in L.ort_last_error()
    for r, sd, o, c, f in ((pts + 4, seeds, sh, rgb, fin), (pts, seeds + 2, sh, rgb, fin), (pts, seeds, sh + 1, rgb, fin), (pts, seeds, sh, rgb + 2, fin),
                           (pts, seeds, sh, rgb, fin + 2), (pts + 2, seeds, sh, None, None)):
        assert call(s.handle, r, sd, 4, 0, 2.0, o, c, f) == api.ERR_INVALID      # a misaligned pointer comes before spp and rr
        assert b"aligned" in L.ort_last_error()
    assert call(s.handle, pts + 4, seeds, 4, 1, 0.8, None, rgb, fin) == api.ERR_INVALID
    assert b"null" in L.ort_last_error()                                        # ... and a null before a misaligned one
    assert call(s.handle, pts, seeds, 4, 0, 2.0, sh, rgb, fin) == api.ERR_INVALID
    assert b"spp" in L.ort_last_error()                                         # ... and spp before rr
    for rr in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert call(s.handle, pts, seeds, 4, 1, rr, sh, rgb, fin) == api.ERR_INVALID, rr
        assert b"rr" in L.ort_last_error()
    assert call(s.handle, pts + 8, seeds + 4, 4, 3, 0.0, sh + 4, None, None) == state
    assert call(s.handle, pts, seeds, 4, 1, 0.999, sh, rgb, fin, api.RENDER_COUNTERS) == state
    assert (b"commit" if not committed else b"upload") in L.ort_last_error()


@pytest.mark.parametrize("device_form", [False, True])
def test_probe_empty_batch_is_ok(api, device_form):
    """count == 0: ORT_OK without a launch, with nulls, whatever the other arguments"""
    call = _caller(api, device_form)
    keep_r, p = _aligned(24)
    for s in (_scene(api), _scene(api, committed=False)):
        assert call(s.handle, None, None, 0, 0, 2.0, None, None, None) == api.OK
        assert call(s.handle, p + 1, p + 1, 0, 1, 0.8, p + 1, p + 1, p + 1) == api.OK
    assert call(None, None, None, 0, 1, 0.8, None, None, None) == api.OK
    st = api.Stats()
    st.rays = 7
    assert call(_scene(api).handle, None, None, 0, 1, 0.8, None, None, None, 0, ctypes.byref(st)) == api.OK
    assert st.rays == 0


def test_python_probe_shapes(api):
    s = _scene(api)
    for bad in (np.zeros((3, 5), "<f4"), np.zeros(6, "<f4"), np.zeros((3, 2, 3), "<f4")):
        with pytest.raises(ValueError):
            s.probe_sh(bad, np.ones(len(bad), "<u4"), 1)
    with pytest.raises(ValueError):
        s.probe_sh(np.zeros((3, 6), "<f4"), np.ones(2, "<u4"), 1)
    for pts in (np.zeros((3, 6), "<f4"), np.zeros((3, 3), "<f4")):   # positions alone: the pole +z is filled in
        with pytest.raises(api.OrtError) as e:
            s.probe_sh(pts, np.ones(3, "<u4"), 2, want_rgb=True, want_states=True)
        assert e.value.code == api.ERR_NO_DEVICE
        with pytest.raises(api.OrtError) as e:
            s.probe_sh(pts, np.ones(3, "<u4"), 0)
        assert e.value.code == api.ERR_INVALID
    assert (api._probe_points(np.ones((2, 3), "<f4")) == np.array([[1, 1, 1, 0, 0, 1]] * 2, "<f4")).all()
    sh, st = s.probe_sh(np.zeros((0, 3), "<f4"), np.zeros(0, "<u4"), 4)
    assert sh.shape == (0, 9, 3) and sh.dtype == np.dtype("<f4") and st["paths"] == 0
    sh, rgb, states, st = s.probe_sh(np.zeros((0, 6), "<f4"), np.zeros(0, "<u4"), 4, want_rgb=True, want_states=True)
    assert rgb.shape == (0, 3) and states.shape == (0,) and states.dtype == np.dtype("<u4")
    with pytest.raises(api.OrtError) as e:
        s.probe_sh_device(64, 64, 4, 1, 0.8, 64)
    assert e.value.code == api.ERR_NO_DEVICE


# ---- 2. the point sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_point_sets_are_not_vacuous(world, oracle, host_sim, tmp_path, name):
    """rr = 0.8, spp = 8, on the composed chain: at least 5 % of the points inside the domain have both a sample that adds light and
    one that does not, and at least one point adds light at a bounce (nothing else tests the cached direction); every kind of point
    the set promises is there"""
    w = world(name)
    p = w.pts
    chain = composed_chain(w, oracle, host_sim, tmp_path)
    mixed, bounced = pc.mixed_share(chain), pc.lit_at_a_bounce(chain, w.osc, w.flat, p)
    print("%s: mixed %.3f (closed form %.3f), lit at a bounce %d of %d points inside the domain" % (name, mixed, pc.mixed_share(w.closed), len(bounced), p.ok.sum()))
    assert mixed >= 0.05 and pc.mixed_share(w.closed) >= 0.05
    assert len(bounced) >= 1
    assert not pc.lit_at_a_bounce(w.closed, w.osc, w.flat, p)   # the helper itself: without bounces nothing is lit at one
    assert (~p.ok).sum() == 8 and p.far.sum() == 8 and p.ok[p.far].all()
    n = p.points[p.ok, 3:6]
    for z in ic.LOBE_Z:
        assert (n[:, 2] == np.float32(z)).any(), z
    for pole in ((0, 0, 1), (0, 0, -1), pc.TILTED):
        assert (n == np.asarray(pole, "<f4")).all(axis=1).sum() >= 4, pole
    assert (p.seeds == 0).sum() == 1 and (p.seeds == 0xFFFFFFFF).sum() == 1 and p.ok[p.seeds == 0].all()
    one = np.flatnonzero(p.seeds == rc.unstep(0xFFFFFFFF))
    assert len(one) == 1 and p.ok[one[0]] and ic.draws(oracle, p.seeds[one])[0][0] == np.float32(1.0)
    # ... whose first direction is the pole's opposite: c = -1
    d = w.closed[int(one[0])][2][0]
    pole = p.points[one[0], 3:6] / np.linalg.norm(p.points[one[0], 3:6])
    assert np.abs(d + pole).max() < 1e-6


# ---- 3. the sphere draw and the basis as the kernels compose them -------------------------------------------------------------
def test_host_op21_is_the_oracles_composition(host_sim, world, oracle, tmp_path):
    rng = np.random.default_rng(21)
    normals, seeds = [rc._units(rng, 256)], [rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype("<u4")]
    for name in pc.SCENES:
        p = world(name).pts
        normals.append(p.points[p.ok, 3:6])
        seeds.append(p.seeds[p.ok])
    seeds, normals = np.concatenate(seeds), np.concatenate(normals).astype("<f4")
    assert (seeds == 0).any() and (seeds == 0xFFFFFFFF).any() and (seeds == rc.unstep(0xFFFFFFFF)).any() and (normals[:, 2] == -1).any()
    ref_io.make_unit_records(21, ic.op20_rows(seeds, normals)).tofile(str(tmp_path / "in.bin"))
    hs.run(host_sim, ["--unit", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = ref_io.read_unit_output(str(tmp_path / "out.bin"))
    pc.assert_bits(got, pc.op21_expected(oracle, seeds, normals), "op 21 on the host")
    # the draw covers the sphere: about half of the directions point away from the pole (op 20's never do)
    cos = (got[:, 0:3] * normals).sum(axis=1) / np.linalg.norm(normals, axis=1)
    assert 0.35 < (cos < 0).mean() < 0.65


def test_sh_basis_is_op22(api, host_sim, tmp_path):
    """api.sh_basis, probe_cases.basis and the lane code's own basis (unit op 22, compiled for the host): the same bits"""
    d = pc.op22_directions()
    ref_io.make_unit_records(22, d).tofile(str(tmp_path / "in.bin"))
    hs.run(host_sim, ["--unit", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = ref_io.read_unit_output(str(tmp_path / "out.bin"))
    want = pc.basis(d)
    pc.assert_bits(got, want[:, 1:9], "op 22 on the host")
    b = api.sh_basis(d)
    assert b.shape == (len(d), 9) and b.dtype == np.dtype("<f4")
    pc.assert_bits(b, want, "api.sh_basis")
    assert api.sh_basis(d[0]).shape == (9,) and api.sh_basis(d.reshape(4, -1, 3)).shape == (4, len(d) // 4, 9)
    with pytest.raises(ValueError):
        api.sh_basis(np.zeros((3, 2), "<f4"))
    # orthonormal over the sphere: the mean of b_i b_j over a fine grid is delta_ij / (4 pi)
    t, ph = np.meshgrid(np.arccos(1 - 2 * (np.arange(400) + 0.5) / 400), 2 * np.pi * (np.arange(800) + 0.5) / 800, indexing="ij")
    g = api.sh_basis(np.stack([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.cos(t)], axis=-1).reshape(-1, 3)).astype(np.float64)
    assert np.abs(g.T @ g / len(g) * 4 * np.pi - np.eye(9)).max() < 1e-4


def test_sh_irradiance_closed_forms(api):
    """constant radiance L gives pi L for every normal; L(d) = a + b (d . u) gives pi a + (2 pi / 3) b (n . u): both to 1e-6
    relative (the coefficients are the exact projections, the float32 constants carry 8 digits)"""
    rng = np.random.default_rng(7)
    normals = np.concatenate([rc._units(rng, 64), np.eye(3), -np.eye(3)])
    L = np.array([0.75, 2.5, 0.125])
    sh = np.zeros((9, 3))
    sh[0] = 0.282094792 * L                         # the mean of Y0 * L over the sphere
    got = api.sh_irradiance(np.broadcast_to(sh, (len(normals), 9, 3)), normals)
    assert got.shape == (len(normals), 3) and got.dtype == np.float64
    assert np.abs(got / (np.pi * L) - 1).max() < 1e-6
    assert np.abs(api.sh_irradiance(sh, normals[0]) / (np.pi * L) - 1).max() < 1e-6
    u = np.array([0.48, -0.6, 0.64])
    a, b = np.array([1.5, 0.5, 3.0]), np.array([0.5, 0.25, -1.0])
    sh = np.zeros((9, 3))
    sh[0] = 0.282094792 * a
    # the mean of Y_1m(d) * b (d . u) over the sphere is 0.488602512 * b * u_m / 3 (m: y, z, x)
    for j, um in ((1, u[1]), (2, u[2]), (3, u[0])):
        sh[j] = 0.488602512 * b * um / 3.0
    want = np.pi * a[None, :] + (2 * np.pi / 3) * b[None, :] * (normals @ u)[:, None]
    got = api.sh_irradiance(np.broadcast_to(sh, (len(normals), 9, 3)), normals)
    assert (want > 0.3).all() and np.abs(got / want - 1).max() < 1e-6
    with pytest.raises(ValueError):
        api.sh_irradiance(np.zeros((4, 8, 3)), normals[:4])


# ---- 4. the lane code on host threads -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_host_sim_without_bounces_is_the_oracles_closed_form(host_sim, world, tmp_path, name):
    """identity I2, rr = 0, spp 1 and 8: all 27 coefficients, the mean and the final states, tables from LDS form and from their
    arrays; the counters' paths; out and states not passed leave the coefficients as they are"""
    w = world(name)
    p = w.pts
    for spp in (1, pc.SPP):
        want = pc.expected_from(w.closed, p, spp)
        for env in ENVS[name]:
            got, r = pc.host_sim(host_sim, tmp_path, name, p.points, p.seeds, spp, 0.0, env=env, threads=8)
            pc.assert_same(got, want, "%s rr 0 spp %d %r" % (name, spp, env))
            assert hs.counters(r)["paths"] == spp * int(p.ok.sum())
    got, _ = pc.host_sim(host_sim, tmp_path, name, p.points, p.seeds, pc.SPP, 0.0, want_rgb=False, want_states=False, env=ENVS[name][0], threads=8)
    pc.assert_same(got, (want[0], None, None), name + " without rgb and states")
    assert np.isnan(want[0][~p.ok]).all() and (want[2][~p.ok] == p.seeds[~p.ok]).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_host_sim_is_a_chain_of_radiance_samples(host_sim, world, oracle, tmp_path, name):
    """identity I1, rr = 0.8, spp 1 and 8: the --probe-sh mode against chained calls of the --radiance mode at spp = 1"""
    w = world(name)
    p = w.pts
    chain = composed_chain(w, oracle, host_sim, tmp_path)
    for spp in (1, pc.SPP):
        want = pc.expected_from(chain, p, spp)
        for k, env in enumerate(ENVS[name]):
            if k and spp == 1:
                continue
            got, _ = pc.host_sim(host_sim, tmp_path, name, p.points, p.seeds, spp, pc.RR, env=env, threads=8 if k == 0 else 3)
            pc.assert_same(got, want, "%s rr 0.8 spp %d %r" % (name, spp, env))
    # one thread, the points in another order: a point's answer is its own
    perm = np.random.default_rng(4).permutation(len(p.points))
    got, _ = pc.host_sim(host_sim, tmp_path, name, p.points[perm], p.seeds[perm], pc.SPP, pc.RR, env=ENVS[name][0], threads=1)
    pc.assert_same(got, tuple(a[perm] for a in want), name + " permuted")


# ---- 5. under the sanitizers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.SCENES))
def test_host_sim_probe_under_sanitizers(host_sim, world, oracle, tmp_path, name):
    """tools/host_sim_san (the stand-alone ASan + UBSan binary, run directly): ends clean, with both chains' answers"""
    san = hs.built("host_sim_san")
    w = world(name)
    p = w.pts
    for env in ENVS[name]:
        got, _ = pc.host_sim(san, tmp_path, name, p.points, p.seeds, pc.SPP, 0.0, env=env, threads=4)
        pc.assert_same(got, pc.expected_from(w.closed, p, pc.SPP), "sanitized %s rr 0 %r" % (name, env))
    chain = composed_chain(w, oracle, host_sim, tmp_path)
    got, _ = pc.host_sim(san, tmp_path, name, p.points, p.seeds, pc.SPP, pc.RR, env=ENVS[name][1], threads=4)
    pc.assert_same(got, pc.expected_from(chain, p, pc.SPP), "sanitized %s rr 0.8" % name)
    got, _ = pc.host_sim(san, tmp_path, name, p.points[:5], p.seeds[:5], 3, pc.RR, want_rgb=False, want_states=False, env=ENVS[name][0], threads=1)
    pc.assert_same(got, (pc.expected_from(chain, p, 3)[0][:5], None, None), "sanitized %s without rgb and states" % name)
