"""SH light-probe queries on the device (ort_probe_sh, ort_probe_sh_device; kernels probe_sh_points): radiance over the sphere as
nine SH coefficients per colour channel, held against what exists (tests/probe_cases.py) -- identity I2 (rr = 0: the oracle's
closed form), identity I1 (rr = 0.8: a chain of ort_radiance calls at spp = 1 along directions composed from the oracle), the
basis and the fold in numpy float32.  All bits of every output; NaN outputs compare by position."""
import zlib

import numpy as np
import pytest

import irradiance_cases as ic
import probe_cases as pc
import radiance_cases as rc
import ref_io

pytestmark = pytest.mark.gpu

# testscene and c2_analytic hold specular materials (the all-lobes kernels); the bunny room is diffuse only (the diffuse kernels)
SCENES = dict(pc.SCENES, c3_bunny_room=64)
RR, SPP = pc.RR, pc.SPP
_worlds = {}


class World:
    pass


@pytest.fixture()
def world(api, oracle, gpu_scene):
    """name -> the uploaded scene, its points, the oracle's closed form of 8 samples at rr = 0 and (filled on demand) the chain of
    ort_radiance calls at rr = 0.8; computed once"""
    def get(name):
        if name not in _worlds:
            w = World()
            w.name, w.scene = name, gpu_scene(name)
            w.flat = w.scene.flatten(1, 1)
            w.osc = oracle.OracleScene(w.flat)
            w.pts = pc.point_set(name, w.flat, w.osc, SCENES[name])
            w.closed = pc.chain_closed_form(oracle, w.osc, w.flat, w.pts, SPP)
            w.chain = None
            _worlds[name] = w
        return _worlds[name]
    return get


def radiance_chain(w, oracle):
    """identity I1's reference: 8 chained ort_radiance calls at spp = 1"""
    if w.chain is None:
        def one(rays, seeds):
            rgb, fin, _ = w.scene.radiance(rays, seeds, 1, RR, want_states=True)
            return rgb, fin
        w.chain = pc.chain_by_radiance(oracle, w.pts, SPP, one)
    return w.chain


# ---- 1. the host form against both chains, every kernel variant ------------------------------------------------------------------
@pytest.mark.parametrize("tables", [True, False], ids=["tables in LDS", "tables in HBM"])
@pytest.mark.parametrize("name", list(SCENES))
def test_host_form_is_both_chains(world, oracle, monkeypatch, name, tables):
    """rr = 0 against the closed form at spp 1 and 8, rr = 0.8 against the chain of ort_radiance samples at spp 8; each with and
    without ORT_RENDER_COUNTERS (the same bits; paths = points inside the domain x spp).  Scenes x tables x counters: the eight
    kernels probe_sh_points<COUNTERS, DIFFUSE, TABS>"""
    w = world(name)
    p = w.pts
    chain = radiance_chain(w, oracle)   # with the tables where the plan puts them: the reference is the radiance query as it ships
    if not tables:
        monkeypatch.setenv("ORT_LDS_TABLES", "0")
    inside = int(p.ok.sum())
    for rr, spp, want in ((0.0, 1, pc.expected_from(w.closed, p, 1)), (0.0, SPP, pc.expected_from(w.closed, p, SPP)), (RR, SPP, pc.expected_from(chain, p, SPP))):
        for counters in (False, True):
            sh, rgb, fin, st = w.scene.probe_sh(p.points, p.seeds, spp, rr, want_rgb=True, want_states=True, counters=counters)
            pc.assert_same((sh, rgb, fin), want, "%s rr %g spp %d counters %d" % (name, rr, spp, counters))
            assert st["kernel_ms"] > 0 and st["paths"] == (inside * spp if counters else 0)
    assert np.isnan(sh[~p.ok]).all() and np.isnan(rgb[~p.ok]).all() and (fin[~p.ok] == p.seeds[~p.ok]).all()
    if name in pc.SCENES:   # the sets test what they claim to
        assert pc.mixed_share(chain) >= 0.05 and len(pc.lit_at_a_bounce(chain, w.osc, w.flat, p)) >= 1


def test_positions_alone_take_the_pole_plus_z(world):
    w = world("testscene")
    idx = np.flatnonzero(w.pts.ok & ~w.pts.far)[:32]
    pos = w.pts.points[idx, 0:3]
    with_pole = np.concatenate([pos, np.tile(np.array([0, 0, 1], "<f4"), (len(pos), 1))], axis=1)
    a, _ = w.scene.probe_sh(pos, w.pts.seeds[idx], 4, RR)
    b, _ = w.scene.probe_sh(with_pole, w.pts.seeds[idx], 4, RR)
    assert a.shape == (len(pos), 9, 3) and a.tobytes() == b.tobytes() and (a != 0).any()


# ---- 2. the sphere draw and the basis as the kernels compose them ---------------------------------------------------------------
def test_op21_on_the_device_is_the_oracles_composition(api, world, oracle):
    rng = np.random.default_rng(21)
    p = world("c2_analytic").pts
    normals = np.concatenate([rc._units(rng, 256), p.points[p.ok, 3:6]]).astype("<f4")
    seeds = np.concatenate([rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype("<u4"), p.seeds[p.ok]])
    assert (seeds == 0).any() and (seeds == 0xFFFFFFFF).any() and (seeds == rc.unstep(0xFFFFFFFF)).any()
    assert (normals == np.array([0, 0, 1], "<f4")).all(axis=1).any() and (normals == np.array([0, 0, -1], "<f4")).all(axis=1).any()
    got = api.unit_eval_device(ref_io.make_unit_records(21, ic.op20_rows(seeds, normals)))
    pc.assert_bits(got, pc.op21_expected(oracle, seeds, normals), "op 21 on the device")


def test_op22_on_the_device_is_the_numpy_basis(api):
    """axis directions, +-0 components and a subnormal component among them; the sign of a zero counts"""
    d = pc.op22_directions()
    assert (d == 0).any() and np.signbit(d[d == 0]).any() and ((d != 0) & (np.abs(d) < 1e-38)).any()
    got = api.unit_eval_device(ref_io.make_unit_records(22, d))
    want = pc.basis(d)
    pc.assert_bits(got, want[:, 1:9], "op 22 on the device")
    pc.assert_bits(api.sh_basis(d), want, "api.sh_basis")


# ---- 3. the device form ------------------------------------------------------------------------------------------------------------
GUARD = 8   # words in front of and behind every output


def torch_probe(scene, points, seeds, spp, rr, skip=(), counters=False, want_stats=False):
    """the device form with torch tensors on a non-default stream, every output between guard words; without stats the call does
    not wait: synchronise.  -> ((sh, rgb, states) with their guards, flat), stats); the outputs in `skip` are not passed"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(points)
    d_pts = torch.from_numpy(np.ascontiguousarray(points, "<f4")).to(dev)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds, "<u4").view("<i4")).to(dev)
    d_sh = torch.full((27 * n + 2 * GUARD,), -7.0, dtype=torch.float32, device=dev)
    d_rgb = torch.full((3 * n + 2 * GUARD,), -7.0, dtype=torch.float32, device=dev)
    d_fin = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ptr = lambda t, what: 0 if what in skip else t.data_ptr() + 4 * GUARD
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        st = scene.probe_sh_device(d_pts.data_ptr(), d_seeds.data_ptr(), n, spp, rr, ptr(d_sh, "sh"), ptr(d_rgb, "rgb"), ptr(d_fin, "states"),
                                   stream=stream.cuda_stream, counters=counters, want_stats=want_stats)
    stream.synchronize()
    return (d_sh.cpu().numpy(), d_rgb.cpu().numpy(), d_fin.cpu().numpy().view("<u4")), st


def inner(a, per):
    return a[GUARD:-GUARD].reshape(-1, per) if per > 1 else a[GUARD:-GUARD]


def guards_stand(a, fill):
    return (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all()


@pytest.mark.parametrize("count", [1, 65, 321])
def test_device_form_on_a_stream_between_guard_words(world, oracle, count):
    """rr = 0.8 against the chain: all three outputs and nothing beyond them; out_rgb and final_states NULL, one and both, leave
    out_sh unchanged and themselves unwritten; the counters' paths"""
    w = world("c2_analytic")
    chain = radiance_chain(w, oracle)
    idx = np.arange(count) % len(w.pts.points)
    p = w.pts.take(idx)
    want = pc.expected_from({j: chain[int(i)] for j, i in enumerate(idx) if int(i) in chain}, p, SPP)
    (sh, rgb, fin), st = torch_probe(w.scene, p.points, p.seeds, SPP, RR)
    assert st is None
    pc.assert_same((inner(sh, 27), inner(rgb, 3), inner(fin, 1)), want, "device form, %d points" % count)
    assert guards_stand(sh, np.float32(-7.0)) and guards_stand(rgb, np.float32(-7.0)) and guards_stand(fin, 0x5A5A5A5A)
    for skip in (("rgb",), ("states",), ("rgb", "states")):
        (sh2, rgb2, fin2), st = torch_probe(w.scene, p.points, p.seeds, SPP, RR, skip=skip, counters=True, want_stats=True)
        assert st["paths"] == SPP * int(p.ok.sum())
        assert sh2.tobytes() == sh.tobytes(), skip
        assert (rgb2 == np.float32(-7.0)).all() if "rgb" in skip else rgb2.tobytes() == rgb.tobytes()
        assert (fin2 == 0x5A5A5A5A).all() if "states" in skip else (fin2 == fin).all()


def test_a_point_outside_the_domain_leaves_its_neighbours_alone(world):
    """every second point made a point outside the domain: NaN in its 27 words and its mean, its seed back -- and the points between
    them keep the bits they have in a batch without such points"""
    w = world("testscene")
    idx = np.flatnonzero(w.pts.ok & ~w.pts.far)[:48]
    pts, seeds = w.pts.points[idx].copy(), w.pts.seeds[idx]
    (sh, rgb, fin), _ = torch_probe(w.scene, pts, seeds, SPP, RR)
    bad = ic.out_of_domain(np.random.default_rng(5), *rc.origin_box(w.flat), 24)
    pts[1::2] = bad
    (sh2, rgb2, fin2), _ = torch_probe(w.scene, pts, seeds, SPP, RR)
    a, b = inner(sh, 27), inner(sh2, 27)
    assert a[0::2].tobytes() == b[0::2].tobytes() and np.isnan(b[1::2]).all() and not np.isnan(b[0::2]).any()
    assert inner(rgb, 3)[0::2].tobytes() == inner(rgb2, 3)[0::2].tobytes() and np.isnan(inner(rgb2, 3)[1::2]).all()
    assert (inner(fin, 1)[0::2] == inner(fin2, 1)[0::2]).all() and (inner(fin2, 1)[1::2] == seeds[1::2]).all()
    assert guards_stand(sh2, np.float32(-7.0)) and guards_stand(rgb2, np.float32(-7.0)) and guards_stand(fin2, 0x5A5A5A5A)


# ---- 4. more jobs than resident lanes --------------------------------------------------------------------------------------------
MANY, MANY_SPP, SLICE, SUBSET = 786432, 2, 65536, 512


def many_points(w):
    """-> points (MANY, 6), seeds (MANY,): 4 096 distinct points -- half near a light, the rest anywhere inside the scene's box, any
    pole, 16 outside the domain -- tiled, every copy on a seed of its own"""
    rng = np.random.default_rng(zlib.crc32(b"many probes"))
    lo, hi = rc.origin_box(w.flat)
    base, k = 4096, (4096 - 16) // 2
    anywhere = np.concatenate([rng.uniform(lo, hi, size=(base - 16 - k, 3)), rc._units(rng, base - 16 - k)], axis=1)
    pts = np.concatenate([ic.near_lights(rng, w.flat, lo, hi, k), anywhere, ic.out_of_domain(rng, lo, hi, 16)]).astype("<f4")
    pts = pts[rng.permutation(base)]
    return np.ascontiguousarray(pts[np.arange(MANY) % base]), rng.integers(0, 1 << 32, MANY, dtype=np.uint64).astype("<u4")


def test_more_points_than_resident_lanes(world, oracle):
    """786 432 points at spp = 2, rr = 0, the host form (staged in slices of its own): a fixed random subset of 512 against the
    closed form, and every point against the same call given in slices of 65 536 -- slicing, order and lanes change no bit"""
    w = world("c2_analytic")
    pts, seeds = many_points(w)
    sh, rgb, fin, st = w.scene.probe_sh(pts, seeds, MANY_SPP, 0.0, want_rgb=True, want_states=True, counters=True)
    ok = ic.in_domain(pts)
    assert st["paths"] == MANY_SPP * int(ok.sum()) and np.isnan(sh[~ok]).all() and not np.isnan(sh[ok]).any()
    sub = np.sort(np.random.default_rng(512).choice(MANY, SUBSET, replace=False))
    sub[:8] = np.flatnonzero(~ok)[:8]   # ... with points outside the domain among them
    p = ic.Points(pts[sub], seeds[sub], ok[sub], np.zeros(SUBSET, bool))
    want = pc.expected_from(pc.chain_closed_form(oracle, w.osc, w.flat, p, MANY_SPP), p, MANY_SPP)
    pc.assert_same((sh[sub], rgb[sub], fin[sub]), want, "a subset of %d of %d points" % (SUBSET, MANY))
    assert (want[0][p.ok] != 0).any(axis=(1, 2)).mean() >= 0.05   # by the oracle: the subset is not black (two samples over the whole sphere see a light from few points)
    for at in range(0, MANY, SLICE):
        s_sh, s_rgb, s_fin, _ = w.scene.probe_sh(pts[at:at + SLICE], seeds[at:at + SLICE], MANY_SPP, 0.0, want_rgb=True, want_states=True)
        assert s_sh.tobytes() == sh[at:at + SLICE].tobytes() and s_rgb.tobytes() == rgb[at:at + SLICE].tobytes(), "slice at %d" % at
        assert (s_fin == fin[at:at + SLICE]).all(), "slice at %d" % at
