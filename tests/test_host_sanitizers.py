"""The host-compiled lane code, the set-up code of ort_setup.h and the loaders under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/host_sim_san is tools/host_sim built with -fsanitize=address,undefined
-fno-sanitize-recover=all (tools/Makefile), a stand-alone program run as a subprocess; nothing loaded into Python is
sanitized.  The other suites compare output bits, which cannot see a read one record past a table slot that returns
harmless data, uninitialised padding that is uploaded, or undefined pointer arithmetic.  Every run here is made with both
binaries and must (1) end with the plain binary's exit status, (2) report nothing (no "runtime error:", no
"AddressSanitizer" on stderr) and (3) write byte-identical files.  Leak checking is on (ASAN_OPTIONS=detect_leaks=1):
host_sim destroys what it creates.  The runs are small: at most 20 x 12 pixels, 2 spp, 120 rays, 2 threads (1 000 rays on the
deep scene, whose point is the traversal stack's scratch tail)."""
import os

import numpy as np
import pytest

import deep_scenes
import host_sim_tool as hs
import radiance_cases
import ref_io
import table_scenes
from conftest import DATA, GOLDEN

SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module")
def tools():
    return hs.built("host_sim"), hs.built("host_sim_san")


def _same_nan_by_position(a, b):
    """the --unit output alone: where both files hold a float32 NaN in the same word, the NaNs' sign may differ.  Which NaN an
    x86 operation makes depends on the order of its operands, which the optimisation level chooses: one word of the records of
    unit_edges.npz (op 7) is 0x7fc00000 at -O2 and 0xffc00000 at -O1.  Every other output of every mode is compared byte for byte"""
    if a is None or b is None or len(a) != len(b) or len(a) % 4:
        return a == b
    x, y = np.frombuffer(a, "<u4"), np.frombuffer(b, "<u4")
    nan = lambda w: ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)
    ne = x != y
    return bool((nan(x[ne]) & nan(y[ne])).all())


def both(tools, args, outs, env=None, threads=2, same=lambda a, b: a == b):
    """one run with each binary -> the plain binary's CompletedProcess, after the three checks"""
    got = []
    for tool, extra in zip(tools, ({}, SAN_ENV)):
        for o in outs:
            if os.path.exists(o):
                os.remove(o)
        r = hs.run(tool, args, env=dict(env or {}, **extra), threads=threads, check=False)
        got.append((r, [open(o, "rb").read() if os.path.exists(o) else None for o in outs]))
    (plain, files), (san, san_files) = got
    what = " ".join(str(a) for a in args if not str(a).startswith("/")) + " " + repr(env or {})
    assert "runtime error:" not in san.stderr and "AddressSanitizer" not in san.stderr and "LeakSanitizer" not in san.stderr, \
        "%s\n%s" % (what, san.stderr[-3000:])
    assert san.returncode == plain.returncode, "%s: exit %d, plain %d\n%s" % (what, san.returncode, plain.returncode, san.stderr[-1500:])
    for o, a, b in zip(outs, files, san_files):
        assert same(a, b), "%s: %s differs from the plain binary's" % (what, os.path.basename(o))
    return plain


@pytest.fixture(scope="module")
def table_scn(api, tmp_path_factory):
    """variant -> (path of its .scn, its directory): the scenes at and past the caps of the LDS tables"""
    made = {}

    def get(variant):
        if variant not in made:
            d = tmp_path_factory.mktemp("san_" + variant)
            table_scenes.build(api, variant, d)
            made[variant] = (str(d / (variant + ".scn")), str(d) + "/")
        return made[variant]
    return get


def _rays(name, n=120):
    z = np.load(os.path.join(GOLDEN, "raycast_edges_%s.npz" % name))
    pick = np.linspace(0, len(z["rays"]) - 1, n).astype(int)   # every category of raycast_cases
    return z["rays"][pick], z["t"][pick]


def _pinholes(n, lo, hi):
    rng = np.random.default_rng(11)
    cams = radiance_cases.inside(rng, np.asarray(lo, "<f4"), np.asarray(hi, "<f4"), n)
    rays = np.array([np.concatenate(radiance_cases.pinhole(p, z)) for p, z in cams], "<f4")
    rays[::17, 3:6] *= np.float32(2)      # outside the per-ray domain: answered without a traversal
    rays[5::31, 0] = np.nan
    return rays, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")


CAMS = np.array([[[5.5, -4.0, 3.0], [0.2, 0.1, 0], [0, 0.1, 0.2], [0.6, -0.7, 0.3]],
                 [[2.0, -1.0, 2.0], [0.2, 0, 0], [0, 0.2, 0], [0.1, -0.9, 0.2]]], "<f4")

QUERY_ENVS = [{}, {"SIM_TABS": "1"}, {"SIM_FORCE_FALLBACK": "0xf"}, {"SIM_TABS": "1", "SIM_FORCE_FALLBACK": "0xf"}]


@pytest.mark.parametrize("env", QUERY_ENVS, ids=lambda e: "+".join(sorted(e)) or "plain")
@pytest.mark.parametrize("name", ["c2_analytic", "letters"])
def test_new_modes(tools, tmp_path, name, env):
    """--raycast, --occluded (with limits at and one ulp either side of the hit, and without), --radiance, --views"""
    d = str(tmp_path)
    rays, t = _rays(name)
    assert both(tools, *hs.raycast_args(d, name, rays), env=env).returncode == 0
    with np.errstate(all="ignore"):
        tm = np.where(np.arange(len(t)) % 3 == 0, t, np.where(np.arange(len(t)) % 3 == 1, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))))
    tm[::7] = np.nan
    tm[3::11] = -1
    assert both(tools, *hs.occluded_args(d, name, rays, tm.astype("<f4")), env=env).returncode == 0
    assert both(tools, *hs.occluded_args(d, name, rays, None), env=env).returncode == 0
    prays, seeds = _pinholes(24, (-1, -1, 0.3), (1, 1, 2))
    for extra in ({}, {"SIM_DIFFUSE": "1"}) if name == "letters" else ({},):
        assert both(tools, *hs.radiance_args(d, name, prays, seeds, 2, 0.8), env=dict(env, **extra)).returncode == 0
    assert both(tools, *hs.views_args(d, name, CAMS, [7, 0xDEADBEEF], 11, 9, 2, "chunk", 1), env=env).returncode == 0
    assert both(tools, *hs.views_args(d, name, CAMS, [7, 0xDEADBEEF], 11, 9, 1, "pixel", 0), env=env).returncode == 0


@pytest.mark.parametrize("variant,commit_env,tabs_fit", [("at_caps", {}, 3), ("mats_over", {}, 1), ("lights_over", {}, 1),
                                                        ("pro_over", {"ORT_ANALYTIC_PROLOGUE": "40"}, 0)])
def test_new_modes_at_and_past_the_table_caps(tools, table_scn, tmp_path, variant, commit_env, tabs_fit):
    """at_caps uses the last float4 of every slot; past a cap the table stays in its array, and SIM_TABS is refused by
    the modes that would need it (tabs_fit: 3 every mode takes SIM_TABS, 1 the ray queries alone, 0 none)"""
    scn, base = table_scn(variant)
    d = str(tmp_path)
    rays = np.load(os.path.join(GOLDEN, "raycast_tables_at_caps.npz"))["rays"][:100]
    prays, seeds = _pinholes(16, (-2, -2, 0.5), (2, 2, 3))
    for tabs in (False, True):
        env = dict(commit_env, **({"SIM_TABS": "1"} if tabs else {}))
        want_q = 0 if (not tabs or tabs_fit >= 1) else 1
        want_p = 0 if (not tabs or tabs_fit >= 3) else 1
        assert both(tools, *hs.raycast_args(d, scn, rays, base), env=env).returncode == want_q
        assert both(tools, *hs.occluded_args(d, scn, rays, np.full(len(rays), 3.0, "<f4"), base), env=env).returncode == want_q
        assert both(tools, *hs.radiance_args(d, scn, prays, seeds, 1, 0.8, base), env=env).returncode == want_p
        assert both(tools, *hs.views_args(d, scn, CAMS, [1, 2], 16, 9, 1, "pixel", 0, base), env=env).returncode == want_p
        assert both(tools, *hs.render_args(d, scn, 16, 9, 2, 5, "chunk", 1, base), env=dict(env, SIM_FORCE_FALLBACK="0xf")).returncode == want_p


@pytest.mark.parametrize("policy,chunk,env,shard", [
    ("pixel", 0, {}, None), ("chunk", 1, {}, None), ("tile32", 0, {}, None), ("whole", 0, {}, None),
    ("chunk", 2, {"SIM_WIDE": "1"}, None), ("pixel", 0, {"SIM_DIFFUSE": "1"}, None), ("pixel", 0, {"SIM_WAVEFRONT": "100"}, None),
    ("chunk", 1, {}, (1, 3)), ("pixel", 0, {"SIM_TABS": "1"}, None), ("chunk", 2, {"SIM_TABS": "1", "SIM_WIDE": "1"}, None),
], ids=lambda v: str(v).replace(" ", ""))
def test_render_modes(tools, tmp_path, policy, chunk, env, shard):
    for name in ("c2_analytic", "letters"):
        if name == "c2_analytic" and ("SIM_WIDE" in env or "SIM_DIFFUSE" in env):
            continue
        args, outs = hs.render_args(str(tmp_path), name, 20, 12, 2, 77, policy, chunk, shard=shard)
        assert both(tools, args, outs, env=env, threads=1 if "SIM_WAVEFRONT" in env else 2).returncode == 0


def test_the_stack_in_its_scratch_tail(api, oracle, tools, tmp_path_factory, tmp_path):
    """the deep scene (tests/deep_scenes.py): nearly every ray's traversal stack runs past its LDS part, up to six entries into spill[], and the
    re-traversal of resolve_hit with it; the wide tree stacks up to three entries a level and gets 44 deep, the wavefront trace
    keeps 16 entries outside spill[].  An index past either array is what the sanitizer sees and the bit comparisons may not"""
    w = deep_scenes.world(api, oracle, tmp_path_factory)
    d = str(tmp_path)
    rays = w.rays[::4]
    r = both(tools, *hs.raycast_args(d, w.scn, rays, w.base))
    assert r.returncode == 0
    main, again = hs.stack_probe(r)[:2]
    assert main["deepest"] >= main["lds"] + 4 and again["above"] > 0
    tm = np.where(np.arange(len(rays)) % 2 == 0, w.t[::4], np.nextafter(w.t[::4], np.float32(np.inf))).astype("<f4")
    assert both(tools, *hs.occluded_args(d, w.scn, rays, tm, w.base)).returncode == 0
    for env in ({}, {"SIM_WIDE": "1"}, {"SIM_WAVEFRONT": "100"}, {"SIM_TABS": "1", "SIM_FORCE_FALLBACK": "0xf"}):
        args, outs = hs.render_args(d, w.scn, 20, 12, 2, 77, "chunk", 1, w.base)
        r = both(tools, args, outs, env=env, threads=1 if "SIM_WAVEFRONT" in env else 2)
        assert r.returncode == 0 and hs.stack_probe(r)[0]["scratch_pops"] > 0


def test_tree_check_on_full_leaves(tools, tmp_path):
    """--tree-check on the cluster scene (tools/make_clusterscene.py) committed under ORT_LEAF_TRI=16 ORT_LEAF_OTHER=16: the
    builder writing 16-primitive leaves of every kind, and the check's own walks of both trees, under the sanitizers; then one
    frame and the scene's aimed rays through those leaves"""
    import tree_shapes
    scn, layout = tree_shapes.make_clusterscene.write_scene(str(tmp_path))
    base, env = str(tmp_path) + "/", tree_shapes.VARIANTS["leaf16"]
    r = both(tools, ["--tree-check", scn, base], [], env=env)
    assert r.returncode == 0 and "max_leaf triangle 16 sphere 16 box 16 cylinder 16" in r.stdout, r.stdout + r.stderr
    rays = tree_shapes.aimed_rays(layout, np.random.default_rng(3))[::7]
    assert both(tools, *hs.raycast_args(str(tmp_path), scn, rays, base), env=env).returncode == 0
    for extra in ({}, {"SIM_WIDE": "1"}, {"SIM_TABS": "1"}):
        args, outs = hs.render_args(str(tmp_path), scn, 20, 12, 2, 77, "chunk", 1, base)
        assert both(tools, args, outs, env=dict(env, **extra)).returncode == 0


def test_unit_records(tools, tmp_path):
    z = np.load(os.path.join(GOLDEN, "unit_edges.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(recs).tofile(src)
    assert both(tools, ["--unit", src, out], [out], same=_same_nan_by_position).returncode == 0
    open(src, "ab").write(b"\0" * 7)   # not a whole record
    assert both(tools, ["--unit", src, out], [out]).returncode == 1


# every malformed text tests/test_host.py feeds the parser, and texts cut mid-token
BAD_SCN = [
    "brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nsphere 0 0 0 1\n",
    "light 1.0 1.0 1.0\n",
    "brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nsphere\t1.0 1.0 1.0 1.0\n",
    "brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nboxes 0.0 0.0 0.0 1.0 1.0 1.0\n",
    "# comment\nbrdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nsphere 0.0 0.0 0.0 1.0\n",
    "brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nmesh nothere.ply 0.0 0.0 0.0 1.0 q 1 0 0 0\n",
    "", "\n", "sphere", "brdf 0.5 0.5", "brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nsphere 0.0 0.0 0.0 1.", "camera 1.0 2.0", "mesh", "mesh x.ply 0.0",
    "brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\ncylinder 0.0 0.0 0.0 0.0 0.0 1.0 0.1\nlight 1 2 3\nsphere 1.0 0.0 0.0 1.0\n",
    "sphere 0.0 0.0 0.0 1.0\n",   # a shape before any material
    "-", "1e", "2.5e+", "brdf -", "light 1 2", "light 99999999999999999999 1 1\n",
    "light -99999999999999999999 1 1\n", "light -2147483648 1 1\n", "light 2147483648 2147483647 -2147483647\n",   # integer literals at and past the i32 range, negated
]


def _load_only(tools, tmp_path, scn, base):
    """the loaders, then one 8 x 8 frame when the scene loads and commits"""
    args, outs = hs.render_args(str(tmp_path), scn, 8, 8, 1, 3, "pixel", 0, base)
    return both(tools, args, outs)


def test_malformed_scn_texts(tools, tmp_path):
    whole = open(os.path.join(DATA, "letters.scn")).read()
    texts = BAD_SCN + [whole[:k] for k in np.linspace(1, len(whole) - 1, 8).astype(int)]
    codes = set()
    for i, text in enumerate(texts):
        p = tmp_path / ("bad%d.scn" % i)
        p.write_text(text)
        codes.add(_load_only(tools, tmp_path, str(p), DATA + "/").returncode)
    assert codes == {0, 1}   # some load (prefix keywords, skipped words), some are refused; none crashes


OBJ = "".join("v %d.0 %d.5 %d.25\n" % (i, i % 3, i % 5) for i in range(12)) + "".join(
    "f %d %d %d\n" % (i + 1, (i + 1) % 12 + 1, (i + 2) % 12 + 1) for i in range(12)) + "f 1/1/1 2/2/2 3/3/3 4/4/4\nf 1 2\nf 99 1 2\nf -1 -2 -3\nf -99999999999999999999 1 2\nf 1 -2147483648 3\nf 99999999999999999999 2 3\n"


@pytest.mark.parametrize("kind", ["ply", "obj"])
def test_truncated_meshes(tools, tmp_path, kind):
    """data/letterX.ply and a small OBJ cut at a spread of byte offsets, the PLY's header mid-token among them"""
    whole = open(os.path.join(DATA, "letterX.ply"), "rb").read() if kind == "ply" else OBJ.encode()
    head = whole.find(b"end_header") if kind == "ply" else 0
    cuts = sorted(set([0, 1, 3, len(whole) - 1, len(whole)] + [int(k) for k in np.linspace(0, len(whole), 9)] +
                      ([head - 30, head - 7, head + 4, head + 10, head + 11, head + 12, head + 40] if kind == "ply" else [])))
    scn = tmp_path / "m.scn"
    scn.write_text("brdf 0.5 0.5 0.5 0.0 0.0 0.0 10\nmesh m.%s 0.0 0.0 0.0 1.0 q 1 0 0 0\n" % kind)
    codes = []
    for cut in cuts:
        (tmp_path / ("m." + kind)).write_bytes(whole[:max(0, cut)])
        codes.append(_load_only(tools, tmp_path, str(scn), str(tmp_path) + "/").returncode)
    assert codes[-1] == 0 or kind == "obj"   # the whole PLY loads
    if kind == "ply":   # indices and counts at and past the i32 range, negated; an index past the vertices
        for a, b in ((b"4 3 2 1 0", b"4 -99999999999999999999 2 1 0"), (b"4 3 2 1 0", b"4 3 -2147483648 1 0"), (b"4 3 2 1 0", b"4 3 2 1 99"),
                     (b"4 3 2 1 0", b"4 99999999999999999999 2 1 0"), (b"element vertex 8", b"element vertex -99999999999999999999"),
                     (b"element face 2", b"element face -2147483648"), (b"4 7 6 5 4", b"-2147483648 7 6 5 4"), (b"4 7 6 5 4", b"2147483647 7 6 5 4")):
            assert whole.count(a) == 1
            (tmp_path / "m.ply").write_bytes(whole.replace(a, b))
            _load_only(tools, tmp_path, str(scn), str(tmp_path) + "/")
