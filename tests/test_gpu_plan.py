"""The sample planner on the device (ort_plan_samples, ort_plan_samples_device; kernels sampleplan_error, sampleplan_want and
sampleplan_scale of ort_sampleplan.h): every shared case of tests/plan_cases.py through the library against the numpy restatement
of the contract (tests/plan_ref.py) and against the host build of the same pixel functions (tools/sampleplan_sim), word for
word; what only a device shows: the device form with the caller's workspace and totals, guard words around everything it may
write, on a stream of the caller's, two plans chained without a wait, a workspace one byte short; and the converge loop on the
bunny room at 64 x 48, host and device.  No case holds anything but ordinary floats in ordinary memory: nothing here can fault."""
import numpy as np
import pytest

import plan_cases as pc
import plan_ref
import views_cases

pytestmark = pytest.mark.gpu

GUARD = 64   # words of 0xA5A5A5A5 either side of every device buffer a call may write


@pytest.fixture(scope="module")
def dev(api):
    assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the planner has no CPU fallback)"
    import torch
    return torch.device("cuda", 0)


def _library(api, name, **more):
    planes, kw = pc.CASES[name]
    kw = dict(kw, **more)
    return api.plan_samples(pc.colour(planes, kw), planes["m2"], planes["count"], **kw)


@pytest.mark.parametrize("name", pc.NAMES)
def test_library_matches_the_contract(api, dev, name):
    smap, totals, st = _library(api, name, want_stats=True)
    pc.assert_same_plan(smap, totals, *pc.reference(name), name)
    assert st["kernel_ms"] > 0 and all(v == 0 for k, v in st.items() if k != "kernel_ms")


@pytest.mark.parametrize("name", pc.VS_HOST_BUILD)
def test_library_matches_the_host_build(api, dev, name, tmp_path):
    planes, kw = pc.CASES[name]
    r, smap, totals = pc.run_sim(pc.built("sampleplan_sim"), planes, kw, tmp_path)
    assert r.returncode == 0, r.stderr
    pc.assert_same_plan(*_library(api, name), smap, totals, name)


@pytest.mark.parametrize("tile", ["0", "1"], ids=["direct", "tile"])
@pytest.mark.parametrize("name", ["hostile", "hostile_sum_r3", "130x9", "64x4", "1x1", "1x9", "radius0", "radius2", "radius3", "batch3_23x19_sum_budget"])
def test_both_windows_give_the_same_plan(api, dev, name, tile, monkeypatch):
    """the window by direct loads and from the LDS tile with halo (ORT_PLAN_TILE, a developer knob read at every call), each forced
    at every radius: frames narrower and lower than a tile, tiles that hang over the frame's edge, hostile pixels in the halo"""
    monkeypatch.setenv("ORT_PLAN_TILE", tile)
    pc.assert_same_plan(*_library(api, name), *pc.reference(name), "%s, ORT_PLAN_TILE=%s" % (name, tile))


def test_batch_frames_equal_their_single_frame_calls(api, dev):
    for name in ("batch3_23x19", "batch3_23x19_sum_budget"):
        planes, kw = pc.CASES[name]
        smap, totals = _library(api, name)
        for v in range(3):
            one = api.plan_samples(pc.colour(planes, kw)[v], planes["m2"][v], planes["count"][v], **kw)
            pc.assert_same_plan(smap[v], totals[v], *one, "%s frame %d" % (name, v))


def test_the_callers_out_is_written_whole(api, dev):
    planes, kw = pc.CASES["67x45_tol0.5"]     # nearly every pixel wants nothing: every word is written all the same
    out = np.full((45, 67), 0xDEAD, "<u4")
    smap, totals = api.plan_samples(planes["rgb"], planes["m2"], planes["count"], out=out, **kw)
    assert smap is out
    pc.assert_same_plan(out, totals, *pc.reference("67x45_tol0.5"), "out")


class _Device:
    """a case's planes as torch tensors; the map, the totals and the workspace between guard words"""

    def __init__(self, api, dev, name):
        import torch
        self.torch, self.api, self.dev = torch, api, dev
        self.planes, self.kw = pc.CASES[name]
        count = self.planes["count"]
        self.shape = count.shape
        self.frames = 1 if count.ndim == 2 else len(count)
        self.h, self.w = count.shape[-2:]
        n = count.size
        self.inputs = dict(rgb=pc.colour(self.planes, self.kw), m2=self.planes["m2"], count=count)
        self.t = {k: self._guarded(np.ascontiguousarray(a).view("<i4").reshape(-1)) for k, a in self.inputs.items()}
        self.ws_bytes = api.plan_workspace_bytes(self.w, self.h, self.frames)
        assert self.ws_bytes == 4 * n
        self.ws = self._guarded(np.full(n, 0x5EED5EED, "<i4"))
        self.map = self._guarded(np.full(n, 0x5EED5EED, "<i4"))
        self.totals = self._guarded(np.full(8 * self.frames, 0x5EED5EED, "<i4"))   # not zero: the call zeroes them itself

    def _guarded(self, words):
        whole = np.full(len(words) + 2 * GUARD, 0xA5A5A5A5, "<u4").view("<i4")
        whole[GUARD:-GUARD] = words
        return self.torch.from_numpy(whole).to(self.dev)

    def ptr(self, t):
        return t.data_ptr() + 4 * GUARD

    def run(self, stream=None, want_stats=False, ws_bytes=None, **more):
        return self.api.plan_samples_device(self.ptr(self.t["rgb"]), self.ptr(self.t["m2"]), self.ptr(self.t["count"]), self.w, self.h, self.ptr(self.map),
                                            self.ptr(self.totals), self.ptr(self.ws), self.ws_bytes if ws_bytes is None else ws_bytes,
                                            frame_count=self.frames, stream=stream, want_stats=want_stats, **dict(self.kw, **more))

    def inner(self, t):
        return t.cpu().numpy()[GUARD:-GUARD].view("<u4")

    def result(self):
        self.torch.cuda.synchronize()
        for k, t in list(self.t.items()) + [("workspace", self.ws), ("map", self.map), ("totals", self.totals)]:
            w = t.cpu().numpy().view("<u4")
            assert (w[:GUARD] == 0xA5A5A5A5).all() and (w[-GUARD:] == 0xA5A5A5A5).all(), "guard words of %s overwritten" % k
        for k, a in self.inputs.items():
            assert np.array_equal(self.inner(self.t[k]), np.ascontiguousarray(a).view("<u4").reshape(-1)), "input plane %s was written" % k
        rec = self.inner(self.totals).view(pc.TOTALS_DTYPE)
        totals = [dict({k: int(r[k]) for k in pc.FIELDS}, worst=np.float32(r["worst"])) for r in rec]
        return self.inner(self.map).reshape(self.shape), totals if self.frames > 1 else totals[0]


@pytest.mark.parametrize("name", ["hostile", "hostile_sum_r3", "batch3_23x19_sum_budget", "130x9", "bigsum_67x45_scaled", "budget_third", "1x1"])
def test_device_form_with_the_callers_workspace(api, dev, name):
    """the totals' base is 256 bytes into a torch allocation: 8-byte aligned.  They hold garbage before the call, which zeroes
    them on the stream itself"""
    d = _Device(api, dev, name)
    st = d.run(want_stats=True)
    assert st["kernel_ms"] > 0 and all(v == 0 for k, v in st.items() if k != "kernel_ms")
    pc.assert_same_plan(*d.result(), *pc.reference(name), name)


def test_device_form_on_a_stream_of_the_callers_two_plans_chained(api, dev):
    """two plans on one non-default stream without a wait between them, into the same map, totals and workspace: the second,
    at another tolerance and under a budget, is what remains"""
    import torch
    d = _Device(api, dev, "67x45")
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    assert d.run(stream=stream.cuda_stream) is None
    assert d.run(stream=stream.cuda_stream, tolerance=0.1, budget=pc.CASES["budget_third"][1]["budget"]) is None
    stream.synchronize()
    planes, kw = pc.CASES["67x45"]
    want = plan_ref.plan(planes["rgb"], planes["m2"], planes["count"], **dict(kw, tolerance=0.1, budget=pc.CASES["budget_third"][1]["budget"]))
    pc.assert_same_plan(*d.result(), *want, "second plan")
    assert want[1]["wanted"] > want[1]["planned"] > 0


def test_a_workspace_one_byte_short_is_refused_without_a_launch(api, dev):
    d = _Device(api, dev, "5x3")
    for kw in (dict(ws_bytes=d.ws_bytes - 1), dict(ws_bytes=0)):
        with pytest.raises(api.OrtError) as e:
            d.run(**kw)
        assert e.value.code == api.ERR_INVALID
    d.torch.cuda.synchronize()
    for k, t in (("map", d.map), ("totals", d.totals), ("workspace", d.ws)):
        assert (d.inner(t) == 0x5EED5EED).all(), "a refused call wrote %s" % k


# ---- the converge loop on a real frame --------------------------------------------------------------------------------
W, H = 64, 48
LOOP = dict(pilot=8, cap=64, passes=3)
TOL, SEED = 0.3, 11


@pytest.fixture(scope="module")
def converge(api, gpu_scene):
    """the bunny room at 64 x 48 from an empty Accumulator, the planes saved before every plan: (scene, budget, acc, history, maps,
    the planes before each plan)"""
    scene = gpu_scene("c3_bunny_room")
    probe = api.Accumulator(W, H)
    scene.render_accumulate(probe, LOOP["pilot"], SEED)
    budget = plan_ref.plan(probe.sum_rgb, probe.m2, probe.count, TOL, pilot=LOOP["pilot"], cap=LOOP["cap"], rgb_is_sum=True)[1]["wanted"] // 3
    acc = api.Accumulator(W, H)
    before = []
    plan = acc.plan

    def recording_plan(*a, **kw):
        before.append({k: getattr(acc, k).copy() for k in ("sum_rgb", "m2", "count", "states")})
        return plan(*a, **kw)
    acc.plan = recording_plan
    history, maps = scene.render_converge(acc, TOL, SEED, budget=budget, keep_maps=True, **LOOP)
    del acc.plan
    return scene, budget, acc, history, maps, before


def test_converge_each_pass_is_the_contracts_plan(api, converge):
    scene, budget, acc, history, maps, before = converge
    assert budget > 0 and len(history) == len(before) == 3 and len(maps) == 3
    assert not before[0]["count"].any(), "the first plan is made from an empty frame"
    spent = 0
    for k, (t, smap, planes) in enumerate(zip(history, maps, before)):
        b = (budget - spent) // (LOOP["passes"] - k)
        assert t["budget"] == b > 0
        want = plan_ref.plan(planes["sum_rgb"], planes["m2"], planes["count"], TOL, pilot=LOOP["pilot"], cap=LOOP["cap"], rgb_is_sum=True, budget=b)
        pc.assert_same_plan(smap, t, *want, "pass %d" % k)
        assert t["planned"] <= b
        spent += t["planned"]
    assert history[0]["unknown"] == W * H and history[0]["wanted"] == LOOP["pilot"] * W * H
    assert history[1]["unknown"] < W * H and history[1]["unconverged"] > 0, "the second plan has estimates to plan from"
    assert spent <= budget and np.array_equal(acc.count, np.sum(maps, axis=0, dtype=np.uint64).astype("<u4"))


def test_converge_is_one_accumulate_of_its_counts(api, converge):
    """split invariance: after the loop all four planes are those of ONE render_accumulate from zero with map = acc.count, so the
    oracle pins of the accumulating render are the driver's as well"""
    scene, _, acc, _, _, _ = converge
    one = api.Accumulator(W, H)
    scene.render_accumulate(one, acc.count, SEED, cap=int(acc.count.max()))
    for k in ("count", "states", "sum_rgb", "m2"):
        assert np.array_equal(getattr(acc, k).view("<u4"), getattr(one, k).view("<u4")), k


def test_converge_device_gives_the_same_planes(api, dev, converge):
    import torch
    scene, budget, acc, history, _, _ = converge
    d_sum = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    d_m2 = torch.zeros((H, W), dtype=torch.float32, device=dev)
    d_count, d_states, d_map = (torch.zeros((H, W), dtype=torch.int32, device=dev) for _ in range(3))
    d_totals = torch.zeros(4, dtype=torch.int64, device=dev)
    d_ws = torch.zeros(api.plan_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
    got = scene.render_converge_device(W, H, d_sum, d_m2, d_count, d_states, d_map, d_totals, d_ws, TOL, SEED, budget=budget, **LOOP)
    torch.cuda.synchronize()
    assert len(got) == len(history)
    for k, (a, b) in enumerate(zip(got, history)):
        assert a["budget"] == b["budget"]
        pc.assert_same_plan(np.zeros(0, "<u4"), a, np.zeros(0, "<u4"), b, "device pass %d" % k)
    for name, t in (("sum_rgb", d_sum), ("m2", d_m2), ("count", d_count), ("states", d_states)):
        assert np.array_equal(t.cpu().numpy().view("<u4"), getattr(acc, name).view("<u4")), name


def test_converge_without_a_budget_ends_on_an_empty_plan(api, gpu_scene):
    """a tolerance no pixel misses once it has an estimate, and passes to spare: the loop ends on the plan that asks for
    nothing, which is converged"""
    scene = gpu_scene("c3_bunny_room")
    acc = api.Accumulator(16, 12)
    history = scene.render_converge(acc, 1e3, SEED, passes=6, pilot=8, cap=256)
    last = history[-1]
    assert len(history) < 6 and last["planned"] == 0 and last["unconverged"] == 0 and last["unknown"] == 0 and last["budget"] is None
    assert (acc.count >= 8).all()


def test_two_views_are_planned_each_on_its_own(api, gpu_scene):
    """the first two views of tests/views_cases.py at 32 x 32, accumulated in one launch: each frame's map and totals are its
    single-frame call's, under a budget that scales them differently"""
    scene = gpu_scene("c3_bunny_room")
    w = h = 32
    flat = scene.flatten(w, h)
    cams = np.stack([api.camera_from_pose(p, q, r, w, h) for p, q, r in views_cases.poses(scene, flat)[:2]])
    acc = api.Accumulator(w, h, views=2)
    scene.render_views_accumulate(cams, views_cases.SEEDS[:2], acc, 8)
    acc.count[1, :4, :4] = 0    # and some unknown pixels in one of them
    for budget in (None, 5000):
        smap, totals = acc.plan(0.3, pilot=8, cap=64, budget=budget)
        want = plan_ref.plan(acc.sum_rgb, acc.m2, acc.count, 0.3, pilot=8, cap=64, rgb_is_sum=True, budget=budget)
        pc.assert_same_plan(smap, totals, *want, "two views, budget %s" % budget)
        for v in range(2):
            one = api.plan_samples(acc.sum_rgb[v], acc.m2[v], acc.count[v], 0.3, pilot=8, cap=64, rgb_is_sum=True, budget=budget)
            pc.assert_same_plan(smap[v], totals[v], *one, "view %d, budget %s" % (v, budget))
    assert totals[0]["wanted"] != totals[1]["wanted"] and totals[1]["unknown"] == 16
