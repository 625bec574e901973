"""The sample planner without a device: the kernels' pixel functions compiled for the host (tools/sampleplan_sim: ort_sampleplan.h
under a host compiler) against the numpy restatement of the contract (tests/plan_ref.py) on every shared case, word for word; the
same program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/sampleplan_sim_san, a stand-alone program run as its
own process: nothing is preloaded, nothing sanitized is loaded into Python); the invariants the header derives; the C ABI's checks
through libort.so, which need no device because every one of them comes before any device work; and the prototype's figures."""
import ctypes as C

import numpy as np
import pytest

import plan_cases as pc
import plan_ref

SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.mark.parametrize("name", pc.NAMES)
def test_host_sim_matches_the_contract(name, tmp_path):
    planes, kw = pc.CASES[name]
    r, smap, totals = pc.run_sim(pc.built("sampleplan_sim"), planes, kw, tmp_path)
    assert r.returncode == 0, r.stderr
    pc.assert_same_plan(smap, totals, *pc.reference(name), name)


@pytest.mark.parametrize("name", pc.SMALL_HOSTILE_AND_BIG)
def test_host_sim_under_sanitizers(name, tmp_path):
    planes, kw = pc.CASES[name]
    r, smap, totals = pc.run_sim(pc.built("sampleplan_sim_san"), planes, kw, tmp_path, env=SAN_ENV)
    assert "runtime error:" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-1500:]
    pc.assert_same_plan(smap, totals, *pc.reference(name), name)


def test_host_sim_judges_its_arguments(tmp_path):
    planes, kw = pc.CASES["5x3"]
    tool = pc.built("sampleplan_sim")
    for bad in (dict(tolerance=0.0), dict(tolerance=float("nan")), dict(tolerance=1e-30), dict(floor=float("inf")), dict(radius=4), dict(min_add=0),
                dict(cap=0), dict(cap=(1 << 24) + 1), dict(budget=(1 << 39) + 1)):
        r, _, _ = pc.run_sim(tool, planes, dict(kw, **bad), tmp_path)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    r, _, _ = pc.run_sim(tool, dict(planes, m2=planes["m2"][:-1]), kw, tmp_path)   # a plane file one row short
    assert r.returncode == 1, r.stderr


# ---- what the header derives ----------------------------------------------------------------------------------------
def test_the_prototypes_figures():
    """the figures the rule was chosen by, on the 67 x 45 x 16-spp frame (floor 0.05, radius 1, pilot 4, min_add 1, cap 4096):
    tolerance 0.25 leaves 1 115 of 3 015 pixels unconverged and asks for 31 649 samples over 41 distinct values, 0.1 leaves all of
    them unconverged and asks for 457 831, 0.5 leaves 3 -- the default case exercises both branches of want, the corners one each"""
    smap, t = pc.reference("67x45")
    assert (t["unconverged"], t["wanted"], t["planned"], t["unknown"], t["invalid"], len(np.unique(smap))) == (1115, 31649, 31649, 0, 0, 41)
    _, t = pc.reference("67x45_tol0.1")
    assert (t["unconverged"], t["wanted"]) == (3015, 457831)
    _, t = pc.reference("67x45_tol0.5")
    assert t["unconverged"] == 3


def test_the_big_sums_are_what_they_should_be():
    _, t = pc.reference("bigsum_64x4")
    assert t["wanted"] == t["planned"] == 1 << 32 and t["unknown"] == 256
    _, t = pc.reference("bigsum_67x45_max")
    assert t["wanted"] == t["planned"] == 3015 << 24 and t["wanted"] > 1 << 35
    smap, t = pc.reference("bigsum_67x45_scaled")
    assert t["wanted"] == 3015 << 24 and t["planned"] <= 1 << 33 and (smap == ((1 << 24) * (1 << 33)) // (3015 << 24)).all()


@pytest.mark.parametrize("name", pc.BUDGETED)
def test_budget_invariants(name):
    """planned <= budget; when scaled, planned > budget - #(want > 0); add <= want <= room"""
    planes, kw = pc.CASES[name]
    smap, totals = pc.reference(name)
    frames = planes["count"].ndim == 3
    for v in range(len(planes["count"]) if frames else 1):
        pick = (lambda a: a[v]) if frames else (lambda a: a)
        t = totals[v] if frames else totals
        args = {k: x for k, x in kw.items() if k != "budget"}
        want, room = plan_ref.wants(pick(pc.colour(planes, kw)), pick(planes["m2"]), pick(planes["count"]), **args)[:2]
        add = pick(smap)
        assert (add <= want).all() and (want <= room).all() and (room <= kw["cap"]).all()
        assert t["wanted"] == int(want.astype(np.uint64).sum()) and t["planned"] == int(add.astype(np.uint64).sum())
        assert t["planned"] <= kw["budget"]
        if t["wanted"] > kw["budget"]:
            assert t["planned"] > kw["budget"] - int((want > 0).sum())
        else:
            assert np.array_equal(add, want)


def test_the_budget_cases_cover_both_sides():
    scaled = [n for n in pc.BUDGETED if any(t["wanted"] > pc.CASES[n][1]["budget"] for t in np.atleast_1d(pc.reference(n)[1]))]
    assert {"budget_third", "budget_one", "budget_below_wanting", "bigsum_67x45_scaled"} <= set(scaled)
    assert not {"budget_exact", "budget_plus1", "budget_max", "bigsum_67x45_max"} & set(scaled)
    smap, t = pc.reference("budget_below_wanting")
    assert t["planned"] < int((pc.reference("67x45")[0] > 0).sum()) and (smap == 0).any()
    smap, t = pc.reference("budget_one")     # exhausted: an all-zero plan, or the single sample, while pixels are unconverged
    assert t["planned"] <= 1 and t["unconverged"] > 0
    per_frame = pc.reference("batch3_23x19_sum_budget")[1]
    assert len({t["wanted"] for t in per_frame}) == 3 and any(t["wanted"] > 2000 for t in per_frame)


def test_batch_frames_equal_their_single_frame_calls():
    """no window crosses from one frame into another and a budget is per frame: the reference's own batch is a loop, so this
    pins the CASE -- three different totals -- and the simulator's and the library's batches are held to it"""
    for name in ("batch3_23x19", "batch3_23x19_sum_budget"):
        planes, kw = pc.CASES[name]
        smap, totals = pc.reference(name)
        for v in range(3):
            one = plan_ref.plan(pc.colour(planes, kw)[v], planes["m2"][v], planes["count"][v], **kw)
            pc.assert_same_plan(smap[v], totals[v], *one, "%s frame %d" % (name, v))
        assert len({t["wanted"] for t in totals}) == 3


def test_sums_and_means_agree_where_the_division_is_exact():
    """the 67 x 45 frame has 16 samples everywhere: sum = 16 * mean and lum(sum) / 16 = lum(mean), both exact, so the two forms
    give one plan.  Elsewhere nothing is claimed: sum / n rounds once more than the mean did"""
    assert (pc.CASES["67x45"][0]["count"] == 16).all()
    pc.assert_same_plan(*pc.reference("67x45_sum"), *pc.reference("67x45"), "sum against mean")


def test_hostile_pixels_are_what_the_header_says():
    planes, kw = pc.CASES["hostile"]
    smap, t = pc.reference("hostile")
    e, unknown, invalid, unconverged, _ = plan_ref.errors(planes["rgb"], planes["m2"], planes["count"], kw["tolerance"], kw["floor"], False)
    assert unknown[20:30, 30:40].all() and unknown[5, 20] and unknown[5, 22] and not unknown[5, 24]
    for y, x in ((0, 0), (44, 66), (38, 50), (11, 33), (13, 40), (6, 25), (40, 2)):   # NaN, a count past 2^24, an error that overflows
        assert invalid[y, x] and e[y, x] == 0, (y, x)
    for y, x in ((0, 66), (44, 0), (36, 44), (3, 9)):   # inf, and 1e30 whose square is inf: v clamps at 0 and e = 0 / inf = 0 -- valid, converged
        assert not invalid[y, x] and not unknown[y, x] and e[y, x] == 0, (y, x)
    for y, x in ((10, 10), (10, 30), (11, 31), (12, 35), (6, 21), (6, 23)):
        assert not invalid[y, x] and not unknown[y, x], (y, x)
    assert unconverged[10, 10] and smap[10, 10] == kw["cap"] and e[10, 10] > 1e30      # need >= 2^24: the cast is never reached
    assert (e.view("<u4") != 0x80000000).all() and np.isfinite(e).all() and (e >= 0).all()
    assert smap[38, 50] == 0 and not smap[37:40, 49:52].any()          # the NaN inside the converged region: nobody plans for it
    assert smap[36, 59] > 0 and smap[37, 58] > 0 and smap[35, 58] > 0    # the large error on its edge: its window plans for it
    assert smap[6, 21] == 1 and smap[6, 23] == 0 and smap[6, 25] == 0 and smap[40, 2] == 0   # room 1, room 0, past the limit
    assert (smap[20:30, 30:40] == kw["pilot"]).all()
    assert t["invalid"] == int(invalid.sum()) and t["unknown"] == int(unknown.sum()) == 102


# ---- the C ABI through libort.so, without a device ------------------------------------------------------------------
PLANES = ("rgb", "m2", "count")
VALID = dict(tolerance=0.25, floor=0.05, radius=1, pilot=4, min_add=1, cap=4096, rgb_is_sum=0, reserved=0, budget=0)


class _Call:
    """one valid host-form call on a 6 x 4 frame; every test bends one argument of it"""

    def __init__(self, api):
        self.api = api
        p = pc.frame(6, 4, 1)
        self.arrays = {k: np.ascontiguousarray(p[k]) for k in PLANES}
        self.map = np.zeros(24 + 2, "<u4")
        self.totals = np.zeros(2, "<u8,<u8,<u8,<u8")
        self.ws = np.zeros(4 * 24 + 16, "u1")

    def ws_ptr(self):
        return (self.ws.ctypes.data + 7) & ~7

    def struct(self, params=None):
        kw = dict(VALID, **(params or {}))
        return self.api.PlanParams(*[kw[k] for k in ("tolerance", "floor", "radius", "pilot", "min_add", "cap", "rgb_is_sum", "reserved", "budget")])

    def run(self, device_form=False, params=None, width=6, height=4, frames=1, map="map", totals="totals", ws="ws", ws_bytes=4 * 24, null_params=False,
            null_planes=False, device=0, **ptrs):
        api = self.api
        p = self.struct(params)
        addr = {k: self.arrays[k].ctypes.data for k in PLANES}
        addr.update(ptrs)
        pl = api.PlanPlanes(*[addr[k] or None for k in PLANES])
        m = self.map.ctypes.data if map == "map" else map
        t = self.totals.ctypes.data if totals == "totals" else totals
        pp = None if null_params else C.byref(p)
        ppl = None if null_planes else C.byref(pl)
        if device_form:
            w = self.ws_ptr() if ws == "ws" else ws
            return api.lib().ort_plan_samples_device(device, pp, ppl, width, height, frames, m or None, t or None, w or None, ws_bytes, None, None)
        return api.lib().ort_plan_samples(device, pp, ppl, width, height, frames, m or None, t or None, None)


@pytest.fixture(scope="module")
def call(api):
    return _Call(api)


def test_abi_version_symbols_and_structs(api):
    L = api.lib()
    assert L.ort_abi_version() == 3
    for name in ("ort_plan_samples", "ort_plan_samples_device", "ort_plan_samples_workspace_bytes"):
        assert hasattr(L, name) and name in api.EXPORTS
    assert C.sizeof(api.PlanTotals) == 32 == api.PLAN_TOTALS_DTYPE.itemsize == pc.TOTALS_DTYPE.itemsize
    assert C.sizeof(api.PlanParams) == 40 and api.PlanParams.budget.offset == 32 and C.sizeof(api.PlanPlanes) == 3 * C.sizeof(C.c_void_p)
    assert set(api.PLAN_DEFAULTS) == {"floor", "radius", "pilot", "min_add", "cap"}


def test_workspace_bytes(api):
    for w, h, f in ((1, 1, 1), (6, 4, 1), (67, 45, 3), (1920, 1080, 1), (1, 1, (1 << 31) - 1), (46340, 46340, 1)):
        assert api.plan_workspace_bytes(w, h, f) == 4 * w * h * f
    assert api.plan_workspace_bytes(6, 4) == 96
    assert api.plan_workspace_bytes(0, -5, 0) == 0
    for w, h, f in ((0, 4, 1), (4, 0, 1), (-1, 4, 1), (1 << 16, 1 << 15, 1), (1 << 15, 1 << 15, 2), (46341, 46341, 1)):
        with pytest.raises(api.OrtError) as e:
            api.plan_workspace_bytes(w, h, f)
        assert e.value.code == api.ERR_INVALID
    assert api.lib().ort_plan_samples_workspace_bytes(4, 4, 1, None) == api.ERR_INVALID


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_zero_frames_is_ok_whatever_the_rest(api, call, device_form):
    assert call.run(device_form, frames=0) == api.OK
    assert call.run(device_form, frames=0, null_params=True, null_planes=True, map=0, totals=0, width=-3, height=0, ws=0, ws_bytes=0) == api.OK


def test_a_valid_call_without_a_device_says_so(api, call):
    if api.device_count() == 0:
        assert call.run(False) == api.ERR_NO_DEVICE
        assert call.run(True) == api.ERR_NO_DEVICE
    else:
        assert call.run(False) == api.OK     # the device form would be handed host pointers: not run
    assert call.run(False, device=1 << 20) == api.ERR_NO_DEVICE
    assert call.run(False, device=-1) == api.ERR_NO_DEVICE


INVALID = [
    ("null params", dict(null_params=True)), ("null planes struct", dict(null_planes=True)), ("null map", dict(map=0)), ("null totals", dict(totals=0)),
] + [("null " + k, {k: 0}) for k in PLANES] + [("misaligned " + k, {k: "+2"}) for k in PLANES] + [
    ("misaligned map", dict(map="+1")), ("misaligned totals", dict(totals="+4")),
    ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width < 0", dict(width=-6)), ("2^31 pixels", dict(width=1 << 16, height=1 << 15)),
    ("2^31 over frames", dict(frames=1 << 27, width=4, height=4)),
    ("tolerance 0", dict(params=dict(tolerance=0.0))), ("tolerance < 0", dict(params=dict(tolerance=-1.0))), ("tolerance nan", dict(params=dict(tolerance=float("nan")))),
    ("tolerance inf", dict(params=dict(tolerance=float("inf")))), ("tolerance whose square is 0", dict(params=dict(tolerance=1e-30))),
    ("floor 0", dict(params=dict(floor=0.0))), ("floor < 0", dict(params=dict(floor=-0.05))), ("floor nan", dict(params=dict(floor=float("nan")))),
    ("floor inf", dict(params=dict(floor=float("inf")))),
    ("radius 4", dict(params=dict(radius=4))), ("min_add 0", dict(params=dict(min_add=0))), ("cap 0", dict(params=dict(cap=0))),
    ("cap over 2^24", dict(params=dict(cap=(1 << 24) + 1))), ("rgb_is_sum 2", dict(params=dict(rgb_is_sum=2))), ("reserved", dict(params=dict(reserved=1))),
    ("budget over 2^39", dict(params=dict(budget=(1 << 39) + 1))),
]


def _bend(call, kw):
    """"+k": the valid pointer of that argument plus k bytes"""
    kw = dict(kw)
    for k, v in list(kw.items()):
        if isinstance(v, str) and v.startswith("+"):
            base = {"map": call.map.ctypes.data, "totals": call.totals.ctypes.data, "ws": call.ws_ptr()}.get(k)
            kw[k] = (call.arrays[k].ctypes.data if base is None else base) + int(v[1:])
    return kw


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what,kw", INVALID, ids=[w for w, _ in INVALID])
def test_invalid_arguments(api, call, device_form, what, kw):
    assert call.run(device_form, **_bend(call, kw)) == api.ERR_INVALID, what
    assert api.lib().ort_last_error()


def test_the_extremes_of_every_field_are_accepted(api, call):
    """valid up to the edge: each of these gets past every check, to the device (or to its absence)"""
    past = (api.OK, api.ERR_NO_DEVICE)
    for params in (dict(radius=0), dict(radius=3), dict(pilot=0), dict(pilot=0xFFFFFFFF), dict(min_add=0xFFFFFFFF), dict(cap=1), dict(cap=1 << 24),
                   dict(rgb_is_sum=1), dict(budget=1), dict(budget=1 << 39), dict(tolerance=1e-18), dict(tolerance=1e19), dict(floor=1e-38), dict(floor=3e38)):
        assert call.run(False, params=params) in past, params


@pytest.mark.parametrize("what,kw", [("null workspace", dict(ws=0)), ("misaligned workspace", dict(ws="+2")), ("short workspace", dict(ws_bytes=4 * 24 - 1)),
                                     ("no workspace bytes", dict(ws_bytes=0))])
def test_invalid_workspace_in_the_device_form(api, call, what, kw):
    assert call.run(True, **_bend(call, kw)) == api.ERR_INVALID, what


def test_the_order_of_the_checks(api, call):
    """each condition outranks every later one: a call with two faults reports the earlier, which its message names.  And every
    ORT_ERR_INVALID outranks ORT_ERR_NO_DEVICE: the device asked for here does not exist on any machine"""
    order = [("null plane", dict(m2=0)), ("null totals", dict(totals=0)), ("4-byte aligned", dict(count="+2")), ("8-byte aligned", dict(totals="+4")),
             ("frame size", dict(width=0)), ("tolerance", dict(params=dict(tolerance=0.0))), ("floor", dict(params=dict(floor=-1.0))),
             ("radius", dict(params=dict(radius=9))), ("min_add", dict(params=dict(min_add=0))), ("cap", dict(params=dict(cap=0))),
             ("rgb_is_sum", dict(params=dict(rgb_is_sum=7))), ("reserved", dict(params=dict(reserved=5))), ("budget", dict(params=dict(budget=1 << 40))),
             ("workspace", dict(ws_bytes=5))]
    for i, (word, first) in enumerate(order):
        for _, later in order[i + 1:]:
            kw = _bend(call, first)
            clash = False
            for k, v in _bend(call, later).items():
                if k == "params":
                    kw[k] = dict(kw.get(k, {}), **v)
                elif k in kw:
                    clash = True     # the same argument cannot be bent two ways
                else:
                    kw[k] = v
            if clash:
                continue
            assert call.run(True, **kw) == api.ERR_INVALID
            assert word in api.lib().ort_last_error().decode(), (word, api.lib().ort_last_error())
    for word, kw in order:
        assert call.run(word == "workspace", device=1 << 20, **_bend(call, kw)) == api.ERR_INVALID, word


def test_python_binding_checks_shapes(api):
    p = pc.frame(6, 4, 1)
    with pytest.raises(ValueError):
        api.plan_samples(p["rgb"][:, :, :2], p["m2"], p["count"], 0.25)
    with pytest.raises(ValueError):
        api.plan_samples(p["rgb"], p["m2"][:-1], p["count"], 0.25)
    with pytest.raises(ValueError):
        api.plan_samples(p["rgb"][0], p["m2"][0], p["count"][0], 0.25)
    with pytest.raises(ValueError):
        api.plan_samples(p["rgb"], p["m2"], p["count"], 0.25, out=np.zeros((4, 6), "<f4"))
    with pytest.raises(ValueError):
        api.plan_samples(p["rgb"], p["m2"], p["count"], 0.25, cap=1 << 32)
    with pytest.raises(ValueError):
        api.plan_samples(p["rgb"], p["m2"], p["count"], 0.25, budget=-1)
    assert hasattr(api.Accumulator, "plan") and hasattr(api.Scene, "render_converge") and hasattr(api.Scene, "render_converge_device")


def test_the_drivers_budget_schedule(api):
    """pass k of the converge loop plans with what is left of the total, shared among the passes left"""
    f = api.Scene._pass_budget
    assert f(None, 0, 8) is None and f(900, 0, 3) == 300 and f(900, 300, 2) == 300 and f(900, 100, 2) == 400 and f(900, 899, 1) == 1
    assert f(900, 900, 1) == 0 and f(900, 1000, 1) == 0 and f(2, 0, 3) == 0
