"""The denoiser without a device: the kernels' pixel functions compiled for the host (tools/denoise_sim: ort_denoise.h under a
host compiler) against the numpy restatement of the contract (tests/denoise_ref.py) on every shared case, bit for bit; the same
program under AddressSanitizer and UndefinedBehaviorSanitizer (tools/denoise_sim_san, a stand-alone program run as its own
process: nothing is preloaded, nothing sanitized is loaded into Python); the C ABI's checks through libort.so, which need no
device because every one of them comes before any device work; and one sanity test of the reference itself."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref

SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.mark.parametrize("name", dc.NAMES)
def test_host_sim_matches_the_contract(name, tmp_path):
    planes, kw = dc.CASES[name]
    r, got = dc.run_sim(dc.built("denoise_sim"), planes, kw, tmp_path)
    assert r.returncode == 0, r.stderr
    dc.assert_same_frame(got, dc.reference(name), name)


def test_batch_frames_equal_their_single_frame_calls():
    """no tap crosses from one frame into another: the reference's own batch is a loop, so this pins the CASE -- the frames
    differ, and each has unusable pixels at its edges -- and the simulator's and the library's batches are held to it"""
    planes, kw = dc.CASES["batch3_23x19"]
    want = dc.reference("batch3_23x19")
    for v in range(3):
        one = denoise_ref.denoise(*[planes[k][v] for k in dc.PLANES], **kw)
        dc.assert_same_frame(want[v], one, "frame %d" % v)
    assert not np.array_equal(want[0], want[1])


def test_host_sim_in_place(tmp_path):
    """out may be rgb itself: the simulator reads rgb whole before it writes, so this pins the file handling alone"""
    planes, kw = dc.CASES["hostile"]
    r, got = dc.run_sim(dc.built("denoise_sim"), planes, kw, tmp_path, in_place=True)
    assert r.returncode == 0, r.stderr
    dc.assert_same_frame(got, dc.reference("hostile"), "in place")


@pytest.mark.parametrize("name", dc.SMALL_AND_HOSTILE)
def test_host_sim_under_sanitizers(name, tmp_path):
    planes, kw = dc.CASES[name]
    r, got = dc.run_sim(dc.built("denoise_sim_san"), planes, kw, tmp_path, env=SAN_ENV)
    assert "runtime error:" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-1500:]
    dc.assert_same_frame(got, dc.reference(name), name)


def test_host_sim_judges_its_arguments(tmp_path):
    planes, kw = dc.CASES["5x3"]
    tool = dc.built("denoise_sim")
    for bad in (dict(iterations=0), dict(iterations=9), dict(normal_squarings=9), dict(sigma_l=0.0), dict(sigma_z=float("nan")), dict(sigma_l=float("inf"))):
        r, _ = dc.run_sim(tool, planes, dict(kw, **bad), tmp_path)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    short = dict(planes, depth=planes["depth"][:-1])   # a plane file one row short
    r, _ = dc.run_sim(tool, dict(short, count=planes["count"]), kw, tmp_path)
    assert r.returncode == 1, r.stderr


# ---- the C ABI through libort.so, without a device ------------------------------------------------------------------
class _Call:
    """one valid host-form call on a 6 x 4 frame; every test bends one argument of it"""

    def __init__(self, api):
        self.api = api
        p = dc.frame(6, 4, 1)[0]
        self.arrays = {k: np.ascontiguousarray(p[k]) for k in dc.PLANES}
        self.out = np.zeros((4, 6, 3), "<f4")
        self.ws = np.zeros(48 * 24 + 64, "u1")

    def ws_ptr(self):
        return (self.ws.ctypes.data + 15) & ~15

    def run(self, device_form=False, params=None, width=6, height=4, frames=1, out="out", ws="ws", ws_bytes=48 * 24, null_params=False,
            null_planes=False, device=0, **ptrs):
        api = self.api
        kw = dict(dc.DEFAULTS, **(params or {}))
        p = api.DenoiseParams(kw["iterations"], kw["normal_squarings"], kw["sigma_l"], kw["sigma_z"])
        addr = {k: self.arrays[k].ctypes.data for k in dc.PLANES}
        addr.update(ptrs)
        pl = api.DenoisePlanes(*[addr[k] or None for k in dc.PLANES])
        o = self.out.ctypes.data if out == "out" else out
        pp = None if null_params else C.byref(p)
        ppl = None if null_planes else C.byref(pl)
        if device_form:
            w = self.ws_ptr() if ws == "ws" else ws
            return api.lib().ort_denoise_device(device, pp, ppl, width, height, frames, o or None, w or None, ws_bytes, None, None)
        return api.lib().ort_denoise(device, pp, ppl, width, height, frames, o or None, None)


@pytest.fixture(scope="module")
def call(api):
    return _Call(api)


def test_abi_version_and_symbols(api):
    L = api.lib()
    assert L.ort_abi_version() == 3
    for name in ("ort_denoise", "ort_denoise_device", "ort_denoise_workspace_bytes"):
        assert hasattr(L, name) and name in api.EXPORTS


def test_workspace_bytes(api):
    for w, h, f in ((1, 1, 1), (6, 4, 1), (67, 45, 3), (1920, 1080, 1), (1, 1, (1 << 31) - 1), (46340, 46340, 1)):
        assert api.denoise_workspace_bytes(w, h, f) == 48 * w * h * f
    assert api.denoise_workspace_bytes(0, -5, 0) == 0
    for w, h, f in ((0, 4, 1), (4, 0, 1), (-1, 4, 1), (1 << 16, 1 << 15, 1), (1 << 15, 1 << 15, 2), (46341, 46341, 1)):
        with pytest.raises(api.OrtError) as e:
            api.denoise_workspace_bytes(w, h, f)
        assert e.value.code == api.ERR_INVALID
    assert api.lib().ort_denoise_workspace_bytes(4, 4, 1, None) == api.ERR_INVALID


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_zero_frames_is_ok_whatever_the_rest(api, call, device_form):
    assert call.run(device_form, frames=0) == api.OK
    assert call.run(device_form, frames=0, null_params=True, null_planes=True, out=0, width=-3, height=0, ws=0, ws_bytes=0) == api.OK


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_a_valid_call_without_a_device_says_so(api, call, device_form):
    if api.device_count() > 0:
        want = api.OK if not device_form else None   # the device form would be handed host pointers: not run
    else:
        want = api.ERR_NO_DEVICE
    if want is not None:
        assert call.run(device_form) == want
    assert api.lib().ort_denoise(1 << 20, *_valid_tail(api, call)) == api.ERR_NO_DEVICE
    assert api.lib().ort_denoise(-1, *_valid_tail(api, call)) == api.ERR_NO_DEVICE


def _valid_tail(api, call):
    kw = dc.DEFAULTS
    p = api.DenoiseParams(kw["iterations"], kw["normal_squarings"], kw["sigma_l"], kw["sigma_z"])
    pl = api.DenoisePlanes(*[call.arrays[k].ctypes.data for k in dc.PLANES])
    call._keep = (p, pl)
    return C.byref(p), C.byref(pl), 6, 4, 1, call.out.ctypes.data, None


INVALID = [
    ("null params", dict(null_params=True)), ("null planes struct", dict(null_planes=True)), ("null out", dict(out=0)),
] + [("null " + k, {k: 0}) for k in dc.PLANES] + [("misaligned " + k, {k: "+2"}) for k in dc.PLANES] + [
    ("misaligned out", dict(out="+1")),
    ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width < 0", dict(width=-6)), ("2^31 pixels", dict(width=1 << 16, height=1 << 15)),
    ("2^31 over frames", dict(frames=1 << 27, width=4, height=4)),
    ("iterations 0", dict(params=dict(iterations=0))), ("iterations 9", dict(params=dict(iterations=9))),
    ("squarings 9", dict(params=dict(normal_squarings=9))),
    ("sigma_l 0", dict(params=dict(sigma_l=0.0))), ("sigma_l < 0", dict(params=dict(sigma_l=-1.0))), ("sigma_l nan", dict(params=dict(sigma_l=float("nan")))),
    ("sigma_l inf", dict(params=dict(sigma_l=float("inf")))), ("sigma_z 0", dict(params=dict(sigma_z=0.0))), ("sigma_z nan", dict(params=dict(sigma_z=float("nan")))),
    ("sigma_z inf", dict(params=dict(sigma_z=float("inf")))),
]


def _bend(call, kw):
    """"+k": the valid pointer of that argument plus k bytes"""
    kw = dict(kw)
    for k, v in list(kw.items()):
        if isinstance(v, str) and v.startswith("+"):
            base = call.out.ctypes.data if k == "out" else call.ws_ptr() if k == "ws" else call.arrays[k].ctypes.data
            kw[k] = base + int(v[1:])
    return kw


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what,kw", INVALID, ids=[w for w, _ in INVALID])
def test_invalid_arguments(api, call, device_form, what, kw):
    assert call.run(device_form, **_bend(call, kw)) == api.ERR_INVALID, what
    assert api.lib().ort_last_error()


@pytest.mark.parametrize("what,kw", [("null workspace", dict(ws=0)), ("misaligned workspace", dict(ws="+8")), ("short workspace", dict(ws_bytes=48 * 24 - 1)),
                                     ("no workspace bytes", dict(ws_bytes=0))])
def test_invalid_workspace_in_the_device_form(api, call, what, kw):
    assert call.run(True, **_bend(call, kw)) == api.ERR_INVALID, what


def test_the_order_of_the_checks(api, call):
    """each condition outranks every later one: a call with two faults reports the earlier, which its message names.  And every
    ORT_ERR_INVALID outranks ORT_ERR_NO_DEVICE: the device asked for here does not exist on any machine"""
    order = [("null", dict(m2=0)), ("aligned", dict(depth="+2")), ("frame size", dict(width=0)), ("iterations", dict(params=dict(iterations=0))),
             ("normal_squarings", dict(params=dict(normal_squarings=9))), ("sigma", dict(params=dict(sigma_z=-1.0))), ("workspace", dict(ws_bytes=5))]
    for i, (word, first) in enumerate(order):
        for _, later in order[i + 1:]:
            kw = _bend(call, first)
            for k, v in _bend(call, later).items():
                kw[k] = dict(kw.get(k, {}), **v) if k == "params" else v
            assert call.run(True, **kw) == api.ERR_INVALID
            assert word in api.lib().ort_last_error().decode(), (word, api.lib().ort_last_error())
    for word, kw in order:
        assert call.run(word == "workspace", device=1 << 20, **_bend(call, kw)) == api.ERR_INVALID, word


def test_python_binding_checks_shapes(api):
    p = dc.frame(6, 4, 1)[0]
    with pytest.raises(ValueError):
        api.denoise(p["rgb"], p["m2"], p["count"], p["albedo"], p["normal"][:, :, :2], p["depth"])
    with pytest.raises(ValueError):
        api.denoise(p["rgb"], p["m2"][:-1], p["count"], p["albedo"], p["normal"], p["depth"])
    with pytest.raises(ValueError):
        api.denoise(p["rgb"][0], p["m2"][0], p["count"][0], p["albedo"][0], p["normal"][0], p["depth"][0])


# ---- the reference itself --------------------------------------------------------------------------------------------
def test_the_reference_denoises():
    """on the synthetic 77 x 61 frame at the default parameters the error against the noise-free truth falls"""
    planes, truth = dc.frame(77, 61, 3, spp=16, surfaces=2)
    out = denoise_ref.denoise(*[planes[k] for k in dc.PLANES], **dc.DEFAULTS)
    rmse = lambda a: float(np.sqrt(np.mean((a.astype("f8") - truth) ** 2)))
    before, after = rmse(planes["rgb"]), rmse(out)
    print("rmse before %.4f after %.4f" % (before, after))
    assert after < before
