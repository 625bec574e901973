"""The denoiser on the device (ort_denoise, ort_denoise_device; kernels denoise_pack and denoise_atrous of ort_denoise.h): every
shared case of tests/denoise_cases.py through the library against the numpy restatement of the contract (tests/denoise_ref.py)
and against the host build of the same pixel functions (tools/denoise_sim), bit for bit, a NaN by position; and what only a device
shows: the device form with the caller's workspace, guard words around everything it may write, in place, on a stream of the
caller's, and a workspace one byte short.  One real frame: the bunny room at 64 x 48.  No case holds anything but ordinary floats
in ordinary memory: nothing here can fault."""
import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref

pytestmark = pytest.mark.gpu

GUARD = 64   # words of 0xA5A5A5A5 either side of every device buffer a call may write


@pytest.fixture(scope="module")
def dev(api):
    assert api.device_count() >= 1, "GPU test on a machine without a HIP device (the denoiser has no CPU fallback)"
    import torch
    return torch.device("cuda", 0)


def _library(api, name, **kw):
    planes, params = dc.CASES[name]
    return api.denoise(*[planes[k] for k in dc.PLANES], **dict(params, **kw))


@pytest.mark.parametrize("name", dc.NAMES)
def test_library_matches_the_contract(api, dev, name):
    out, st = _library(api, name)
    dc.assert_same_frame(out, dc.reference(name), name)
    assert st["kernel_ms"] > 0 and all(v == 0 for k, v in st.items() if k != "kernel_ms")


@pytest.mark.parametrize("name", ["hostile", "hostile_it8_sq0", "67x45", "batch3_23x19", "corner_sl1e-20", "corner_sl1e20", "1x1"])
def test_library_matches_the_host_build(api, dev, name, tmp_path):
    planes, params = dc.CASES[name]
    r, want = dc.run_sim(dc.built("denoise_sim"), planes, params, tmp_path)
    assert r.returncode == 0, r.stderr
    dc.assert_same_frame(_library(api, name)[0], want, name)


def test_batch_frames_equal_their_single_frame_calls(api, dev):
    planes, params = dc.CASES["batch3_23x19"]
    whole, _ = _library(api, "batch3_23x19")
    for v in range(3):
        one, _ = api.denoise(*[planes[k][v] for k in dc.PLANES], **params)
        dc.assert_same_frame(whole[v], one, "frame %d" % v)


def test_host_form_in_place(api, dev):
    planes, params = dc.CASES["hostile"]
    rgb = planes["rgb"].copy()
    out, _ = api.denoise(rgb, *[planes[k] for k in dc.PLANES[1:]], out=rgb, **params)
    assert out is rgb
    dc.assert_same_frame(rgb, dc.reference("hostile"), "in place")


class _Device:
    """a case's planes as torch tensors, out and the workspace between guard words"""

    def __init__(self, api, dev, name, in_place=False):
        import torch
        self.torch, self.api = torch, api
        self.planes, self.params = dc.CASES[name]
        count = self.planes["count"]
        self.shape = count.shape
        self.frames = 1 if count.ndim == 2 else len(count)
        self.h, self.w = count.shape[-2:]
        n = count.size
        self.t = {k: self._guarded(np.ascontiguousarray(self.planes[k]).view("<i4").reshape(-1), dev) for k in dc.PLANES}
        self.ws_bytes = api.denoise_workspace_bytes(self.w, self.h, self.frames)
        assert self.ws_bytes == 48 * n
        self.ws = self._guarded(np.zeros(12 * n, "<i4"), dev)
        self.out = self.t["rgb"] if in_place else self._guarded(np.full(3 * n, 0x5EED5EED, "<i4"), dev)

    def _guarded(self, words, dev):
        whole = np.full(len(words) + 2 * GUARD, 0xA5A5A5A5, "<u4").view("<i4")
        whole[GUARD:-GUARD] = words
        return self.torch.from_numpy(whole).to(dev)

    def ptr(self, t):
        return t.data_ptr() + 4 * GUARD

    def run(self, stream=None, want_stats=False, ws_bytes=None):
        return self.api.denoise_device(*[self.ptr(self.t[k]) for k in dc.PLANES], self.w, self.h, self.ptr(self.out), self.ptr(self.ws),
                                       self.ws_bytes if ws_bytes is None else ws_bytes, frame_count=self.frames, stream=stream, want_stats=want_stats,
                                       **self.params)

    def frame(self):
        self.torch.cuda.synchronize()
        for k, t in list(self.t.items()) + [("workspace", self.ws), ("out", self.out)]:
            w = t.cpu().numpy().view("<u4")
            assert (w[:GUARD] == 0xA5A5A5A5).all() and (w[-GUARD:] == 0xA5A5A5A5).all(), "guard words of %s overwritten" % k
        for k in dc.PLANES:
            if self.t[k] is not self.out:
                assert np.array_equal(self.t[k].cpu().numpy()[GUARD:-GUARD].view("<u4"), np.ascontiguousarray(self.planes[k]).view("<u4").reshape(-1)), \
                    "input plane %s was written" % k
        return self.out.cpu().numpy()[GUARD:-GUARD].view("<f4").reshape(self.shape + (3,))


@pytest.mark.parametrize("name", ["hostile", "batch3_23x19", "33x17_it6", "corner_it1", "1x1"])
def test_device_form_with_the_callers_workspace(api, dev, name):
    """the workspace's base is 256 bytes into a torch allocation: 16-byte aligned; an odd and an even iteration count end on
    either of its two colour planes"""
    d = _Device(api, dev, name)
    st = d.run(want_stats=True)
    assert st["kernel_ms"] > 0 and all(v == 0 for k, v in st.items() if k != "kernel_ms")
    dc.assert_same_frame(d.frame(), dc.reference(name), name)


@pytest.mark.parametrize("name", ["hostile", "batch3_23x19"])
def test_device_form_in_place(api, dev, name):
    d = _Device(api, dev, name, in_place=True)
    assert d.run() is None
    dc.assert_same_frame(d.frame(), dc.reference(name), name + " in place")


def test_device_form_on_a_stream_of_the_callers(api, dev):
    """two calls chained on one non-default stream without a wait between them, the second on the first's output in place of the
    colour: what the stream orders is what the reference computes in that order"""
    import torch
    d = _Device(api, dev, "67x45")
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    d.run(stream=stream.cuda_stream)
    first = d.out
    d.t = dict(d.t, rgb=first)
    d.out = d._guarded(np.zeros(3 * d.planes["count"].size, "<i4"), dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    d.run(stream=stream.cuda_stream)
    stream.synchronize()
    planes, params = dc.CASES["67x45"]
    once = dc.reference("67x45")
    twice = denoise_ref.denoise(once, *[planes[k] for k in dc.PLANES[1:]], **params)
    torch.cuda.synchronize()
    dc.assert_same_frame(first.cpu().numpy()[GUARD:-GUARD].view("<f4").reshape(once.shape), once, "first call")
    dc.assert_same_frame(d.out.cpu().numpy()[GUARD:-GUARD].view("<f4").reshape(once.shape), twice, "second call")


def test_a_workspace_one_byte_short_is_refused_without_a_launch(api, dev):
    d = _Device(api, dev, "5x3")
    for kw in (dict(ws_bytes=d.ws_bytes - 1), dict(ws_bytes=0)):
        with pytest.raises(api.OrtError) as e:
            d.run(**kw)
        assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.OrtError) as e:
        api.denoise_device(*[d.ptr(d.t[k]) for k in dc.PLANES], d.w, d.h, d.ptr(d.out), d.ptr(d.ws) + 4, d.ws_bytes, **d.params)
    assert e.value.code == api.ERR_INVALID
    d.torch.cuda.synchronize()
    out = d.out.cpu().numpy().view("<u4")
    assert (out[GUARD:-GUARD] == 0x5EED5EED).all() and (d.ws.cpu().numpy()[GUARD:-GUARD] == 0).all(), "a refused call wrote"


def test_a_real_frame(api, gpu_scene):
    """the bunny room at 64 x 48: render_adaptive(min == max == 8) gives rgb, spp and m2, render_features(spp = 8) the guides; the
    Accumulator's own denoise() on the same samples gives the same frame"""
    scene = gpu_scene("c3_bunny_room")
    w, h = 64, 48
    rgb, spp, m2, _ = scene.render_adaptive(w, h, 8, 8, 0.3, seed=11)
    assert (spp == 8).all()
    planes, _ = scene.render_features(w, h, 8, 11, want=("albedo", "normal", "depth"))
    out, st = api.denoise(rgb, m2, spp, planes["albedo"], planes["normal"], planes["depth"], **dc.DEFAULTS)
    want = denoise_ref.denoise(rgb, m2, spp, planes["albedo"], planes["normal"], planes["depth"], **dc.DEFAULTS)
    dc.assert_same_frame(out, want, "bunny room")
    changed = (out.view("<u4") != rgb.view("<u4")).any(axis=-1).mean()
    assert changed > 0.5, "the filter left %.0f %% of the frame as it was" % (100 * (1 - changed))
    acc = api.Accumulator(w, h)
    scene.render_accumulate(acc, 8, 11)
    got, _ = acc.denoise(planes, **dc.DEFAULTS)
    dc.assert_same_frame(got, denoise_ref.denoise(acc.rgb(), acc.m2, acc.count, planes["albedo"], planes["normal"], planes["depth"], **dc.DEFAULTS), "accumulator")
