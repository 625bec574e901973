"""What the host-side contract tests of the ray queries and the views (tests/test_*_host.py) share: a scene that is committed or
not, never uploaded, the render params of the pixel-job renders' cases, and caller's memory at a known alignment (test
infrastructure, next to raycast_cases.py)."""
import os

import numpy as np

from conftest import DATA


def scene(api, committed=True):
    s = api.Scene.load_scn(os.path.join(DATA, "c2_analytic.scn"))
    return s.commit() if committed else s


def params(api, **kw):
    """the render params of the pixel-job renders' contract tests: 8 x 8, 4 spp, seed 1, PIXEL, rr 0.8, unless named otherwise"""
    p = api.Scene.params(kw.pop("width", 8), kw.pop("height", 8), kw.pop("spp", 4), 1, kw.pop("policy", "pixel"), kw.pop("chunk", 0),
                         kw.pop("rect", None), kw.pop("rr", 0.8), shard=kw.pop("shard", (0, 1)), packed=kw.pop("packed", False))
    assert not kw
    return p


def adaptive_params(api, **kw):
    """the same for the adaptive render, which does not read spp: 0 unless named otherwise"""
    return params(api, **{"spp": 0, **kw})


def aligned(nbytes):
    """-> (the array that owns the memory, a 16-byte aligned address with nbytes behind it)"""
    buf = np.zeros(nbytes + 64, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf, buf.ctypes.data + off
