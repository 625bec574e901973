"""What the host-side contract tests of the ray queries and the views (tests/test_*_host.py) share: a scene that is committed or
not, never uploaded, and caller's memory at a known alignment (test infrastructure, next to raycast_cases.py)."""
import os

import numpy as np

from conftest import DATA


def scene(api, committed=True):
    s = api.Scene.load_scn(os.path.join(DATA, "c2_analytic.scn"))
    return s.commit() if committed else s


def aligned(nbytes):
    """-> (the array that owns the memory, a 16-byte aligned address with nbytes behind it)"""
    buf = np.zeros(nbytes + 64, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf, buf.ctypes.data + off
