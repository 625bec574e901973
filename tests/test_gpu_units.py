"""Per-function parity on the device at the edges: the generic ops 1-11 against the reference's outputs on the corner
sets of tests/unit_cases.py (tests/golden/unit_edges.npz); the kernels' specialised forms (ops 14-19: the box forms of
the fast paths, pdf_eval_scattering, the diffuse pdf / BSDF, the BSDF sample as produce_ray composes it, ort_sincosf)
against the generic functions' answers; 2^20 seeded records per op against the oracle; and the deterministic libm
swept over the path's argument ranges, 2^22 arguments per function.  Bit for bit; a NaN matches any NaN, and the t of
the two _finite box forms may differ from hit_aab's in the sign of a zero (all the forms claim)."""
import os

import numpy as np
import pytest

import ref_io
import unit_cases as U
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CHUNK = 1 << 18


def _device(api, recs):
    out = [api.unit_eval_device(recs[k:k + CHUNK]) for k in range(0, len(recs), CHUNK)]
    return np.concatenate(out) if out else np.zeros((0, 8), np.float32)


def test_device_generic_ops_match_reference_on_edges(api):
    z = np.load(os.path.join(GOLDEN, "unit_edges.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    got = _device(api, recs)
    for op in range(1, 12):
        sel = recs["op"] == op
        cols = 4 if op <= 4 else 8
        U.assert_match(got[sel][:, :cols], z["ref_det"][sel][:, :cols], recs["a"][sel], "device op %d vs the reference" % op)


@pytest.mark.parametrize("op", U.KERNEL_FORMS)
def test_device_kernel_forms_match_generic_on_corners(api, oracle, op):
    """each form == the device's own generic op and == the oracle's, on the corner set (op 15 / 16: p across 1e-6 too)"""
    rows = U.corners(op)
    p0 = oracle.unit_batch(U.records(6, U.variant_to_generic(op, rows)))[:, 0] if op in (15, 16) else None
    rows = U.kernel_form_rows(op, rows, p0)
    got = _device(api, U.records(op, rows))
    U.check_kernel_form(op, rows, got, lambda r: _device(api, r), "device vs device generic")
    U.check_kernel_form(op, rows, got, oracle.unit_batch, "device vs oracle")


@pytest.mark.parametrize("op", list(range(1, 12)) + list(U.KERNEL_FORMS))
def test_device_bulk_matches_oracle(api, oracle, op):
    """2^20 seeded records per op (diffuse forms: those of 2^20 that pass the upload guard, about all), in chunks"""
    n = 1 << 20
    done = 0
    for k in range(4):
        rows = U.bulk(op, n // 4, seed=100 + k)
        got = _device(api, U.records(op, rows))
        if op in U.KERNEL_FORMS:
            U.check_kernel_form(op, rows, got, oracle.unit_batch, "device bulk")
        else:
            want = oracle.unit_batch(U.records(op, rows))
            cols = 4 if op <= 4 else 8
            U.assert_match(got[:, :cols], want[:, :cols], rows, "device bulk op %d vs the oracle" % op)
        done += len(rows)
    assert done >= (n * 9) // 10


def test_device_libm_sweeps_match_oracle(api, oracle):
    """sinf / cosf (op 9) and ort_sincosf (op 19) on [0, 2 pi), atan2f(rough sqrt(e0), sqrt(1 - e0)), powf(x, 5),
    powf(x, 4) and logf on [0, 1], powf(e, y) for y <= 0 down to -inf: 2^22 arguments each, device == oracle"""
    n = 1 << 22
    seen = {}
    for name, rows in U.libm_sweeps(n):
        recs = U.records(9, rows)
        got, want = _device(api, recs), oracle.unit_batch(recs)
        U.assert_match(got[:, :5], want[:, :5], rows, "libm sweep %s" % name)
        if name == "sincos":
            sc = _device(api, U.records(19, rows[:, :1]))
            U.assert_match(sc[:, :2], want[:, :2], rows, "ort_sincosf sweep")
        seen[name] = seen.get(name, 0) + len(rows)
    assert seen == {k: n for k in ("sincos", "atan2", "pow5", "pow4", "exp")}
