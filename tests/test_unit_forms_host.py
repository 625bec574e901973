"""The kernels' specialised lane functions (unit ops 14-19: the box forms, pdf_eval_scattering, the diffuse pdf / BSDF,
the BSDF sample as produce_ray composes it, ort_sincosf) against the generic functions' answers, and the generic ops
1-11 against the reference's own outputs on the corner sets of tests/unit_cases.py (tests/golden/unit_edges.npz).

Run here through tools/host_sim --unit: the lane code's own dispatch (ort_lane.h unit_eval_op) compiled for the host
with -ffp-contract=off, so the generators and the comparisons are checked without a device.  The device runs the same
records in tests/test_gpu_units.py: that is the real test of the kernels' machine code."""
import os
import subprocess

import numpy as np
import pytest

import host_sim_tool
import ref_io
import unit_cases as U
from conftest import GOLDEN


@pytest.fixture(scope="module")
def host_sim():
    return host_sim_tool.built("host_sim")


@pytest.fixture(scope="module")
def host_eval(host_sim, tmp_path_factory):
    d = tmp_path_factory.mktemp("unit")

    def run(recs):
        recs = np.ascontiguousarray(recs)
        recs.tofile(str(d / "in.bin"))
        r = subprocess.run([host_sim, "--unit", str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        return ref_io.read_unit_output(str(d / "out.bin"))
    return run


def test_host_generic_ops_match_reference_on_edges(host_eval):
    """ops 1-11 of the lane code == the reference (ref_det) on every corner record (ops 1-4: t and normal)"""
    z = np.load(os.path.join(GOLDEN, "unit_edges.npz"))
    recs = z["records"].view(ref_io.UNIT_REC_DTYPE).reshape(-1)
    got = host_eval(recs)
    for op in range(1, 12):
        sel = recs["op"] == op
        cols = 4 if op <= 4 else 8
        U.assert_match(got[sel][:, :cols], z["ref_det"][sel][:, :cols], recs["a"][sel], "host op %d vs the reference" % op)


@pytest.mark.parametrize("op", U.KERNEL_FORMS)
def test_host_kernel_forms_match_generic(host_eval, oracle, op):
    """each kernel form == the oracle's generic answer, on the corner set and 2^16 bulk records (op 15 / 16 with rr placed
    so that p straddles the 1e-6 guard as well)"""
    for name, rows in (("corners", U.corners(op)), ("bulk", U.bulk(op, 1 << 16, seed=3))):
        p0 = oracle.unit_batch(U.records(6, U.variant_to_generic(op, rows)))[:, 0] if op in (15, 16) else None
        rows = U.kernel_form_rows(op, rows, p0)
        got = host_eval(U.records(op, rows))
        U.check_kernel_form(op, rows, got, oracle.unit_batch, "host %s" % name)


def test_corner_sets_reach_their_edges(oracle):
    """the generator's corner classes are really there: radicands of exactly 0 and one step either side, p within one
    step of 1e-6, every ulp of k pi / 4, normals on both sides of the 1e-4 band, +-0 / infinite 1/d with finite and
    NaN slab products, diffuse materials with 0/0 weights, roughness other than 0.01"""
    rows = U.corners(15)
    r = U.radicand(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 18])
    assert (r == 0).sum() >= 6 and ((r > 0) & (r < 1e-6)).any() and ((r < 0) & (r > -1e-6)).any()
    assert set(np.unique(rows[:, 19])) >= {np.float32(0.01), np.float32(0.5), np.float32(1.0)}
    p0 = oracle.unit_batch(U.records(6, U.variant_to_generic(15, rows)))[:, 0]
    st = U.straddle_rr(rows, p0)
    with np.errstate(all="ignore"):
        rr0 = np.float32(1e-6) / p0
    p = p0[np.isfinite(rr0) & (rr0 > 0) & (rr0 <= 1)]
    assert len(st) == 3 * len(p) and len(p) > 100
    n = rows[:, 0:3]
    band = np.abs(np.abs(n[:, 2]) - 1)
    assert (band == 0).any() and ((band > 0) & (band < 1e-4)).any() and ((band > 1e-4) & (band < 1e-3)).any()
    q = U.quadrant_args()
    assert len(q) == 17 * 9 and all((np.abs(q - np.float32(k * np.pi / 4)) <= 4 * np.spacing(np.float32(k * np.pi / 4))).sum() == 9
                                    for k in range(1, 9))
    box = U.corners(3)
    with np.errstate(all="ignore"):
        inv = np.float32(1) / box[:, 9:12]
        prod = (box[:, 0:3] - box[:, 6:9]) * inv
    assert np.isinf(inv).any() and np.isnan(prod).any() and (np.signbit(prod) & (prod == 0)).any()
    assert len(U.finite_box_rows(box)) > 50
    d = U.corners(16)
    assert len(d) > 50 and U.is_diffuse_material(d[:, 9:12], d[:, 12:15], d[:, 15:18]).all()
    assert (np.abs(d[:, 9:18]).sum(axis=1) == 0).any()
