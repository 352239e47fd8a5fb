"""CPU: the scalar twins (tests/hostcheck mock library) of the one-pass ring preparation, qemb_op_ccsd_ring_prep, and of the rank-n_occ update of U with its
transposed addend, qemb_op_ccsd_u_update, against the extended-precision NumPy references on random operands (tests/ring_prep_cases.py), the shape rule, and the wiring in CcsdSolver::update_amps with the rule forced on against forced off."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import pytest

import ring_prep_cases as cases

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


@pytest.mark.parametrize("o,v", cases.SHAPES)
def test_ring_prep_mock_matches_reference(hlib, o, v):
    first = cases.run(hlib, o, v)
    cases.check_outputs(o, v, *first)
    again = cases.run(hlib, o, v)
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(first, again))


@pytest.mark.parametrize("o,v", cases.SHAPES)
def test_u_update_mock_matches_reference(hlib, o, v):
    first = cases.run_u(hlib, o, v)
    cases.check_u(o, v, *first)
    again = cases.run_u(hlib, o, v)
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(first, again))


def test_shape_rule(hlib):
    """a shape outside the kernel's limits is an error of the operation and 'off' for the solver whatever the switch says; a fragment in the replay regime
    reports 'off' unless the switch forces the pass; outside it the pass is on unless the switch forbids it"""
    o, v = cases.REFUSED
    one = np.zeros(o * v * o * v)
    p = one.ctypes.data
    assert hlib.qemb_op_ccsd_ring_prep(o, v, p, p, p, p, p, p, p, p, p, p) != 0
    assert b"shape" in hlib.qemb_last_error()
    assert hlib.qemb_op_ccsd_ring_prep(4, 4097, p, p, p, p, p, p, p, p, p, p) != 0
    assert hlib.qemb_op_ccsd_u_update(o, v, p, p, p, p) != 0 and hlib.qemb_op_ccsd_u_update(4, 4097, p, p, p, p) != 0
    saved = os.environ.get("QEMB_RING_PREP")
    try:
        os.environ.pop("QEMB_RING_PREP", None)
        for (o, v) in cases.SHAPES + [(20, 200), (32, 4096)]:
            assert hlib.qemb_op_ccsd_ring_prep_rule(o, v, 1) == 0      # replay regime: the recorded sequence stays
            assert hlib.qemb_op_ccsd_ring_prep_rule(o, v, 0) == 1
        for sw, want_replay, want_large in (("0", 0, 0), ("1", 1, 1)):
            os.environ["QEMB_RING_PREP"] = sw
            assert hlib.qemb_op_ccsd_ring_prep_rule(6, 40, 1) == want_replay
            assert hlib.qemb_op_ccsd_ring_prep_rule(20, 200, 0) == want_large
            assert hlib.qemb_op_ccsd_ring_prep_rule(*cases.REFUSED, 0) == 0 and hlib.qemb_op_ccsd_ring_prep_rule(4, 4097, 0) == 0
    finally:
        if saved is None:
            os.environ.pop("QEMB_RING_PREP", None)
        else:
            os.environ["QEMB_RING_PREP"] = saved


def test_solver_ring_prep_on_against_off_on_the_mock(hlib):
    """the wiring in CcsdSolver::update_amps (the first ring product with beta = 0 as P1, the raw ZB and ZC, the two slab images of ovoo, R and W2 out; U += ZB^T inside the rank-n_occ update of U) on the mock:
    one fragment of (o, v) = (4, 20) with QEMB_RING_PREP=1 against =0 (read at every solver set-up): the same iteration count and |dE_corr| <= 1e-11 Eh, an
    order below the solver's convergence threshold -- the two paths differ in the order of a few additions only"""
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    n, o, nf = 24, 4, 5
    h, e1 = synthetic_fragment(n, o, 2400 + o)
    s4 = eri.pack_s4(e1)
    outs = {}
    saved = os.environ.get("QEMB_RING_PREP")
    try:
        for sw in ("0", "1"):
            os.environ["QEMB_RING_PREP"] = sw
            fr = DeviceFragment(n, nf, lib=hlib)
            fr.set_eri_s4(s4)
            outs[sw] = fr.solve(o, h, opts=default_opts(lib=hlib), eeval=False)
    finally:
        if saved is None:
            os.environ.pop("QEMB_RING_PREP", None)
        else:
            os.environ["QEMB_RING_PREP"] = saved
    off, on = outs["0"], outs["1"]
    de = abs(on["e_corr_mo"] - off["e_corr_mo"])
    print(f"ring preparation on / off (mock): n_iter {on['n_iter']} / {off['n_iter']}  |dE_corr| {de:.3e}")
    assert on["n_iter"] == off["n_iter"]
    assert de <= 1e-11
    assert np.abs(on["rdm1_emb"] - off["rdm1_emb"]).max() <= 1e-8
