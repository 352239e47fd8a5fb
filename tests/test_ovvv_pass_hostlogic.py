"""CPU: the scalar twins (tests/hostcheck mock library) of the one-pass ovvv operations -- qemb_op_ccsd_ovvv_pass and the variant of the
particle-hole layouts that writes the ring operands alone, qemb_op_ccsd_ph_layouts_ring -- against numpy.einsum on random operands (tests/ovvv_pass_cases.py), and the shape rule."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import ovvv_pass_cases as cases

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))

SHAPES = [(1, 1), (3, 5), (8, 16), (9, 33), (13, 31), (25, 20)]


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


@pytest.mark.parametrize("o,v", SHAPES)
def test_ovvv_pass_mock_matches_einsum(hlib, o, v):
    G, zb_img, pa_img = cases.run_pass(hlib, o, v)
    cases.check_pass(o, v, G, zb_img, pa_img)
    G2, zb2, pa2 = cases.run_pass(hlib, o, v)
    assert G2 == G and np.array_equal(zb2, zb_img, equal_nan=True) and np.array_equal(pa2, pa_img, equal_nan=True)


@pytest.mark.parametrize("o,v", SHAPES[:4])
def test_ph_layouts_ring_mock_matches_numpy(hlib, o, v):
    cases.check_layouts_ring(o, v, cases.run_layouts_ring(hlib, o, v))


def test_shape_rule_refuses_what_the_kernel_does_not_take(hlib):
    o, v = cases.REFUSED
    assert hlib.qemb_op_ccsd_ovvv_slabs(o, v) == 0
    one = np.zeros(o * v * v * v)
    assert hlib.qemb_op_ccsd_ovvv_pass(o, v, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data) != 0
    for (o, v) in cases.SHAPES:
        assert hlib.qemb_op_ccsd_ovvv_slabs(o, v) > 0
    # n_virt beyond the accumulator tiles (ceil(v/16) NT <= 48) or the staged rows (ceil(v/16) + NT <= 18) of the kernel
    assert hlib.qemb_op_ccsd_ovvv_slabs(20, 240) > 0 and hlib.qemb_op_ccsd_ovvv_slabs(20, 241) == 0
    assert hlib.qemb_op_ccsd_ovvv_slabs(30, 192) > 0 and hlib.qemb_op_ccsd_ovvv_slabs(30, 193) == 0
    assert hlib.qemb_op_ccsd_ovvv_slabs(8, 272) > 0 and hlib.qemb_op_ccsd_ovvv_slabs(8, 273) == 0


def test_solver_one_pass_rule_on_against_off_on_the_mock(hlib):
    """the wiring in CcsdSolver::update_amps (S as Theta in slab order, ZB and the PA slabs from the one pass, PB from t2 itself) on the mock: one fragment of (o, v) = (4, 20)
    with QEMB_OVVV_PASS=1 against =0 (read at every solver set-up): same iteration count, |dE_corr| <= conv_tol = 1e-10, 1-RDM within conv_tol_normt = 1e-8"""
    import os
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    n, o, nf = 24, 4, 5
    h, e1 = synthetic_fragment(n, o, 2400 + o)
    s4 = eri.pack_s4(e1)
    outs = {}
    saved = os.environ.get("QEMB_OVVV_PASS")
    try:
        for sw in ("0", "1"):
            os.environ["QEMB_OVVV_PASS"] = sw
            fr = DeviceFragment(n, nf, lib=hlib)
            fr.set_eri_s4(s4)
            outs[sw] = fr.solve(o, h, opts=default_opts(lib=hlib), eeval=False)
    finally:
        if saved is None:
            os.environ.pop("QEMB_OVVV_PASS", None)
        else:
            os.environ["QEMB_OVVV_PASS"] = saved
    off, on = outs["0"], outs["1"]
    assert on["n_iter"] == off["n_iter"]
    assert abs(on["e_corr_mo"] - off["e_corr_mo"]) <= 1e-10
    assert np.abs(on["rdm1_emb"] - off["rdm1_emb"]).max() <= 1e-8
