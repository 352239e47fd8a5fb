"""-m gpu: the one-pass ovvv kernel (qemb_op_ccsd_ovvv_pass: ZB and the partial slabs of the long-K T1 term from one read of ovvv) and the variant
of the particle-hole layouts that writes the ring operands alone against NumPy, at the shapes where the kernel takes another path (tests/ovvv_pass_cases.py), and the CCSD solver with the
one-pass rule forced on against forced off.

Bound of the op test: the a-priori bound of a length-K dot product, |err| <= gamma_K (|A| . |B|), gamma_K = K u / (1 - K u), u = 2^-53, K = v for ZB and
o v^2 for the sum of the PA slabs; it holds for any order of summation, so also for the MFMA's four-term steps and the slab order."""
import os

import numpy as np
import pytest

import ovvv_pass_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("o,v", cases.SHAPES)
def test_ovvv_pass_matches_numpy(qlib, o, v):
    """outputs within the a-priori bound, NaN pads around both outputs untouched, idle workgroups (o v < G at the small shapes: check_pass looks at each slab) write zeros,
    and a second call gives the same bits"""
    G, zb_img, pa_img = cases.run_pass(qlib, o, v)
    cases.check_pass(o, v, G, zb_img, pa_img)
    G2, zb2, pa2 = cases.run_pass(qlib, o, v)
    assert G2 == G
    assert np.array_equal(zb2.view(np.uint64), zb_img.view(np.uint64)) and np.array_equal(pa2.view(np.uint64), pa_img.view(np.uint64))


def test_ovvv_pass_refuses_shapes_outside_the_rule(qlib):
    o, v = cases.REFUSED
    assert qlib.qemb_op_ccsd_ovvv_slabs(o, v) == 0
    from quemb_amd._lib import DeviceBuffer
    b = DeviceBuffer(o * v * v * v)
    assert qlib.qemb_op_ccsd_ovvv_pass(o, v, b.ptr, b.ptr, b.ptr, b.ptr, b.ptr) != 0      # the caller keeps the two products


@pytest.mark.parametrize("o,v", [(1, 1), (3, 5), (9, 33), (12, 40)])
def test_ph_layouts_ring_operands_alone(qlib, o, v):
    cases.check_layouts_ring(o, v, cases.run_layouts_ring(qlib, o, v))


def test_solver_one_pass_rule_on_against_off(qlib):
    """One fragment of (o, v) = (6, 40) solved with the rule forced on (QEMB_OVVV_PASS=1; the switch is read at every solver set-up) and forced off (=0):
    the same iteration count, |dE_corr| <= conv_tol (1e-10 Eh) and the 1-RDM within conv_tol_normt (1e-8) -- the solver's own thresholds: a
    re-association of two sums cannot move a converged result further."""
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    n, o, nf = 46, 6, 6
    h, e1 = synthetic_fragment(n, o, 4600 + o)
    s4 = eri.pack_s4(e1)
    outs = {}
    saved = os.environ.get("QEMB_OVVV_PASS")
    try:
        for sw in ("0", "1"):
            os.environ["QEMB_OVVV_PASS"] = sw
            fr = DeviceFragment(n, nf)
            fr.set_eri_s4(s4)
            outs[sw] = fr.solve(o, h, opts=default_opts(), eeval=False)
    finally:
        if saved is None:
            os.environ.pop("QEMB_OVVV_PASS", None)
        else:
            os.environ["QEMB_OVVV_PASS"] = saved
    off, on = outs["0"], outs["1"]
    de = abs(on["e_corr_mo"] - off["e_corr_mo"])
    dr = float(np.abs(on["rdm1_emb"] - off["rdm1_emb"]).max())
    print(f"one-pass rule on / off: n_iter {on['n_iter']} / {off['n_iter']}  |dE_corr| {de:.3e}  max |d rdm1| {dr:.3e}")
    assert on["n_iter"] == off["n_iter"]
    assert de <= 1e-10
    assert dr <= 1e-8
