"""-m gpu: the slabbed solver == "FCI-hip" (qemb_frag_fci_slab) on the device -- the slab kernels, the fragment solve at every slab height, a mid-size fragment,
determinism, the guard and the BE driver -- the cases of tests/fci_slab_cases.py, which tests/test_fci_slab_hostlogic.py runs on the scalar mock.  Bars as stated
there."""
import numpy as np
import pytest

import fci_cases as fc
import fci_slab_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,o", sc.SHAPES)
def test_slab_ops_equal_the_twin(qlib, n, o):
    sc.check_ops(qlib, n, o)


@pytest.mark.parametrize("n,o,rows", sc.CASES)
def test_slabbed_equals_unslabbed_equals_twin(qlib, n, o, rows):
    sc.check_slab_equals_unslabbed_and_twin(qlib, n, o, rows)


def test_mid_size_twelve_orbitals_in_ten_slabs(qlib):
    """(12, 6): ns = 924, 853 776 determinants; rows = 100 is nine slabs and a ragged tenth of 24 rows.  Against the unslabbed solve at the bars of the small cases
    (the twin does not reach this size)."""
    n, o = 12, 6
    h = fc.inputs(n, o)[0]
    outs = []
    for rows in (0, 100):
        fr = fc.fragment(qlib, n, o)
        fr.set_fci_slab(rows)
        out = fr.solve_fci(o, h, opts=fc.scf_opts(qlib), eeval=True, want_civec=True)
        out["slab_used"] = fr.fci_slab_used()
        out["dm2"] = fr.make_rdm2("FCI-hip", with_dm1=True)
        out["dm2_cumulant"] = fr.make_rdm2("FCI-hip", with_dm1=False)
        fr.free()
        assert out["residual"] <= 1e-9
        outs.append(out)
    assert outs[0]["slab_used"] == (0, 1) and outs[1]["slab_used"] == (100, 10)
    assert np.array_equal(outs[0]["mo_coeff"], outs[1]["mo_coeff"])
    errs = sc.check_against_unslabbed(outs[1], outs[0])
    print(f"(12,6) rows = 100: n_iter = {outs[1]['n_iter']} (unslabbed {outs[0]['n_iter']}) " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert abs(np.trace(outs[1]["rdm1_mo"]) - 2 * o) < 1e-10


@pytest.mark.parametrize("n,o,rows", sc.COLLAPSE)
def test_collapse_of_the_davidson_basis(qlib, n, o, rows):
    sc.check_collapse(qlib, n, o, rows)


def test_two_slabbed_solves_same_bits(qlib):
    sc.check_deterministic(qlib)


def test_guard_automatic_height_and_byte_count(qlib):
    sc.check_guard(qlib)


def test_solve_fci_function_takes_slab_rows(qlib):
    sc.check_solve_fci_function(qlib)


def test_h8_be2_slabbed_equals_default(qlib):
    sc.check_driver(qlib)
