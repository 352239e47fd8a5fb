"""CPU: the second-order correction of solver == "SCI-hip" from the device operations to BE.sci_pt2, with the device layer replaced by the scalar mock
(tests/hostcheck), against the twin of tests/sci_pt2_numpy.py.  The cases are those of tests/sci_pt2_cases.py, which tests/test_gpu_sci_pt2.py runs on the device.
The twin itself is pinned first, against the dense brute-force Hamiltonian of tests/fci_numpy.py, on which it does not depend."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import fci_numpy as fnp
import sci_cases as sc
import sci_numpy as snp
import sci_pt2_cases as pc
import sci_pt2_numpy as ptn

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


# ---------------------------------------------------------------- the twin against the existing references
@pytest.mark.parametrize("n,o,family,eps_var", pc.ROWS)
def test_twin_is_the_dense_sum(n, o, family, eps_var):
    """at a threshold no product falls under, the twin is sum_{a outside V} (H c)_a^2 / (E - H_aa) from the brute-force matrix, and every determinant that H
    connects to the space with a non-zero product (or whose partner is so connected) is counted"""
    hm, Vm, dets, c, e = pc.state(n, o, family, eps_var)
    r = ptn.pt2(hm, Vm, n, dets, c, e, 1e-300)
    H = fnp.hamiltonian_matrix(hm, Vm, o)
    full = snp.full_vector(dets, c, n, o).reshape(-1)
    outside = snp.full_vector(dets, np.ones(len(dets)), n, o).reshape(-1) == 0.0
    sig = (H @ full)[outside]
    contrib = sig ** 2 / (e - np.diag(H)[outside])
    assert abs(r["e_pt2"] - contrib.sum()) <= 1e-13 * np.abs(contrib).sum()
    assert r["n_ext"] <= int(outside.sum()) and r["e_pt2"] < 0.0


def test_twin_on_arrays_is_the_twin_on_integers():
    hm, Vm, dets, c, e = pc.state(7, 3, "default", 1e-3)
    for eps_pt in (1e-4, 1e-6):
        a, b = ptn.pt2(hm, Vm, 7, dets, c, e, eps_pt), ptn.pt2_many(hm, Vm, 7, dets, c, e, eps_pt)
        assert a["keys"] == b["keys"] and a["products"] == b["products"] and abs(a["margin"] - b["margin"]) <= 1e-9 * a["margin"]
        assert np.abs(a["contrib"] - b["contrib"]).max() <= 1e-13 * a["abs_sum"]


def test_twin_partner_without_a_passing_product_counts_and_adds_nothing():
    hm, Vm, dets, c, e = pc.state(6, 3, "default", 1e-2)
    r = ptn.pt2(hm, Vm, 6, dets, c, e, 1e-4)
    keys = set(r["keys"])
    assert all((b, a) in keys for a, b in keys)      # closed under the exchange of the spins
    assert all(x <= 0.0 for x in r["contrib"])       # e_var lies below every diagonal element outside the space here


# ---------------------------------------------------------------- the cases on the mock
@pytest.mark.parametrize("n,o,family,eps_var,eps_pt,n_ext", pc.OPS)
def test_op_against_the_twin(hlib, n, o, family, eps_var, eps_pt, n_ext):
    pc.check_op_against_twin(hlib, n, o, family, eps_var, eps_pt, n_ext)


@pytest.mark.parametrize("n,o,family,eps_var", pc.ROWS)
def test_vanishing_threshold_is_the_operator_form_sum(hlib, n, o, family, eps_var):
    pc.check_independent_of_the_twin(hlib, n, o, family, eps_var)


@pytest.mark.parametrize("n,o,family,eps_var,eps_pt,products", pc.WIDE)
def test_wide_words(hlib, n, o, family, eps_var, eps_pt, products):
    pc.check_wide_words(hlib, n, o, family, eps_var, eps_pt, products)


def test_ranges_of_the_alpha_word(hlib):
    pc.check_batches(hlib, wide_max_ext=16384)


def test_two_calls_same_bits(hlib):
    pc.check_same_bits(hlib)


@pytest.mark.parametrize("n,o,family,eps_var", pc.ROWS)
def test_it_is_the_second_order_correction(hlib, n, o, family, eps_var):
    pc.check_is_the_second_order_correction(hlib, n, o, family, eps_var)


def test_exact_zero_at_the_cutoff_of_a_converged_solve(hlib):
    pc.check_exact_zero(hlib)


@pytest.mark.parametrize("residency", ["block", "factor"])
@pytest.mark.parametrize("n,o,family,eps_var", pc.FRAGMENTS)
def test_fragment(hlib, n, o, family, eps_var, residency):
    pc.check_fragment(hlib, n, o, family, eps_var, residency)


def test_single_determinant_gives_zero(hlib):
    pc.check_single_determinant(hlib)


def test_refusals_and_limits(hlib):
    pc.check_refusals(hlib)


def test_h8_be2_driver(hlib):
    pc.check_h8_be2(hlib)
