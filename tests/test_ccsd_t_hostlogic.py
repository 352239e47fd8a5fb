"""CPU: the perturbative triples correction E_(T) from the device operations to BE.ccsd_t, with the device layer replaced by the scalar mock (tests/hostcheck),
against the twin of tests/ccsd_t_numpy.py.  The cases are those of tests/ccsd_t_cases.py, which tests/test_gpu_ccsd_t.py runs on the device.  The twin itself is
pinned first: to the brute-force evaluation in the determinant basis, on which it does not depend, to zero where there are no triples, and to size consistency."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import ccsd_t_cases as tc
import ccsd_t_numpy as tn

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize("n,o", [(4, 2), (5, 2), (5, 3)])
def test_twin_is_the_determinant_sum(n, o):
    h, e4, t1, t2, eo, ev = tn.random_system(n, o, 7 + n)
    ref = tn.brute_force(h, e4, o, t1, t2, eo, ev)
    got = tn.full(t1, t2, *tn.blocks(e4, o), eo, ev)
    print(f"twin ({n},{o}): {got['e_t']:.15f}, determinant basis {ref:.15f}, |d| = {abs(got['e_t'] - ref):.2e}")
    assert ref != 0.0 and abs(got["e_t"] - ref) <= 1e-12 * max(1.0, abs(ref))


@pytest.mark.parametrize("n,o", [(4, 1), (5, 1), (3, 2), (4, 3)])
def test_twin_vanishes_without_triples(n, o):
    """one occupied or one virtual orbital: no three electrons can leave the reference (zero to the rounding of the terms that cancel)"""
    h, e4, t1, t2, eo, ev = tn.random_system(n, o, 11 + n)
    got = tn.full(t1, t2, *tn.blocks(e4, o), eo, ev, skip_diagonal=False)      # (the expression itself, every element)
    scale = np.abs(t2).max() * np.abs(e4).max() ** 2 * n ** 6
    assert abs(got["e_t"]) <= 1e-13 * scale
    assert tn.full(t1, t2, *tn.blocks(e4, o), eo, ev)["e_t"] == 0.0
    assert tn.brute_force(h, e4, o, t1, t2, eo, ev) == 0.0


@pytest.mark.parametrize("n,o", [(5, 2), (7, 3)])
def test_twin_diagonal_elements_vanish(n, o):
    """a = b = c: W and V are invariant under the permutations of ijk, r3 of them is zero -- leaving these elements out changes the sum by their rounding only"""
    h, e4, t1, t2, eo, ev = tn.random_system(n, o, 13 + n)
    a, b = tn.full(t1, t2, *tn.blocks(e4, o), eo, ev, skip_diagonal=False), tn.full(t1, t2, *tn.blocks(e4, o), eo, ev)
    assert abs(a["e_t"] - b["e_t"]) <= 1e-13 * a["abs_sum"] and b["e_t"] != 0.0


@pytest.mark.parametrize("n,o", [(4, 2), (5, 3)])
def test_twin_is_size_consistent(n, o):
    h, e4, t1, t2, eo, ev = tn.random_system(n, o, 7 + n)
    one = tn.full(t1, t2, *tn.blocks(e4, o), eo, ev)
    two = tn.full(*tn.two_copies(t1, t2, *tn.blocks(e4, o), eo, ev))
    assert abs(two["e_t"] - 2.0 * one["e_t"]) <= 1e-12 * max(1.0, abs(one["e_t"]))


@pytest.mark.parametrize("n,o", [(5, 2), (7, 3), (9, 2)])
def test_tiled_twin_is_the_full_twin(n, o):
    h, e4, t1, t2, eo, ev = tn.random_system(n, o, 5 + n)
    a, b = tn.full(t1, t2, *tn.blocks(e4, o), eo, ev), tn.tiled(t1, t2, *tn.blocks(e4, o), eo, ev)
    assert abs(a["e_t"] - b["e_t"]) <= 1e-12 * a["abs_sum"] and abs(a["abs_sum"] - b["abs_sum"]) <= 1e-12 * a["abs_sum"]


# ---------------------------------------------------------------- the cases on the mock
@pytest.mark.parametrize("o,v", tc.op_shapes())
def test_op_against_the_twin(hlib, o, v):
    tc.check_op_against_twin(hlib, o, v)


def test_empty_cases_and_bad_arguments(hlib):
    tc.check_empty_and_bad_arguments(hlib)


@pytest.mark.parametrize("residency", tc.RESIDENCIES)
@pytest.mark.parametrize("n,o", tc.FRAGMENTS)
def test_fragment(hlib, n, o, residency):
    tc.check_fragment(hlib, n, o, residency)


def test_solver_function_appends_it(hlib):
    tc.check_solver_function(hlib)


def test_refusals(hlib):
    tc.check_refusals(hlib)


def test_memory_guard(hlib):
    tc.check_memory_guard(hlib)


def test_h8_be2_driver(hlib):
    tc.check_be(hlib, "h8")
