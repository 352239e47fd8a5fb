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


@pytest.mark.parametrize("o,v", [(3, 5), (5, 17), (7, 9), (11, 8)])
def test_slabbed_twin_is_the_full_twin(o, v):
    """two NumPy summation orders of the same terms: 1e-13 of abs_sum (measured: at most 6e-16)"""
    args = tc.pin_inputs(o, v)
    a, b = tn.full(*args), tn.slabbed(*args)
    print(f"slabbed ({o},{v}): |d e_t| / abs_sum = {abs(a['e_t'] - b['e_t']) / a['abs_sum']:.2e}, |d abs_sum| / abs_sum = {abs(a['abs_sum'] - b['abs_sum']) / a['abs_sum']:.2e}")
    assert a["e_t"] != 0.0 and abs(a["e_t"] - b["e_t"]) <= 1e-13 * a["abs_sum"] and abs(a["abs_sum"] - b["abs_sum"]) <= 1e-13 * a["abs_sum"]


def test_stored_pins_are_the_twin():
    """tests/golden/ccsd_t_pins.npz holds every pinned shape, and every one of them but (20, 64) -- minutes of NumPy -- is what `slabbed` gives today"""
    pins = tc.stored_pins()
    assert list(pins) == tc.pinned_shapes()
    for (o, v), ref in pins.items():
        if (o, v) == tc.PRODUCTION_PIN[:2]:
            continue
        now = tn.slabbed(*tc.pin_inputs(o, v))
        assert abs(now["e_t"] - ref["e_t"]) <= 1e-13 * ref["abs_sum"] and abs(now["abs_sum"] - ref["abs_sum"]) <= 1e-13 * ref["abs_sum"], (o, v, now, ref)


# ---------------------------------------------------------------- the cases on the mock
@pytest.mark.parametrize("o,v", tc.op_shapes())
def test_op_against_the_twin(hlib, o, v):
    tc.check_op_against_twin(hlib, o, v)


@pytest.mark.parametrize("o,v,tile", tc.PIN_CASES)
def test_op_against_the_stored_twin(hlib, o, v, tile):
    """the production tile, the wave counts between one and sixteen, both sides of the LDS cap; (20, 64) takes the scalar mock minutes and runs on the device only"""
    tc.check_op_against_pin(hlib, o, v, tile)


def test_empty_cases_and_bad_arguments(hlib):
    tc.check_empty_and_bad_arguments(hlib)


@pytest.mark.parametrize("residency", tc.RESIDENCIES)
@pytest.mark.parametrize("n,o", tc.FRAGMENTS)
def test_fragment(hlib, n, o, residency):
    tc.check_fragment(hlib, n, o, residency)


@pytest.mark.parametrize("n,o,residency", tc.CAP_FRAGMENTS)
def test_fragment_at_the_tile_caps(hlib, n, o, residency):
    tc.check_cap_fragment(hlib, n, o, residency)


def test_expected_tile_at_the_borders():
    """the restated rule at the borders derived from the constants: o <= 10: 16, o = 11 .. 20: 8, o = 21 .. 40: 4, and the cut to v"""
    assert [tc.expected_tile(o, 64) for o in (2, 10, 11, 20, 21, 40, 41)] == [16, 16, 8, 8, 4, 4, 2]
    assert tc.expected_tile(21, 5) == 5 and tc.expected_tile(6, 14) == 14 and tc.expected_tile(11, 19) == 8 and tc.expected_tile(1000, 64) == 1


def test_solver_function_appends_it(hlib):
    tc.check_solver_function(hlib)


def test_refusals(hlib):
    tc.check_refusals(hlib)


def test_memory_guard(hlib):
    tc.check_memory_guard(hlib)


def test_h8_be2_driver(hlib):
    tc.check_be(hlib, "h8")
