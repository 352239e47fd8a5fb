"""CPU: solver == "SCI-hip" from the device operations to BE.optimize, with the device layer replaced by the scalar mock (tests/hostcheck), against the twin of
tests/sci_numpy.py.  The cases are those of tests/sci_cases.py, which tests/test_gpu_sci.py runs on the device.  The twin itself is pinned first, against the
dense brute-force Hamiltonian of tests/fci_numpy.py, on which it does not depend."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import fci_numpy as fnp
import sci_cases as sc
import sci_numpy as snp
from helpers import synthetic_fragment

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


def full_space(n, o):
    st = [int(s) for s in fnp.strings(n, o)]
    return [(a, b) for a in st for b in st]


# ---------------------------------------------------------------- the twin against the existing references
@pytest.mark.parametrize("n,o", [(4, 2), (5, 3), (6, 3)])
def test_twin_hij_is_the_brute_force_matrix(n, o):
    h, e1 = synthetic_fragment(n, o, 900 + 10 * n + o)
    H = fnp.hamiltonian_matrix(h, e1, o)
    dets = full_space(n, o)
    H2 = np.array([[snp.hij(h, e1, A, B) for B in dets] for A in dets])
    assert np.abs(H - H2).max() < 1e-13 * max(1.0, np.abs(H).max())


@pytest.mark.parametrize("n,o", [(4, 2), (5, 3), (6, 3)])
def test_twin_at_vanishing_cutoff_is_fci(n, o):
    h, e1 = synthetic_fragment(n, o, 900 + 10 * n + o)
    E, c, _ = fnp.ground_state(h, e1, o)
    r = snp.select(h, e1, o, 1e-12)
    assert r["converged"] and abs(r["e"] - E) < 1e-12
    assert np.abs(snp.full_vector(r["dets"], r["c"], n, o) - c).max() < 1e-10
    d1, d2 = snp.rdm12(r["dets"], r["c"], n)
    f1, f2 = fnp.rdm12(c, n, o)
    assert np.abs(d1 - f1).max() < 1e-10 and np.abs(d2 - f2).max() < 1e-10


@pytest.mark.parametrize("n,o,family,eps", [(5, 3, "default", 1e-3), (6, 3, "strong", 1e-2)])
def test_twin_rules_on_arrays_are_the_rules_on_integers(n, o, family, eps):
    """hij_many on every pair of the full space is hij; candidates_many finds the determinants and the margin of candidates in every round"""
    h, e1 = synthetic_fragment(n, o, 900 + 10 * n + o, **sc.FAMILY[family])
    dets = full_space(n, o)
    a, b = sc.words(dets)
    N = len(dets)
    ref = np.array([[snp.hij(h, e1, A, B) for B in dets] for A in dets])
    got = snp.hij_many(h, e1, np.repeat(a, N), np.repeat(b, N), np.tile(a, N), np.tile(b, N)).reshape(N, N)
    assert np.abs(got - ref).max() < 1e-13 * max(1.0, np.abs(ref).max())
    sub = dets[::3]
    assert np.abs(snp.hamiltonian_many(h, e1, sub) - snp.hamiltonian(h, e1, sub)).max() < 1e-13 * max(1.0, np.abs(ref).max())
    for d, c, joined in snp.select(h, e1, o, eps)["history"]:
        j2, m2 = snp.candidates_many(h, e1, n, d, c, eps)
        j1, m1 = snp.candidates(h, e1, n, d, c, eps)
        assert j1 == j2 and (abs(m1 - m2) <= 1e-9 * m1 or (m2 == 0.5 and m1 >= 0.5))      # (the sums of a single's element run in another order)


@pytest.mark.parametrize("family", ["default", "strong"])
def test_twin_energy_is_variational_and_monotone_in_the_cutoff(family):
    n, o = 6, 3
    h, e1 = synthetic_fragment(n, o, 900 + 10 * n + o, **sc.FAMILY[family])
    E = fnp.ground_state(h, e1, o)[0]
    es = [snp.select(h, e1, o, eps)["e"] for eps in (1e-1, 1e-2, 3e-3, 1e-3)]
    assert all(a >= b - 1e-12 for a, b in zip(es, es[1:])) and all(e >= E - 1e-12 for e in es)
    r = snp.select(h, e1, o, 1e-2)
    assert set(r["dets"]) == {(b, a) for a, b in r["dets"]}      # closed under the exchange of the spins


# ---------------------------------------------------------------- the device operations on the mock
@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_screen_and_merge(hlib, n, o, family, eps):
    sc.check_screen_and_merge(hlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family,eps", sc.WIDE)
def test_screen_and_merge_wide_words(hlib, n, o, family, eps):
    sc.check_screen_and_merge(hlib, n, o, family, eps, state=sc.wide_state)


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_matrix(hlib, n, o, family, eps):
    sc.check_matrix(hlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family,eps", sc.WIDE)
def test_matrix_wide_words(hlib, n, o, family, eps):
    sc.check_matrix(hlib, n, o, family, eps, state=sc.wide_state)


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_spmv(hlib, n, o, family, eps):
    sc.check_spmv(hlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_rdm_op(hlib, n, o, family, eps):
    sc.check_rdm_op(hlib, n, o, family, eps)


# ---------------------------------------------------------------- the solve
@pytest.mark.parametrize("n,o,family", sc.SOLVE + [(4, 4, "default")])
def test_solve(hlib, n, o, family):
    sc.check_solve(hlib, n, o, family)


def test_collapse_of_the_davidson_basis(hlib):
    sc.check_collapse(hlib)


def test_frags_energy_for_both_values_of_use_cumulant(hlib):
    sc.check_frags_energy(hlib)


# On the scalar mock a whole solve of (10, 5) at this cutoff takes 281 s (55 M stored pairs screened, multiplied and accumulated in scalar loops, round after
# round) and a whole solve at n = 64 takes 311 s (the mock's n^6 integral transformation and its CCSD).  Here the two cases run by their single operations
# instead: (10, 5) on the twin's recorded state, against the recorded joiners and eigenpair; two electrons in 64 orbitals round by round against the oracle's
# CCSD.  tests/test_gpu_sci.py runs the whole solves as well.
def test_vanishing_cutoff_at_10_5_by_operations_on_the_recorded_state(hlib):
    sc.check_recorded_state_ops(hlib)


def test_two_electrons_in_64_orbitals_equal_ccsd_by_operations(hlib):
    sc.check_two_electrons_by_operations(hlib)


@pytest.mark.parametrize("n,o", [(6, 3), (7, 3)])
def test_vanishing_cutoff_is_fci(hlib, n, o):
    sc.check_full_space_is_fci(hlib, n, o)


@pytest.mark.parametrize("n,o,family", [(4, 2, "default"), (6, 3, "strong")])
def test_two_calls_same_bits_and_both_residencies(hlib, n, o, family):
    sc.check_repeatable_and_residencies(hlib, n, o, family)


def test_refusals_and_limits(hlib):
    sc.check_refusals(hlib)


def test_solve_sci_function(hlib):
    sc.check_solve_sci_function(hlib)


# ---------------------------------------------------------------- the BE driver
def test_h8_be2_oneshot_optimize_parallel_jacobian_and_full_basis_energy(hlib):
    sc.check_h8_be2(hlib)
