"""CPU: solver == "FCI-hip" from the C ABI to BE.optimize, with the device layer replaced by the scalar mock (tests/hostcheck), against the NumPy reference of
tests/fci_numpy.py (a brute-force determinant Hamiltonian and a string-space operator form).  The cases are those of tests/fci_cases.py, which
tests/test_gpu_fci.py runs on the device.  The reference itself is pinned first, by identities."""
import ctypes as C
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

import fci_cases as fc
import fci_numpy as fnp
import fci_pipeline as fp
from helpers import synthetic_fragment
from qemb_oracle import scf

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


# ---------------------------------------------------------------- the restatement pins itself
@pytest.mark.parametrize("n,o", [(2, 1), (3, 1), (4, 2), (5, 2), (5, 3), (6, 3), (6, 1)])
def test_the_two_forms_of_the_reference_agree_and_satisfy_the_rdm_identities(n, o):
    h, e1 = synthetic_fragment(n, o, 40 + n)
    E, c, H = fnp.ground_state(h, e1, o)
    assert np.abs(H - H.T).max() < 1e-13
    x = np.random.default_rng(n).standard_normal(c.shape)
    assert np.abs(H @ x.reshape(-1) - fnp.sigma(h, e1, x, o).reshape(-1)).max() < 1e-12
    dm1, dm2 = fnp.rdm12(c, n, o)
    assert abs(fnp.energy_from_rdms(h, e1, dm1, dm2) - E) < 1e-12
    assert abs(np.trace(dm1) - 2 * o) < 1e-12
    assert np.abs(np.einsum("pqrr->pq", dm2) - (2 * o - 1) * dm1).max() < 1e-12
    mf = scf.rhf(h, e1, o, conv_tol=1e-13, conv_tol_grad=1e-10)
    assert E < mf["e_tot"] + 1e-12


def test_reference_two_electrons_equal_the_closed_form_singlet_problem():
    """two electrons: the singlet ground state is a symmetric c[p,q]; its eigenproblem H2[(pq),(rs)] = h_pr d_qs + d_pr h_qs + (pr|qs) (the matrix of
    tests/test_oracle_ccsd.py) is solved directly"""
    n = 5
    h, e1 = synthetic_fragment(n, 1, 11)
    H2 = (np.einsum("pr,qs->pqrs", h, np.eye(n)) + np.einsum("pr,qs->pqrs", np.eye(n), h) + e1.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
    E, c, _ = fnp.ground_state(h, e1, 1)
    assert abs(E - np.linalg.eigvalsh(H2)[0]) < 1e-12
    assert np.abs(c - c.T).max() < 1e-10


def test_reference_single_determinant_is_the_mean_field_energy():
    n = 4
    h, e1 = synthetic_fragment(n, n, 5)
    E, c, H = fnp.ground_state(h, e1, n)
    assert H.shape == (1, 1)
    e_hf = 2 * np.trace(h) + 2 * np.einsum("iijj->", e1) - np.einsum("ijji->", e1)
    assert abs(E - e_hf) < 1e-12


# ---------------------------------------------------------------- the device layers on the mock
@pytest.mark.parametrize("n,o", fc.SHAPES)
def test_sigma_op(hlib, n, o):
    fc.check_sigma(hlib, n, o)


@pytest.mark.parametrize("n,o", [(4, 2), (5, 3), (7, 3)])
def test_rdm_op(hlib, n, o):
    fc.check_rdm_op(hlib, n, o)


def test_link_tables_are_the_operator_matrices(hlib):
    from quemb_amd.fragsolver import fci_links
    for n, o in [(4, 2), (5, 3), (6, 1)]:
        st, links = fci_links(n, o, lib=hlib)
        assert np.array_equal(st, fnp.strings(n, o)) and links.shape == (o * (n - o + 1), len(st))
        A = np.zeros_like(fnp.e_matrices(n, o))
        for l in range(links.shape[0]):
            for I, w in enumerate(links[l]):
                A[(w >> 1) & 255, I, w >> 9] += -1.0 if w & 1 else 1.0
        assert np.array_equal(A, fnp.e_matrices(n, o))


@pytest.mark.parametrize("n,o", fc.SHAPES)
def test_solve(hlib, n, o):
    fc.check_solve(hlib, n, o)


@pytest.mark.parametrize("n,o", [(4, 2), (6, 3)])
def test_two_calls_same_bits_and_both_residencies(hlib, n, o):
    fc.check_repeatable_and_residencies(hlib, n, o)


def test_refusals(hlib):
    fp.check_refusals(hlib)


def test_frags_energy_for_both_values_of_use_cumulant(hlib):
    fp.check_frags_energy(hlib)


def test_solve_fci_function_and_work_bytes(hlib):
    fp.check_solve_fci_function(hlib)


# ---------------------------------------------------------------- the BE driver
def test_h8_be1_fci_equals_ccsd(hlib):
    fp.check_h8_be1_equals_ccsd(hlib)


def test_h4_single_fragment_is_the_molecular_fci(hlib):
    fp.check_h4_whole_system(hlib)


def test_h8_be2_sweeps_optimize_jacobian_and_full_basis_rdms(hlib):
    fp.check_h8_be2(hlib)


def test_h8_reference_goldens(hlib):
    fp.check_goldens(hlib)
