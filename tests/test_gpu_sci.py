"""-m gpu: solver == "SCI-hip" on the device -- the screen, the merge, the CSR matrix, its product, the RDMs, the fragment solve, the limits and the BE driver --
the cases of tests/sci_cases.py, which tests/test_sci_hostlogic.py runs on the scalar mock, against the twin of tests/sci_numpy.py.  Bars as stated there."""
import pytest

import sci_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_screen_and_merge(qlib, n, o, family, eps):
    sc.check_screen_and_merge(qlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family,eps", sc.WIDE)
def test_screen_and_merge_wide_words(qlib, n, o, family, eps):
    sc.check_screen_and_merge(qlib, n, o, family, eps, state=sc.wide_state)


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_matrix(qlib, n, o, family, eps):
    sc.check_matrix(qlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family,eps", sc.WIDE)
def test_matrix_wide_words(qlib, n, o, family, eps):
    sc.check_matrix(qlib, n, o, family, eps, state=sc.wide_state)


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_spmv(qlib, n, o, family, eps):
    sc.check_spmv(qlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family,eps", sc.OPS)
def test_rdm_op(qlib, n, o, family, eps):
    sc.check_rdm_op(qlib, n, o, family, eps)


@pytest.mark.parametrize("n,o,family", sc.SOLVE + [(4, 4, "default")])
def test_solve(qlib, n, o, family):
    sc.check_solve(qlib, n, o, family)


def test_collapse_of_the_davidson_basis(qlib):
    sc.check_collapse(qlib)


def test_frags_energy_for_both_values_of_use_cumulant(qlib):
    sc.check_frags_energy(qlib)


@pytest.mark.parametrize("n,o", [(6, 3), (7, 3), (10, 5)])
def test_vanishing_cutoff_is_fci(qlib, n, o):
    sc.check_full_space_is_fci(qlib, n, o)


def test_two_electrons_in_64_orbitals_equal_ccsd(qlib):
    sc.check_two_electrons_in_64_orbitals(qlib)


def test_vanishing_cutoff_at_10_5_by_operations_on_the_recorded_state(qlib):
    sc.check_recorded_state_ops(qlib)


def test_two_electrons_in_64_orbitals_equal_ccsd_by_operations(qlib):
    sc.check_two_electrons_by_operations(qlib)


@pytest.mark.parametrize("n,o,family", [(4, 2, "default"), (6, 3, "strong"), (7, 3, "default")])
def test_two_calls_same_bits_and_both_residencies(qlib, n, o, family):
    sc.check_repeatable_and_residencies(qlib, n, o, family)


def test_refusals_and_limits(qlib):
    sc.check_refusals(qlib)


def test_solve_sci_function(qlib):
    sc.check_solve_sci_function(qlib)


def test_h8_be2_oneshot_optimize_parallel_jacobian_and_full_basis_energy(qlib):
    sc.check_h8_be2(qlib)
