"""-m gpu: solver == "FCI-hip" on the device -- one application of H, the RDM build, the fragment solve, the refusals, the BE driver and the reference's golden
energies -- the cases of tests/fci_cases.py and tests/fci_pipeline.py, which tests/test_fci_hostlogic.py runs on the scalar mock, against the NumPy reference of
tests/fci_numpy.py.  Bars as stated there."""
import pytest

import fci_cases as fc
import fci_pipeline as fp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,o", fc.SHAPES)
def test_sigma_op(qlib, n, o):
    fc.check_sigma(qlib, n, o)


@pytest.mark.parametrize("n,o", [(4, 2), (5, 3), (7, 3)])
def test_rdm_op(qlib, n, o):
    fc.check_rdm_op(qlib, n, o)


@pytest.mark.parametrize("n,o", fc.SHAPES)
def test_solve(qlib, n, o):
    fc.check_solve(qlib, n, o)


@pytest.mark.parametrize("n,o", [(4, 2), (6, 3), (7, 3)])
def test_two_calls_same_bits_and_both_residencies(qlib, n, o):
    fc.check_repeatable_and_residencies(qlib, n, o)


def test_refusals(qlib):
    fp.check_refusals(qlib)


def test_frags_energy_for_both_values_of_use_cumulant(qlib):
    fp.check_frags_energy(qlib)


def test_solve_fci_function(qlib):
    fp.check_solve_fci_function(qlib)


def test_h8_be1_fci_equals_ccsd(qlib):
    fp.check_h8_be1_equals_ccsd(qlib)


def test_h4_single_fragment_is_the_molecular_fci(qlib):
    fp.check_h4_whole_system(qlib)


def test_h8_be2_sweeps_optimize_jacobian_and_full_basis_rdms(qlib):
    fp.check_h8_be2(qlib)


def test_h8_reference_goldens(qlib):
    fp.check_goldens(qlib)
