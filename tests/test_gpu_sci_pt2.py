"""-m gpu: the second-order correction of solver == "SCI-hip" on the device -- the row pass, the range-restricted screen, the driver over ranges of the alpha word,
the fragment call and BE.sci_pt2 -- the cases of tests/sci_pt2_cases.py, which tests/test_sci_pt2_hostlogic.py runs on the scalar mock, against the twin of
tests/sci_pt2_numpy.py.  Bars as stated there."""
import pytest

import sci_pt2_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,o,family,eps_var,eps_pt,n_ext", pc.OPS)
def test_op_against_the_twin(qlib, n, o, family, eps_var, eps_pt, n_ext):
    pc.check_op_against_twin(qlib, n, o, family, eps_var, eps_pt, n_ext)


@pytest.mark.parametrize("n,o,family,eps_var", pc.ROWS)
def test_vanishing_threshold_is_the_operator_form_sum(qlib, n, o, family, eps_var):
    pc.check_independent_of_the_twin(qlib, n, o, family, eps_var)


@pytest.mark.parametrize("n,o,family,eps_var,eps_pt,products", pc.WIDE)
def test_wide_words(qlib, n, o, family, eps_var, eps_pt, products):
    pc.check_wide_words(qlib, n, o, family, eps_var, eps_pt, products)


def test_ranges_of_the_alpha_word(qlib):
    pc.check_batches(qlib)


def test_two_calls_same_bits(qlib):
    pc.check_same_bits(qlib)


@pytest.mark.parametrize("n,o,family,eps_var", pc.ROWS)
def test_it_is_the_second_order_correction(qlib, n, o, family, eps_var):
    pc.check_is_the_second_order_correction(qlib, n, o, family, eps_var)


def test_exact_zero_at_the_cutoff_of_a_converged_solve(qlib):
    pc.check_exact_zero(qlib)


@pytest.mark.parametrize("residency", ["block", "factor"])
@pytest.mark.parametrize("n,o,family,eps_var", pc.FRAGMENTS)
def test_fragment(qlib, n, o, family, eps_var, residency):
    pc.check_fragment(qlib, n, o, family, eps_var, residency)


def test_single_determinant_gives_zero(qlib):
    pc.check_single_determinant(qlib)


def test_refusals_and_limits(qlib):
    pc.check_refusals(qlib)


def test_h8_be2_driver(qlib):
    pc.check_h8_be2(qlib)
