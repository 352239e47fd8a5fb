"""-m gpu: the perturbative triples correction E_(T) on the device -- the batched products of the particle term, the assembly kernel in its LDS and global
forms, the fixed-order sums, the fragment call and BE.ccsd_t -- the cases of tests/ccsd_t_cases.py, which tests/test_ccsd_t_hostlogic.py runs on the scalar
mock, against the twin of tests/ccsd_t_numpy.py.  Bars as stated there."""
import pytest

import ccsd_t_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("o,v", tc.op_shapes())
def test_op_against_the_twin(qlib, o, v):
    tc.check_op_against_twin(qlib, o, v)


def test_empty_cases_and_bad_arguments(qlib):
    tc.check_empty_and_bad_arguments(qlib)


@pytest.mark.parametrize("residency", tc.RESIDENCIES)
@pytest.mark.parametrize("n,o", tc.FRAGMENTS)
def test_fragment(qlib, n, o, residency):
    tc.check_fragment(qlib, n, o, residency)


def test_solver_function_appends_it(qlib):
    tc.check_solver_function(qlib)


def test_refusals(qlib):
    tc.check_refusals(qlib)


def test_memory_guard(qlib):
    tc.check_memory_guard(qlib)


@pytest.mark.parametrize("which", ["h8", "octane"])
def test_be2_driver(qlib, which):
    tc.check_be(qlib, which)
