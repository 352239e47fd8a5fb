"""-m gpu: the tail the CCSD, MP2 and FCI-hip fragment solvers share, on the device -- the cases of tests/solve_tail_cases.py, which
tests/test_solve_tail_hostlogic.py runs on the scalar mock.  Bars as stated there."""
import pytest

import solve_tail_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,o", tc.SHAPES)
def test_mean_field_part_is_the_same_bits_on_every_path(qlib, n, o):
    tc.check_mean_field_part_is_shared(qlib, n, o)


@pytest.mark.parametrize("path", tc.PATHS)
@pytest.mark.parametrize("n,o", tc.SHAPES)
def test_rdm1_emb_is_symmetric_and_the_back_rotated_rdm1_mo(qlib, n, o, path):
    tc.check_back_rotation(qlib, n, o, path)


@pytest.mark.parametrize("solver", ["CCSD", "MP2", "FCI-hip"])
def test_energy_evaluation_without_energy_data_is_refused(qlib, solver):
    tc.check_energy_data_is_required(qlib, solver)


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_batch_equals_serial(qlib, solver):
    tc.check_batch_equals_serial(qlib, solver)
