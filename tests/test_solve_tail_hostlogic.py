"""CPU: the tail the CCSD, MP2 and FCI-hip fragment solvers share, with the device layer replaced by the scalar mock (tests/hostcheck).  The cases are those of
tests/solve_tail_cases.py, which tests/test_gpu_solve_tail.py runs on the device."""
import ctypes as C
import sys
from pathlib import Path

import pytest

import solve_tail_cases as tc

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


@pytest.mark.parametrize("n,o", tc.SHAPES)
def test_mean_field_part_is_the_same_bits_on_every_path(hlib, n, o):
    tc.check_mean_field_part_is_shared(hlib, n, o)


@pytest.mark.parametrize("path", tc.PATHS)
@pytest.mark.parametrize("n,o", tc.SHAPES)
def test_rdm1_emb_is_symmetric_and_the_back_rotated_rdm1_mo(hlib, n, o, path):
    tc.check_back_rotation(hlib, n, o, path)


@pytest.mark.parametrize("solver", ["CCSD", "MP2", "FCI-hip"])
def test_energy_evaluation_without_energy_data_is_refused(hlib, solver):
    tc.check_energy_data_is_required(hlib, solver)


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_batch_equals_serial(hlib, solver):
    tc.check_batch_equals_serial(hlib, solver)
