"""CPU: the slabbed solver == "FCI-hip" (qemb_frag_fci_slab) from the slab operations to BE, with the device layer replaced by the scalar mock (tests/hostcheck),
against the NumPy twin of tests/fci_numpy.py and against the unslabbed solver.  The cases are those of tests/fci_slab_cases.py, which
tests/test_gpu_fci_slab.py runs on the device."""
import ctypes as C
import sys
from pathlib import Path

import pytest

import fci_slab_cases as sc

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


@pytest.mark.parametrize("n,o", sc.SHAPES)
def test_slab_ops_equal_the_twin(hlib, n, o):
    sc.check_ops(hlib, n, o)


@pytest.mark.parametrize("n,o,rows", sc.CASES)
def test_slabbed_equals_unslabbed_equals_twin(hlib, n, o, rows):
    sc.check_slab_equals_unslabbed_and_twin(hlib, n, o, rows)


@pytest.mark.parametrize("n,o,rows", sc.COLLAPSE)
def test_collapse_of_the_davidson_basis(hlib, n, o, rows):
    sc.check_collapse(hlib, n, o, rows)


def test_two_slabbed_solves_same_bits(hlib):
    sc.check_deterministic(hlib)


def test_guard_automatic_height_and_byte_count(hlib):
    sc.check_guard(hlib)


def test_solve_fci_function_takes_slab_rows(hlib):
    sc.check_solve_fci_function(hlib)


def test_h8_be2_slabbed_equals_default(hlib):
    sc.check_driver(hlib)
