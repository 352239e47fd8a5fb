"""The Cholesky-decomposed AO integrals (csrc/int4c.cpp: int4c_cholesky) through the scalar twin of the mock library: the whole blocked decomposition -- diagonal,
panel selection, panel columns by the kTile form, the GEMM update, the in-panel factorisation, the new vectors, the diagonal update and the final permutation --
the identity-metric DF context, the memory guard, the refusals and the Python surface up to BE(int_transform="cholesky-hip"), without a device."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import cholesky_cases as cases
from quemb_amd import _lib


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("tol", cases.TOLS)
@pytest.mark.parametrize("name", ["h8_sto3g", "h4_ccpvdz", "spd3", "spd_atom"])
def test_bound_and_rank(hlib, name, tol):
    cases.check_bound_and_rank(hlib, name, tol)


def test_panel_independence(hlib):
    cases.check_panel_independence(hlib)


def test_reproducible(hlib):
    cases.check_reproducible(hlib)


def test_layout_in_the_df_context(hlib):
    cases.check_layout(hlib)


@pytest.mark.parametrize("tol", cases.TOLS)
@pytest.mark.parametrize("name", ["h8_sto3g", "spd3"])
def test_consumer_against_the_stored_route(hlib, name, tol):
    cases.check_consumer(hlib, name, tol)


@pytest.mark.parametrize("case", ["rank7", "twins", "one", "n86", "n140"])
def test_panel_kernel(hlib, case):
    cases.check_panel_kernel(hlib, case)


def test_diag_update_kernel(hlib):
    cases.check_diag_kernel(hlib)


def test_permute_kernel(hlib):
    cases.check_permute_kernel(hlib)


@pytest.mark.parametrize("solver", ["MP2", "CCSD"])
def test_be_end_to_end(hlib, solver):
    cases.check_end_to_end(hlib, solver)


def test_refusals(hlib):
    cases.check_refusals(hlib)
