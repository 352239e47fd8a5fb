"""The Cholesky-decomposed AO integrals on the device (csrc/cd_ops.hip: cd_gather_kernel, cd_panel_kernel, cd_newrows_kernel, cd_diag_kernel, cd_pairmax_kernel,
cd_unpack_kernel; driver csrc/int4c.cpp: int4c_cholesky): the element-wise bound against the stored integrals, the rank against full pivoting, panel
independence, bit reproducibility across execution contexts, the layout inside the DF context, the consumer against the stored route, the new kernels on
their own, BE end to end and the refusals.  The cases are those of cholesky_cases.py, shared with the scalar-twin tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import cholesky_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tol", cases.TOLS)
@pytest.mark.parametrize("name", ["h8_sto3g", "h4_ccpvdz", "spd3", "spd_atom"])
def test_bound_and_rank(qlib, name, tol):
    cases.check_bound_and_rank(qlib, name, tol)


def test_panel_independence(qlib):
    cases.check_panel_independence(qlib)


def test_reproducible(qlib):
    cases.check_reproducible(qlib)


def test_layout_in_the_df_context(qlib):
    cases.check_layout(qlib)


@pytest.mark.parametrize("tol", cases.TOLS)
@pytest.mark.parametrize("name", ["h8_sto3g", "spd3"])
def test_consumer_against_the_stored_route(qlib, name, tol):
    cases.check_consumer(qlib, name, tol)


@pytest.mark.parametrize("case", ["rank7", "twins", "one", "n86", "n140"])
def test_panel_kernel(qlib, case):
    cases.check_panel_kernel(qlib, case)


def test_diag_update_kernel(qlib):
    cases.check_diag_kernel(qlib)


def test_permute_kernel(qlib):
    cases.check_permute_kernel(qlib)


@pytest.mark.parametrize("solver", ["MP2", "CCSD"])
def test_be_end_to_end(qlib, solver):
    cases.check_end_to_end(qlib, solver)


def test_refusals(qlib):
    cases.check_refusals(qlib)
