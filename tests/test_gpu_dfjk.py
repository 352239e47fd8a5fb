"""The DF mean field on the device: J and K from the resident 3-index tensor on the FP64 MFMA GEMM (csrc/ao2mo.cpp: DfContext::jk), the Cholesky contexts,
RHF(density_fit=...) and BE(reuse_mf_df=True).  The cases are those of dfjk_cases.py, shared with the mock-library tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import dfjk_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["h2", "ch"])
def test_jk_against_numpy(qlib, name):
    cases.check_jk(qlib, name)


def test_options(qlib):
    cases.check_options(qlib)


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["h2", "ch"])
def test_cholesky_context(qlib, name, tol):
    cases.check_cholesky(qlib, name, tol)


def test_guards(qlib):
    cases.check_guards(qlib)


def test_df_mean_field(qlib):
    cases.check_df_rhf(qlib)


def test_cholesky_mean_field(qlib):
    cases.check_cholesky_rhf(qlib)


def test_borrowed_context_and_bad_combinations(qlib):
    cases.check_borrowed_and_bad(qlib)


@pytest.mark.parametrize("solver", ["MP2", "CCSD"])
@pytest.mark.parametrize("route", ["df", "cholesky"])
def test_be_shares_the_tensor(qlib, route, solver):
    cases.check_be_reuse(qlib, route, solver)


def test_routes_without_density_fit_keep_the_one_argument_jk(qlib):
    cases.check_one_argument_jk(qlib)


def test_be_reuse_without_a_context(qlib):
    cases.check_be_reuse_refused(qlib)
