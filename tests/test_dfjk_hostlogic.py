"""J and K from the resident 3-index tensor (csrc/ao2mo.cpp: DfContext::jk), RHF(density_fit=...) and BE(reuse_mf_df=True) through the mock library: the driver --
density factor, slabs, signs, metric and identity routes, guard and refusals -- and the Python surface, without a device."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import dfjk_cases as cases
from quemb_amd import _lib


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("name", ["h2", "ch"])
def test_jk_against_numpy(hlib, name):
    cases.check_jk(hlib, name)


def test_options(hlib):
    cases.check_options(hlib)


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["h2", "ch"])
def test_cholesky_context(hlib, name, tol):
    cases.check_cholesky(hlib, name, tol)


def test_guards(hlib):
    cases.check_guards(hlib)


def test_df_mean_field(hlib):
    cases.check_df_rhf(hlib)


def test_cholesky_mean_field(hlib):
    cases.check_cholesky_rhf(hlib)


def test_borrowed_context_and_bad_combinations(hlib):
    cases.check_borrowed_and_bad(hlib)


@pytest.mark.parametrize("route", ["df", "cholesky"])
def test_be_shares_the_tensor(hlib, route):
    """solver="MP2" only on the mock library (the scalar CCSD is slow); test_gpu_dfjk.py runs MP2 and CCSD on both routes at the same 1e-12"""
    cases.check_be_reuse(hlib, route, "MP2")


def test_routes_without_density_fit_keep_the_one_argument_jk(hlib):
    cases.check_one_argument_jk(hlib)


def test_be_reuse_without_a_context(hlib):
    cases.check_be_reuse_refused(hlib)
