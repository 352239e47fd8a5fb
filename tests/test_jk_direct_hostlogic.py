"""Integral-direct J and K (csrc/int4c.cpp: int4c_jk_direct) through the scalar twin of the mock library: the digest weights of int4c_core.h, the driver --
cached pair stage, screening with the density, guard and refusals -- and the Python surface up to RHF(direct=True) and BE, without a device.  In the twin the
accumulation is a plain += in one fixed order."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import jk_direct_cases as cases
from quemb_amd import _lib


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("name", ["d_only", "spd_atom"])
def test_coincidence_weights(hlib, name):
    cases.check_molecule(hlib, name)


def test_h2_by_hand(hlib):
    cases.check_h2_by_hand(hlib)


@pytest.mark.parametrize("density", ["random", "rhf"])
@pytest.mark.parametrize("name", ["spd3", "h4_ccpvdz", "h8_sto3g"])
def test_every_class(hlib, name, density):
    cases.check_molecule(hlib, name, density)


def test_exact_properties(hlib):
    cases.check_properties(hlib)


def test_density_weighted_screening(hlib):
    cases.check_screening(hlib)


@pytest.mark.parametrize("name", ["h8_sto3g", "h4_ccpvdz"])
def test_direct_rhf(hlib, name):
    cases.check_rhf(hlib, name)


@pytest.mark.parametrize("route", ["in-core", "df"])
def test_be_on_a_direct_mean_field(hlib, route):
    cases.check_end_to_end(hlib, "MP2", route)


def test_memory_guard(hlib):
    cases.check_memory(hlib)


def test_refusals(hlib):
    cases.check_refusals(hlib)
