"""The one-electron integrals S, T, V (csrc/int1e_core.h, driver int1e_fill in csrc/int3c.cpp) through the scalar twin of the mock library: the arithmetic the
kernel instantiates per lane, the 64-lane partition and its fixed-order tree, the Cartesian -> spherical step, the driver and the Python surface, without a device."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import int1e_cases as cases
from quemb_amd import _lib


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("la,lb", cases.PAIR_CLASSES)
def test_pair_class_against_host(hlib, la, lb):
    cases.check_pair_class(hlib, la, lb)


def test_both_boys_branches(hlib):
    cases.check_boys_branches(hlib)


def test_ss_closed_forms(hlib):
    cases.check_closed_forms(hlib)


def test_hydrogen_atom(hlib):
    cases.check_h_atom(hlib)


def test_rotation_invariance(hlib):
    cases.check_rotation(hlib)


def test_refusals_and_reproducibility(hlib):
    cases.check_refusals_and_bits(hlib)
