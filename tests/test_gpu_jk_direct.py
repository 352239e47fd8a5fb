"""Integral-direct J and K on the device (csrc/int4c_ops.hip: int4c_jk_kernel): the digest of every canonical class against J and K of the host integral
source, the coincidence weights, exact symmetry, screening with the density, RHF(direct=True), BE on a direct mean field, the memory guard and the refusals.
The cases are those of jk_direct_cases.py, shared with the scalar-twin tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import jk_direct_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["d_only", "spd_atom"])
def test_coincidence_weights(qlib, name):
    cases.check_molecule(qlib, name)


def test_h2_by_hand(qlib):
    cases.check_h2_by_hand(qlib)


@pytest.mark.parametrize("density", ["random", "rhf"])
@pytest.mark.parametrize("name", ["spd3", "h4_ccpvdz", "h8_sto3g"])
def test_every_class(qlib, name, density):
    cases.check_molecule(qlib, name, density)


def test_exact_properties(qlib):
    cases.check_properties(qlib)


def test_density_weighted_screening(qlib):
    cases.check_screening(qlib)


@pytest.mark.parametrize("name", ["h8_sto3g", "h4_ccpvdz"])
def test_direct_rhf(qlib, name):
    cases.check_rhf(qlib, name)


@pytest.mark.parametrize("solver", ["MP2", "CCSD"])
@pytest.mark.parametrize("route", ["in-core", "df"])
def test_be_on_a_direct_mean_field(qlib, route, solver):
    cases.check_end_to_end(qlib, solver, route)


def test_memory_guard(qlib):
    cases.check_memory(qlib)


def test_refusals(qlib):
    cases.check_refusals(qlib)
