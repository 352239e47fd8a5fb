"""Four-centre AO integrals on the device (csrc/int4c_ops.hip): every canonical class against the host integral source csrc_host/gto_ints.c, the unit-s
reduction to the stored quadrature blocks and the s.s ket through the Gaussian product rule (neither knows Boys or Hermite code), whole molecules in the
three output forms, Schwarz screening, the in-core BE route and RHF from device integrals, and the refusals.  The cases are those of int4c_cases.py,
shared with the scalar-twin tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import int4c_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ls", cases.CLASSES, ids=lambda c: "%d%d%d%d" % c)
def test_class_against_host_source(qlib, ls):
    cases.check_class(qlib, ls)


@pytest.mark.parametrize("case", cases.unit_s_cases(), ids=lambda c: c["name"])
def test_unit_s_reduction_to_the_quadrature_reference(qlib, case):
    cases.check_unit_s(qlib, case)


@pytest.mark.parametrize("pc", cases.PAIR_CLASSES, ids=lambda c: "%d%d" % c)
def test_ss_ket_by_the_product_rule(qlib, pc):
    cases.check_ss_ket(qlib, *pc)


@pytest.mark.parametrize("name", ["h8_sto3g", "h4_ccpvdz", "spd3"])
def test_whole_molecule(qlib, name):
    cases.check_molecule(qlib, name)


def test_schwarz_screening(qlib):
    cases.check_screening(qlib)


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_in_core_route_from_geometry(qlib, solver):
    cases.check_end_to_end(qlib, solver)


def test_reference_golden_energy_with_device_integrals(qlib):
    """the H8 BE2 CCSD one-shot golden of test_gpu_be.test_h8_oneshot_golden, at its bar, with (mu nu|la si) evaluated on the device and never held on the host"""
    e, be = cases.be_energies(qlib, "CCSD", True)
    print(f"H8 BE2 CCSD one-shot with device integrals: E_corr = {e[0]:.12f}, golden -0.13198886164212092")
    assert abs(be.hf_err) < 1e-8
    assert abs(e[0] - (-0.13198886164212092)) < 3e-7      # tests/_expected_data_for_fragmentation_test.py:983 (PySCF conv_tol 1e-7)


def test_rhf_on_device_integrals(qlib):
    cases.check_rhf(qlib)


def test_refusals(qlib):
    cases.check_refusals(qlib)
