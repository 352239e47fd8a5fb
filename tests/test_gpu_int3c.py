"""DF integrals on the device (csrc/int3c_ops.hip) against the host integral source (csrc_host/gto_ints.c behind integrals.aux_e2 / int2c2e):
the Boys function, every angular class at the smallest shape, whole molecules, the pair list, the in-place fill of a DF context and the
from-geometry BE drivers with integral_backend="hip" -- and against the independent quadrature reference of int3c_reference.py (blocks stored in
golden/int3c_ref.npz): every class in both shell orders, the metric classes, the stress families, the three dense layouts.  The Boys function is
compared with mpmath for every m_max.  The cases are those of int3c_cases.py, shared with the scalar-twin tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import int3c_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m_max", range(cases.BOYS_M_MAX + 1))
def test_boys_function(qlib, m_max):
    cases.check_boys(qlib, on_device=True, m_max=m_max)


@pytest.mark.parametrize("case", cases.reference_cases(family="class"), ids=lambda c: c["name"])
def test_class_against_quadrature_reference(qlib, case):
    """All 45 classes in both shell orders of qemb_op_int3c_class (l_a >= l_b and l_a <= l_b: both output orders of the block layout) and the 25
    metric classes."""
    cases.check_class_against_reference(qlib, case)


@pytest.mark.parametrize("case", [c for c in cases.reference_cases() if c["family"] != "class"], ids=lambda c: c["name"])
def test_stress_family_against_quadrature_reference(qlib, case):
    cases.check_class_against_reference(qlib, case)


def test_dense_layouts_on_the_device(qlib):
    """pqL, Lpq and packed as kernels (the latter two split the item index by the pair count), on counts that are coprime."""
    cases.check_layouts_on(qlib)


@pytest.mark.parametrize("cls", cases.CLASSES, ids=lambda c: "%d%d%d" % c)
def test_angular_class(qlib, cls):
    cases.check_class(qlib, *cls)


@pytest.mark.parametrize("system", ["h8_sto3g", "h4_ccpvdz", "octane12_sto3g"])
def test_whole_molecule(qlib, system):
    mol, aux = {"h8_sto3g": cases.h8, "h4_ccpvdz": lambda: cases.h8("cc-pvdz", 4), "octane12_sto3g": cases.octane12}[system]()
    cases.check_molecule(qlib, mol, aux, system)


def test_pair_list(qlib):
    cases.check_pair_list(qlib)


def test_inplace_fill(qlib):
    cases.check_inplace_fill(qlib, *cases.h8("cc-pvdz", 12), alloc_stats=True)      # N = 60, naux = 372: the tensor is 7.7 x the three naux^2 images


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_from_geometry_df_driver(qlib, solver):
    cases.check_end_to_end(qlib, "int-direct-DF-hip", solver)


def test_semisparse_pipeline(qlib):
    cases.check_end_to_end(qlib, "sparse-DF-hip", "CCSD", MO_coeff_epsilon=0.0)
