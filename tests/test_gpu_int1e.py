"""The one-electron integrals S, T, V on the device (csrc/int1e_ops.hip: one wavefront per shell pair): the six pair classes against the host source, both Boys
branches, closed forms, the hydrogen atom, rotational invariance, refusals and bit-reproducibility.  The cases are those of int1e_cases.py, shared with the
scalar-twin tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import int1e_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("la,lb", cases.PAIR_CLASSES)
def test_pair_class_against_host(qlib, la, lb):
    cases.check_pair_class(qlib, la, lb)


def test_both_boys_branches(qlib):
    cases.check_boys_branches(qlib)


def test_ss_closed_forms(qlib):
    cases.check_closed_forms(qlib)


def test_hydrogen_atom(qlib):
    cases.check_h_atom(qlib)


def test_rotation_invariance(qlib):
    cases.check_rotation(qlib)


def test_refusals_and_reproducibility(qlib):
    cases.check_refusals_and_bits(qlib)
