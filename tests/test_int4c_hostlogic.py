"""Four-centre AO integrals from the basis (csrc/int4c.cpp) through the scalar twin of the mock library: the driver logic -- shell pairs per pair class, the
pair stage, canonical quartets, the three output forms, screening, guard and refusals -- and the arithmetic of int4c_core.h, without a device."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import int4c_cases as cases
from quemb_amd import _lib
from quemb_amd import integrals as I


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("ls", [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (1, 0, 1, 0), (1, 1, 1, 0), (2, 0, 1, 1), (2, 1, 2, 0), (2, 2, 2, 2)], ids=lambda c: "%d%d%d%d" % c)
def test_class_against_host_source(hlib, ls):
    """a low, the mixed and the highest class (all 21 run on the device, chosen by the same dispatcher, csrc/int_dispatch.h; all 21 take 24 s on the mock)"""
    cases.check_class(hlib, ls)


@pytest.mark.parametrize("case", [c for c in cases.unit_s_cases() if c["name"] in ("class_00_0", "class_01_1", "class_10_2", "class_21_1", "class_22_2")],
                         ids=lambda c: c["name"])
def test_unit_s_reduction_to_the_quadrature_reference(hlib, case):
    cases.check_unit_s(hlib, case)


def test_unit_s_cases_cover_every_class_in_both_orders():
    got = {(c["a"]["l"], c["b"]["l"], c["p"]["l"]) for c in cases.unit_s_cases()}
    assert got == {(a, b, p) for a in range(3) for b in range(3) for p in range(3)}


@pytest.mark.parametrize("pc", cases.PAIR_CLASSES, ids=lambda c: "%d%d" % c)
def test_ss_ket_by_the_product_rule(hlib, pc):
    cases.check_ss_ket(hlib, *pc)


@pytest.mark.parametrize("name", ["h8_sto3g", "h4_ccpvdz", "spd3"])
def test_whole_molecule(hlib, name):
    cases.check_molecule(hlib, name)


def test_schwarz_screening(hlib):
    cases.check_screening(hlib)


def test_rhf_on_device_integrals(hlib):
    cases.check_rhf(hlib)


def test_in_core_route_from_geometry(hlib):
    cases.check_end_to_end(hlib, "MP2")


def test_refusals(hlib):
    cases.check_refusals(hlib)


def test_host_backend_without_integrals_keeps_the_reference_error(hlib):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    with pytest.raises(ValueError, match="ERIs have to be available in memory"):
        BE(cases.NoEriMF(cases.h8_mf()), fobj, lib=hlib, distribute=False, int_transform="in-core-hip", integral_backend="host")


def test_packed_jk_matches_the_full_tensor():
    mf = cases.h8_mf()
    rng = np.random.default_rng(3)
    dm = rng.standard_normal((mf.mol.nao,) * 2)
    dm = dm + dm.T
    J, K = mf._jk(dm)
    for sym in (4, 8):
        pk = I.RHF(mf.mol)
        pk._eri = I.pack_eri(mf._eri, sym)
        Jp, Kp = pk._jk(dm)
        assert np.abs(Jp - J).max() < 1e-12 and np.abs(Kp - K).max() < 1e-12
