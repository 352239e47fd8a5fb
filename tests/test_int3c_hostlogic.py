"""DF integrals from the basis (csrc/int3c.cpp) through the scalar twin of the mock library: the driver logic -- shells from the records, work lists per
angular class, layouts, the in-place fill of a DF context -- and the arithmetic of int3c_core.h, without a device."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import int3c_cases as cases
from quemb_amd import _lib
from quemb_amd import integrals as I


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("m_max", range(cases.BOYS_M_MAX + 1))
def test_boys_function(hlib, m_max):
    cases.check_boys(hlib, on_device=False, m_max=m_max)


def _twin_subset():
    """Two classes per stress family (the lowest and (2,2|4)), one low and one high class in each shell order, and three metric classes."""
    keep = ("_00_0", "_22_4")
    names = {"class_01_1", "class_10_1", "class_12_3", "class_21_3", "class_22_4", "class_m4_4", "class_m1_3", "class_m3_1"}
    keep4 = ("_00_0", "_12_2")                             # T1e4 holds no (2,2|4): no such block reaches 1e-8 above T = 1e3
    return [c for c in cases.reference_cases() if c["name"] in names or (c["family"] != "class" and c["name"].endswith(keep4 if c["family"] == "T1e4" else keep))]


@pytest.mark.parametrize("case", _twin_subset(), ids=lambda c: c["name"])
def test_against_quadrature_reference(hlib, case):
    cases.check_class_against_reference(hlib, case)


def test_twin_subset_covers_every_family():
    got = {}
    for c in _twin_subset():
        got[c["family"]] = got.get(c["family"], 0) + 1
    assert set(got) == set(cases.reference_families()) and all(n >= 2 for n in got.values()), got


@pytest.mark.parametrize("cls", [(0, 1, 1), (2, 2, 4)], ids=lambda c: "%d%d%d" % c)
def test_one_low_and_one_high_class(hlib, cls):
    cases.check_class(hlib, *cls)


def test_h8_whole_molecule(hlib):
    cases.check_molecule(hlib, *cases.h8(), "H8 / STO-3G")


def test_layouts_agree(hlib):
    mol, aux = cases.h8("cc-pvdz", 3)
    pql = I.aux_e2(mol, aux, backend="hip", lib=hlib)
    lpq = I._int3c_hip(mol, aux, "Lpq", lib=hlib)
    packed = I._int3c_hip(mol, aux, "packed", lib=hlib)
    assert (lpq == pql.transpose(2, 0, 1)).all()
    il = np.tril_indices(mol.nao)
    assert (packed == lpq[:, il[0], il[1]]).all()
    cases.check_layouts_on(hlib)          # and on coprime counts per class, with the pqL blocks against the quadrature reference


def test_pair_list(hlib):
    cases.check_pair_list(hlib)


def test_inplace_fill(hlib):
    cases.check_inplace_fill(hlib, *cases.h8("cc-pvdz", 4), alloc_stats=False)


def test_semisparse_from_geometry_end_to_end(hlib):
    cases.check_end_to_end(hlib, "sparse-DF-hip", "MP2", MO_coeff_epsilon=0.0)


def test_argument_errors(hlib):
    mol, aux = cases.h8(n=2)
    b, a = I.DeviceBasis(mol, hlib), I.DeviceBasis(aux, hlib)
    out = np.empty((mol.nao, mol.nao, aux.nao))
    assert hlib.qemb_int3c2e(b.h, a.h, None, 0, 7, out.ctypes.data, 0) == _lib.QEMB_ERR_ARG
    assert b"layout" in hlib.qemb_last_error()
    with pytest.raises(ValueError):
        I.aux_e2(mol, aux, backend="cuda")
    # an f orbital shell: the basis itself uploads (it could be an auxiliary one), the 3-centre call names the shell
    fmol = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]})
    fb = I.DeviceBasis(fmol, hlib)
    big = np.empty((fmol.nao, fmol.nao, aux.nao))
    assert hlib.qemb_int3c2e(fb.h, a.h, None, 0, 0, big.ctypes.data, 0) == _lib.QEMB_ERR_UNSUPPORTED
    assert b"orbital shell 1" in hlib.qemb_last_error() and b"l = 3" in hlib.qemb_last_error()
    with pytest.raises(_lib.QembError) as ei:
        I.aux_e2(fmol, aux, backend="hip", lib=hlib)
    assert ei.value.status == _lib.QEMB_ERR_UNSUPPORTED
    tab = I.c2s_table()
    rec = fmol.bfs[fmol.shells[1][5]]
    o = np.empty(7 * 7)
    assert hlib.qemb_op_int3c_class(3, 0, 0, C.addressof(rec), C.addressof(rec), C.addressof(rec), tab.ctypes.data, o.ctypes.data) == _lib.QEMB_ERR_UNSUPPORTED
    # a freed handle
    h = C.c_void_p(fb.h.value)
    fb.free()
    assert hlib.qemb_int3c2e(h, a.h, None, 0, 0, big.ctypes.data, 0) == _lib.QEMB_ERR_ARG
    assert b"live basis handle" in hlib.qemb_last_error()
    assert hlib.qemb_int_basis_free(h) == _lib.QEMB_ERR_ARG
    # a record that does not continue its shell
    arr = mol._arr() if False else fmol._arr()
    arr[2].lmn[0] += 1
    hh = C.c_void_p()
    assert hlib.qemb_int_basis_create(fmol.ncart, C.addressof(arr), C.sizeof(I._BF), tab.ctypes.data, C.byref(hh)) == _lib.QEMB_ERR_UNSUPPORTED
    assert hlib.qemb_int_basis_create(fmol.ncart, C.addressof(arr), C.sizeof(I._BF) - 8, tab.ctypes.data, C.byref(hh)) == _lib.QEMB_ERR_ARG
    # Cartesian -> spherical matrices of s / p that are not the identity are refused, not silently ignored
    bad = tab.copy(); bad[1], bad[5] = 0.0, 0.0; bad[2], bad[4] = 1.0, 1.0      # p functions in y, x, z order
    assert hlib.qemb_int_basis_create(mol.ncart, C.addressof(mol._arr()), C.sizeof(I._BF), bad.ctypes.data, C.byref(hh)) == _lib.QEMB_ERR_UNSUPPORTED
    assert b"identity" in hlib.qemb_last_error()
    b.free(); a.free()


def test_be_refuses_hip_backend_with_caller_integrals():
    from quemb_amd.mbe import BE
    with pytest.raises(ValueError, match="df_ints"):
        BE(None, None, int_transform="int-direct-DF-hip", df_ints=(None, None, "pqL"), integral_backend="hip")
