"""Shared cases of the one-electron integral tests (test_gpu_int1e.py on the device, test_int1e_hostlogic.py through the scalar twin): every check takes the
library handle, so the same comparison runs on both.  References: the host source csrc_host/gto_ints.c behind Mole.one_electron() (independent code: its own Boys
function, recursive E coefficients and R table, one Cartesian pair at a time) and, independent of that too, closed forms, the textbook H atom and rotational
invariance.  The bar is the project's integral bar: max |dev - ref| <= BAR max |ref| of the matrix or block compared."""
import ctypes as C
import math

import numpy as np

import int4c_cases as c4
from quemb_amd import _lib
from quemb_amd import integrals as I

BAR = 1e-10
PAIR_CLASSES = c4.PAIR_CLASSES
_R0, _R1 = (0.13, -0.21, 0.32), (0.94, 0.55, -0.47)      # Bohr


def class_molecule(la, lb, prims):
    """three shells: la and lb on one centre (H), lb again on a second centre (C; Z = 6).  prims = (table of the first shell, of the second, of the third).  Its
    blocks: same-shell (diagonal), two shells on one centre, shells on different centres -- of the classes (la, lb), (la, la), (lb, lb)."""
    t = prims
    basis = {"H": [(la, *t[0][la]), (lb, *t[1][lb])], "C": [(lb, *t[2][lb])]}
    return I.Mole([("H", _R0), ("C", _R1)], basis=basis, unit="Bohr")


def rel(a, ref):
    return float(np.abs(a - ref).max()) / float(np.abs(ref).max())


def dev_one_electron(lib, mol):
    b = I.DeviceBasis(mol, lib)
    try:
        return b.one_electron()
    finally:
        b.free()


def check_pair_class(lib, la, lb):
    """S, T, V of the three-shell molecules of one pair class against the host source: the whole matrices and the block of the two centres alone"""
    for label, prims in (("3 / 1 / 3 prim", (c4._EXP3, c4._EXP1, c4._EXP3)), ("1 / 3 / 1 prim", (c4._EXP1, c4._EXP3, c4._EXP1))):
        mol = class_molecule(la, lb, prims)
        host = mol.one_electron()
        dev = dev_one_electron(lib, mol)
        na, nb = 2 * la + 1, 2 * lb + 1
        for name, d, h in zip("STV", dev, host):
            whole = rel(d, h)
            blk = (slice(0, na), slice(na + nb, na + 2 * nb))      # shell la on H against shell lb on C
            cross = rel(d[blk], h[blk])
            one = (slice(0, na), slice(na, na + nb))               # the two shells of H (one centre)
            print(f"class ({la},{lb}) {label}: {name} whole {whole:.2e} of {np.abs(h).max():.3e}, two-centre block {cross:.2e} of {np.abs(h[blk]).max():.3e}, "
                  f"one-centre block |dev - host| {np.abs(d[one] - h[one]).max():.2e}")
            assert whole <= BAR and cross <= BAR, (la, lb, label, name, whole, cross)
            assert np.abs(d[one] - h[one]).max() <= BAR * np.abs(h).max()
            assert (d == d.T).all()


def boys_arguments(mol):
    """p |P - C|^2 of every (primitive pair, nucleus) of the molecule"""
    out = []
    nuc = [np.asarray(a[1]) for a in mol.atom]
    for sa in mol.shells:
        for sb in mol.shells:
            A, B = np.asarray(mol.atom[sa[0]][1]), np.asarray(mol.atom[sb[0]][1])
            for a in sa[2]:
                for b in sb[2]:
                    p = a + b
                    P = (a * A + b * B) / p
                    out += [p * ((P - c) ** 2).sum() for c in nuc]
    return np.array(out)


def far_molecule():
    """an s p d centre and a nucleus more than 12 Bohr away that carries one tight s function"""
    basis = {"H": c4._SPD["H"], "C": [(0, [3.0], [1.0])]}
    return I.Mole([("H", _R0), ("C", (7.3, 8.1, 9.2))], basis=basis, unit="Bohr")


def check_boys_branches(lib):
    mol = far_molecule()
    x = boys_arguments(mol)
    assert x.min() == 0.0 and x.max() > 35.0 and ((x > 0) & (x < 35.0)).any()      # argument 0, the series and the asymptotic branch are all hit
    assert np.linalg.norm(np.asarray(mol.atom[0][1]) - np.asarray(mol.atom[1][1])) >= 12.0
    host, dev = mol.one_electron(), dev_one_electron(lib, mol)
    for name, d, h in zip("STV", dev, host):
        print(f"far nucleus: {name} differs by {rel(d, h):.2e} of {np.abs(h).max():.3e}; Boys arguments 0 .. {x.max():.1f}")
        assert rel(d, h) <= BAR
    # the block of the s p d centre alone feels the far nucleus through the asymptotic branch only
    n = 9
    Vfar = dev[2][:n, :n] - dev_one_electron(lib, I.Mole([("H", _R0)], basis={"H": c4._SPD["H"]}, unit="Bohr"))[2]
    Vfar_h = host[2][:n, :n] - I.Mole([("H", _R0)], basis={"H": c4._SPD["H"]}, unit="Bohr").one_electron()[2]
    print(f"far nucleus: its own attraction on the s p d centre differs by {np.abs(Vfar - Vfar_h).max():.2e} of max |V| = {np.abs(host[2]).max():.3e}")
    assert np.abs(Vfar - Vfar_h).max() <= BAR * np.abs(host[2]).max()


def _f0(x):
    return 1.0 if x == 0.0 else 0.5 * math.sqrt(math.pi / x) * math.erf(math.sqrt(x))


def check_closed_forms(lib):
    """class ss: two normalised s primitives on different centres against the textbook formulas (Szabo & Ostlund A.9, A.11, A.33), F0 from math.erf"""
    a, b = 0.9, 1.7
    mol = I.Mole([("H", _R0), ("C", _R1)], basis={"H": [(0, [a], [1.0])], "C": [(0, [b], [1.0])]}, unit="Bohr")
    S, T, V = dev_one_electron(lib, mol)
    A, B = np.asarray(_R0), np.asarray(_R1)
    Sr, Tr, Vr = np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2))
    fn = [(a, A), (b, B)]
    for i, (x, X) in enumerate(fn):
        for j, (y, Y) in enumerate(fn):
            p, mu, R2 = x + y, x * y / (x + y), float(((X - Y) ** 2).sum())
            nrm = (2 * x / math.pi) ** 0.75 * (2 * y / math.pi) ** 0.75
            s = nrm * (math.pi / p) ** 1.5 * math.exp(-mu * R2)
            Sr[i, j] = s
            Tr[i, j] = mu * (3.0 - 2.0 * mu * R2) * s
            P = (x * X + y * Y) / p
            Vr[i, j] = sum(-Zc * nrm * (2.0 * math.pi / p) * math.exp(-mu * R2) * _f0(p * float(((P - Cc) ** 2).sum())) for Zc, Cc in ((1.0, A), (6.0, B)))
    for name, d, r in (("S", S, Sr), ("T", T, Tr), ("V", V, Vr)):
        print(f"ss closed form: {name} differs by {rel(d, r):.2e}")
        assert rel(d, r) <= BAR


def check_h_atom(lib):
    """H / STO-3G: <T + V> = -0.4665819 Eh (Szabo & Ostlund, the STO-3G hydrogen atom)"""
    mol = I.Mole([("H", (0.0, 0.0, 0.0))])
    S, T, V = dev_one_electron(lib, mol)
    e = float(T[0, 0] + V[0, 0])
    print(f"H / STO-3G: S = {S[0, 0]:.15f}, <T + V> = {e:.9f}")
    assert abs(S[0, 0] - 1.0) <= 1e-12 and abs(e + 0.4665819) <= 1e-6


def _rotation(axis, angle):
    k = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def _core_spectrum(S, T, V):
    w, U = np.linalg.eigh(S)
    X = U / np.sqrt(w) @ U.T
    return np.linalg.eigvalsh(X @ (T + V) @ X)


def check_rotation(lib):
    """two s p d centres: the spectrum of S^-1/2 (T + V) S^-1/2 does not change under a rigid rotation by a generic angle -- every class and the d c2s step"""
    R = _rotation((0.3, -1.1, 0.7), 0.83)
    basis = {"H": c4._SPD["H"], "C": [(0, [2.1, 0.6], [0.4, 0.7]), (1, [1.1], [1.0]), (2, [0.9, 0.4], [0.6, 0.5])]}
    at = [("H", _R0), ("C", _R1)]
    m0 = I.Mole(at, basis=basis, unit="Bohr")
    m1 = I.Mole([(s, tuple(R @ np.asarray(x))) for s, x in at], basis=basis, unit="Bohr")
    S0, T0, V0 = dev_one_electron(lib, m0)
    S1, T1, V1 = dev_one_electron(lib, m1)
    assert np.abs(np.diag(S0) - 1.0).max() <= 1e-12 and np.abs(np.diag(S1) - 1.0).max() <= 1e-12
    assert np.abs(V0 - V1).max() > 1e-3      # the matrices themselves do change
    e0, e1 = _core_spectrum(S0, T0, V0), _core_spectrum(S1, T1, V1)
    d = float(np.abs(e0 - e1).max())
    print(f"rotation: spectrum of S^-1/2 (T + V) S^-1/2 moves by {d:.2e} (largest |eigenvalue| {np.abs(e0).max():.3f})")
    assert d <= 1e-10


def check_refusals_and_bits(lib):
    mol = c4.molecules()["spd3"]()
    N = mol.nao
    b = I.DeviceBasis(mol, lib)
    try:
        S, T, V = b.one_electron()
        S2, T2, V2 = b.one_electron()
        for x, y in ((S, S2), (T, T2), (V, V2)):
            assert (x == y).all() and (x == x.T).all()
        assert np.abs(np.diag(S) - 1.0).max() <= 1e-12
        # null outputs are skipped: each matrix alone has the bits of the joint call
        xyz, Z = b._xyz, b._Z
        for k, ref in enumerate((S, T, V)):
            out = np.full((N, N), np.nan)
            ptr = [None, None, None]; ptr[k] = out.ctypes.data
            assert lib.qemb_int1e(b.h, len(Z), xyz.ctypes.data, Z.ctypes.data, *ptr) == 0
            assert (out == ref).all()
        assert lib.qemb_int1e(b.h, len(Z), xyz.ctypes.data, Z.ctypes.data, None, None, None) == 0
        assert lib.qemb_int1e(b.h, -1, xyz.ctypes.data, Z.ctypes.data, S2.ctypes.data, None, None) == _lib.QEMB_ERR_ARG
        assert lib.qemb_int1e(b.h, len(Z), None, Z.ctypes.data, None, None, V2.ctypes.data) == _lib.QEMB_ERR_ARG
        V0 = np.full((N, N), np.nan)      # no nuclei: the attraction vanishes
        assert lib.qemb_int1e(b.h, 0, None, None, None, None, V0.ctypes.data) == 0 and (V0 == 0.0).all()
        dead = C.c_void_p(b.h.value)
    finally:
        b.free()
    assert lib.qemb_int1e(dead, 0, None, None, S2.ctypes.data, None, None) == _lib.QEMB_ERR_ARG and b"live basis handle" in lib.qemb_last_error()
    for x, h in zip(I.one_electron(mol, "hip", lib), mol.one_electron()):
        assert rel(x, h) <= BAR
    for x, h in zip(I.one_electron(mol, "host"), mol.one_electron()):
        assert (x == h).all()
    with np.testing.assert_raises(ValueError):
        I.one_electron(mol, "cuda")
    # an f orbital shell: the basis uploads, the call names the shell
    fmol = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]})
    fb = I.DeviceBasis(fmol, lib)
    try:
        out = np.empty((fmol.nao,) * 2)
        assert lib.qemb_int1e(fb.h, 1, fb._xyz.ctypes.data, fb._Z.ctypes.data, out.ctypes.data, None, None) == _lib.QEMB_ERR_UNSUPPORTED
        assert b"orbital shell 1" in lib.qemb_last_error() and b"l = 3" in lib.qemb_last_error()
        try:
            fb.one_electron()
            raise AssertionError("an f shell was accepted")
        except _lib.QembError as err:
            assert err.status == _lib.QEMB_ERR_UNSUPPORTED
    finally:
        fb.free()
