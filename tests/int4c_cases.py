"""Shared cases of the four-centre integral tests (test_gpu_int4c.py on the device, test_int4c_hostlogic.py through the scalar twin): every check takes the
library handle, so the same comparison runs on both.  References: the host integral source csrc_host/gto_ints.c (independent code: its own Boys function,
E coefficients and R table, one Cartesian quartet at a time), the stored quadrature blocks of golden/int3c_ref.npz (unit-s reduction) and the quadrature of
int3c_reference.primitive through the Gaussian product rule (s.s ket): neither of the latter two knows Boys or Hermite code."""
import ctypes as C
import functools

import numpy as np

import int3c_cases as c3
from quemb_amd import _lib
from quemb_amd import integrals as I

BAR = 1e-10                      # max |dev - ref| <= BAR * max |ref| of the block: the project's bar of the 3-centre classes
E_RHF_BAR = 1e-10                # Eh, RHF total energy device integrals against host integrals
PARITY_ZERO = 1e-14              # a block that vanishes by symmetry (one centre, no multipole common to bra and ket): both sources <= this in absolute terms (integrals of order one, 50 ulp)
BE_BAR = 1e-9                    # the bar int3c_cases.check_end_to_end uses for the two DF backends

PAIR_CLASSES = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
CLASSES = [(la, lb, lc, ld) for i, (la, lb) in enumerate(PAIR_CLASSES) for (lc, ld) in PAIR_CLASSES[: i + 1]]      # the 21 canonical classes
assert len(CLASSES) == 21

# exponents / coefficients per l for a 3-primitive and a 1-primitive contraction (ordinary valence functions)
_EXP3 = {0: ([2.3, 0.7, 0.25], [0.3, 0.5, 0.4]), 1: ([1.6, 0.45, 0.9], [0.55, 0.6, 0.2]), 2: ([1.2, 0.5, 0.3], [0.4, 0.5, 0.3])}
_EXP1 = {0: ([0.8], [1.0]), 1: ([0.6], [1.0]), 2: ([0.7], [1.0])}
_R = ((0.13, -0.21, 0.32), (0.94, 0.55, -0.47), (-0.38, 0.81, 0.66), (0.52, -0.77, -0.29))
GEOMETRIES = {      # centres of the shells a, b, c, d (Bohr)
    "four": _R,                                               # four distinct centres, non-collinear, off the axes
    "two": (_R[0], _R[1], _R[0], _R[1]),                      # two coincident centres: a = c, b = d
    "one": (_R[0],) * 4,                                      # one centre: Boys at x = 0
    "far": (_R[0], _R[1], (10.1, 9.3, -8.2), (10.6, 8.8, -7.9)),      # the ket pair ~ 15 Bohr away: alpha |PQ|^2 >= 35 for every primitive quartet (asserted)
}


def shell_records(l, xyz, exps, coefs):
    """the Cartesian records of one shell as Mole builds them"""
    return [I.Mole._make_bf(tuple(xyz), lmn, exps, coefs, common=(l >= 2)) for lmn in I.cart_components(l)]


def host_block(ls, centres, prims):
    """(ab|cd) of four explicit shells from the host source: gto_eri_s1 over their Cartesian functions, then the Cartesian -> spherical matrices"""
    recs, offs = [], [0]
    for l, r, (ex, co) in zip(ls, centres, prims):
        recs += shell_records(l, r, ex, co)
        offs.append(len(recs))
    n = len(recs)
    arr = (I._BF * n)(*recs)
    out = np.zeros((n, n, n, n))
    I._load().gto_eri_s1(n, arr, out.ctypes.data_as(C.c_void_p))
    blk = out[offs[0]:offs[1], offs[1]:offs[2], offs[2]:offs[3], offs[3]:offs[4]]
    m = [I.cart2sph(l) for l in ls]
    return np.einsum("pqrs,pi,qj,rk,sl->ijkl", blk, *m, optimize=True), recs, offs


def dev_block(lib, ls, first_records):
    out = np.empty(tuple(2 * l + 1 for l in ls))
    tab = I.c2s_table()
    _lib.check(lib.qemb_op_int4c_class(*ls, *[C.addressof(r) for r in first_records], tab.ctypes.data, out.ctypes.data), "qemb_op_int4c_class", lib)
    return out


def min_boys_argument(centres, prims):
    """the smallest alpha |P - Q|^2 over the primitive quartets of (ab|cd)"""
    A, B, Cc, D = (np.asarray(r) for r in centres)
    x = np.inf
    for a in prims[0][0]:
        for b in prims[1][0]:
            for c in prims[2][0]:
                for d in prims[3][0]:
                    p, q = a + b, c + d
                    P, Q = (a * A + b * B) / p, (c * Cc + d * D) / q
                    x = min(x, p * q / (p + q) * ((P - Q) ** 2).sum())
    return x


def check_class(lib, ls):
    """one canonical class: four geometries x (1-primitive, 3-primitive) contractions against the host source, to BAR of the block's largest element.
    (The host source has one entry point, the whole tensor of the functions it is given: every Cartesian quartet among the four shells is evaluated to read
    one block, 81 primitive quartets each with 3-primitive shells -- about 2 s per geometry for (dd|dd), the slowest case.)"""
    worst = 0.0
    for geom, centres in GEOMETRIES.items():
        for name, table in (("1 prim", _EXP1), ("3 prim", _EXP3)):
            prims = [table[l] for l in ls]
            host, recs, offs = host_block(ls, centres, prims)
            if geom == "far":
                assert min_boys_argument(centres, prims) >= 35.0
            dev = dev_block(lib, ls, [recs[o] for o in offs[:4]])
            top = float(np.abs(host).max())
            if geom == "one" and not (set(range(ls[0] - ls[1], ls[0] + ls[1] + 1, 2)) & set(range(ls[2] - ls[3], ls[2] + ls[3] + 1, 2))):
                # one centre: the bra product carries the multipoles |la - lb|, |la - lb| + 2, .. la + lb, the ket product likewise; without a common one the
                # block vanishes by symmetry and "of the block's largest element" has no scale.  Both sources must then give zero up to the rounding of
                # cancelling terms of order one (the host source leaves ~1e-17, the kernels zeros or the same)
                zero = max(top, float(np.abs(dev).max()))
                print(f"class ({ls[0]}{ls[1]}|{ls[2]}{ls[3]}) {geom}, {name}: zero by symmetry, max |host| = {top:.2e}, max |dev| = {np.abs(dev).max():.2e}")
                assert zero <= PARITY_ZERO, (ls, geom, name, zero)
                continue
            assert top > PARITY_ZERO
            d = float(np.abs(dev - host).max()) / top
            worst = max(worst, d)
            print(f"class ({ls[0]}{ls[1]}|{ls[2]}{ls[3]}) {geom}, {name}: max |dev - host| = {d:.2e} of max |host| = {top:.3e}")
            assert d <= BAR, (ls, geom, name, d)
    return worst


# ---- independent of Boys and Hermite code ----------------------------------------------------------------------------------------------------------
def unit_s_cases():
    """the stored 3-centre class cases (both shell orders) whose third shell is an orbital-type shell, l_c <= 2"""
    return [c for c in c3.reference_cases(kind="3c", family="class") if c["p"]["l"] <= 2]


def unit_s_record(xyz):
    b = I._BF()
    b.ctr[:] = xyz; b.lmn[:] = (0, 0, 0); b.nprim = 1
    b.ex[0] = 0.0; b.co[0] = 1.0
    return b


def check_unit_s(lib, case):
    """(ab|c 1) with the fourth function a unit s (exponent 0): the stored quadrature block (ab|c) of int3c_reference.block3c"""
    ref = c3.reference()[1]["ref/" + case["name"]]
    mol, aux = c3.case_moles(case)
    ls = (case["a"]["l"], case["b"]["l"], case["p"]["l"], 0)
    rec = [mol.bfs[mol.shells[0][5]], mol.bfs[mol.shells[1][5]], aux.bfs[0], unit_s_record(case["p"]["r"])]
    got = dev_block(lib, ls, rec)[..., 0]
    d = c3.rel_dev(got, ref)
    print(f"unit-s {case['name']}: max |got - ref| = {d:.2e} of max |ref| = {np.abs(ref).max():.3e}")
    assert got.shape == ref.shape and d <= BAR, (case["name"], d)
    return d


_SS = (([1.1, 0.4], [0.6, 0.5]), ([0.9, 0.35], [0.45, 0.7]))      # the two s shells of the s.s ket, 2 primitives each


@functools.lru_cache(None)
def ss_ket_reference(la, lb):
    """(ab|cd) with c, d two s shells on different centres by the Gaussian product rule: sum over their primitives of cc cd K_cd (ab|s') with s' the
    product Gaussian (exponent c + d at the product centre), each (ab|s') from the quadrature of int3c_reference.primitive; (2 la + 1, 2 lb + 1)"""
    import int3c_reference as ref
    LD = ref.LD
    A, B, Cc, D = (np.asarray(r, dtype=float) for r in GEOMETRIES["four"])
    sh = [shell_records(l, r, *pr) for l, r, pr in ((la, A, _EXP3[la]), (lb, B, _EXP3[lb]), (0, Cc, _SS[0]), (0, D, _SS[1]))]
    co = lambda recs: np.array([[r.co[j] for j in range(r.nprim)] for r in recs])
    coa, cob, coc, cod = (co(s) for s in sh)
    acc = np.zeros((len(sh[0]), len(sh[1])), dtype=LD)
    for x, a in enumerate(_EXP3[la][0]):
        for y, b in enumerate(_EXP3[lb][0]):
            for z, c in enumerate(_SS[0][0]):
                for w, d in enumerate(_SS[1][0]):
                    q = c + d
                    Q = (c * Cc + d * D) / q
                    Kcd = np.exp(LD(-(c * d / q)) * LD(((Cc - D) ** 2).sum()))
                    acc += coa[:, x, None] * cob[None, :, y] * (coc[0, z] * cod[0, w] * Kcd) * ref.primitive(a, A, la, b, B, lb, q, Q, 0)[:, :, 0]
    out = np.einsum("ab,ai,bj->ij", acc, ref.harmonic(I.cart2sph(la), la), ref.harmonic(I.cart2sph(lb), lb)).astype(np.float64)
    return out, tuple(s[0] for s in sh)


def check_ss_ket(lib, la, lb):
    """(ab|ss) and, bra and ket swapped, (ss|ab) -- the second runs the same canonical class with the block put back into the caller's order"""
    ref, rec = ss_ket_reference(la, lb)
    got = dev_block(lib, (la, lb, 0, 0), rec)[:, :, 0, 0]
    swapped = dev_block(lib, (0, 0, la, lb), (rec[2], rec[3], rec[0], rec[1]))[0, 0]
    d, ds = c3.rel_dev(got, ref), c3.rel_dev(swapped, ref)
    print(f"s.s ket ({la}{lb}|ss): max |got - ref| = {d:.2e}, swapped (ss|{la}{lb}) {ds:.2e}, of max |ref| = {np.abs(ref).max():.3e}")
    assert d <= BAR and ds <= BAR, (la, lb, d, ds)
    assert (la, lb) == (0, 0) or (swapped == got).all()      # the same canonical launch, put back in the other order ((ss|ss) has no other order: both run as given)


# ---- molecules -----------------------------------------------------------------------------------------------------------------------------------------
_SPD = {"H": [(0, [1.3, 0.4], [0.5, 0.6]), (1, [0.9, 0.35], [0.6, 0.5]), (2, [0.8], [1.0])]}


def molecules():
    return {"h8_sto3g": lambda: I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)]),
            "h4_ccpvdz": lambda: I.Mole([["H", (0.0, 0.0, float(i))] for i in range(4)], basis="cc-pvdz"),
            "spd3": lambda: I.Mole([("H", (0.0, 0.0, 0.0)), ("H", (0.9, 0.3, -0.2)), ("H", (-0.4, 1.1, 0.7))], basis=_SPD)}      # one s, p, d shell per atom: N = 27


@functools.lru_cache(None)
def host_eri(name):
    """the host [N]^4 tensor of a molecule, computed once and shared (left unchanged by the checks)"""
    mol = molecules()[name]()
    e = mol.eri_s1()
    e.setflags(write=False)
    return mol, e


def check_molecule(lib, name):
    mol, host = host_eri(name)
    top = float(np.abs(host).max())
    dev = {}
    for sym in (1, 4, 8):
        dev[sym] = I.eri(mol, sym, backend="hip", lib=lib)
        want = I.pack_eri(host, sym)
        d = float(np.abs(dev[sym] - want).max()) / top
        print(f"{name}: N = {mol.nao}, sym = {sym}: max |dev - host| = {d:.2e} of max |host| = {top:.3e}")
        assert dev[sym].shape == want.shape and d <= BAR, (name, sym, d)
        again = I.eri(mol, sym, backend="hip", lib=lib)
        assert again.tobytes() == dev[sym].tobytes()                      # every element stored once: the same bits
    s1 = dev[1]
    for perm in ((1, 0, 2, 3), (0, 1, 3, 2), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 0, 1), (2, 3, 1, 0), (3, 2, 1, 0)):
        assert (s1 == s1.transpose(perm)).all(), perm                      # the 8 images are copies of one value
    assert (I.pack_eri(s1, 4) == dev[4]).all() and (I.pack_eri(s1, 8) == dev[8]).all()      # the three forms hold the same numbers
    assert (I.eri(mol, 8, backend="host") == I.pack_eri(host, 8)).all()


def check_screening(lib, thresh=1e-12):
    """a stretched H8 chain (2.5 Angstrom spacing): distant pairs fall below the threshold"""
    mol = I.Mole([["H", (0.0, 0.0, 2.5 * i)] for i in range(8)])
    b = I.DeviceBasis(mol, lib)
    try:
        full = b.eri(8)
        nq0, nz0 = b.eri_stats()
        scr = b.eri(8, thresh=thresh)
        nq, nz = b.eri_stats()
    finally:
        b.free()
    d = float(np.abs(full - scr).max())
    print(f"screening at {thresh:g}: {nz} of {nq} canonical shell quartets stored as zeros, {int((scr == 0).sum())} zero integrals, largest deviation {d:.2e}")
    assert nz0 == 0 and nq0 == nq == 36 * 37 // 2
    assert 0 < nz < nq
    assert (scr == 0).sum() >= nz and ((scr == full) | (scr == 0)).all()
    assert d < thresh


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
class NoEriMF:
    """a mean field that keeps no integrals in memory (PySCF's direct SCF leaves mf._eri = None): everything else is the wrapped object's"""
    _eri = None

    def __init__(self, mf):
        self._mf = mf

    def __getattr__(self, k):
        return getattr(self._mf, k)


@functools.lru_cache(None)
def h8_mf():
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
    mf = I.RHF(mol)
    mf.kernel()
    return mf


def be_energies(lib, solver, from_geometry, frag="test_autogen_h_linear_be2"):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mf = h8_mf()
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", frag)
    if from_geometry:
        be = BE(NoEriMF(mf), fobj, lib=lib, distribute=False, int_transform="in-core-hip", integral_backend="hip")
        assert be._eri_from_geometry
    else:
        be = BE(mf, fobj, lib=lib, distribute=False, int_transform="in-core-hip")
    e, comp = be.oneshot(solver=solver)[:2]
    be.compute_energy_full(approx_cumulant=True, return_rdm=False)
    return np.array([e, *comp, be.e_full["EKapprox"], be.e_full["EKumul"]]), be


def check_end_to_end(lib, solver):
    host, _ = be_energies(lib, solver, False)
    dev, _ = be_energies(lib, solver, True)
    print(f"in-core-hip {solver}: E_corr eri_s1 {host[0]:.12f} device integrals {dev[0]:.12f}, pieces and full-basis energies differ by {np.abs(host - dev).max():.2e}")
    assert np.abs(host - dev).max() <= BE_BAR, (host, dev)


def check_rhf(lib):
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
    mf = I.RHF(mol, integral_backend="hip", lib=lib)
    e = mf.kernel()
    npair = mol.nao * (mol.nao + 1) // 2
    assert mf._eri.shape == (npair * (npair + 1) // 2,)
    print(f"RHF H8 / STO-3G: e_tot device integrals {e:.12f}, host {h8_mf().e_tot:.12f}, difference {abs(e - h8_mf().e_tot):.2e}")
    assert abs(e - h8_mf().e_tot) <= E_RHF_BAR
    dm = h8_mf().make_rdm1()
    assert np.abs(mf.get_veff(dm) - h8_mf().get_veff(dm)).max() <= 1e-10


def check_refusals(lib):
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(2)])
    b = I.DeviceBasis(mol, lib)
    npair = mol.nao * (mol.nao + 1) // 2
    out = np.empty(mol.nao ** 4)
    assert lib.qemb_int4c2e(b.h, 2, 0.0, out.ctypes.data, 0) == _lib.QEMB_ERR_ARG and b"sym" in lib.qemb_last_error()
    assert lib.qemb_int4c2e(b.h, 8, -1.0, out.ctypes.data, 0) == _lib.QEMB_ERR_ARG
    assert lib.qemb_int4c2e(b.h, 8, 0.0, None, 0) == _lib.QEMB_ERR_ARG
    with np.testing.assert_raises(ValueError):
        I.eri(mol, 2)
    with np.testing.assert_raises(ValueError):
        I.eri(mol, 8, backend="cuda")
    # the memory guard: a byte limit on the basis, nothing oversized is allocated
    assert lib.qemb_int4c_mem_limit(b.h, 64) == 0
    assert lib.qemb_int4c2e(b.h, 8, 0.0, out.ctypes.data, 0) == _lib.QEMB_ERR_ALLOC
    assert f"N = {mol.nao}".encode() in lib.qemb_last_error()
    h = C.c_void_p()
    assert lib.qemb_aoeri_from_basis(b.h, 0.0, C.byref(h)) == _lib.QEMB_ERR_ALLOC and f"N = {mol.nao}".encode() in lib.qemb_last_error()
    assert lib.qemb_int4c_mem_limit(b.h, -1) == 0
    assert lib.qemb_int4c2e(b.h, 8, 0.0, out.ctypes.data, 0) == 0
    assert (out[: npair * (npair + 1) // 2] == I.eri(mol, 8, backend="hip", lib=lib)).all()
    # an f orbital shell: the basis itself uploads, the four-centre calls name the shell
    fmol = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]})
    fb = I.DeviceBasis(fmol, lib)
    big = np.empty(fmol.nao ** 4)
    assert lib.qemb_int4c2e(fb.h, 1, 0.0, big.ctypes.data, 0) == _lib.QEMB_ERR_UNSUPPORTED
    assert b"orbital shell 1" in lib.qemb_last_error() and b"l = 3" in lib.qemb_last_error()
    assert lib.qemb_aoeri_from_basis(fb.h, 0.0, C.byref(h)) == _lib.QEMB_ERR_UNSUPPORTED and b"orbital shell 1" in lib.qemb_last_error()
    try:
        I.eri(fmol, 8, backend="hip", lib=lib)
        raise AssertionError("an f shell was accepted")
    except _lib.QembError as e:
        assert e.status == _lib.QEMB_ERR_UNSUPPORTED
    rec = fmol.bfs[fmol.shells[1][5]]
    tab = I.c2s_table()
    o = np.empty(7)
    s = fmol.bfs[0]
    assert lib.qemb_op_int4c_class(3, 0, 0, 0, C.addressof(rec), C.addressof(s), C.addressof(s), C.addressof(s), tab.ctypes.data, o.ctypes.data) == _lib.QEMB_ERR_UNSUPPORTED
    # a freed handle
    dead = C.c_void_p(fb.h.value)
    fb.free()
    assert lib.qemb_int4c2e(dead, 8, 0.0, big.ctypes.data, 0) == _lib.QEMB_ERR_ARG and b"live basis handle" in lib.qemb_last_error()
    assert lib.qemb_aoeri_from_basis(dead, 0.0, C.byref(h)) == _lib.QEMB_ERR_ARG
    assert lib.qemb_int4c_mem_limit(dead, 1) == _lib.QEMB_ERR_ARG and lib.qemb_int4c_stats(dead, None, None) == _lib.QEMB_ERR_ARG
    b.free()
