"""Shared cases of the integral-direct J / K tests (test_gpu_jk_direct.py on the device, test_jk_direct_hostlogic.py through the scalar twin): every check
takes the library handle, so the same comparison runs on both.  The reference of every comparison is the host integral source: J and K by einsum from
Mole.eri_s1() (csrc_host/gto_ints.c, independent code); the bar is the project's integral bar, max |dev - ref| <= BAR max |ref| per matrix."""
import ctypes as C
import functools

import numpy as np

import int3c_cases as c3
import int4c_cases as c4
from quemb_amd import _lib
from quemb_amd import integrals as I

BAR = c4.BAR
E_RHF_BAR = c4.E_RHF_BAR
BE_BAR = c4.BE_BAR

_ONE = (0.1, -0.2, 0.3)


def molecules():
    m = dict(c4.molecules())
    m["d_only"] = lambda: I.Mole([("H", _ONE)], basis={"H": [(2, [0.8], [1.0])]})                      # N = 5: one quartet with sameAB, sameCD and diag all true
    m["spd_atom"] = lambda: I.Mole([("H", _ONE)], basis=c4._SPD)                                        # N = 9: every class, every pair on one centre
    m["h2_sto3g"] = lambda: I.Mole([["H", (0.0, 0.0, 0.0)], ["H", (0.0, 0.0, 0.74)]])                   # N = 2: six unique integrals
    return m


@functools.lru_cache(None)
def host_eri(name):
    """the host [N]^4 tensor of a molecule, computed once and shared (left unchanged by the checks)"""
    if name in c4.molecules():
        return c4.host_eri(name)
    mol = molecules()[name]()
    e = mol.eri_s1()
    e.setflags(write=False)
    return mol, e


def host_jk(eri, dm):
    return np.einsum("pqrs,rs->pq", eri, dm, optimize=True), np.einsum("pqrs,qs->pr", eri, dm, optimize=True)


def random_density(n, seed):
    """a random symmetric matrix, entries of order one on and off the diagonal"""
    d = np.random.default_rng(seed).standard_normal((n, n))
    return 0.5 * (d + d.T)


@functools.lru_cache(None)
def host_rhf(name):
    mol, e = host_eri(name)
    mf = I.RHF(mol)
    mf._eri = e
    mf.kernel()
    return mf


def rel(a, ref):
    return float(np.abs(a - ref).max()) / float(np.abs(ref).max())


def compare(label, J, K, Jr, Kr):
    dj, dk = rel(J, Jr), rel(K, Kr)
    print(f"{label}: max |J - ref| = {dj:.2e} of max |J| = {np.abs(Jr).max():.3e}, max |K - ref| = {dk:.2e} of max |K| = {np.abs(Kr).max():.3e}")
    assert dj <= BAR and dk <= BAR, (label, dj, dk)
    assert (J == J.T).all() and (K == K.T).all(), label      # one triangle accumulated, then mirrored


def check_molecule(lib, name, density="random"):
    """J and K of one molecule against the host source, through DeviceBasis.get_jk and the module-level get_jk"""
    mol, e = host_eri(name)
    dm = random_density(mol.nao, 11) if density == "random" else host_rhf(name).make_rdm1()
    dm = 0.5 * (dm + dm.T)
    Jr, Kr = host_jk(e, dm)
    J, K = I.get_jk(mol, dm, backend="hip", lib=lib)
    compare(f"{name} (N = {mol.nao}, {density} D)", J, K, Jr, Kr)
    return J, K


def check_h2_by_hand(lib):
    """H2 / STO-3G: the six unique integrals (11|11) (21|11) (21|21) (22|11) (22|21) (22|22) written out -- the weights of the digest checked without einsum"""
    mol, e = host_eri("h2_sto3g")
    dm = np.array([[0.7, -0.4], [-0.4, 1.3]])
    a, b, c, d, f, g = e[0, 0, 0, 0], e[1, 0, 0, 0], e[1, 0, 1, 0], e[1, 1, 0, 0], e[1, 1, 1, 0], e[1, 1, 1, 1]
    D00, D10, D11 = dm[0, 0], dm[1, 0], dm[1, 1]
    Jr = np.array([[a * D00 + 2 * b * D10 + d * D11, 0.0], [b * D00 + 2 * c * D10 + f * D11, d * D00 + 2 * f * D10 + g * D11]])
    Kr = np.array([[a * D00 + 2 * b * D10 + c * D11, 0.0], [b * D00 + (c + d) * D10 + f * D11, c * D00 + 2 * f * D10 + g * D11]])
    Jr[0, 1], Kr[0, 1] = Jr[1, 0], Kr[1, 0]
    J, K = I.get_jk(mol, dm, backend="hip", lib=lib)
    compare("H2 / STO-3G by hand", J, K, Jr, Kr)
    Jh, Kh = I.get_jk(mol, dm, backend="host")
    assert rel(Jh, Jr) < 1e-14 and rel(Kh, Kr) < 1e-14      # the hand formulas are those of the einsum reference


def check_properties(lib, name="spd3"):
    """exact symmetry, one-sided calls, linearity, a second call on the same basis"""
    mol, e = host_eri(name)
    D1, D2 = random_density(mol.nao, 21), random_density(mol.nao, 22)
    b = I.DeviceBasis(mol, lib)
    try:
        J1, K1 = b.get_jk(D1)
        assert (J1 == J1.T).all() and (K1 == K1.T).all()
        Jonly, none_k = b.get_jk(D1, with_k=False)
        none_j, Konly = b.get_jk(D1, with_j=False)
        assert none_k is None and none_j is None
        J2, K2 = b.get_jk(D2)
        J12, K12 = b.get_jk(D1 + D2)
        Ja, Ka = b.get_jk(D1)      # the cached pair stage and Schwarz factors serve this call
    finally:
        b.free()
    Jr, Kr = host_jk(e, D1)
    compare(f"{name} joint call", J1, K1, Jr, Kr)
    figs = dict(j_only=rel(Jonly, J1), k_only=rel(Konly, K1), lin_j=rel(J12, J1 + J2), lin_k=rel(K12, K1 + K2), again_j=rel(Ja, J1), again_k=rel(Ka, K1))
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert max(figs.values()) <= BAR, figs
    assert (Jonly == Jonly.T).all() and (Konly == Konly.T).all()


def banded_density(n):
    """a density with the decay of a wide-gap chain, largest |element| exactly 1 (on the diagonal): D[i,j] = (-0.01)^|i-j|"""
    i = np.arange(n)
    return (-0.01) ** np.abs(i[:, None] - i[None, :])


def check_screening(lib, thresh=1e-12):
    """the stretched H8 chain of int4c_cases.check_screening (2.5 Angstrom).  A skipped quartet has Q_ab Q_cd < thresh or Q_ab Q_cd dmax < thresh; by Schwarz
    |(ab|cd)| <= Q_ab Q_cd, so every term (ab|cd) D[..] it leaves out of an element of J or K is below thresh max(1, max|D|) in magnitude, and an element is a
    sum of N^2 terms: |J - J_unscreened|, |K - K_unscreened| <= thresh N^2 max|D| once max|D| >= 1 (asserted: the density used has max|D| = 1)."""
    mol = I.Mole([["H", (0.0, 0.0, 2.5 * i)] for i in range(8)])
    dm = banded_density(mol.nao)
    assert np.abs(dm).max() == 1.0
    b = I.DeviceBasis(mol, lib)
    try:
        J0, K0 = b.get_jk(dm)
        nq0, nz0 = b.eri_stats()
        J1, K1 = b.get_jk(dm, thresh=thresh)
        nq1, nz1 = b.eri_stats()
        b.eri(8, thresh=thresh)
        _, nz_fill = b.eri_stats()      # the stored fill skips by Q_ab Q_cd alone
    finally:
        b.free()
    bound = thresh * mol.nao ** 2 * np.abs(dm).max()
    dj, dk = float(np.abs(J1 - J0).max()), float(np.abs(K1 - K0).max())
    print(f"screening at {thresh:g}: {nz1} of {nq1} canonical quartets skipped (Schwarz alone: {nz_fill}); |J - J0| = {dj:.2e}, |K - K0| = {dk:.2e}, bound {bound:.2e}")
    assert nz0 == 0 and nq0 == nq1 == 36 * 37 // 2
    assert 0 < nz_fill < nz1 < nq1      # the density weight skips quartets the Schwarz bound alone keeps
    assert dj <= bound and dk <= bound
    Jr, Kr = I.get_jk(mol, dm, backend="host")
    compare("stretched H8, unscreened", J0, K0, Jr, Kr)


def check_rhf(lib, name):
    """RHF(direct=True): no integrals kept, the energy and the mean-field potential of the host RHF"""
    mol, _ = host_eri(name)
    ref = host_rhf(name)
    mf = I.RHF(mol, integral_backend="hip", lib=lib, direct=True)
    try:
        e = mf.kernel()
        assert mf._eri is None and mf.converged
        print(f"direct RHF {name}: e_tot {e:.12f}, host {ref.e_tot:.12f}, difference {abs(e - ref.e_tot):.2e}")
        assert abs(e - ref.e_tot) <= E_RHF_BAR
        dm = ref.make_rdm1()
        core = 2.0 * np.outer(ref.mo_coeff[:, 0], ref.mo_coeff[:, 0])      # the density a frozen core hands to get_veff (BE.core_veff)
        for lab, d in (("HF density", dm), ("core density", core)):
            dv = float(np.abs(mf.get_veff(d) - ref.get_veff(d)).max())
            print(f"direct RHF {name}: get_veff({lab}) differs by {dv:.2e}")
            assert dv <= 1e-10
        assert np.abs(mf.get_veff() - ref.get_veff()).max() <= 1e-8      # at its own converged density (orbitals agree to the SCF's convergence, not to 1e-10)
        assert mf._eri is None
    finally:
        mf.free()
    assert mf._basis is None


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
_DIRECT_MF = {}


def direct_h8_mf(lib):
    """the direct mean field of H8 / STO-3G on this library, converged once and shared by the end-to-end cases"""
    if id(lib) not in _DIRECT_MF:
        mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
        mf = I.RHF(mol, integral_backend="hip", lib=lib, direct=True)
        mf.kernel()
        _DIRECT_MF[id(lib)] = (lib, mf)
    return _DIRECT_MF[id(lib)][1]


def check_end_to_end(lib, solver, route):
    """BE on a direct mean field (`_eri` None) against the same route on the host mean field: H8, BE2.  route "in-core": int_transform="in-core-hip" from the
    geometry, with the full-basis energies of compute_energy_full; route "df": the from-geometry DF construction of int3c_cases.check_end_to_end."""
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mf = direct_h8_mf(lib)
    assert mf._eri is None
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    if route == "in-core":
        host, _ = c4.be_energies(lib, solver, True)
        be = BE(mf, fobj, lib=lib, distribute=False, int_transform="in-core-hip", integral_backend="hip")
        assert be._eri_from_geometry
        e, comp = be.oneshot(solver=solver)[:2]
        be.compute_energy_full(approx_cumulant=True, return_rdm=False)
        dev = np.array([e, *comp, be.e_full["EKapprox"], be.e_full["EKumul"]])
    else:
        host = c3.be_energies(lib, "int-direct-DF-hip", solver, "hip")
        be = BE(mf, fobj, lib=lib, distribute=False, int_transform="int-direct-DF-hip", auxbasis="etb", integral_backend="hip")
        e, comp = be.oneshot(solver=solver)[:2]
        dev = np.array([e, *comp])
    assert mf._eri is None
    print(f"{route} {solver}: E_corr host mean field {host[0]:.12f}, direct mean field {dev[0]:.12f}, pieces differ by {np.abs(host - dev).max():.2e}")
    assert np.abs(host - dev).max() <= BE_BAR, (host, dev)
    assert np.abs(be.hf_veff - c4.h8_mf().get_veff()).max() <= 1e-8


def check_memory(lib, name="spd3"):
    """with the four-centre limit of the basis at the direct call's own figure the stored [N]^4 fill is refused and the direct call runs and is right"""
    mol, e = host_eri(name)
    N = mol.nao
    dm = random_density(N, 31)
    b = I.DeviceBasis(mol, lib)
    try:
        need, margin = b.jk_bytes(), 1024
        # the stored fill needs its work space (part of `need`) plus 8 N^4 bytes of output: more than need + margin as soon as 8 N^4 exceeds what the
        # direct call adds to the work space (3 N^2 + nshell^2 doubles and 4 KiB) plus the margin
        assert 8 * N ** 4 > 8 * (3 * N * N + mol.nbas ** 2) + 4096 + margin
        assert need + margin < 8 * N ** 4
        print(f"{name}: N = {N}, direct J / K takes {need} bytes on the device, the [N]^4 tensor alone {8 * N ** 4}")
        assert lib.qemb_int4c_mem_limit(b.h, need + margin) == 0
        out = np.empty((N,) * 4)
        assert lib.qemb_int4c2e(b.h, 1, 0.0, out.ctypes.data, 0) == _lib.QEMB_ERR_ALLOC
        J, K = b.get_jk(dm)
        compare(f"{name} under the memory limit", J, K, *host_jk(e, dm))
        assert lib.qemb_int4c_mem_limit(b.h, 64) == 0
        Jb, Kb = np.empty((N, N)), np.empty((N, N))
        assert lib.qemb_int_jk_direct(b.h, dm.ctypes.data, 0.0, Jb.ctypes.data, Kb.ctypes.data, 0) == _lib.QEMB_ERR_ALLOC
        assert f"N = {N}".encode() in lib.qemb_last_error()
        assert lib.qemb_int4c_mem_limit(b.h, -1) == 0
        J2, K2 = b.get_jk(dm)
        assert rel(J2, J) <= BAR and rel(K2, K) <= BAR
    finally:
        b.free()


def check_refusals(lib):
    mol, _ = host_eri("h2_sto3g")
    N = mol.nao
    dm, J, K = np.eye(N), np.empty((N, N)), np.empty((N, N))
    b = I.DeviceBasis(mol, lib)
    try:
        call = lambda d, t, j, k: lib.qemb_int_jk_direct(b.h, d, t, j, k, 0)
        assert call(None, 0.0, J.ctypes.data, K.ctypes.data) == _lib.QEMB_ERR_ARG
        assert call(dm.ctypes.data, 0.0, None, None) == _lib.QEMB_ERR_ARG
        assert call(dm.ctypes.data, -1.0, J.ctypes.data, K.ctypes.data) == _lib.QEMB_ERR_ARG
        assert lib.qemb_int_jk_direct_bytes(b.h, None) == _lib.QEMB_ERR_ARG
        assert call(dm.ctypes.data, 0.0, J.ctypes.data, None) == 0 and call(dm.ctypes.data, 0.0, None, K.ctypes.data) == 0
        with np.testing.assert_raises(ValueError):
            b.get_jk(np.array([[1.0, 0.2], [0.1, 1.0]]))
        dead = C.c_void_p(b.h.value)
    finally:
        b.free()
    assert lib.qemb_int_jk_direct(dead, dm.ctypes.data, 0.0, J.ctypes.data, K.ctypes.data, 0) == _lib.QEMB_ERR_ARG and b"live basis handle" in lib.qemb_last_error()
    with np.testing.assert_raises(ValueError):
        I.get_jk(mol, np.array([[1.0, 0.2], [0.1, 1.0]]), backend="hip", lib=lib)
    with np.testing.assert_raises(ValueError):
        I.get_jk(mol, np.array([[1.0, 0.2], [0.1, 1.0]]), backend="host")
    with np.testing.assert_raises(ValueError):
        I.RHF(mol, integral_backend="host", direct=True)
    with np.testing.assert_raises(ValueError):
        I.RHF(mol, direct=True)
    # an f orbital shell: the basis uploads, the direct call names the shell
    fmol = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]})
    fb = I.DeviceBasis(fmol, lib)
    try:
        fd, fj = np.eye(fmol.nao), np.empty((fmol.nao,) * 2)
        assert lib.qemb_int_jk_direct(fb.h, fd.ctypes.data, 0.0, fj.ctypes.data, None, 0) == _lib.QEMB_ERR_UNSUPPORTED
        assert b"orbital shell 1" in lib.qemb_last_error() and b"l = 3" in lib.qemb_last_error()
        try:
            fb.get_jk(fd)
            raise AssertionError("an f shell was accepted")
        except _lib.QembError as err:
            assert err.status == _lib.QEMB_ERR_UNSUPPORTED
    finally:
        fb.free()
