"""Shared cases of the DF mean-field tests (test_gpu_dfjk.py on the device, test_dfjk_hostlogic.py through the scalar twin): J and K from the resident 3-index tensor
of a DF context (csrc/ao2mo.cpp: DfContext::jk), RHF(density_fit=...) and BE(reuse_mf_df=True).  The reference of the fitted J and K is NumPy on the host integrals:
B = L^-1 T from integrals.aux_e2 / int2c2e, J = einsum("Ppq,Prs,rs"), K = einsum("Ppr,Pqs,rs").  Bars: 1e-10 of the largest element for J and K, 1e-10 Eh for SCF
energies, 1e-9 Eh for BE energies against another integral source and 1e-12 Eh where both sides read the same tensor."""
import functools

import numpy as np

import int4c_cases as c4
from quemb_amd import _lib
from quemb_amd import eri_transform as et
from quemb_amd import integrals as I

BAR = 1e-10

_CH_BASIS = {"C": [(0, [2.9, 0.68, 0.22], [-0.1, 0.4, 0.7]), (1, [2.9, 0.68, 0.22], [0.16, 0.61, 0.39]), (2, [0.8], [1.0])],
             "H": [(0, [3.4, 0.62, 0.17], [0.15, 0.54, 0.44]), (1, [0.73], [1.0])]}


def molecules():
    return {"h2": lambda: I.Mole([["H", (0.0, 0.0, 0.0)], ["H", (0.0, 0.0, 0.74)]]),                                          # N = 2, n_occ = 1: the smallest
            "ch": lambda: I.Mole([("C", (0.0, 0.0, 0.0)), ("H", (0.3, -0.2, 1.05))], basis=_CH_BASIS),                         # s p d + s p: N = 13, n_occ = 3
            "h8": lambda: I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])}


@functools.lru_cache(None)
def host_df(name):
    """(mol, auxmol, T = (P|mu nu) as [naux][N][N], j2c, B = L^-1 T) from the host integral source, computed once and shared (left unchanged by the checks)"""
    mol = molecules()[name]()
    aux = I.make_auxmol(mol, "etb")
    T = np.ascontiguousarray(I.aux_e2(mol, aux).transpose(2, 0, 1))
    j2c = I.int2c2e(aux)
    B = np.linalg.solve(np.linalg.cholesky(j2c), T.reshape(aux.nao, -1)).reshape(T.shape)
    for a in (T, j2c, B):
        a.setflags(write=False)
    return mol, aux, T, j2c, B


def ref_jk(B, dm):
    return np.einsum("Ppq,Prs,rs->pq", B, B, dm, optimize=True), np.einsum("Ppr,Pqs,rs->pq", B, B, dm, optimize=True)


def context(lib, name):
    """a DF context holding the host integrals of the molecule: the device adds the metric factorisation and the J / K driver"""
    mol, aux, T, j2c, _ = host_df(name)
    df = et.DFContext(j2c=j2c, lib=lib)
    df.set_ints(T, mol.nao, "Lpq")
    return df


def orbitals(name, shift=0):
    """n_occ orthonormal orbitals (S-metric) of the molecule: eigenvectors of the core Hamiltonian, `shift` levels up"""
    mol = host_df(name)[0]
    S, T, V = mol.one_electron()
    w, U = np.linalg.eigh(S)
    X = U / np.sqrt(w) @ U.T
    _, c = np.linalg.eigh(X @ (T + V) @ X)
    no = max(1, mol.nelectron // 2)
    return (X @ c)[:, shift: shift + no]


def densities(name):
    mol = host_df(name)[0]
    N = mol.nao
    C0, C1 = orbitals(name), orbitals(name, 1)
    r = np.random.default_rng(5).standard_normal((N, N))
    return {"orbitals": 2.0 * C0 @ C0.T, "random": 0.5 * (r + r.T), "indefinite": 2.0 * C0 @ C0.T - 2.0 * C1 @ C1.T}


def jk_bytes_formula(naux, N, ncol, kb, identity=False):
    """the documented figure of qemb_df_jk_bytes: buffers of the driver plus the most split-K slices (N x N each) the last product, of K-dimension naux kb, may leave"""
    K, t = naux * kb, ((N + 255) // 256) ** 2
    s = 0 if K < 1024 or t >= 256 else min(-(-768 // t), K // 256)
    s = s if s > 1 else 0
    return 8 * ((1 if identity else 2) * naux * N * kb + N * ncol + (3 + s) * N * N + 3 * naux)


def rel(a, ref):
    return float(np.abs(a - ref).max()) / float(np.abs(ref).max())


def check_jk(lib, name):
    """J and K of the three non-trivial densities and of the zero density against the NumPy reference"""
    mol, aux, T, j2c, B = host_df(name)
    N = mol.nao
    no = max(1, mol.nelectron // 2)
    if name == "ch":
        assert N % 16 and N % 32 and no % 4 and aux.nao % 16      # no dimension is a multiple of the GEMM tiles
    df = context(lib, name)
    try:
        for label, dm in densities(name).items():
            w = np.linalg.eigvalsh(dm)
            if label == "indefinite":
                assert w.min() < -0.1 and w.max() > 0.1      # negative columns do run
            Jr, Kr = ref_jk(B, dm)
            J, K = df.get_jk(dm)
            dj, dk = rel(J, Jr), rel(K, Kr)
            print(f"{name} (N = {N}, naux = {aux.nao}) {label}: max |J - ref| = {dj:.2e} of {np.abs(Jr).max():.3e}, max |K - ref| = {dk:.2e} of {np.abs(Kr).max():.3e}")
            assert dj <= BAR and dk <= BAR, (name, label, dj, dk)
            assert (K == K.T).all()
        C0 = orbitals(name)
        Jo, Ko = df.get_jk_orbitals(C0, 2.0)
        Jr, Kr = ref_jk(B, 2.0 * C0 @ C0.T)
        print(f"{name} from orbitals: J {rel(Jo, Jr):.2e}, K {rel(Ko, Kr):.2e}")
        assert rel(Jo, Jr) <= BAR and rel(Ko, Kr) <= BAR and (Ko == Ko.T).all()
        Jz, Kz = df.get_jk(np.zeros((N, N)))
        assert (Jz == 0.0).all() and (Kz == 0.0).all()      # exact zeros
    finally:
        df.free()


def check_options(lib, name="ch"):
    mol, aux, T, j2c, B = host_df(name)
    dm = densities(name)["random"]      # full rank, both signs: the slabs of every occ_block below cut the positive and the negative columns
    w = np.linalg.eigvalsh(dm)
    assert (w > 1e-3).sum() >= 3 and (w < -1e-3).sum() >= 3
    df = context(lib, name)
    try:
        J, K = df.get_jk(dm)
        Jonly, nk = df.get_jk(dm, with_k=False)
        nj, Konly = df.get_jk(dm, with_j=False)
        assert nk is None and nj is None and (Jonly == J).all() and (Konly == K).all()
        with np.testing.assert_raises(ValueError):
            df.get_jk(dm, with_j=False, with_k=False)
        with np.testing.assert_raises(ValueError):
            df.get_jk(dm + np.triu(np.ones_like(dm), 1))      # not symmetric
        ncol = int((np.abs(np.linalg.eigvalsh(dm)) > 1e-10).sum())
        top = np.abs(K).max()
        for kb in (1, 2, ncol):
            Kb = df.get_jk(dm, with_j=False, occ_block=kb)[1]
            Kb2 = df.get_jk(dm, with_j=False, occ_block=kb)[1]
            d = float(np.abs(Kb - K).max()) / top
            print(f"{name} occ_block = {kb} of {ncol} columns: K moves by {d:.2e} of max |K|")
            assert d <= 1e-13 and (Kb == Kb2).all() and (Kb == Kb.T).all()
    finally:
        df.free()


def check_cholesky(lib, name, tol):
    """J and K from the Cholesky factor of the AO integrals against the exact ones of Mole.eri_s1(): |(ij|kl) - sum L L| <= tol element by element, so every element
    of J and of K is off by at most tol sum |D|"""
    mol = molecules()[name]()
    e = mol.eri_s1()
    dm = densities(name)["orbitals"]
    Jr, Kr = np.einsum("pqrs,rs->pq", e, dm, optimize=True), np.einsum("pqrs,qs->pr", e, dm, optimize=True)
    bound = tol * np.abs(dm).sum()
    df = et.DFContext.from_cholesky(mol, tol=tol, lib=lib)
    try:
        J, K = df.get_jk(dm)
        dj, dk = float(np.abs(J - Jr).max()), float(np.abs(K - Kr).max())
        print(f"{name} Cholesky tol {tol:g} (rank {df.naux}): |J - exact| = {dj:.2e}, |K - exact| = {dk:.2e}, bound tol sum |D| = {bound:.2e}")
        assert dj <= bound and dk <= bound
        assert (K == K.T).all()
        assert df.jk_bytes(3, 2) == jk_bytes_formula(df.naux, mol.nao, 3, 2, identity=True) == 8 * (df.naux * mol.nao * 2 + mol.nao * 3 + 3 * mol.nao ** 2 + 3 * df.naux)
        assert df.layout == "dense" and df.identity_metric and df.cd_tol == tol
    finally:
        df.free()


def check_guards(lib, name="ch"):
    mol, aux, T, j2c, B = host_df(name)
    N, na = mol.nao, aux.nao
    dm = densities(name)["orbitals"]
    Cw = np.ascontiguousarray(orbitals(name))
    J, K = np.empty((N, N)), np.empty((N, N))
    df = context(lib, name)
    try:
        for ncol, kb, eff in ((3, 0, 3), (3, 2, 2), (5, 9, 5), (0, 0, 0)):
            assert df.jk_bytes(ncol, kb) == jk_bytes_formula(na, N, ncol, eff) == 8 * (2 * na * N * eff + N * ncol + 3 * N * N + 3 * na)
        assert na * 13 >= 1024      # long enough for the last product to be split: its slices are counted
        assert df.jk_bytes(13, 0) == jk_bytes_formula(na, N, 13, 13) == 8 * (2 * na * N * 13 + N * 13 + (3 + na * 13 // 256) * N * N + 3 * na)
        assert df.layout == "dense" and not df.identity_metric
        call = lambda *a: lib.qemb_df_jk(df.h, *a)
        assert call(N, dm.ctypes.data, Cw.ctypes.data, Cw.shape[1], 0, 0, None, None) == _lib.QEMB_ERR_ARG
        assert call(N + 1, dm.ctypes.data, Cw.ctypes.data, Cw.shape[1], 0, 0, J.ctypes.data, K.ctypes.data) == _lib.QEMB_ERR_ARG
        assert call(N, dm.ctypes.data, None, Cw.shape[1], 0, 0, J.ctypes.data, K.ctypes.data) == _lib.QEMB_ERR_ARG
        assert call(N, dm.ctypes.data, Cw.ctypes.data, -1, 0, 0, J.ctypes.data, K.ctypes.data) == _lib.QEMB_ERR_ARG
        assert lib.qemb_df_jk_bytes(df.h, 3, 0, None) == _lib.QEMB_ERR_ARG
        # the memory guard with a faked limit: refused before anything is allocated, and the call works again once the limit is lifted
        df.jk_mem_limit(64)
        assert call(N, dm.ctypes.data, Cw.ctypes.data, Cw.shape[1], 0, 0, J.ctypes.data, K.ctypes.data) == _lib.QEMB_ERR_ALLOC
        msg = lib.qemb_last_error()
        assert f"N = {N}".encode() in msg and f"naux = {na}".encode() in msg
        # a limit that holds one column but not all: the default slab shrinks instead of failing
        df.jk_mem_limit(df.jk_bytes(Cw.shape[1], 1) + 8)
        K1 = df.get_jk_orbitals(Cw, 2.0, with_j=False)[1]
        df.jk_mem_limit(None)
        K0 = df.get_jk_orbitals(Cw, 2.0, with_j=False)[1]
        assert np.abs(K1 - K0).max() <= 1e-13 * np.abs(K0).max()
    finally:
        df.free()
    # layouts out of scope are refused by name
    sp = et.DFContext(j2c=j2c, lib=lib)
    try:
        reach = [list(range(N)) for _ in range(N)]
        sp.set_ints_semisparse(et.SemiSparseSym3DTensor.from_dense(T, reach))
        assert sp.layout == "semisparse"
        with np.testing.assert_raises(ValueError):      # refused where the mean field is made, not inside kernel()
            I.RHF(mol, integral_backend="hip", lib=lib, density_fit=sp)
        try:
            sp.get_jk(dm)
            raise AssertionError("a semi-sparse context was accepted")
        except _lib.QembError as err:
            assert err.status == _lib.QEMB_ERR_UNSUPPORTED and "semi-sparse" in str(err)
    finally:
        sp.free()
    pb = et.DFContext.periodic(j2c, lib=lib)
    try:
        pb.alloc_ints(N)
        assert pb.layout == "periodic"
        with np.testing.assert_raises(ValueError):
            I.RHF(mol, integral_backend="hip", lib=lib, density_fit=pb)
        try:
            pb.get_jk(dm)
            raise AssertionError("a periodic context was accepted")
        except _lib.QembError as err:
            assert err.status == _lib.QEMB_ERR_UNSUPPORTED and "periodic" in str(err)
    finally:
        pb.free()


# ---- the mean field ---------------------------------------------------------------------------------------------------------------------------------------
_MF = {}


def df_h8_mf(lib, density_fit="etb"):
    """the density-fitted mean field of H8 / STO-3G on this library, converged once per source of the tensor and shared"""
    key = (id(lib), density_fit)
    if key not in _MF:
        mf = I.RHF(molecules()["h8"](), integral_backend="hip", lib=lib, density_fit=density_fit)
        mf.kernel()
        _MF[key] = (lib, mf)
    return _MF[key][1]


def check_df_rhf(lib):
    mol, aux, T, j2c, B = host_df("h8")
    mf = df_h8_mf(lib)
    assert mf._eri is None and mf.converged and isinstance(mf.with_df, et.DFContext)
    D = mf.make_rdm1()
    S, Tk, V = mol.one_electron()
    assert rel(mf.get_ovlp(), S) <= BAR and rel(mf.get_hcore(), Tk + V) <= BAR      # hcore and S came from the device
    ne = float(np.trace(D @ S))
    Jr, Kr = ref_jk(B, D)
    F = Tk + V + Jr - 0.5 * Kr
    comm = float(np.linalg.norm(F @ D @ S - S @ D @ F))
    e_ref = 0.5 * float(np.sum((Tk + V + F) * D)) + mol.energy_nuc()
    print(f"DF RHF H8: e_tot {mf.e_tot:.12f}, NumPy DF energy at the same density {e_ref:.12f} (difference {abs(e_ref - mf.e_tot):.2e}), "
          f"tr(D S) - n_elec = {ne - mol.nelectron:.2e}, |FDS - SDF| = {comm:.2e}")
    assert abs(ne - mol.nelectron) <= 1e-10
    assert comm < 1e-7
    assert abs(e_ref - mf.e_tot) <= 1e-10
    # get_veff on densities BE hands over: the HF density and a core-like one
    core = 2.0 * np.outer(mf.mo_coeff[:, 0], mf.mo_coeff[:, 0])
    for d in (D, core):
        j, k = ref_jk(B, d)
        assert np.abs(mf.get_veff(d) - (j - 0.5 * k)).max() <= BAR * np.abs(j).max()
    assert mf._eri is None


def check_cholesky_rhf(lib, tol=1e-10):
    """first-order bound: E[D] is stationary in D, so the error of the converged energy is that of the energy functional at fixed D, 1/2 sum D (dJ - dK / 2) D with
    |d(ij|kl)| <= tol: |dE| <= (1/2 + 1/4) tol (sum |D|)^2"""
    ref = c4.h8_mf()
    mf = I.RHF(molecules()["h8"](), integral_backend="hip", lib=lib, density_fit=("cholesky", tol))
    try:
        e = mf.kernel()
        D = mf.make_rdm1()
        bound = 0.75 * tol * np.abs(D).sum() ** 2 + 1e-10
        print(f"Cholesky RHF H8 at tol {tol:g} (rank {mf.with_df.naux}): e_tot {e:.12f}, exact host RHF {ref.e_tot:.12f}, difference {abs(e - ref.e_tot):.2e}, bound {bound:.2e}")
        assert mf._eri is None and mf.converged
        assert abs(e - ref.e_tot) <= bound
    finally:
        mf.free()
    assert mf.with_df is None


def check_borrowed_and_bad(lib):
    mol, aux, T, j2c, B = host_df("h2")
    df = context(lib, "h2")
    try:
        mf = I.RHF(mol, integral_backend="hip", lib=lib, density_fit=df)
        assert mf.with_df is df
        e = mf.kernel()
        S, Tk, V = mol.one_electron()
        D = mf.make_rdm1()
        Jr, Kr = ref_jk(B, D)
        e_ref = 0.5 * float(np.sum((2 * (Tk + V) + Jr - 0.5 * Kr) * D)) + mol.energy_nuc()
        print(f"borrowed context, H2: e_tot {e:.12f}, NumPy DF energy {e_ref:.12f}")
        assert abs(e - e_ref) <= 1e-10
        mf.free()
        assert df.h is not None and mf.with_df is df      # borrowed: left alone
        J, K = df.get_jk(D)
        assert rel(J, Jr) <= BAR and rel(K, Kr) <= BAR
    finally:
        df.free()
    for kw in (dict(density_fit="etb"), dict(integral_backend="host", density_fit="etb"), dict(integral_backend="hip", direct=True, density_fit="etb"),
               dict(integral_backend="hip", direct=True, density_fit=("cholesky", 1e-8))):
        with np.testing.assert_raises(ValueError):
            I.RHF(mol, lib=lib, **kw)


def _be(lib, mf, solver, **kw):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    be = BE(mf, fobj, lib=lib, distribute=False, integral_backend="hip", **kw)
    e, comp = be.oneshot(solver=solver)[:2]
    return np.array([e, *comp])


def check_be_reuse(lib, route, solver):
    """H8 BE2: the fragments transformed from the mean field's own tensor against BE filling a second context from the same auxiliaries / tolerance -- the same
    tensor, so the energies agree to rounding"""
    if route == "df":
        mf = df_h8_mf(lib)
        own = _be(lib, mf, solver, int_transform="int-direct-DF-hip", auxbasis="etb")
        shared = _be(lib, mf, solver, int_transform="int-direct-DF-hip", reuse_mf_df=True)      # no auxbasis needed
    else:
        mf = df_h8_mf(lib, ("cholesky", 1e-8))
        own = _be(lib, mf, solver, int_transform="cholesky-hip", cd_tol=1e-8)
        shared = _be(lib, mf, solver, int_transform="cholesky-hip", cd_tol=1e-8, reuse_mf_df=True)
    assert mf.with_df is not None and mf.with_df.h is not None      # BE did not free the borrowed context
    print(f"BE2 {route} {solver}: E_corr own tensor {own[0]:.12f}, mean field's tensor {shared[0]:.12f}, pieces differ by {np.abs(own - shared).max():.2e}")
    assert np.abs(own - shared).max() <= 1e-12, (own, shared)


def check_one_argument_jk(lib):
    """routes without density_fit keep calling `_jk(dm)` with one argument: a one-argument wrapper around it (what tools/jk_direct_bench.py installs to count the
    J / K builds) still works on the stored and on the direct route"""
    mol = molecules()["h2"]()
    for kw in (dict(), dict(integral_backend="hip", lib=lib, direct=True)):
        mf = I.RHF(mol, **kw)
        calls, jk0 = [0], mf._jk
        mf._jk = lambda d, _f=jk0, _c=calls: (_c.__setitem__(0, _c[0] + 1), _f(d))[1]
        e = mf.kernel()
        mf.free()
        assert mf.converged and calls[0] >= 2 and abs(e + 1.1167) < 1e-3


def check_be_reuse_refused(lib):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    kw = dict(lib=lib, distribute=False, integral_backend="hip", reuse_mf_df=True)
    with np.testing.assert_raises(ValueError):      # a mean field without with_df
        BE(c4.h8_mf(), fobj, int_transform="int-direct-DF-hip", auxbasis="etb", **kw)
    # the tensor must be the kind the branch would have filled: a fitted tensor is no Cholesky factor, and the other way round
    with np.testing.assert_raises(ValueError):
        BE(df_h8_mf(lib), fobj, int_transform="cholesky-hip", **kw)
    with np.testing.assert_raises(ValueError):
        BE(df_h8_mf(lib, ("cholesky", 1e-8)), fobj, int_transform="int-direct-DF-hip", **kw)
    with np.testing.assert_raises(ValueError):      # a branch that reads no 3-index tensor
        BE(df_h8_mf(lib), fobj, int_transform="in-core-hip", **kw)

    class NoMol:      # a mean field without `mol`: the ValueError of the option, not an AttributeError
        with_df = df_h8_mf(lib).with_df
    with np.testing.assert_raises(ValueError):
        BE(NoMol(), fobj, int_transform="int-direct-DF-hip", **kw)
    # a semi-sparse context on the mean field is refused although it is a DFContext
    mol, aux, T, j2c, _ = host_df("h8")
    sp = et.DFContext(j2c=j2c, lib=lib)
    try:
        sp.set_ints_semisparse(et.SemiSparseSym3DTensor.from_dense(T, [list(range(mol.nao)) for _ in range(mol.nao)]))
        mf = c4.h8_mf()
        mf.with_df = sp
        with np.testing.assert_raises(ValueError):
            BE(mf, fobj, int_transform="int-direct-DF-hip", **kw)
    finally:
        sp.free()
