"""Shared cases of the Cholesky-decomposed AO integrals (test_gpu_cholesky.py on the device, test_cholesky_hostlogic.py through the scalar twin): every check
takes the library handle, so the same comparison runs on both.  There is no second implementation of the route to compare with; the yardsticks are the
project's own stored integrals V = integrals.eri(mol, 4, backend="hip") -- the panel columns are the kTile form, which equals them bit for bit, so the integral
error drops out -- the stored route AOEri.from_basis(...).transform(TA) and BE on int_transform="in-core-hip" from the geometry.

The bound of the decomposition is a theorem: on a positive semidefinite residual R = V - L^T L, |R[ij,kl]| <= sqrt(R[ij,ij] R[kl,kl]) <= tol.  ROUND adds the
rounding of the at most a few hundred products of order-one numbers that form an element of L^T L (M eps ~ 1e-13), as a fraction of max |V|."""
import ctypes as C
import threading

import numpy as np

import ao2mo_direct_cases as ca
import int4c_cases as c4
import jk_direct_cases as cj
from quemb_amd import _lib
from quemb_amd import eri_transform as et
from quemb_amd import integrals as I
from quemb_amd.fragsolver import DeviceFragment

ROUND = 1e-12                    # of max |V| (or max |G|): rounding beside the theorem's tol
RANK_SLACK = 1.25                # panel pivoting is greedy only within the span factor: a few more vectors than full pivoting, never a multiple
TOLS = (1e-4, 1e-8)

# End to end, H8 / STO-3G BE2, one-shot correlation energy against int_transform="in-core-hip" from the geometry, measured on the CPU mock (Eh):
#   solver   cd_tol = 1e-6   cd_tol = 1e-8   cd_tol = 1e-10
#   CCSD     2.42e-08        1.21e-11        1.21e-11
#   MP2      4.93e-10        6.06e-12        6.06e-12
# (rank 21 at 1e-6 and 26 at 1e-8 and at 1e-10, of 36 pairs: the minimal basis has no vector between those two tolerances, so their factors are the same.)
# The bar for cd_tol = 1e-10 is ten times the measured mock difference (the GPU's GEMM sums in another order than the mock's); the 1e-6 run may not beat the
# 1e-10 run by more than that bar (a tolerance that is not threaded through would make all three runs equal).
E2E_MOCK_1E10 = {"CCSD": 1.21e-11, "MP2": 6.06e-12}
E2E_BAR = {k: 10.0 * v for k, v in E2E_MOCK_1E10.items()}


def molecules():
    m = dict(c4.molecules())
    m["spd_atom"] = lambda: I.Mole([("H", (0.0, 0.0, 0.0))], basis=c4._SPD)      # one centre: rank 40 of 45 pairs at every tol, the heaviest linear dependence
    return m


_MOL, _V, _CD = {}, {}, {}


def mole(name):
    if name not in _MOL:
        _MOL[name] = molecules()[name]()
    return _MOL[name]


def stored(lib, name):
    """V, the stored 4-fold packed integrals of this library: computed once, shared, left unchanged"""
    if (id(lib), name) not in _V:
        v = I.eri(mole(name), 4, backend="hip", lib=lib)
        v.setflags(write=False)
        _V[(id(lib), name)] = (lib, v)
    return _V[(id(lib), name)][1]


def decompose(lib, name, tol, panel_pairs=None):
    """(L, stats) of one decomposition, computed once per (library, molecule, tol, panel) and shared"""
    k = (id(lib), name, tol, panel_pairs)
    if k not in _CD:
        b = I.DeviceBasis(mole(name), lib)
        try:
            L = b.cholesky(tol, panel_pairs=panel_pairs)
            st = b.cholesky_stats()
        finally:
            b.free()
        L.setflags(write=False)
        _CD[k] = (lib, L, st)
    return _CD[k][1:]


def numpy_cd(V, tol):
    """full-pivot incomplete Cholesky of V: the reference rank"""
    d = np.diag(V).copy()
    L = []
    while True:
        p = int(np.argmax(d))
        if not d[p] > tol:
            return np.array(L).reshape(len(L), V.shape[0])
        v = V[:, p].copy()
        for l in L:
            v -= l * l[p]
        v /= np.sqrt(d[p])
        L.append(v)
        d = np.maximum(d - v * v, 0.0)
        d[p] = 0.0


def bound(V, tol):
    return tol + ROUND * float(np.abs(V).max())


# ---- 1. the bound, 2. the rank -----------------------------------------------------------------------------------------------------------------------------
def check_bound_and_rank(lib, name, tol):
    V = stored(lib, name)
    npair = V.shape[0]
    L, st = decompose(lib, name, tol)
    err = float(np.abs(V - L.T @ L).max())
    ref = numpy_cd(V, tol)
    assert float(np.abs(V - ref.T @ ref).max()) <= bound(V, tol)      # the reference itself
    print(f"{name}, tol = {tol:g}: N = {mole(name).nao}, npair = {npair}, device rank {L.shape[0]} in {st['panels']} panels ({st['columns']} columns evaluated), "
          f"full-pivot NumPy rank {ref.shape[0]}; max |V - L^T L| = {err:.2e} (bound {bound(V, tol):.2e}), final max d = {st['max_d']:.2e}")
    assert L.shape == (st["rank"], npair) and st["columns"] >= st["rank"] and st["panels"] >= 1
    assert err <= bound(V, tol), (name, tol, err)
    assert st["max_d"] <= tol
    assert L.shape[0] <= RANK_SLACK * ref.shape[0] and L.shape[0] <= npair, (L.shape[0], ref.shape[0])
    if name == "spd_atom":
        assert L.shape[0] < 45
    return L.shape[0], ref.shape[0]


# ---- 3. panel independence ---------------------------------------------------------------------------------------------------------------------------------
def check_panel_independence(lib, name="spd3", tol=1e-8):
    V = stored(lib, name)
    npair = V.shape[0]
    runs = {k: decompose(lib, name, tol, pp) for k, pp in (("one shell pair", 1), ("default", None), ("one panel per sweep", npair))}
    prods = {}
    for k, (L, st) in runs.items():
        prods[k] = L.T @ L
        err = float(np.abs(V - prods[k]).max())
        print(f"{name}, tol = {tol:g}, {k}: rank {L.shape[0]}, {st['panels']} panels, {st['columns']} columns, max |V - L^T L| = {err:.2e}")
        assert err <= bound(V, tol), (k, err)
    ks = list(runs)
    for i in range(3):
        for j in range(i):
            assert float(np.abs(prods[ks[i]] - prods[ks[j]]).max()) <= 2.0 * tol
    assert len({st["panels"] for _, st in runs.values()}) == 3, {k: st["panels"] for k, (_, st) in runs.items()}
    assert runs["one shell pair"][1]["panels"] > runs["default"][1]["panels"] > runs["one panel per sweep"][1]["panels"]


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------------------------------------
def check_reproducible(lib, name="spd3", tol=1e-8):
    mol = mole(name)
    first, _ = decompose(lib, name, tol)
    b = I.DeviceBasis(mol, lib)
    try:
        again = b.cholesky(tol)
        assert again.tobytes() == first.tobytes()
        # ... and from a host thread bound to a second execution context (where the backend has one)
        out, err = {}, []
        n = lib.qemb_ctx_count(2)

        def work():
            try:
                if n >= 2:
                    _lib.check(lib.qemb_ctx_bind(1), "qemb_ctx_bind", lib)
                b2 = I.DeviceBasis(mol, lib)
                try:
                    out["L"] = b2.cholesky(tol)
                finally:
                    b2.free()
            except Exception as e:  # noqa: BLE001
                err.append(e)

        t = threading.Thread(target=work)
        t.start(); t.join()
        assert not err, err
        assert out["L"].tobytes() == first.tobytes()
        assert b.cholesky(tol).tobytes() == first.tobytes()      # and on the first context again, on a basis whose pair stage is resident
    finally:
        b.free()
    print(f"{name}, tol = {tol:g}: four decompositions ({n} execution contexts) give the same {first.nbytes} bytes")


# ---- 5. layout -----------------------------------------------------------------------------------------------------------------------------------------------
def unpack(L, N):
    out = np.zeros((L.shape[0], N, N))
    iu = np.tril_indices(N)
    out[:, iu[0], iu[1]] = L
    out[:, iu[1], iu[0]] = L
    return out


def df_image(df):
    out, ident = np.full((df.naux, df.nao, df.nao), np.nan), C.c_int(-1)
    _lib.check(df.lib.qemb_op_df_get_ints(df.h, out.ctypes.data, C.byref(ident)), "qemb_op_df_get_ints", df.lib)
    return out, ident.value


def check_layout(lib, name="spd3", tol=1e-8):
    mol = mole(name)
    L, st = decompose(lib, name, tol)
    df = et.DFContext.from_cholesky(mol, tol=tol, lib=lib)
    try:
        assert df.naux == L.shape[0] and df.cd_stats == st
        img, ident = df_image(df)
        assert ident == 1
        assert (img == img.transpose(0, 2, 1)).all()                  # symmetric in mu, nu to the bit
        assert img.tobytes() == unpack(L, mol.nao).tobytes()          # the unpacked packed factor, the same decomposition
        G = df.transform(np.eye(mol.nao))
    finally:
        df.free()
    ref = L.T @ L
    d = float(np.abs(G - ref).max())
    print(f"{name}: [M][N][N] image = unpacked packed factor (M = {L.shape[0]}); transform(TA = 1) against L^T L: {d:.2e}")
    assert d <= ROUND * float(np.abs(ref).max())


# ---- 6. the consumer -------------------------------------------------------------------------------------------------------------------------------------------
def check_consumer(lib, name, tol):
    mol = mole(name)
    N = mol.nao
    n = N - 3
    TA = ca.random_ta(N, n, 400 + N)
    ref = ca.stored_transform(lib, name, ("cd", n), TA)
    c = float(np.abs(TA).sum(axis=0).max())
    bar = tol * c ** 4 + ROUND * float(np.abs(ref).max())
    df = et.DFContext.from_cholesky(mol, tol=tol, lib=lib)
    fr = DeviceFragment(n, min(4, n), lib)
    try:
        G = df.transform(TA)
        assert df.transform(TA, frag=fr, want_host=False, factor_only=True) is None
        naux = fr.mo_route_used()[1]
        B = np.empty((naux, n * (n + 1) // 2))
        _lib.check(lib.qemb_frag_get_df_factor(fr.h, B.ctypes.data), "qemb_frag_get_df_factor", lib)
    finally:
        fr.free(); df.free()
    d_block, d_factor = float(np.abs(G - ref).max()), float(np.abs(B.T @ B - ref).max())
    print(f"{name}, tol = {tol:g}, n = {n}: c = {c:.3f}, max |G - stored route| = {d_block:.2e} (block), {d_factor:.2e} (from the factor, {naux} vectors); bound {bar:.2e}")
    assert naux == df.cd_stats["rank"]
    assert d_block <= bar and d_factor <= bar, (d_block, d_factor, bar)


# ---- 7. the new kernels on their own -----------------------------------------------------------------------------------------------------------------------------
def panel_factor(lib, A, thr):
    n = A.shape[0]
    A = np.ascontiguousarray(A)
    T, piv, rank, lds = np.full((n, n), np.nan), np.full(n, -1, dtype=np.int32), C.c_int32(-1), C.c_int(-1)
    _lib.check(lib.qemb_op_cd_panel_factor(n, A.ctypes.data, float(thr), T.ctypes.data, piv.ctypes.data, C.byref(rank), C.byref(lds)), "qemb_op_cd_panel_factor", lib)
    return T, piv, rank.value, lds.value


def psd(n, rank, seed):
    X = np.random.default_rng(seed).standard_normal((rank, n))
    return X.T @ X


def check_panel_kernel(lib, case):
    thr = 1e-9
    if case == "rank7":
        A, want = psd(12, 7, 1), 7
    elif case == "twins":      # two identical columns: the second must never be a pivot
        A = psd(6, 6, 2)
        A = np.block([[A, A[:, 3:4]], [A[3:4, :], A[3:4, 3:4]]])
        want = 6
    elif case == "one":
        A, want = np.array([[2.25]]), 1
    elif case == "n140":       # beyond the LDS limit (86 columns): the factor and the panel's diagonal in global memory
        A, want = psd(140, 100, 3), 100
    else:                      # n86: the largest block held in LDS
        A, want = psd(86, 86, 4), 86
    n = A.shape[0]
    T, piv, r, lds = panel_factor(lib, A, thr)
    res = A - T[:r].T @ T[:r]
    print(f"panel {case}: n = {n}, rank {r} (expected {want}), in LDS {lds}, max residual diagonal {np.diag(res).max():.2e}, max |residual| {np.abs(res).max():.2e}")
    assert r == want
    assert lds == (1 if n <= 86 else 0)
    assert len(set(piv[:r])) == r and (piv[:r] >= 0).all() and (piv[:r] < n).all()
    scale = float(np.abs(A).max())
    assert np.diag(res).max() <= thr + 1e-12 * scale and np.abs(res).max() <= thr + 1e-12 * scale
    for j in range(r):         # triangular in pivot order: vector j vanishes at the earlier pivots, exactly, and its own pivot entry is its diagonal
        assert (T[j, piv[:j]] == 0.0).all() and T[j, piv[j]] > 0.0
    # greedy: every pivot is the largest remaining diagonal (ties to the lower column)
    d = np.diag(A).copy()
    for j in range(r):
        left = np.delete(np.arange(n), piv[:j])
        assert d[piv[j]] >= d[left].max() - 1e-10 * scale
        d = d - T[j] ** 2
    if case == "twins":
        assert not (3 in piv[:r] and 6 in piv[:r])
    if case == "one":
        assert piv[0] == 0 and T[0, 0] == 1.5
    assert panel_factor(lib, A, thr)[0].tobytes() == T.tobytes()
    # a threshold above every diagonal: nothing to do
    assert panel_factor(lib, A, 2.0 * float(np.diag(A).max()))[2] == 0


def check_diag_kernel(lib):
    rng = np.random.default_rng(5)
    np_, r = 300, 3                                   # more than one workgroup of 256 rows
    Ln = rng.standard_normal((r, np_))
    d = (Ln ** 2).sum(axis=0) + rng.uniform(0.5, 1.5, np_)
    pivrow = np.array([7, 256, 299], dtype=np.int32)
    d[11] = (Ln[:, 11] ** 2).sum() - 1e-3             # a difference below zero: clamped to 0
    d[7] = (Ln[:, 7] ** 2).sum() + 0.25               # a pivot whose subtraction leaves something: exactly 0 all the same
    cnt = np.array([1] * 20 + [3] * 40 + [5] * 32, dtype=np.int32)      # 92 "shell pairs" covering the 300 rows
    row0 = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    assert cnt.sum() == np_
    want = d - (Ln ** 2).sum(axis=0)
    want[want < 0] = 0.0
    want[pivrow] = 0.0
    got, spmax, dmax = d.copy(), np.full(len(cnt), np.nan), C.c_double(-1.0)
    _lib.check(lib.qemb_op_cd_diag_update(np_, r, Ln.ctypes.data, pivrow.ctypes.data, got.ctypes.data, len(cnt), row0.ctypes.data, cnt.ctypes.data, spmax.ctypes.data,
                                          C.byref(dmax)), "qemb_op_cd_diag_update", lib)
    assert (got[pivrow] == 0.0).all() and got[11] == 0.0 and (got >= 0.0).all()
    assert np.abs(got - want).max() <= 1e-14 * np.abs(d).max()
    ref_max = np.array([got[a:a + c].max() for a, c in zip(row0, cnt)])
    assert (spmax == ref_max).all() and dmax.value == got.max()
    # r = 0: the maxima of the diagonal as it is
    g0, sp0, m0 = d.copy(), np.full(len(cnt), np.nan), C.c_double(-1.0)
    _lib.check(lib.qemb_op_cd_diag_update(np_, 0, None, None, g0.ctypes.data, len(cnt), row0.ctypes.data, cnt.ctypes.data, sp0.ctypes.data, C.byref(m0)),
               "qemb_op_cd_diag_update", lib)
    assert (g0 == d).all() and m0.value == d.max()
    # more shell pairs than one workgroup of the first stage holds: the second stage reduces several partials
    n2 = 700
    d2 = rng.uniform(0.0, 1.0, n2)
    one, r0 = np.ones(n2, dtype=np.int32), np.arange(n2, dtype=np.int32)
    sp2, m2 = np.empty(n2), C.c_double()
    _lib.check(lib.qemb_op_cd_diag_update(n2, 0, None, None, d2.ctypes.data, n2, r0.ctypes.data, one.ctypes.data, sp2.ctypes.data, C.byref(m2)), "qemb_op_cd_diag_update", lib)
    assert (sp2 == d2).all() and m2.value == d2.max()


def check_permute_kernel(lib):
    rng = np.random.default_rng(6)
    N, M = 7, 5
    npair = N * (N + 1) // 2
    L = rng.standard_normal((M, npair))
    pos = rng.permutation(npair).astype(np.int32)
    packed, full = np.full((M, npair), np.nan), np.full((M, N, N), np.nan)
    _lib.check(lib.qemb_op_cd_permute(M, N, L.ctypes.data, pos.ctypes.data, 0, packed.ctypes.data), "qemb_op_cd_permute", lib)
    _lib.check(lib.qemb_op_cd_permute(M, N, L.ctypes.data, pos.ctypes.data, 1, full.ctypes.data), "qemb_op_cd_permute", lib)
    assert (packed == L[:, pos]).all()
    assert (full == unpack(L[:, pos], N)).all()
    bad = pos.copy(); bad[3] = npair
    assert lib.qemb_op_cd_permute(M, N, L.ctypes.data, bad.ctypes.data, 0, packed.ctypes.data) == _lib.QEMB_ERR_ARG


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------------------------------------
_E2E_REF = {}


def be_oneshot(lib, solver, route, **kw):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mf = cj.direct_h8_mf(lib)
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    be = BE(mf, fobj, lib=lib, distribute=False, int_transform=route, integral_backend="hip", **kw)
    assert be._eri_from_geometry and mf._eri is None
    return float(be.oneshot(solver=solver)[0]), be


def check_end_to_end(lib, solver):
    if (id(lib), solver) not in _E2E_REF:
        _E2E_REF[(id(lib), solver)] = (lib, be_oneshot(lib, solver, "in-core-hip")[0])
    ref = _E2E_REF[(id(lib), solver)][1]
    diff, be = {}, None
    for tol in (1e-6, 1e-8, 1e-10):
        e, be = be_oneshot(lib, solver, "cholesky-hip", cd_tol=tol)
        diff[tol] = abs(e - ref)
        assert be.cd_stats["rank"] < 36 and be.cd_stats["max_d"] <= tol, be.cd_stats
        print(f"H8 BE2 {solver}, cd_tol = {tol:g}: rank {be.cd_stats['rank']} of 36 pairs, one-shot E_corr {e:.12f}, in-core-hip {ref:.12f}, difference {diff[tol]:.2e}")
    bar = E2E_BAR[solver]
    assert diff[1e-10] <= bar, (diff, bar)
    assert diff[1e-6] >= diff[1e-10] - bar, diff
    be.optimize(solver=solver)                 # the matching iterations run on this route (the fragments live on the factor)
    assert np.isfinite(be.e_corr)
    print(f"H8 BE2 {solver}, cd_tol = 1e-10: optimize E_corr {be.e_corr:.12f}")


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mol = mole("h8_sto3g")
    npair = 36
    b = I.DeviceBasis(mol, lib)
    out, m = np.empty((npair, npair)), C.c_int64()
    call = lambda tol, span, panel, max_rank: lib.qemb_int_cholesky(b.h, tol, span, panel, max_rank, out.ctypes.data, C.byref(m))
    try:
        assert call(0.0, 0.01, 0, 0) == _lib.QEMB_ERR_ARG and b"tolerance" in lib.qemb_last_error()
        assert call(-1e-8, 0.01, 0, 0) == _lib.QEMB_ERR_ARG
        assert call(1e-8, 0.0, 0, 0) == _lib.QEMB_ERR_ARG and b"span" in lib.qemb_last_error()
        assert call(1e-8, 1.5, 0, 0) == _lib.QEMB_ERR_ARG
        assert lib.qemb_int_cholesky(b.h, 1e-8, 0.01, 0, 0, out.ctypes.data, None) == _lib.QEMB_ERR_ARG
        assert lib.qemb_int_cholesky_bytes(b.h, 0, 0, None) == _lib.QEMB_ERR_ARG
        with np.testing.assert_raises(_lib.QembError):
            b.cholesky(tol=0.0)
        with np.testing.assert_raises(ValueError):
            I.cholesky_eri(mol, 1e-8, backend="host")
        # memory: a limit one byte below the call's own figure is refused before anything is allocated, at the figure it runs
        need = b.cholesky_bytes(max_rank=npair)
        assert need > 8 * npair * npair      # (at N = 8 the pair stage and the panel outweigh npair^2 doubles: the saving is a matter of larger N)
        assert lib.qemb_int4c_mem_limit(b.h, need - 1) == 0
        assert call(1e-8, 0.01, 0, npair) == _lib.QEMB_ERR_ALLOC
        msg = lib.qemb_last_error()
        assert f"N = {mol.nao}".encode() in msg and str(need).encode() in msg, msg
        assert lib.qemb_int4c_mem_limit(b.h, need) == 0
        assert call(1e-8, 0.01, 0, npair) == 0 and m.value == 26
        assert lib.qemb_int4c_mem_limit(b.h, -1) == 0
        # max_rank: no silently worse factor
        assert call(1e-8, 0.01, 0, 5) == _lib.QEMB_ERR_NOCONV
        msg = lib.qemb_last_error().decode()
        st = b.cholesky_stats()
        assert f"N = {mol.nao}" in msg and "rank 5" in msg and f"{st['max_d']:.3e}" in msg and st["rank"] == 5 and st["max_d"] > 1e-8, (msg, st)
        df = et.DFContext.empty(lib)
        try:
            assert lib.qemb_df_set_ints_from_cholesky(df.h, b.h, 1e-8, 0.01, 0, 5) == _lib.QEMB_ERR_NOCONV
            assert lib.qemb_df_set_ints_from_cholesky(df.h, b.h, 0.0, 0.01, 0, 0) == _lib.QEMB_ERR_ARG
            assert lib.qemb_df_set_ints_from_cholesky(None, b.h, 1e-8, 0.01, 0, 0) == _lib.QEMB_ERR_ARG
        finally:
            df.free()
        dead = C.c_void_p(b.h.value)
    finally:
        b.free()
    assert lib.qemb_int_cholesky(dead, 1e-8, 0.01, 0, 0, None, C.byref(m)) == _lib.QEMB_ERR_ARG and b"live basis handle" in lib.qemb_last_error()
    assert lib.qemb_int_cholesky_stats(dead, (C.c_double * 4)()) == _lib.QEMB_ERR_ARG
    # an f orbital shell: the existing refusal, naming the shell
    fmol = I.Mole([("H", (0.0, 0.0, 0.0))], basis={"H": [(0, [1.0], [1.0]), (3, [0.8], [1.0])]})
    fb = I.DeviceBasis(fmol, lib)
    try:
        assert lib.qemb_int_cholesky(fb.h, 1e-8, 0.01, 0, 0, None, C.byref(m)) == _lib.QEMB_ERR_UNSUPPORTED
        assert b"orbital shell 1" in lib.qemb_last_error() and b"l = 3" in lib.qemb_last_error()
        assert lib.qemb_int_cholesky_bytes(fb.h, 0, 0, C.byref(C.c_int64())) == _lib.QEMB_ERR_UNSUPPORTED
    finally:
        fb.free()
    # BE: the route needs the device integrals and a geometry
    fobj = lambda: FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    mf = c4.h8_mf()
    assert "cholesky-hip" in et.HIP_INT_TRANSFORMS
    with np.testing.assert_raises(ValueError):
        BE(mf, fobj(), lib=lib, distribute=False, int_transform="cholesky-hip", integral_backend="host")
    with np.testing.assert_raises(ValueError):
        BE(mf, fobj(), lib=lib, distribute=False, int_transform="cholesky-hip")

    class NoMol:
        mol = None

        def __init__(self, m_):
            self._m = m_

        def __getattr__(self, k):
            return getattr(self._m, k)

    with np.testing.assert_raises(ValueError):
        BE(NoMol(mf), fobj(), lib=lib, distribute=False, int_transform="cholesky-hip", integral_backend="hip")
