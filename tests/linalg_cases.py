"""Shared cases and checks of the dense linear algebra tests (csrc/linalg_f64.hip: Jacobi eigh / SVD, blocked Cholesky, triangular inverse) on the spectra the
solves really see: projector, graded, exactly degenerate, nearly diagonal, rank deficient, ill conditioned.  test_gpu_linalg.py runs them on the device,
test_linalg_hostlogic.py on NumPy (the bars are meetable, the builders are right) and on the hostcheck mock.

Every check takes a SOLVER (LibSolver for the device library and for the mock, NumpySolver for LAPACK), returns the measured value / bar ratios and asserts each
ratio < 1.  The bars ("Dense linear algebra: what is pinned"):

  eigh      |w - eigvalsh(A)| < 1e-12 S, |V^T V - I| < 1e-12, |A V - V w| < 1e-11 S, w non-decreasing, finite, 0 <= sweeps <= 40;
            S = the largest absolute row sum of A: the scale of the kernels themselves (thr = tol x S, sigma = 1.0625 x Gershgorin; the one-sided path solves
            A + sigma I, so its absolute error is proportional to eps x sigma by construction)
  SVD       |s - s_ref| < 1e-12 s_max, |U diag(s) V^T - G| < 1e-12 s_max, |V^T V - I| < 1e-12, U[:, :r] orthonormal to 1e-12 (r = #(s_ref > 1e-10 s_max)),
            s non-increasing and >= 0, finite, a column of U whose singular value is below the zero-vector floor (1e-15 ||G||_F) exactly zero
  Cholesky  |A - L L^T|_ij <= 8 gamma_{n+1} (|L| |L^T|)_ij elementwise (Higham's bound for any order of summation, gamma_k = k u / (1 - k u), u = 2^-53; the factor 8
            is for the panel step, which multiplies by the explicit inverse of the 32 x 32 diagonal block), upper triangle exactly zero
  inverse   |Linv L - I|_ij <= 8 gamma_n (|Linv| |L|)_ij and |L Linv - I|_ij <= 8 gamma_n (|L| |Linv|)_ij on the lower triangle, strict upper triangle exactly zero
"""
import ctypes as C
import functools
import os
import sys

import numpy as np

QEMB_ERR_NOCONV, QEMB_ERR_NUMERIC = -4, -5
U_ROUND = 2.0 ** -53


def gamma(k):
    return k * U_ROUND / (1.0 - k * U_ROUND)


# ------------------------------------------------------------------------------------------------ solvers
class LibSolver:
    """The C ABI of libqemb_hip.so or of the hostcheck mock."""
    name = "lib"

    def __init__(self, lib):
        from quemb_amd._lib import DeviceBuffer
        self.lib, self.DB = lib, DeviceBuffer

    def _buf(self, a):
        return self.DB.from_numpy(np.ascontiguousarray(a, dtype=np.float64), lib=self.lib)

    def last_error(self):
        return self.lib.qemb_last_error().decode(errors="replace")

    def eigh(self, A):
        n = A.shape[0]
        dA, dw, dV = self._buf(A), self.DB(n, lib=self.lib), self.DB(n * n, lib=self.lib)
        sw = C.c_int(-7)
        rc = self.lib.qemb_op_jacobi_eigh(n, dA.ptr, dw.ptr, dV.ptr, C.byref(sw))
        out = (rc, dw.numpy((n,)), dV.numpy((n, n)), sw.value)
        for b in (dA, dw, dV):
            b.free()
        return out

    def eigh_in_basis(self, F, Cp, nocc, stop_below):
        """(rc, w, C, C2, dm, sweeps); with a basis C2 is written over Cp, as the SCF cycle does"""
        n = F.shape[0]
        dF, dw, dC, dD = self._buf(F), self.DB(n, lib=self.lib), self.DB(n * n, lib=self.lib), self.DB(n * n, lib=self.lib)
        d2 = self._buf(Cp) if Cp is not None else self.DB(n * n, lib=self.lib)
        sw = C.c_int(-7)
        rc = self.lib.qemb_op_jacobi_eigh_in_basis(n, dF.ptr, d2.ptr if Cp is not None else None, dw.ptr, dC.ptr, d2.ptr, nocc, dD.ptr, stop_below, C.byref(sw))
        out = (rc, dw.numpy((n,)), dC.numpy((n, n)), d2.numpy((n, n)), dD.numpy((n, n)), sw.value)
        for b in (dF, dw, dC, dD, d2):
            b.free()
        return out

    def svd(self, G):
        m, n = G.shape
        dG, ds, dU, dV = self._buf(G), self.DB(n, lib=self.lib), self.DB(m * n, lib=self.lib), self.DB(n * n, lib=self.lib)
        sw = C.c_int(-7)
        rc = self.lib.qemb_op_jacobi_svd(m, n, dG.ptr, ds.ptr, dU.ptr, dV.ptr, C.byref(sw))
        out = (rc, ds.numpy((n,)), dU.numpy((m, n)), dV.numpy((n, n)), sw.value)
        for b in (dG, ds, dU, dV):
            b.free()
        return out

    def cholesky(self, A):
        n = A.shape[0]
        dA = self._buf(A)
        rc = self.lib.qemb_op_cholesky_lower(n, dA.ptr)
        L = dA.numpy((n, n))
        dA.free()
        return rc, L

    def tri_inverse(self, L):
        n = L.shape[0]
        dL, dX = self._buf(L), self.DB(n * n, lib=self.lib)
        rc = self.lib.qemb_op_tri_inverse_lower(n, dL.ptr, dX.ptr)
        X = dX.numpy((n, n))
        dL.free(); dX.free()
        return rc, X


class NumpySolver:
    """LAPACK behind the same interface: the rehearsal that shows every bar can be met and every builder builds what it says."""
    name = "numpy"

    def __init__(self):
        self._err = ""

    def last_error(self):
        return self._err

    def _refuse(self, who, *arrays):
        if all(np.isfinite(a).all() for a in arrays if a is not None):
            return False
        self._err = f"{who}: non-finite input"
        return True

    def eigh(self, A):
        n = A.shape[0]
        if self._refuse("jacobi_eigh", A):
            return QEMB_ERR_NUMERIC, np.zeros(n), np.zeros((n, n)), -2
        w, V = np.linalg.eigh(A)
        return 0, w, V, 0

    def eigh_in_basis(self, F, Cp, nocc, stop_below):
        n = F.shape[0]
        if self._refuse("jacobi_eigh_in_basis", F, Cp):
            z = np.zeros((n, n))
            return QEMB_ERR_NUMERIC, np.zeros(n), z, z, z, -2
        A = F if Cp is None else Cp.T @ F @ Cp
        w, V = np.linalg.eigh(0.5 * (A + A.T))
        Cm = V if Cp is None else Cp @ V
        return 0, w, Cm, Cm.copy(), 2.0 * Cm[:, :nocc] @ Cm[:, :nocc].T, 0

    def svd(self, G):
        m, n = G.shape
        if self._refuse("jacobi_svd", G):
            return QEMB_ERR_NUMERIC, np.zeros(n), np.zeros((m, n)), np.zeros((n, n)), -2
        U, s, Vt = np.linalg.svd(G, full_matrices=False)
        U = U * (s > svd_floor(G))                   # (the product's convention: no left vector for a numerically zero singular value)
        return 0, s, U, Vt.T.copy(), 0

    def cholesky(self, A):
        if self._refuse("cholesky_lower", A):
            return QEMB_ERR_NUMERIC, A
        try:
            return 0, np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            self._err = "cholesky_lower: matrix is not positive definite"
            return QEMB_ERR_NUMERIC, A

    def tri_inverse(self, L):
        # forward substitution in extended precision, rounded once: |X - L^-1| <= u |L^-1| nearly, which is what BOTH residual bounds ask for (a substitution in
        # working precision guarantees only the residual of the system it solves, L X = I, and misses the other on an ill-conditioned metric)
        n = L.shape[0]
        Lx = L.astype(np.longdouble)
        X = np.zeros((n, n), dtype=np.longdouble)
        for i in range(n):
            X[i, :i] = -(Lx[i, :i] @ X[:i, :i]) / Lx[i, i]
            X[i, i] = 1.0 / Lx[i, i]
        return 0, X.astype(np.float64)


# ------------------------------------------------------------------------------------------------ eigen families
EIGH_FAMILIES = ("zero", "scalar", "diagonal", "clusters", "projector", "graded", "negdef", "pairs", "kron", "fock")
# n -> dispatch path of dev_jacobi_eigh (linalg_f64.hip)
EIGH_SIZES = {1: "one-barrier", 2: "one-barrier", 3: "one-barrier", 79: "one-barrier", 80: "one-barrier",      # odd bye; the MAXI = 4 items per thread limit
              81: "block<16,4>", 96: "block<16,4>",                                                           # last block of one row; full blocks
              97: "block<16,4>",                                                                              # odd number of blocks: the phantom block
              129: "block<16,7>", 224: "block<16,7>",
              225: "block<16,10>", 300: "block<16,10>",                                                       # 300: ldr = 600, the limit
              301: "per-pair"}                                                                                # odd n
EIGH_SCALED_SIZES = (80, 96, 224, 300, 301)              # one size per path for the 2^+-40 scalings
IN_BASIS_SIZES = (1, 2, 3, 79, 80)
PROJECTOR_NF = 6


def _sym(a):
    return 0.5 * (a + a.T)


def _orth(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def _seed(*key):
    fams = EIGH_FAMILIES + SVD_FAMILIES
    return [fams.index(k) + 1 if isinstance(k, str) else int(k) for k in key]


def _from_spectrum(rng, w):
    Q = _orth(rng, len(w))
    return _sym((Q * w) @ Q.T)


@functools.lru_cache(None)
def eigh_matrix(family, n, scale_exp=0):
    """The matrix of a family at size n, times 2^scale_exp (exact), read-only; its reference comes from eigh_reference."""
    rng = np.random.default_rng(_seed(family, n))
    if family == "zero":
        A = np.zeros((n, n))
    elif family == "scalar":
        A = -0.75 * np.eye(n)
    elif family == "diagonal":                            # unsorted, repeated entries
        A = np.diag(rng.choice(np.array([-2.0, -0.5, 0.0, 0.25, 0.25, 1.5, 3.0]), size=n))
    elif family == "clusters":                            # three values of width 1e-13, a quarter of the entries spread by 1e-9
        w = rng.choice(np.array([-1.0, 0.3, 2.0]), size=n) + 1e-13 * rng.standard_normal(n)
        wide = rng.random(n) < 0.25
        w[wide] += 1e-9 * rng.standard_normal(int(wide.sum()))
        A = _from_spectrum(rng, w)
    elif family == "projector":                           # environment block of an idempotent density: 0 / 1 and up to six in between
        nf = min(PROJECTOR_NF, n // 3)
        N = n + nf
        nocc = max(nf, N // 3)
        Cm = np.linalg.qr(rng.standard_normal((N, max(nocc, 1))))[0][:, :nocc]
        A = _sym((Cm @ Cm.T)[nf:, nf:])
    elif family == "graded":                              # +-logspace(0, -14)
        npos = (n + 1) // 2
        w = np.concatenate([np.logspace(0, -14, npos), -np.logspace(0, -14, n - npos)]) if n > 1 else np.array([1.0])
        A = _from_spectrum(rng, w)
    elif family == "negdef":
        A = _from_spectrum(rng, -np.logspace(0, -6, n))
    elif family == "pairs":                               # [[0, B], [B^T, 0]]: eigenvalues in +- pairs
        p = n // 2
        A = np.zeros((n, n))
        A[:p, p:] = rng.standard_normal((p, n - p))
        A = A + A.T
    elif family == "kron":                                # S (x) I_2 cut to n: exact double degeneracy, rotations with d = 0
        k = (n + 1) // 2
        A = np.kron(_sym(rng.standard_normal((k, k))), np.eye(2))[:n, :n].copy()
    elif family == "fock":                                # a nearly converged Fock matrix in its own orbitals
        A = np.diag(3.0 * np.arange(n)) + 1e-6 * _sym(rng.standard_normal((n, n)))
    else:
        raise KeyError(family)
    A = np.ascontiguousarray(A * 2.0 ** scale_exp)
    assert np.array_equal(A, A.T)
    A.setflags(write=False)
    return A


@functools.lru_cache(None)
def eigh_reference(family, n, scale_exp=0):
    w, V = np.linalg.eigh(eigh_matrix(family, n, scale_exp))
    w.setflags(write=False); V.setflags(write=False)
    return w, V


def row_scale(A):
    return float(np.abs(A).sum(axis=1).max()) if A.size else 0.0


def _ratio(err, bar):
    """measured / bar; a zero bar (the zero matrix) admits a zero error only"""
    err = float(err)
    if not np.isfinite(err):
        return np.inf
    if bar == 0.0:
        return 0.0 if err == 0.0 else np.inf
    return err / bar


def _assert_ratios(ratios, label):
    bad = {k: v for k, v in ratios.items() if not v < 1.0}
    assert not bad, f"{label}: measured / bar = {bad} (all: {ratios})"


def eigh_ratios(A, w, V, w_ref):
    n = A.shape[0]
    S = row_scale(A)
    if not (np.isfinite(w).all() and np.isfinite(V).all()):
        return {"finite": np.inf}
    return {"w": _ratio(np.abs(w - w_ref).max(), 1e-12 * S),
            "orth": _ratio(np.abs(V.T @ V - np.eye(n)).max(), 1e-12),
            "resid": _ratio(np.abs(A @ V - V * w).max(), 1e-11 * S)}


def check_eigh(solver, family, n, scale_exp=0):
    A = eigh_matrix(family, n, scale_exp)
    w_ref, V_ref = eigh_reference(family, n, scale_exp)
    label = f"eigh {family} n={n} 2^{scale_exp} [{solver.name}]"
    rc, w, V, sweeps = solver.eigh(A.copy())
    assert rc == 0, f"{label}: status {rc}: {solver.last_error()}"
    ratios = eigh_ratios(A, w, V, w_ref)
    ratios["sweeps"] = sweeps
    print(f"{label}: {ratios}")
    sweeps = ratios.pop("sweeps")
    _assert_ratios(ratios, label)
    assert np.all(np.diff(w) >= 0.0), f"{label}: eigenvalues not sorted"
    assert 0 <= sweeps <= 40, f"{label}: {sweeps} sweeps"
    if family == "diagonal":                              # nothing to rotate: V is a signed permutation, exactly
        assert np.array_equal(np.abs(V) @ np.ones(n), np.ones(n)) and np.array_equal(np.ones(n) @ np.abs(V), np.ones(n)) and set(np.unique(np.abs(V))) <= {0.0, 1.0}, label
    if family == "projector":                             # the Schmidt use: the subspace of the eigenvalues strictly between 0 and 1
        unit = 2.0 ** scale_exp
        sel = (w > 1e-10 * unit) & (w < (1 - 1e-10) * unit)
        selr = (w_ref > 1e-10 * unit) & (w_ref < (1 - 1e-10) * unit)
        assert sel.sum() == selr.sum() == min(PROJECTOR_NF, n // 3), (label, int(sel.sum()), int(selr.sum()))
        Pg, Pr = V[:, sel] @ V[:, sel].T, V_ref[:, selr] @ V_ref[:, selr].T
        ratios["projector"] = _ratio(np.abs(Pg - Pr).max(), 1e-11)
        _assert_ratios(ratios, label)
    ratios["sweeps"] = sweeps
    return ratios


IN_BASIS_STOP = 1e-10


def check_eigh_in_basis(solver, family, n):
    """The fused SCF eigensolve on the same families: with a random orthogonal basis and with none, nocc in {0, n // 3, n}."""
    F = eigh_matrix(family, n)
    w_ref, _ = eigh_reference(family, n)
    S = row_scale(F)
    rng = np.random.default_rng(_seed(family, n, 77))
    worst = {}
    for Cp in (_orth(rng, n), None):
        for nocc in sorted({0, n // 3, n}):
            label = f"eigh_in_basis {family} n={n} basis={Cp is not None} nocc={nocc} [{solver.name}]"
            rc, w, Cm, C2, dm, sweeps = solver.eigh_in_basis(F.copy(), None if Cp is None else Cp.copy(), nocc, IN_BASIS_STOP)
            assert rc == 0, f"{label}: status {rc}: {solver.last_error()}"
            assert all(np.isfinite(x).all() for x in (w, Cm, C2, dm)), label
            ratios = {"w": _ratio(np.abs(w - w_ref).max(), 1e-12 * S),
                      "orth": _ratio(np.abs(Cm.T @ Cm - np.eye(n)).max(), 1e-12),
                      "resid": _ratio(np.abs(F @ Cm - Cm * w).max(), 1e-11 * S)}
            if nocc == 0:
                assert not dm.any(), label
            elif nocc == n:
                ratios["dm"] = _ratio(np.abs(dm - 2.0 * np.eye(n)).max(), 1e-13)
            else:
                ratios["dm"] = _ratio(np.abs(dm - 2.0 * Cm[:, :nocc] @ Cm[:, :nocc].T).max(), 1e-13)
            print(f"{label}: {ratios} sweeps {sweeps}")
            _assert_ratios(ratios, label)
            assert np.array_equal(C2, Cm), label
            assert np.all(np.diff(w) >= 0.0) and 0 <= sweeps <= 40, (label, sweeps)
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
            worst["sweeps"] = max(worst.get("sweeps", 0), sweeps)
    return worst


# ------------------------------------------------------------------------------------------------ SVD families
SVD_FAMILIES = ("gaussian", "lowrank", "zerocols", "zeromat", "orthonormal", "clustered", "gradedsv", "schmidt")
# (m, n) -> dispatch path of jacobi_rows (nvec = n rows of length m)
SVD_SHAPES = {(5, 1): "LDS", (7, 7): "LDS", (96, 64): "LDS",                       # (5, 1): nvec < 2, nothing to rotate
              (150, 40): "block<16,4>", (100, 70): "block<16,4>",
              (300, 40): "block<16,7>",
              (500, 64): "block<16,10>", (520, 80): "block<16,10>",              # (520, 80): m + n = 600, the limit
              (561, 40): "per-pair",                                              # one past the limit
              (2000, 40): "per-pair"}


def svd_floor(G):
    """singular values at or below this are numerically zero for dev_jacobi_svd (floor2 = 1e-30 ||G||_F^2 on the squared norms)"""
    return 1e-15 * float(np.sqrt((G * G).sum()))


@functools.lru_cache(None)
def svd_matrix(family, m, n):
    rng = np.random.default_rng(_seed(family, m, n))
    ortho_cols = lambda r, c: np.linalg.qr(rng.standard_normal((r, c)))[0]
    if family == "gaussian":
        G = rng.standard_normal((m, n))
    elif family == "lowrank":                             # rank 3 of n
        r = min(3, n)
        G = rng.standard_normal((m, r)) @ rng.standard_normal((r, n))
    elif family == "zerocols":                            # two exactly zero columns
        G = rng.standard_normal((m, n))
        G[:, [0, n // 2]] = 0.0
    elif family == "zeromat":
        G = np.zeros((m, n))
    elif family == "orthonormal":
        G = ortho_cols(m, n)
    elif family == "clustered":                           # sigma = 1 + 1e-9 xi
        G = (ortho_cols(m, n) * (1.0 + 1e-9 * rng.standard_normal(n))) @ _orth(rng, n).T
    elif family == "gradedsv":                            # sigma = logspace(0, -12)
        G = (ortho_cols(m, n) * np.logspace(0, -12, n)) @ _orth(rng, n).T
    elif family == "schmidt":                             # the environment-fragment block of an idempotent density, C_env C_f^T
        N = m + n
        Co = ortho_cols(N, max(1, N // 3))
        G = Co[n:] @ Co[:n].T
    else:
        raise KeyError(family)
    G = np.ascontiguousarray(G)
    G.setflags(write=False)
    return G


@functools.lru_cache(None)
def svd_reference(family, m, n):
    s = np.linalg.svd(svd_matrix(family, m, n), compute_uv=False)
    s.setflags(write=False)
    return s


def check_svd(solver, family, m, n):
    G = svd_matrix(family, m, n)
    s_ref = svd_reference(family, m, n)
    label = f"svd {family} {m}x{n} [{solver.name}]"
    rc, s, U, V, sweeps = solver.svd(G.copy())
    assert rc == 0, f"{label}: status {rc}: {solver.last_error()}"
    assert all(np.isfinite(x).all() for x in (s, U, V)), label
    smax = float(s_ref.max())
    r = int((s_ref > 1e-10 * smax).sum())
    ratios = {"s": _ratio(np.abs(s - s_ref).max(), 1e-12 * smax),
              "recon": _ratio(np.abs((U * s) @ V.T - G).max(), 1e-12 * smax),
              "orthV": _ratio(np.abs(V.T @ V - np.eye(n)).max(), 1e-12),
              "orthU": _ratio(np.abs(U[:, :r].T @ U[:, :r] - np.eye(r)).max(), 1e-12) if r else 0.0}
    print(f"{label}: {ratios} sweeps {sweeps}")
    _assert_ratios(ratios, label)
    assert np.all(np.diff(s) <= 0.0) and np.all(s >= 0.0), label
    floor = svd_floor(G)
    dead = s <= floor * (1.0 - 1e-6)                      # (safely below the floor: the device sums the squares in another order)
    assert not U[:, dead].any(), f"{label}: a left vector of a zero singular value is not zero"
    if family in ("zerocols", "zeromat"):
        assert dead.sum() >= (n if family == "zeromat" else min(2, n)), label
    assert 0 <= sweeps <= 40, (label, sweeps)
    ratios["sweeps"] = sweeps
    return ratios


# ------------------------------------------------------------------------------------------------ Cholesky / triangular inverse
CHOL_SIZES = (1, 31, 32, 33, 64, 65, 129, 300)           # the edges of the 32-blocks
CHOL_DECADES = (0, 4, 8, 12)


@functools.lru_cache(None)
def spd_matrix(n, decades):
    """Q diag(logspace(0, -decades)) Q^T, symmetrised"""
    rng = np.random.default_rng([n, decades, 5])
    A = _from_spectrum(rng, np.logspace(0, -decades, n))
    A.setflags(write=False)
    return A


@functools.lru_cache(None)
def octane_metric():
    """(P|Q) of the even-tempered auxiliary set of the first twelve atoms of octane / STO-3G (int3c_cases.octane12): a metric from the project's own integral source"""
    import int3c_cases
    from quemb_amd import integrals as I
    A = np.ascontiguousarray(I.int2c2e(int3c_cases.octane12()[1]))
    A = _sym(A)
    A.setflags(write=False)
    return A


def _elem_ratio(err, bound, mask=None):
    """the largest err_ij / bound_ij; where the bound is zero only a zero error passes"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    r = np.where(np.isfinite(err), r, np.inf)
    return float(r.max() if mask is None else r[mask].max())


def cholesky_ratios(A, L):
    n = A.shape[0]
    bound = 8.0 * gamma(n + 1) * (np.abs(L) @ np.abs(L).T)
    return {"backward": _elem_ratio(np.abs(A - L @ L.T), bound)}


def check_cholesky(solver, A, label):
    n = A.shape[0]
    label = f"cholesky {label} n={n} [{solver.name}]"
    rc, L = solver.cholesky(A.copy())
    assert rc == 0, f"{label}: status {rc}: {solver.last_error()}"
    assert np.isfinite(L).all() and np.all(np.diag(L) > 0.0), label
    assert not np.triu(L, 1).any(), f"{label}: upper triangle not zero"
    ratios = cholesky_ratios(A, L)
    print(f"{label}: {ratios}")
    _assert_ratios(ratios, label)
    return ratios


def check_tri_inverse(solver, A, label):
    """the inverse of LAPACK's factor of A (the input does not depend on the Cholesky under test)"""
    n = A.shape[0]
    label = f"tri_inverse {label} n={n} [{solver.name}]"
    L = np.linalg.cholesky(A)
    rc, X = solver.tri_inverse(L.copy())
    assert rc == 0, f"{label}: status {rc}: {solver.last_error()}"
    assert np.isfinite(X).all(), label
    assert not np.triu(X, 1).any(), f"{label}: strict upper triangle not zero"
    low = np.tril(np.ones((n, n), dtype=bool))
    I = np.eye(n)
    ratios = {"left": _elem_ratio(np.abs(X @ L - I), 8.0 * gamma(n) * (np.abs(X) @ np.abs(L)), low),
              "right": _elem_ratio(np.abs(L @ X - I), 8.0 * gamma(n) * (np.abs(L) @ np.abs(X)), low)}
    print(f"{label}: {ratios}")
    _assert_ratios(ratios, label)
    return ratios


@functools.lru_cache(None)
def indefinite_matrix(n, k):
    """L diag(1, ..., -delta at k, ..., 1) L^T of a positive definite L L^T: the leading k x k block is positive definite, the pivot at row k is negative (exact
    arithmetic breaks down THERE), and delta is set so that the one negative eigenvalue is -1e-3 ||A||_2."""
    rng = np.random.default_rng([n, k, 9])
    X = rng.standard_normal((n, n))
    L = np.linalg.cholesky(X @ X.T / n + np.eye(n))
    make = lambda delta: _sym((L * np.where(np.arange(n) == k, -delta, 1.0)) @ L.T)
    f = lambda delta: (lambda w: w[0] + 1e-3 * np.abs(w).max())(np.linalg.eigvalsh(make(delta)))      # decreasing in delta
    lo, hi = 0.0, 1.0
    while f(hi) > 0.0:
        hi *= 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0.0 else (lo, mid)
    A = make(hi)
    w = np.linalg.eigvalsh(A)
    assert w[0] < 0.0 < w[1] and abs(w[0] / np.abs(w).max() + 1e-3) < 1e-6
    assert np.linalg.eigvalsh(A[:k, :k])[0] > 1e-3 * np.abs(w).max()
    A.setflags(write=False)
    return A


def refusal_cases():
    """(label, matrix) that dev_cholesky_lower must refuse with QEMB_ERR_NUMERIC"""
    inf_first = np.array(spd_matrix(33, 0)); inf_first[5, 5] = np.inf
    inf_later = np.array(spd_matrix(70, 4)); inf_later[40, 40] = np.inf
    return [("n=70, negative pivot in the second 32-block", indefinite_matrix(70, 45)),
            ("n=33, negative pivot in row 32", indefinite_matrix(33, 32)),
            ("+Inf on the diagonal, first block", inf_first),
            ("+Inf on the diagonal, second block", inf_later)]


def check_cholesky_refuses(solver, A, label):
    rc, _ = solver.cholesky(np.array(A))
    assert rc == QEMB_ERR_NUMERIC, f"cholesky {label} [{solver.name}]: status {rc}"
    assert "cholesky" in solver.last_error().lower(), solver.last_error()


# ------------------------------------------------------------------------------------------------ non-finite input
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)
NONFINITE_PLACES = ("diagonal", "offdiagonal", "lastrow")
NONFINITE_EIGH_SIZES = (40, 90, 310)                     # one-launch kernel, block rounds, per-pair rounds
NONFINITE_SVD_SHAPES = ((96, 64), (300, 40), (300, 22))  # LDS kernel, block rounds, per-pair rounds
NONFINITE_CHOL_SIZES = (20, 70)


def plant(M, value, place, symmetric):
    """a copy of M with `value` on the diagonal, off it, or in the last row (mirrored for a symmetric matrix)"""
    M = np.array(M)
    m, n = M.shape
    i, j = {"diagonal": (n // 2, n // 2), "offdiagonal": (min(1, m - 1), n - 1), "lastrow": (m - 1, n // 3)}[place]
    M[i, j] = value
    if symmetric:
        M[j, i] = value
    return M


def check_nonfinite(solver, op, size, value, place):
    """a NaN or an infinity in the input is QEMB_ERR_NUMERIC with the routine named, found before any sweep -- never QEMB_OK, never 40 sweeps"""
    rng = np.random.default_rng(3)
    label = f"{op} {size} {value} {place} [{solver.name}]"
    sweeps = None
    if op == "eigh":
        rc, _, _, sweeps = solver.eigh(plant(_sym(rng.standard_normal((size, size))), value, place, True))
        who = "jacobi_eigh"
    elif op == "eigh_in_basis":
        F = plant(_sym(rng.standard_normal((size, size))), value, place, True)
        for Cp in (None, _orth(rng, size)):
            rc, _, _, _, _, sweeps = solver.eigh_in_basis(F, Cp, size // 3, IN_BASIS_STOP)
            assert rc == QEMB_ERR_NUMERIC and "jacobi_eigh_in_basis" in solver.last_error(), (label, rc, solver.last_error())
        who = "jacobi_eigh_in_basis"
    elif op == "svd":
        rc, _, _, _, sweeps = solver.svd(plant(rng.standard_normal(size), value, place, False))
        who = "jacobi_svd"
    elif op == "cholesky":
        rc, _ = solver.cholesky(plant(spd_matrix(size, 0), value, place, True))
        who = "cholesky"
    else:
        raise KeyError(op)
    assert rc == QEMB_ERR_NUMERIC, f"{label}: status {rc} ({solver.last_error()})"
    assert who in solver.last_error().lower(), (label, solver.last_error())
    assert sweeps is None or sweeps < 1, f"{label}: {sweeps} sweeps spent on non-finite input"


# ------------------------------------------------------------------------------------------------ A/B paths, one fresh process per setting
AB_SETTINGS = ("QEMB_JACOBI_DB", "QEMB_JACOBI_TWOSIDED", "QEMB_JACOBI_BLOCK")       # each "=0" selects the older path; read once per process
AB_FAMILIES = ("clusters", "kron", "fock")
AB_SIZES = (57, 96, 131)


def run_ab_child():
    """The body of a child process of the A/B test (the environment already holds the setting): the three families at the three sizes through check_eigh."""
    from quemb_amd import _lib
    solver = LibSolver(_lib.init(int(os.environ.get("LOCAL_RANK", "0"))))
    for family in AB_FAMILIES:
        for n in AB_SIZES:
            check_eigh(solver, family, n)
    print("ab child ok:", {k: os.environ.get(k) for k in AB_SETTINGS})


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    run_ab_child()
