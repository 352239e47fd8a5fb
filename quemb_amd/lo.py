"""Orbital localisation on the device -- the mirror of `get_loc` (molbe/lo.py:268-323), which the reference sends through PySCF's localisers.

Foster-Boys and Pipek-Mezey are one problem: rotate m orbitals so that f = sum_k sum_i (Q^k_ii)^2 is maximal for a stack of K symmetric m x m matrices
(Boys: the K = 3 dipole matrices; PM: one population matrix per atom; ER on a 3-index factor: K = naux).  That is joint diagonalisation by plane rotations and runs as Jacobi sweeps in
libqemb_hip (`qemb_op_joint_diag`, csrc/loc_ops.hip; angle rule and variant limits: csrc/loc_core.h).  A sweep costs K m^3 operations.

Deviations from PySCF, all deliberate:
* the optimiser is the Jacobi sweep, not PySCF's second-order (CIAH) solver: both stop at a stationary point of the same functional, in general not at the same
  one when the functional has several maxima;
* `init_guess`: the start is `C` itself.  None and "atomic" are accepted and change nothing (PySCF projects onto atomic orbitals first); anything else raises;
* PM: `pop_method` defaults to "lowdin" (PySCF: "meta-lowdin", which needs reference atomic orbitals that do not exist here); "mulliken" is there too;
* ER is defined on FACTORISED integrals: (ii|ii) = sum_P (B^P_ii)^2 with B the 3-index factor of the columns from a dense DFContext (fitted or Cholesky), so it is
  the same problem with K = naux.  It is exact to the factor's own error (the fitting error of the auxiliary basis; `cd_tol` for a Cholesky factor), where PySCF
  uses the exact four-index integrals.  The factor is formed by the quarter transforms of the DF transform and stays on the device (`qemb_df_localize_er`).
"""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import DeviceBuffer, check

METHODS = ("boys", "PM", "ER", "cholesky")


def joint_diag(Q, stop_angle=1e-10, max_sweeps=200, lib=None):
    """Joint diagonalisation of the symmetric matrices Q[K][m][m] on the device.  -> (Q_rot, U, info): U orthogonal (from the identity), Q_rot[k] = U^T Q[k] U,
    info = dict(sweeps, f, converged, in_lds); f = sum_k sum_i Q_rot[k]_ii^2."""
    lib = lib or _lib.init()
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    if Q.ndim != 3 or Q.shape[1] != Q.shape[2]:
        raise ValueError("joint_diag: Q is a stack [K][m][m] of square matrices")
    K, m = Q.shape[0], Q.shape[1]
    nbytes, lds = C.c_int64(), C.c_int()
    check(lib.qemb_op_joint_diag_bytes(K, m, C.byref(nbytes), C.byref(lds)), "qemb_op_joint_diag_bytes", lib)
    dQ = DeviceBuffer.from_numpy(Q, lib=lib)
    dU = DeviceBuffer(m * m, lib=lib)
    try:
        sw, f, cv = C.c_int(), C.c_double(), C.c_int()
        check(lib.qemb_op_joint_diag(K, m, dQ.ptr, dU.ptr, float(stop_angle), int(max_sweeps), C.byref(sw), C.byref(f), C.byref(cv)), "qemb_op_joint_diag", lib)
        return dQ.numpy((K, m, m)), dU.numpy((m, m)), dict(sweeps=sw.value, f=f.value, converged=bool(cv.value), in_lds=bool(lds.value))
    finally:
        dQ.free()
        dU.free()


def cholesky_mos(C_):
    """PySCF's `cholesky_mos`: the pivoted Cholesky factor of the projector D = C C^T, its first m columns -- orbitals L with L L^T = C C^T, each with its weight
    near the pivot AO.  Pivots by the largest remaining diagonal, ties to the lowest index.  O(N m^2) on an N x N matrix once: host code."""
    C_ = np.asarray(C_, dtype=np.float64)
    N, m = C_.shape
    D = C_ @ C_.T
    d = np.diag(D).copy()
    L = np.zeros((N, m))
    for j in range(m):
        p = int(np.argmax(d))      # argmax returns the first of equal maxima: the lowest index
        if not d[p] > 0.0:
            raise np.linalg.LinAlgError(f"cholesky_mos: C C^T has rank {j} < {m}")
        L[:, j] = (D[:, p] - L[:, :j] @ L[p, :j]) / np.sqrt(d[p])
        d -= L[:, j] ** 2
        d[p] = 0.0
    return L


def population_stack(mol, C_, S, pop_method, cache=None):
    """Pipek-Mezey: one matrix per atom, Q^A = X^T P_A X with X = S^1/2 C (lowdin), or the symmetrised C^T S P_A C (mulliken).  sum_A Q^A = C^T S C."""
    ao_atom = np.asarray(mol.ao_atom)
    if pop_method == "lowdin":
        if cache is None or "S_half" not in cache:
            w, v = np.linalg.eigh(S)
            S_half = (v * np.sqrt(w)) @ v.T
            if cache is not None:
                cache["S_half"] = S_half
        else:
            S_half = cache["S_half"]
        X = S_half @ C_
        return np.array([X[ao_atom == A].T @ X[ao_atom == A] for A in range(mol.natm)])
    if pop_method == "mulliken":
        SC = S @ C_
        Q = np.array([C_[ao_atom == A].T @ SC[ao_atom == A] for A in range(mol.natm)])
        return 0.5 * (Q + Q.transpose(0, 2, 1))
    if pop_method == "meta-lowdin":
        raise NotImplementedError("pop_method='meta-lowdin' (PySCF's default) needs reference atomic orbitals (ANO / MINAO) that are not available here; "
                                  "use 'lowdin' (the default here) or 'mulliken'")
    raise ValueError(f"pop_method {pop_method!r}: 'lowdin', 'mulliken' ('meta-lowdin' is not available)")


def get_loc(mol, C_, method="ER", pop_method=None, init_guess="atomic", *, df=None, backend="hip", stop_angle=1e-10, max_sweeps=200, lib=None, stats=None, cache=None):
    """Localise the columns of `C_` (orthonormal under the overlap of `mol`) by `method`; returns C_loc = C_ U with U orthogonal (cholesky: L with L L^T = C C^T).  The U applied
    is the sweeps' U after one Newton-Schulz step (_finish): it differs from the U whose functional `stats` reports by the ~1e-13 the step removes.

    boys     Q = C^T r_x C, C^T r_y C, C^T r_z C.  The functional does not depend on the origin of r: a shift by c changes Q^d by -c_d C^T S C = -c_d 1, which
             moves every diagonal element of Q^d by the same amount and leaves the differences Q_pp - Q_qq and the off-diagonal elements -- all the angle rule
             reads -- as they are; equivalently, maximising sum_i <i|r|i>^2 is minimising the spread sum_i <i|r^2|i> - <i|r|i>^2, whose first term is invariant.
    PM       one matrix per atom (population_stack); pop_method None = "lowdin".
    ER       Q^P = the 3-index factor of the columns, formed on the device from `df`, a dense DFContext (fitted or Cholesky) of the molecule, and kept there;
             without `df` (or with a semi-sparse / periodic one) a ValueError.  Exact to the factor's own error (module text).
    cholesky cholesky_mos (host).
    Not converged in `max_sweeps`: a RuntimeWarning, and the result is returned -- any orthogonal rotation of the input is a valid answer for BE.
    `cache` (a dict the caller keeps, e.g. BE over its fragments' baths): what depends on the molecule alone -- the dipole integrals, the overlap and S^1/2 -- is
    put there on first use and read from there afterwards, so that a call per fragment costs the small products and the sweeps only.
    `stats` (a dict) receives sweeps, f_before, f_after, converged, K, m, in_lds.  backend: "hip" only (the sweeps have no host twin in the package)."""
    if backend != "hip":
        raise ValueError("get_loc: backend='hip' is the only one (the sweeps run on the device)")
    if not (init_guess is None or (isinstance(init_guess, str) and init_guess == "atomic")):
        raise NotImplementedError("get_loc: init_guess None or 'atomic' only; the start is C itself either way")
    if method not in METHODS:
        raise NotImplementedError(f"Localization scheme {method} not understood")      # molbe/lo.py:311
    if pop_method is not None and method != "PM":
        raise ValueError("pop_method goes with method='PM' only")
    C_ = np.ascontiguousarray(C_, dtype=np.float64)
    if method == "cholesky":
        return cholesky_mos(C_)
    if method == "ER":
        if df is None or getattr(df, "layout", None) != "dense" or getattr(df, "h", None) is None or df.nao != C_.shape[0]:
            raise ValueError("get_loc: method='ER' is defined on factorised integrals and needs `df`, a dense DFContext (fitted or Cholesky) of the molecule")
        lib = lib or df.lib
        m = C_.shape[1]
        U = np.empty((m, m))
        sw, f0, f1, cv = C.c_int(), C.c_double(), C.c_double(), C.c_int()
        check(lib.qemb_df_localize_er(df.h, C_.ctypes.data, m, float(stop_angle), int(max_sweeps), U.ctypes.data, C.byref(sw), C.byref(f0), C.byref(f1), C.byref(cv)),
              "qemb_df_localize_er", lib)
        nb, lds = C.c_int64(), C.c_int()
        check(lib.qemb_op_joint_diag_bytes(df.naux, m, C.byref(nb), C.byref(lds)), "qemb_op_joint_diag_bytes", lib)
        info = dict(sweeps=sw.value, f=f1.value, converged=bool(cv.value), in_lds=bool(lds.value))
        return _finish(C_, U, info, f0.value, df.naux, method, stop_angle, stats)
    from . import integrals
    cache = {} if cache is None else cache
    if method == "boys":
        if "dipole" not in cache:
            cache["dipole"] = integrals.dipole(mol, backend="hip", lib=lib)      # the device kernel (csrc/int1e_ops.hip)
        Q = np.array([C_.T @ x @ C_ for x in cache["dipole"]])
    else:
        if "S" not in cache:
            cache["S"] = np.asarray(mol.intor("int1e_ovlp"))
        Q = population_stack(mol, C_, cache["S"], pop_method or "lowdin", cache=cache)
    Q = 0.5 * (Q + Q.transpose(0, 2, 1))
    f0 = float(np.einsum("kii,kii->", Q, Q))
    _, U, info = joint_diag(Q, stop_angle=stop_angle, max_sweeps=max_sweeps, lib=lib)
    return _finish(C_, U, info, f0, Q.shape[0], method, stop_angle, stats)


def _finish(C_, U, info, f0, K, method, stop_angle, stats):
    if stats is not None:
        stats.update(sweeps=info["sweeps"], f_before=f0, f_after=info["f"], converged=info["converged"], K=K, m=C_.shape[1], in_lds=info["in_lds"])
    if not info["converged"]:
        warnings.warn(RuntimeWarning(f"get_loc({method}): largest rotation still above {stop_angle} after {info['sweeps']} sweeps; the orbitals returned "
                                     "are an orthogonal rotation of the input"), stacklevel=3)
    # U is a product of (sweeps x m) plane rotations per column and leaves orthogonality by about sqrt(that) roundings; the columns of C can be large (S^-1/2 of a
    # diffuse basis), so one Newton-Schulz step U (3 - U^T U) / 2 -- the nearest orthogonal matrix to second order -- is taken before C U is formed
    U = 0.5 * U @ (3.0 * np.eye(U.shape[0]) - U.T @ U)
    return C_ @ U
