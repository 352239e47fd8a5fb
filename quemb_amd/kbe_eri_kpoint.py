"""k-point density-fitted fragment ERIs of the periodic driver on the device -- the route kbe/pbe.py:529-565 takes by default
(`int_transform="out-core-DF"`: libdmet's `get_emb_eri_fast_gdf(cell, mf.with_df, C_ao_eo=TA)` on the k-point GDF tensor).

The integral SOURCE is the k-point tensor itself: one complex block per k-point pair,

    L^{ki,kj}[P, mu, nu] = (P | mu_ki* nu_kj) = sum_{R,R'} exp(-i ki.T_R) exp(+i kj.T_R') b[P; (R,mu), (R',nu)]      (naux, nao, nao) complex128

(PySCF's `with_df.sr_loop((ki, kj))` with un-normalised Bloch sums; b = the rows of the supercell's translationally invariant factor that
belong to the auxiliary functions of cell 0, cells in `kbe_pfrag.get_phase` order).  With C^k = TA_k and q = kj - ki

    M^q[P, pq] = sum_ki (C^ki)^H L^{ki,ki+q}[P] C^{ki+q},        (pq|rs) = N_k^-3 sum_q sum_P Re( M^q[P,pq] conj(M^q[P,rs]) )

so a fragment owns a REAL 3-index factor with N_k naux rows, built by `qemb_kdf_transform` from the resident blocks:
two FP64 MFMA products per pair and three HBM passes.  16 N_k^2 naux nao^2 bytes are resident where `"supercell-DF-hip"` holds
8 N_k^3 naux nao^2, and nothing of size N_k^3 exists anywhere.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import c_vp, check
from .kbe_pfrag import get_phase1


def momentum_classes(a_vec, kpts, tol=1e-8):
    """(qclass, qconj): qclass[ki, kj] = the index of the k-point kj - ki (modulo a reciprocal lattice vector), qconj[q] = the index of -k_q.
    Raises ValueError when the differences leave the mesh (a mesh that does not contain Gamma, or an incomplete one)."""
    kf = (np.asarray(kpts, dtype=np.float64) @ np.asarray(a_vec, dtype=np.float64).T) / (2.0 * np.pi)
    nk = kf.shape[0]

    def find(v, what):
        d = kf - v[None, :]
        d = np.abs(d - np.round(d)).max(axis=1)
        hit = np.flatnonzero(d < tol)
        if len(hit) != 1:
            raise ValueError(f"the k-point mesh does not close: {what} is {'not a k-point of the mesh' if len(hit) == 0 else 'met more than once'}")
        return int(hit[0])

    qclass = np.empty((nk, nk), dtype=np.int32)
    for i in range(nk):
        for j in range(nk):
            qclass[i, j] = find(kf[j] - kf[i], f"kj - ki for (ki, kj) = ({i}, {j})")
    qconj = np.array([find(-kf[q], f"-k for k-point {q}") for q in range(nk)], dtype=np.int32)
    return qclass, qconj


class KPointDFSource:
    """The k-point GDF tensor as the device route consumes it: kpts / kmesh / lattice, the pair blocks and the class tables of kj - ki.

    `set_pair(ki, kj, L)` takes one (naux, nao, nao) complex block; pairs whose class is the -q partner of a kept class (the class with the
    lower number of q and -q is kept) need not be given.  A PySCF adapter is `for ki, kj: set_pair(ki, kj, sum of with_df.sr_loop blocks)`."""

    def __init__(self, nao, naux, a_vec, kpts, kmesh):
        self.nao, self.naux = int(nao), int(naux)
        self.a_vec, self.kpts, self.kmesh = np.asarray(a_vec, dtype=np.float64), np.asarray(kpts, dtype=np.float64), [int(x) for x in kmesh]
        self.nk = self.kpts.shape[0]
        if int(np.prod(self.kmesh)) != self.nk:
            raise ValueError("kmesh and kpts disagree")
        self.qclass, self.qconj = momentum_classes(self.a_vec, self.kpts)
        self.blocks = {}

    def kept(self, q):
        return q <= int(self.qconj[q])

    def needed_pairs(self):
        return [(i, j) for i in range(self.nk) for j in range(self.nk) if self.kept(int(self.qclass[i, j]))]

    def set_pair(self, ki, kj, L):
        L = np.asarray(L)
        if L.shape != (self.naux, self.nao, self.nao):
            raise ValueError(f"pair block ({ki}, {kj}) must be ({self.naux}, {self.nao}, {self.nao}), got {L.shape}")
        self.blocks[(int(ki), int(kj))] = np.ascontiguousarray(L, dtype=np.complex128)

    @classmethod
    def from_supercell_factor(cls, B, nk, naux_cell, a_vec, kpts, kmesh, all_pairs=False):
        """The Fourier sum above of a translationally invariant supercell factor B (nk * naux_cell, nk * nao, nk * nao), auxiliary functions
        and orbitals ordered (cell, function) with the cells in `get_phase` order; only the rows of cell 0 are read.  all_pairs: also the
        blocks of the classes that are not kept."""
        B = np.asarray(B, dtype=np.float64)
        nao = B.shape[1] // nk
        if B.shape != (nk * naux_cell, nk * nao, nk * nao):
            raise ValueError(f"supercell factor of shape {B.shape} is not ({nk} x {naux_cell}, {nk} x nao, {nk} x nao)")
        src = cls(nao, naux_cell, a_vec, kpts, kmesh)
        b = B[:naux_cell].reshape(naux_cell, nk, nao, nk, nao)
        ph = get_phase1(a_vec, kpts, kmesh)                              # exp(-i k.T_R), (NR, nk)
        half = np.einsum("Ra,PRmSn->aPmSn", ph, b, optimize=True)       # the sum over R, for every ki
        for (i, j) in ([(i, j) for i in range(nk) for j in range(nk)] if all_pairs else src.needed_pairs()):
            src.set_pair(i, j, np.einsum("S,PmSn->Pmn", ph[:, j].conj(), half[i], optimize=True))
        return src


class KdfContext:
    """Handle on the device-resident k-point tensor (C ABI qemb_kdf_*)."""

    def __init__(self, source: KPointDFSource, lib=None):
        self.lib = lib or _lib.init()
        self.nk, self.naux, self.nao = source.nk, source.naux, source.nao
        qc = np.ascontiguousarray(source.qclass, dtype=np.int32)
        qj = np.ascontiguousarray(source.qconj, dtype=np.int32)
        h = c_vp()
        IP = C.POINTER(C.c_int)
        check(self.lib.qemb_kdf_create(self.nk, self.naux, self.nao, qc.ctypes.data_as(IP), qj.ctypes.data_as(IP), C.byref(h)), "qemb_kdf_create", self.lib)
        self.h = h
        try:
            for (i, j), L in source.blocks.items():
                check(self.lib.qemb_kdf_set_pair(self.h, i, j, L.ctypes.data), "qemb_kdf_set_pair", self.lib)
        except Exception:
            self.free()
            raise

    def transform(self, TA_k, frag=None, factor_only=True, want_host=False):
        """TA_k: (nk, nao, n) complex.  frag: a DeviceFragment (or None with want_host).  Returns the packed block when want_host."""
        TA_k = np.ascontiguousarray(TA_k, dtype=np.complex128)
        if TA_k.ndim != 3 or TA_k.shape[:2] != (self.nk, self.nao):
            raise ValueError(f"TA_k must be ({self.nk}, {self.nao}, n), got {TA_k.shape}")
        n = TA_k.shape[2]
        out = np.empty((n * (n + 1) // 2,) * 2) if want_host else None
        check(self.lib.qemb_kdf_transform(self.h, TA_k.ctypes.data, n, None if out is None else out.ctypes.data, None if frag is None else frag.h,
                                          1 if factor_only else 0), "qemb_kdf_transform", self.lib)
        return out

    def free(self):
        if getattr(self, "h", None):
            self.lib.qemb_kdf_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def integral_kpoint_DF(source: KPointDFSource, frags, lib=None, factor_only=True, want_host=False):
    """Fragment ERIs of a k-point sampled system from its k-point GDF tensor.  frags: fragments with `.TA` (nk, nao, n) complex and a device
    fragment `.dev`.  factor_only: every fragment lives on its N_k naux-row factor; else it keeps the 4-fold packed block (and the factor beside
    it while the factor route of the MO integrals pays).  Returns the packed blocks when want_host, else None."""
    ctx = KdfContext(source, lib=lib)
    out = []
    try:
        for f in frags:
            TA = np.asarray(f.TA)
            if TA.shape[:2] != (source.nk, source.nao):
                raise ValueError(f"integral_kpoint_DF: the fragment's TA is {TA.shape}, the source has nk = {source.nk}, nao = {source.nao}")
            out.append(ctx.transform(TA, frag=f.dev, factor_only=factor_only, want_host=want_host))
    finally:
        ctx.free()
    return out if want_host else None
