"""The two-particle half of the reference's `rdm1_fullbasis` (molbe/mbe.py:543-646) and the N^4 energy contraction of `compute_energy_full`
(mbe.py:781-789) on the device.  Everything here works on device buffers; BE.rdm12_fullbasis / BE.compute_energy_full (mbe.py of this package) drive it.

Per fragment (reference: einsum "ijkl,pi,qj,rk,sl" with mo_coeffs, then "xi,ijkl,px,qj,rk,sl" with P_c and TA):
    out[p,q,r,s] += sum A[p,a] B[q,b] B[r,c] B[s,d] rdm2[a,b,c,d],   B = TA mo_coeffs,   A = TA P_c mo_coeffs = U V,
    P_c = TA^T S W_c W_c^T S TA,   U = TA TA^T S W_c (N x n_c),   V = W_c^T S TA mo_coeffs (n_c x n).
P_c has rank n_c (the centre orbitals), so the first quarter transform runs with V: n_c n^3 elements survive it, and U comes last, straight into the
resident N^4 accumulator.  Each quarter transform is ONE product of the FP64 MFMA GEMM: the tensor is read as a (first index) x (the other three) matrix,
transposed by the operand loader, and the new index is appended at the end -- four cyclic rotations bring the indices back in order, no transposition pass.
The fragment tensor (qemb_frag_rdm2_dev), the subtraction of its non-connected part, the symmetrisation with nc_AO and the contraction with the packed
AO integrals are kernels of csrc/rdm2_ops.hip."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DeviceBuffer, check
from .fragsolver import RDM2_KINDS


def _gemm(lib, M, N, K, A, lda, a_kc, B, ldb, b_kc, Cp, ldc, beta=0.0):
    check(lib.qemb_op_gemm(M, N, K, 1.0, A, lda, int(a_kc), 0, B, ldb, int(b_kc), 0, float(beta), Cp, ldc, 0, 1), "qemb_op_gemm", lib)


def _quarter(lib, X, first, rest, mat, rows, out):
    """out[(rest), x] = sum_a X[a, (rest)] mat[x, a]: X is first x rest, mat rows x first (device pointers), out rest x rows"""
    _gemm(lib, rest, rows, first, X, rest, False, mat, first, True, out, rows)


def eri_form(eri_, nao):
    """which of PySCF's forms `mf._eri` has: 1 ([N]^4), 4 ([npair][npair]) or 8 (npair(npair))"""
    npair = nao * (nao + 1) // 2
    size = int(np.size(eri_))
    if size == nao ** 4:
        return 1
    if size == npair * npair:
        return 4
    if size == npair * (npair + 1) // 2:
        return 8
    raise ValueError(f"the AO integrals have {size} elements: not a form of (N N|N N) with N = {nao}")


def workspace_words(nao, frags, transform):
    """doubles the accumulation allocates beside the N^4 accumulator: the fragment tensor and the two buffers the quarter transforms alternate between (sized for
    the largest fragment), and the two N^4 buffers of an LO / MO re-expression"""
    w = 0
    for f in frags:
        n, nc = f.nao, len(f.weight_and_relAO_per_center[1])
        w = max(w, n ** 4 + 2 * nc * nao ** 3)
    return w + (2 * nao ** 4 if transform else 0)


def guard(lib, nao, frags, transform, eri_words, limit):
    need = 8 * (nao ** 4 + workspace_words(nao, frags, transform) + eri_words)
    check(lib.qemb_rdm2_full_guard(nao, need, -1 if limit is None else int(limit)), "qemb_rdm2_full_guard", lib)


def accumulate(lib, acc, nao, S, W, frags, subtract_nc):
    """adds the centre-projected 2-RDMs (with_dm1=False tensors of the fragments' last solve; minus the non-connected part of rdm1__ - 2 I_occ when
    subtract_nc, mbe.py:546-558) of `frags` into the device accumulator `acc` ([N]^4), in the order given"""
    N3 = nao ** 3
    for f in frags:
        if f.rdm1__ is None or f._solver is None:
            raise RuntimeError("rdm12_fullbasis: run oneshot() or optimize() first")
        n = f.nao
        cind = [f.AO_in_frag[i] for i in f.weight_and_relAO_per_center[1]]
        nc = len(cind)
        SW = S @ W[:, cind]
        Bm = f.TA @ f.mo_coeffs
        bufs = [DeviceBuffer.from_numpy(SW.T @ Bm, lib=lib), DeviceBuffer.from_numpy(Bm, lib=lib), DeviceBuffer.from_numpy(f.TA @ (f.TA.T @ SW), lib=lib),
                DeviceBuffer(n ** 4, lib=lib), DeviceBuffer(nc * N3, lib=lib), DeviceBuffer(nc * N3, lib=lib)]
        V, B, U, X, T1, T2 = bufs
        try:
            try:
                check(lib.qemb_frag_rdm2_dev(f.dev.h, RDM2_KINDS[f._solver], 0, X.ptr), "qemb_frag_rdm2_dev", lib)
            except _lib.QembError as e:
                if e.status == _lib.QEMB_ERR_UNSUPPORTED:
                    raise NotImplementedError(str(e)) from None
                raise
            if subtract_nc:
                d = np.array(f.rdm1__, dtype=np.float64)
                d[np.diag_indices(f.nsocc)] -= 2.0
                dd = DeviceBuffer.from_numpy(d, lib=lib)
                bufs.append(dd)
                check(lib.qemb_op_rdm2_add_nc(n, dd.ptr, -1.0, X.ptr), "qemb_op_rdm2_add_nc", lib)
            _quarter(lib, X.ptr, n, n ** 3, V.ptr, nc, T1.ptr)                    # (a,b,c,d) -> (b,c,d,x)
            _quarter(lib, T1.ptr, n, n * n * nc, B.ptr, nao, T2.ptr)              # -> (c,d,x,q)
            _quarter(lib, T2.ptr, n, n * nc * nao, B.ptr, nao, T1.ptr)            # -> (d,x,q,r)
            _quarter(lib, T1.ptr, n, nc * nao * nao, B.ptr, nao, T2.ptr)          # -> (x,q,r,s)
            _gemm(lib, nao, N3, nc, U.ptr, nc, True, T2.ptr, N3, False, acc.ptr, N3, beta=1.0)      # acc[p,(qrs)] += U[p,x] T2[x,(qrs)]
            check(lib.qemb_sync(), "qemb_sync", lib)
        finally:
            for b in bufs:
                b.free()


def symmetrize(lib, acc, nao, rdm1AO=None):
    """acc = (acc + acc^T) / 2 over all four indices, plus nc_AO of the full-basis 1-RDM when it is given (mbe.py:601-620)"""
    g = DeviceBuffer.from_numpy(rdm1AO, lib=lib) if rdm1AO is not None else None
    try:
        check(lib.qemb_op_rdm2_symmetrize(nao, g.ptr if g else None, acc.ptr), "qemb_op_rdm2_symmetrize", lib)
        check(lib.qemb_sync(), "qemb_sync", lib)
    finally:
        if g:
            g.free()


def reexpress(lib, acc, nao, MtS):
    """einsum("ijkl,pi,qj,rk,sl->pqrs", acc, MtS, MtS, MtS, MtS) (mbe.py:623-646; MtS = C^T S or W^T S, rows x N) -> host array"""
    m = MtS.shape[0]
    Md = DeviceBuffer.from_numpy(MtS, lib=lib)
    A, B = DeviceBuffer(max(m, nao) ** 4, lib=lib), DeviceBuffer(max(m, nao) ** 4, lib=lib)
    try:
        _quarter(lib, acc.ptr, nao, nao ** 3, Md.ptr, m, A.ptr)
        _quarter(lib, A.ptr, nao, nao * nao * m, Md.ptr, m, B.ptr)
        _quarter(lib, B.ptr, nao, nao * m * m, Md.ptr, m, A.ptr)
        _quarter(lib, A.ptr, nao, m ** 3, Md.ptr, m, B.ptr)
        return B.numpy((m, m, m, m))
    finally:
        for b in (Md, A, B):
            b.free()


class AOIntegrals:
    """`mf._eri` on the device in the form it has (never unpacked: the kernel reads it through the pair indices)"""

    def __init__(self, lib, eri_, nao):
        self.lib, self.nao, self.sym = lib, nao, eri_form(eri_, nao)
        self.buf = DeviceBuffer.from_numpy(np.asarray(eri_, dtype=np.float64).reshape(-1), lib=lib)

    @classmethod
    def from_mol(cls, lib, mol, nao):
        """the 8-fold packed integrals evaluated on the device from the geometry (qemb_int4c2e) and left there"""
        from .integrals import DeviceBasis
        self = cls.__new__(cls)
        npair = nao * (nao + 1) // 2
        self.lib, self.nao, self.sym = lib, nao, 8
        self.buf = DeviceBuffer(npair * (npair + 1) // 2, lib=lib)
        b = DeviceBasis(mol, lib)
        try:
            b.eri(8, out_dev=self.buf.ptr)
        except BaseException:
            self.buf.free()
            raise
        finally:
            b.free()
        return self

    def dot(self, K):
        """sum eri[pqrs] K[pqrs] with K an [N]^4 device buffer (two-stage reduction in a fixed order)"""
        e = C.c_double()
        check(self.lib.qemb_op_rdm2_eri_dot(self.nao, self.sym, self.buf.ptr, K.ptr, C.byref(e)), "qemb_op_rdm2_eri_dot", self.lib)
        return e.value

    def free(self):
        self.buf.free()
