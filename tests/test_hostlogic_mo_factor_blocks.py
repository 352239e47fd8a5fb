"""The gathers of the factor route that read the pair product S[P(p,q)][P(r,s)] = (pq|rs) directly (a pair-first image only of its vv|vv part), the 3/4-transformed
integrals restricted to their (occupied, virtual) pair rows, and the pair product itself -- each kernel against the chain it replaces, element by
element and to the bit (they only move numbers, or add two of them in the same order).  The check functions take the library: here the host-logic
mock, in tests/test_gpu_mo_factor_blocks.py the HIP library."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))

# (n, o, naux, nf): npair = 210 (one block of the pair product; v = 16 takes the untiled passes), npair = 2211 and 2145 (>= 2048: block columns and
# the mirror; v = 59: nm = 1711 is odd, so the minus operands carry a padding column; odd n at the slab edges)
SHAPES = ((20, 4, 30, 4), (66, 7, 70, 8), (65, 6, 64, 6))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


def pidx(i, j):
    i, j = np.maximum(i, j), np.minimum(i, j)
    return i * (i + 1) // 2 + j


def block_column_product(lib, dB, npair, naux):
    """bb^T bb the way df_pair_product has formed it so far: block columns at and below the diagonal, one product each.  Entries above a diagonal
    block are not written (zero here).  Returns (device buffer, number of block columns)."""
    from quemb_amd._lib import DeviceBuffer, check
    dS = DeviceBuffer.from_numpy(np.zeros(npair * npair), lib=lib)
    nblk = 8 if npair >= 2048 else 1
    w = ((npair + nblk - 1) // nblk + 127) // 128 * 128
    for c0 in range(0, npair, w):
        cw = min(w, npair - c0)
        check(lib.qemb_op_gemm(npair - c0, cw, naux, 1.0, dB.at(c0), npair, 0, 0, dB.at(c0), npair, 0, 0, 0.0, dS.at(c0 * npair + c0), npair, 0, 1), lib=lib)
    return dS, nblk


def check_pair_product(lib, n, naux):
    from quemb_amd._lib import DeviceBuffer, check
    npair = n * (n + 1) // 2
    rng = np.random.default_rng(1000 + n)
    Bp = rng.standard_normal((naux, npair))
    dB = DeviceBuffer.from_numpy(Bp, lib=lib)
    dS = DeviceBuffer(npair * npair, lib=lib)
    check(lib.qemb_op_df_pair_product(npair, naux, dB.ptr, dS.ptr), lib=lib)
    S = dS.numpy((npair, npair))
    dR, nblk = block_column_product(lib, dB, npair, naux)
    R = dR.numpy((npair, npair))
    assert np.array_equal(np.tril(S), np.tril(R))                 # the lower triangle: the block-column result, to the bit
    if nblk == 1:
        assert np.array_equal(S, R)                                # one block: the plain product, unchanged
    else:
        check(lib.qemb_op_mirror_lower(npair, dR.ptr, npair), lib=lib)
        assert np.array_equal(S, dR.numpy((npair, npair)))
    assert np.array_equal(S, S.T) or nblk == 1                    # mirrored: symmetric to the bit
    assert np.abs(S - Bp.T @ Bp).max() < 1e-12 * naux
    for b in (dB, dS, dR):
        b.free()


def check_blocks_from_pair_product(lib, n, o, naux):
    """every gather from S against the pair-first chain it replaces (unpack of S, then the gathers from Mp)"""
    from quemb_amd._lib import DeviceBuffer, QembError, check
    v, npair = n - o, n * (n + 1) // 2
    rng = np.random.default_rng(2000 + n)
    Bp = rng.standard_normal((naux, npair))
    dB = DeviceBuffer.from_numpy(Bp, lib=lib)
    dS, dM = DeviceBuffer(npair * npair, lib=lib), DeviceBuffer(npair * n * n, lib=lib)
    check(lib.qemb_op_df_pair_product(npair, naux, dB.ptr, dS.ptr), lib=lib)
    check(lib.qemb_op_unpack_tril_rows(npair, n, dS.ptr, dM.ptr), lib=lib)
    S = dS.numpy((npair, npair))
    blocks = {}
    for name, (p0, q0, r0, s0, sp, sq, sr, ss) in {"oooo": (0, 0, 0, 0, o, o, o, o), "ovoo": (0, o, 0, 0, o, v, o, o), "ovov": (0, o, 0, o, o, v, o, v),
                                                    "oovv": (0, 0, o, o, o, o, v, v), "ovvo": (0, o, o, 0, o, v, v, o), "ovvv": (0, o, o, o, o, v, v, v),
                                                    "odd": (1, 2, 3, 0, o - 1, v - 1, v - 2, o + 1)}.items():
        d0, d1 = DeviceBuffer(sp * sq * sr * ss, lib=lib), DeviceBuffer(sp * sq * sr * ss, lib=lib)
        check(lib.qemb_op_extract_pf(n, dM.ptr, p0, q0, r0, s0, sp, sq, sr, ss, d0.ptr), lib=lib)
        check(lib.qemb_op_extract_ps(n, dS.ptr, p0, q0, r0, s0, sp, sq, sr, ss, d1.ptr), lib=lib)
        blocks[name] = d1.numpy((sp, sq, sr, ss))
        assert np.array_equal(d0.numpy((sp, sq, sr, ss)), blocks[name]), name
        P, Q, R, T = np.ix_(p0 + np.arange(sp), q0 + np.arange(sq), r0 + np.arange(sr), s0 + np.arange(ss))
        assert np.array_equal(blocks[name], S[pidx(P, Q), pidx(R, T)]), name
        d0.free(); d1.free()
    # ovvv with its (a,c) pair left packed: rows of S; unpacked it is ovvv
    npv, nmv = v * (v + 1) // 2, v * (v - 1) // 2
    dO, dP0, dP1 = DeviceBuffer.from_numpy(blocks["ovvv"], lib=lib), DeviceBuffer(o * v * npv, lib=lib), DeviceBuffer(o * v * npv, lib=lib)
    check(lib.qemb_op_pack_tril_rows(o * v, v, dO.ptr, dP0.ptr), lib=lib)
    check(lib.qemb_op_extract_ps_packed(n, dS.ptr, 0, o, o, o, v, v, dP1.ptr), lib=lib)
    assert np.array_equal(dP0.numpy((o * v, npv)), dP1.numpy((o * v, npv)))
    ilv = np.tril_indices(v)
    assert np.array_equal(dP1.numpy((o, v, npv)), blocks["ovvv"][:, :, ilv[0], ilv[1]])
    # (+/-) ladder operands
    ldp, ldm = npv + (npv & 1), max(nmv + (nmv & 1), 2)
    bufs = [DeviceBuffer.from_numpy(np.full(sz, 7.0), lib=lib) for sz in (npv * ldp, max(nmv, 1) * ldm) * 2]     # (a padding column left unwritten shows)
    check(lib.qemb_op_ladder_pack_vvvv_pf(n, o, dM.ptr, bufs[0].ptr, ldp, bufs[1].ptr, ldm), lib=lib)
    # ... from the pair-first image of the vv|vv part of S alone, rows ldv >= v apart (the gaps are never read: they hold NaN here)
    ldv = (v + 15) // 16 * 16 if v >= 32 else v + 3
    dV = DeviceBuffer.from_numpy(np.full(npv * v * ldv, np.nan), lib=lib)
    check(lib.qemb_op_unpack_pair_block(n, o, dS.ptr, dV.ptr, ldv), lib=lib)
    Mv = dV.numpy((npv, v, ldv))
    A, Cc, Bb, Dd = np.ix_(np.arange(v), np.arange(v), np.arange(v), np.arange(v))
    full = S[pidx(o + A, o + Cc), pidx(o + Bb, o + Dd)]                                   # [a][c][b][d]
    assert np.array_equal(Mv[:, :, :v], full[np.tril_indices(v)]) and np.isnan(Mv[:, :, v:]).all()
    del full, Mv
    check(lib.qemb_op_ladder_pack_vvvv_pf_ld(v, 0, dV.ptr, ldv, bufs[2].ptr, ldp, bufs[3].ptr, ldm), lib=lib)
    dV.free()
    assert np.array_equal(bufs[0].numpy((npv, ldp)), bufs[2].numpy((npv, ldp)))
    assert np.array_equal(bufs[1].numpy((nmv, ldm)), bufs[3].numpy((nmv, ldm)))
    a, b = ilv
    x = S[pidx(o + a[:, None], o + a[None, :]), pidx(o + b[:, None], o + b[None, :])]     # (a c|b d) at [P(a,b)][P(c,d)]
    y = S[pidx(o + b[:, None], o + a[None, :]), pidx(o + a[:, None], o + b[None, :])]     # (b c|a d)
    Vp = bufs[2].numpy((npv, ldp))
    assert np.array_equal(Vp[:, :npv], x + y) and not Vp[:, npv:].any()
    # OVp / OVm straight from ovvv against the permuted copy + pack_pm_cols
    OVl = np.ascontiguousarray(blocks["ovvv"].transpose(0, 2, 3, 1))                       # [k,a,c,d] = ovvv[k,d,a,c]
    dL = DeviceBuffer.from_numpy(OVl, lib=lib)
    pm = [DeviceBuffer.from_numpy(np.full(sz, 7.0), lib=lib) for sz in (o * v * ldp, o * v * ldm) * 2]
    check(lib.qemb_op_pack_pm_cols(o * v, v, dL.ptr, pm[0].ptr, ldp, pm[1].ptr, ldm), lib=lib)
    if v >= 32:
        check(lib.qemb_op_pack_pm_ovvv(o, v, dO.ptr, pm[2].ptr, ldp, pm[3].ptr, ldm), lib=lib)
        assert np.array_equal(pm[0].numpy((o * v, ldp)), pm[2].numpy((o * v, ldp)))
        assert np.array_equal(pm[1].numpy((o * v, ldm)), pm[3].numpy((o * v, ldm)))
    else:
        with pytest.raises(QembError):                            # the tiled pass only: small fragments keep the copy (CcsdSolver::setup)
            check(lib.qemb_op_pack_pm_ovvv(o, v, dO.ptr, pm[2].ptr, ldp, pm[3].ptr, ldm), lib=lib)
    # the (j,b) pair columns of the packed factor as a dense operand
    dG = DeviceBuffer(naux * o * v, lib=lib)
    check(lib.qemb_op_gather_pair_cols(naux, n, dB.ptr, 0, o, o, v, dG.ptr), lib=lib)
    J, Bv = np.ix_(np.arange(o), o + np.arange(v))
    assert np.array_equal(dG.numpy((naux, o, v)), Bp[:, pidx(J, Bv)])
    for b in [dB, dS, dM, dO, dP0, dP1, dL, dG] + bufs + pm:
        b.free()


def check_three_quarter_rows(lib, n, o, nf):
    """A1 / A2 from a T that holds only its (j,b) pair rows against the gather from the whole T: every element, on a hand-built T"""
    from quemb_amd._lib import DeviceBuffer, check
    v, npair = n - o, n * (n + 1) // 2
    rng = np.random.default_rng(3000 + n)
    T = rng.standard_normal((npair, n, n))
    J, Bv = np.ix_(np.arange(o), o + np.arange(v))
    rows = pidx(J, Bv).reshape(-1)                                 # row j * v + b of the compact T is row P(j, o+b) of the whole
    dT = DeviceBuffer.from_numpy(T, lib=lib)
    for slab_rows in (n, nf):                                      # whole slabs, and the first nf rows of every slab (what the factor route forms)
        dC = DeviceBuffer.from_numpy(T[rows][:, :slab_rows, :], lib=lib)
        for x0, sx in ((o, v), (0, o)):                            # A1[a,j,b,P] = (P a|j b),  A2[i,j,b,P] = (P i|j b)
            d0, d1 = DeviceBuffer(sx * o * v * nf, lib=lib), DeviceBuffer(sx * o * v * nf, lib=lib)
            check(lib.qemb_op_extract_pf_t(n, dT.ptr, x0, 0, o, 0, sx, o, v, nf, d0.ptr), lib=lib)
            check(lib.qemb_op_extract_pf_t_compact(n, dC.ptr, x0, 0, sx, o, v, nf, d1.ptr, slab_rows * n), lib=lib)
            ref = T[rows][:, :nf, x0:x0 + sx].reshape(o, v, nf, sx).transpose(3, 0, 1, 2)
            assert np.array_equal(d0.numpy((sx, o, v, nf)), ref)
            assert np.array_equal(d1.numpy((sx, o, v, nf)), ref)
            d0.free(); d1.free()
        dC.free()
    dT.free()


@pytest.mark.parametrize("n,o,naux,nf", SHAPES)
def test_pair_product(hlib, n, o, naux, nf):
    check_pair_product(hlib, n, naux)


@pytest.mark.parametrize("n,o,naux,nf", SHAPES)
def test_blocks_from_pair_product(hlib, n, o, naux, nf):
    check_blocks_from_pair_product(hlib, n, o, naux)


@pytest.mark.parametrize("n,o,naux,nf", SHAPES)
def test_three_quarter_rows(hlib, n, o, naux, nf):
    check_three_quarter_rows(hlib, n, o, nf)
