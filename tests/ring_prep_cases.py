"""Operands, the extended-precision reference and the a-priori bound shared by the tests of the one-pass ring preparation (qemb_op_ccsd_ring_prep):
tests/test_ring_prep_hostlogic.py (mock library, CPU) and tests/test_gpu_ring_prep.py (device).

  W2[i,a,k,c] = W2base[i,a,k,c] + ZC[k,i,a,c] - sum_l t1[l,a] ovoo[l,c,k,i]
  R [i,a,k,c] = P1[i,a,k,c] + W1base[i,a,k,c] + ZB[k,c,a,i] - sum_l t1[l,a] ovoo[k,c,l,i] - W2[i,a,k,c] / 2

Bound, elementwise, for the result under test alone (the reference is accumulated in np.longdouble):
  |got - ref| <= (o + 6) 2^-53 (|P1| + |W1base| + |ZB| + |W2base|/2 + |ZC|/2 + sum_l |t1 ovoo| of both corrections, the W2 one halved)
for R, and the W2 terms alone (unhalved) for W2: a sum of o + 5 terms in any order, each product rounded once.

The rank-n_occ update of U with its transposed addend in the same sweep (qemb_op_ccsd_u_update), at the same shapes:
  U[i,j,a,b] <- U[i,j,a,b] + Z[i,a,b,j] - sum_k A[i,j,k,a] t1[k,b],      |got - ref| <= (o + 2) 2^-53 (|U| + |Z| + sum_k |A t1|)."""
import functools

import numpy as np

U = 2.0 ** -53
PAD = 64                        # doubles of NaN on each side of an output
# (o, v): minimal; odd v twice (8-byte path); one element past a 16-wide tile edge; exact tiles; edges in both tile directions with odd v, twice; the
# flagship n_occ over several tiles
SHAPES = [(1, 1), (2, 3), (3, 5), (5, 17), (8, 16), (9, 33), (13, 31), (20, 40)]
REFUSED = (33, 8)               # n_occ beyond the LDS image of the kernel


def _scaled(rng, shape, steps):
    """standard normal entries times a distinct factor per value of every index: a transposed or shifted read changes the magnitudes"""
    x = rng.standard_normal(shape)
    for ax, (n, st) in enumerate(zip(shape, steps)):
        f = 1.0 + st * np.arange(n)
        x = x * f.reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return x


@functools.lru_cache(maxsize=None)
def operands(o, v):
    """the inputs, the two slab images of ovoo the operation reads, the reference outputs (np.longdouble) and their bounds; computed once per shape, read-only"""
    rng = np.random.default_rng(9100 + 100 * o + v)
    t1 = _scaled(rng, (o, v), (0.29, 0.013))
    ovoo = _scaled(rng, (o, v, o, o), (0.37, 0.011, 0.23, 0.19))
    P1 = _scaled(rng, (o, v, o, v), (0.41, 0.017, 0.19, 0.0093))
    W1b = _scaled(rng, (o, v, o, v), (0.13, 0.021, 0.31, 0.0077))
    W2b = _scaled(rng, (o, v, o, v), (0.23, 0.0091, 0.17, 0.015))
    ZB = _scaled(rng, (o, v, v, o), (0.31, 0.012, 0.019, 0.27))          # [k,c,a,i]
    ZC = _scaled(rng, (o, o, v, v), (0.17, 0.33, 0.014, 0.0083))         # [k,i,a,c]
    OB = np.ascontiguousarray(ovoo.transpose(0, 3, 2, 1))                # OB[k,i,l,c] = ovoo[k,c,l,i]
    OC = np.ascontiguousarray(ovoo.transpose(2, 3, 0, 1))                # OC[k,i,l,c] = ovoo[l,c,k,i]
    L = np.longdouble
    sC = np.einsum("la,lcki->iakc", t1.astype(L), ovoo.astype(L))
    sB = np.einsum("la,kcli->iakc", t1.astype(L), ovoo.astype(L))
    zb = ZB.transpose(3, 2, 0, 1).astype(L)                              # -> [i,a,k,c]
    zc = ZC.transpose(1, 2, 0, 3).astype(L)
    W2 = W2b.astype(L) + zc - sC
    R = P1.astype(L) + W1b.astype(L) + zb - sB - W2 / 2
    aC = np.einsum("la,lcki->iakc", np.abs(t1), np.abs(ovoo))
    aB = np.einsum("la,kcli->iakc", np.abs(t1), np.abs(ovoo))
    mag_W2 = np.abs(W2b) + np.abs(ZC.transpose(1, 2, 0, 3)) + aC
    mag_R = np.abs(P1) + np.abs(W1b) + np.abs(ZB.transpose(3, 2, 0, 1)) + aB + 0.5 * mag_W2
    out = dict(t1=t1, P1=P1, W1b=W1b, W2b=W2b, ZB=ZB, ZC=ZC, OB=OB, OC=OC, W2=W2, R=R,
               bound_W2=(o + 6) * U * mag_W2, bound_R=(o + 6) * U * mag_R)
    for a in out.values():
        a.setflags(write=False)
    return out


def padded(n):
    """a host image of n output doubles between two NaN pads, everything NaN"""
    return np.full(n + 2 * PAD, np.nan)


def pads_untouched(img, n):
    bits = img.view(np.uint64)
    nan = np.array([np.nan]).view(np.uint64)[0]
    return bool(np.all(bits[:PAD] == nan) and np.all(bits[PAD + n:] == nan))


def run(lib, o, v):
    """one call of qemb_op_ccsd_ring_prep on the operands of (o, v), outputs between NaN pads; returns the host images (R, W2) and ZB, ZC as they are afterwards"""
    from quemb_amd._lib import DeviceBuffer, check
    c = operands(o, v)
    n = o * v * o * v
    d = {k: DeviceBuffer.from_numpy(c[k], lib=lib) for k in ("t1", "P1", "W1b", "W2b", "ZB", "ZC", "OB", "OC")}
    dR, dW2 = DeviceBuffer.from_numpy(padded(n), lib=lib), DeviceBuffer.from_numpy(padded(n), lib=lib)
    check(lib.qemb_op_ccsd_ring_prep(o, v, d["t1"].ptr, d["P1"].ptr, d["W1b"].ptr, d["W2b"].ptr, d["ZB"].ptr, d["ZC"].ptr, d["OB"].ptr, d["OC"].ptr,
                                     dR.at(PAD), dW2.at(PAD)), "ccsd_ring_prep", lib=lib)
    return dR.numpy(), dW2.numpy(), d["ZB"].numpy(), d["ZC"].numpy()


def check_outputs(o, v, r_img, w2_img, zb_after, zc_after):
    """asserts outputs within the bound, the NaN pads untouched and ZB, ZC bit-unchanged; prints the largest error / bound first"""
    c = operands(o, v)
    n = o * v * o * v
    assert pads_untouched(r_img, n) and pads_untouched(w2_img, n), (o, v)
    R = r_img[PAD:PAD + n].reshape(o, v, o, v)
    W2 = w2_img[PAD:PAD + n].reshape(o, v, o, v)
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(W2)), (o, v)
    eR, eW = np.abs(R.astype(np.longdouble) - c["R"]), np.abs(W2.astype(np.longdouble) - c["W2"])      # (the references stay in extended precision)
    print(f"ring_prep (o, v) = ({o}, {v}): max err / bound  R {float(np.max(eR / c['bound_R'])):.3f}  W2 {float(np.max(eW / c['bound_W2'])):.3f}")
    assert np.all(eR <= c["bound_R"]), (o, v, float(np.max(eR / c["bound_R"])))
    assert np.all(eW <= c["bound_W2"]), (o, v, float(np.max(eW / c["bound_W2"])))
    assert np.array_equal(zb_after.view(np.uint64), c["ZB"].reshape(-1).view(np.uint64)), (o, v, "ZB was written")
    assert np.array_equal(zc_after.view(np.uint64), c["ZC"].reshape(-1).view(np.uint64)), (o, v, "ZC was written")


@functools.lru_cache(maxsize=None)
def u_operands(o, v):
    """U[i,j,a,b], Z[i,a,b,j], A[i,j,k,a], t1[k,b], the reference of the updated U (np.longdouble) and its bound; computed once per shape, read-only"""
    rng = np.random.default_rng(9700 + 100 * o + v)
    U0 = _scaled(rng, (o, o, v, v), (0.21, 0.37, 0.013, 0.0089))
    Z = _scaled(rng, (o, v, v, o), (0.33, 0.016, 0.0097, 0.23))
    A = _scaled(rng, (o, o, o, v), (0.19, 0.29, 0.41, 0.012))
    t1 = _scaled(rng, (o, v), (0.31, 0.014))
    L = np.longdouble
    ref = U0.astype(L) + Z.transpose(0, 3, 1, 2).astype(L) - np.einsum("ijka,kb->ijab", A.astype(L), t1.astype(L))
    mag = np.abs(U0) + np.abs(Z.transpose(0, 3, 1, 2)) + np.einsum("ijka,kb->ijab", np.abs(A), np.abs(t1))
    out = dict(U0=U0, Z=Z, A=A, t1=t1, ref=ref, bound=(o + 2) * U * mag)
    for a in out.values():
        a.setflags(write=False)
    return out


def run_u(lib, o, v):
    """one call of qemb_op_ccsd_u_update on the operands of (o, v), U between NaN pads; returns the host image of U and Z as it is afterwards"""
    from quemb_amd._lib import DeviceBuffer, check
    c = u_operands(o, v)
    n = o * o * v * v
    img = padded(n)
    img[PAD:PAD + n] = c["U0"].reshape(-1)
    dU = DeviceBuffer.from_numpy(img, lib=lib)
    d = {k: DeviceBuffer.from_numpy(c[k], lib=lib) for k in ("A", "t1", "Z")}
    check(lib.qemb_op_ccsd_u_update(o, v, d["A"].ptr, d["t1"].ptr, d["Z"].ptr, dU.at(PAD)), "ccsd_u_update", lib=lib)
    return dU.numpy(), d["Z"].numpy()


def check_u(o, v, u_img, z_after):
    c = u_operands(o, v)
    n = o * o * v * v
    assert pads_untouched(u_img, n), (o, v)
    got = u_img[PAD:PAD + n].reshape(o, o, v, v)
    assert np.all(np.isfinite(got)), (o, v)
    err = np.abs(got.astype(np.longdouble) - c["ref"])
    print(f"u_update (o, v) = ({o}, {v}): max err / bound {float(np.max(err / c['bound'])):.3f}")
    assert np.all(err <= c["bound"]), (o, v, float(np.max(err / c["bound"])))
    assert np.array_equal(z_after.view(np.uint64), c["Z"].reshape(-1).view(np.uint64)), (o, v, "Z was written")
