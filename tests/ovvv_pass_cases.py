"""Operands, references and a-priori error bounds shared by the tests of the one-pass ovvv operations (qemb_op_ccsd_ovvv_pass, qemb_op_ccsd_ph_layouts_ring):
tests/test_ovvv_pass_hostlogic.py (mock library, CPU) and tests/test_gpu_ovvv_pass.py (device)."""
import functools

import numpy as np

U = 2.0 ** -53
PAD = 64                        # doubles of NaN on each side of an output
# (o, v) of the shapes table: smallest; one row tile plus one row; 2 o < 16; 2 o = 16 and v = one tile; NT = 2 with a ragged v; 2 o = 24;
# NT = 2 at its boundary 2 o = 26 -> 32 with v no multiple of the K chunk; the flagship's NT = 3 with a short v; 2 o = 48; NT = 4 twice
SHAPES = [(1, 1), (1, 17), (3, 5), (8, 16), (9, 33), (12, 40), (13, 31), (20, 50), (24, 16), (25, 20), (32, 12)]
REFUSED = (33, 8)


def gamma(K):
    return K * U / (1.0 - K * U)


def _scaled(rng, shape, steps):
    """standard normal entries times a distinct factor per value of every index: a transposed or shifted read changes the magnitudes"""
    x = rng.standard_normal(shape)
    for ax, (n, st) in enumerate(zip(shape, steps)):
        f = 1.0 + st * np.arange(n)
        x = x * f.reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return x


@functools.lru_cache(maxsize=None)
def operands(o, v):
    """ovvv[k,c,a,d], t1[i,d], t2[k,i,c,d] (not symmetrised: the layouts are defined for any t2), Thk[k,c,i,d] = S = 2 t2[k,i,c,d] - t2[k,i,d,c], and the
    references ZB[k,c,a,i] = sum_d ovvv[kcad] t1[id], PA[i,a] = sum_kcd Thk[kcid] ovvv[kcad] with the products of absolute values their bounds need.
    The references are NumPy einsum, accumulated in np.longdouble where the platform has more than 53 bits there, so that the a-priori bound of a length-K
    dot product applies to the result under test alone.  Computed once per shape and never modified (arrays are read-only)."""
    rng = np.random.default_rng(7000 + 100 * o + v)
    ovvv = _scaled(rng, (o, v, v, v), (0.37, 0.011, 0.023, 0.0071))
    t1 = _scaled(rng, (o, v), (0.29, 0.013))
    t2 = _scaled(rng, (o, o, v, v), (0.41, 0.19, 0.017, 0.0093))
    thk = np.ascontiguousarray(2.0 * t2.transpose(0, 2, 1, 3) - t2.transpose(0, 3, 1, 2))       # [k,c,i,d] <- 2 t2[k,i,c,d] - t2[k,i,d,c]: the S of the layouts
    L = np.longdouble
    zb = np.einsum("kcad,id->kcai", ovvv.astype(L), t1.astype(L)).astype(np.float64)
    pa = np.einsum("kcid,kcad->ia", thk.astype(L), ovvv.astype(L)).astype(np.float64)
    zb_abs = np.einsum("kcad,id->kcai", np.abs(ovvv), np.abs(t1))
    pa_abs = np.einsum("kcid,kcad->ia", np.abs(thk), np.abs(ovvv))
    out = dict(ovvv=ovvv, t1=t1, t2=t2, thk=thk, zb=zb, pa=pa, zb_abs=zb_abs, pa_abs=pa_abs)
    for a in out.values():
        a.setflags(write=False)
    return out


def layouts_reference(t2, t1):
    """the four outputs of ccsd_ph_layouts_ring, all [o][v][o][v]"""
    T = t2.transpose(0, 2, 1, 3)
    Tp = t2.transpose(0, 3, 1, 2)
    tt = 2.0 * np.einsum("jc,kb->kcjb", t1, t1)
    return Tp, 2.0 * T - Tp, 2.0 * T - Tp - tt, Tp + tt


def padded(n):
    """a host image of n output doubles between two NaN pads, everything NaN"""
    return np.full(n + 2 * PAD, np.nan)


def pads_untouched(img, n):
    bits = img.view(np.uint64)
    nan = np.array([np.nan]).view(np.uint64)[0]
    return bool(np.all(bits[:PAD] == nan) and np.all(bits[PAD + n:] == nan))


def check_pass(o, v, G, zb_img, pa_img):
    """zb_img / pa_img: the padded host images after the call.  Returns nothing; asserts outputs and padding."""
    c = operands(o, v)
    nzb, npa = o * v * v * o, G * o * v
    assert pads_untouched(zb_img, nzb) and pads_untouched(pa_img, npa), (o, v)
    zb = zb_img[PAD:PAD + nzb].reshape(o, v, v, o)
    slabs = pa_img[PAD:PAD + npa].reshape(G, o, v)
    assert np.all(np.isfinite(zb)) and np.all(np.isfinite(slabs)), (o, v)
    pa = np.zeros((o, v))
    for g in range(G):                      # slab order, as dev_ccsd_t1_assemble adds them
        pa = pa + slabs[g]
    ezb = np.abs(zb - c["zb"]); bzb = gamma(v) * c["zb_abs"]
    epa = np.abs(pa - c["pa"]); bpa = gamma(o * v * v) * c["pa_abs"]
    print(f"ovvv_pass (o, v) = ({o}, {v}) G = {G}: max err / bound  ZB {np.max(ezb / bzb):.3f}  PA {np.max(epa / bpa):.3f}")
    assert np.all(ezb <= bzb), (o, v, float(np.max(ezb / bzb)))
    assert np.all(epa <= bpa), (o, v, float(np.max(epa / bpa)))
    # idle workgroups (more slabs of PA than (k,c) pairs) write zeros
    nslab = o * v
    for g in range(G):
        if g * nslab // G == (g + 1) * nslab // G:
            assert np.array_equal(slabs[g], np.zeros((o, v))), (o, v, g)


def run_pass(lib, o, v):
    """one call of qemb_op_ccsd_ovvv_pass on the operands of (o, v), outputs between NaN pads; returns (G, zb image, pa image) on the host"""
    from quemb_amd._lib import DeviceBuffer, check
    c = operands(o, v)
    G = lib.qemb_op_ccsd_ovvv_slabs(o, v)
    assert G > 0, (o, v, G)
    nzb, npa = o * v * v * o, G * o * v
    d_ovvv, d_t1, d_thk = (DeviceBuffer.from_numpy(c[k], lib=lib) for k in ("ovvv", "t1", "thk"))
    d_zb, d_pa = DeviceBuffer.from_numpy(padded(nzb), lib=lib), DeviceBuffer.from_numpy(padded(npa), lib=lib)
    check(lib.qemb_op_ccsd_ovvv_pass(o, v, d_ovvv.ptr, d_t1.ptr, d_thk.ptr, d_zb.at(PAD), d_pa.at(PAD)), "ccsd_ovvv_pass")
    return G, d_zb.numpy(), d_pa.numpy()


def run_layouts_ring(lib, o, v):
    """qemb_op_ccsd_ph_layouts_ring on the t2 / t1 of (o, v): Tp, S, Ut, Tpt, each from between NaN pads that must stay untouched"""
    from quemb_amd._lib import DeviceBuffer, check
    c = operands(o, v)
    n = o * v * o * v
    d2, d1 = DeviceBuffer.from_numpy(c["t2"], lib=lib), DeviceBuffer.from_numpy(c["t1"], lib=lib)
    outs = [DeviceBuffer.from_numpy(padded(n), lib=lib) for _ in range(4)]
    check(lib.qemb_op_ccsd_ph_layouts_ring(o, v, d2.ptr, d1.ptr, *[b.at(PAD) for b in outs]), "ccsd_ph_layouts_ring")
    imgs = [b.numpy() for b in outs]
    for k, img in enumerate(imgs):
        assert pads_untouched(img, n), (o, v, k)
    return [img[PAD:PAD + n].reshape(o, v, o, v) for img in imgs]


def check_layouts_ring(o, v, got):
    c = operands(o, v)
    Tp, S, Ut, Tpt = layouts_reference(c["t2"], c["t1"])
    assert np.array_equal(got[0], Tp)
    # each entry is one or two roundings of a sum of at most three terms: 4 u of the terms' magnitudes covers any association
    mag = 2 * np.abs(c["t2"].transpose(0, 2, 1, 3)) + np.abs(Tp) + 2.0 * np.einsum("jc,kb->kcjb", np.abs(c["t1"]), np.abs(c["t1"]))
    for name, g, r in (("S", got[1], S), ("Ut", got[2], Ut), ("Tpt", got[3], Tpt)):
        assert np.all(np.abs(g - r) <= 4 * U * mag), (o, v, name)
    assert np.array_equal(S, c["thk"])      # S is the Thk operand the update hands to the one pass
