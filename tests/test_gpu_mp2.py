"""-m gpu: solver == "MP2" on the device -- the fragment solve, the amplitude kernel on its own, the benchmark-size fragment that lives on its factor,
the sweep modes and the BE driver -- against the NumPy restatement of PySCF's MP2 in tests/mp2_numpy.py.  1e-8 (absolute; Eh for energies) is the
project's figure for every fragment-vs-oracle comparison."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import mp2_numpy as mpn
from helpers import GOLDEN, synthetic_fragment_factor
from qemb_oracle import eri

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-8


def _energy_data(n, seed):
    rng = np.random.default_rng(seed + 1)
    sym = lambda: (lambda a: a + a.T)(rng.standard_normal((n, n)))
    return sym(), sym(), sym()


def test_fragment_mp2_matches_numpy_on_randomised_cases(qlib):
    """12 seeded cases n = 8 ... 96 over the three residencies (gap parameter 2.0 of helpers.synthetic_fragment: every fragment RHF converges, so no
    case is skipped)"""
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    rng = np.random.default_rng(20260)
    sizes = [8, 11, 16, 23, 31, 33, 40, 48, 57, 64, 80, 96]
    skipped = 0
    for k, n in enumerate(sizes):
        o = int(rng.integers(1, max(2, n // 3)))
        nf = int(rng.integers(1, min(n, 12)))
        cen = sorted(set(int(c) for c in rng.integers(0, nf, size=2)))
        residency = ["block", "block+factor", "factor"][k % 3]
        h, e1, Bp = synthetic_fragment_factor(n, o, 900 + k)
        h1, veff0, veff = _energy_data(n, 900 + k)
        fr = DeviceFragment(n, nf)
        if residency == "factor":
            fr.set_df_only(Bp)
        else:
            fr.set_eri_s4(eri.pack_s4(e1))
            if residency == "block+factor":
                fr.set_df_factor(Bp)
        fr.set_energy_data(h1, veff0, veff, 0.75, cen)
        out = fr.solve_mp2(o, h, opts=default_opts(scf_conv_tol=1e-13, scf_conv_tol_grad=1e-9), eeval=True, want_t2=True)
        assert fr.mo_route_used()[0] == (residency != "block")
        ref = mpn.fragment_mp2(out["mo_coeff"], out["mo_energy"], o, e1, nf, 0.75, cen, h1, veff0, veff)
        errs = dict(e_corr=abs(out["e_corr_mo"] - ref["e_corr"]), t2=np.abs(out["t2"] - ref["t2"]).max(), rdm1_mo=np.abs(out["rdm1_mo"] - ref["rdm1_mo"]).max(),
                    rdm1_emb=np.abs(out["rdm1_emb"] - ref["rdm1_emb"]).max(), e_frag=np.abs(out["e_frag"] - ref["e_frag"]).max())
        print(f"n={n} o={o} nf={nf} {residency}: " + " ".join(f"{a}={b:.2e}" for a, b in errs.items()))
        assert max(errs.values()) < TOL, (n, o, residency, errs)
        assert abs(np.trace(out["rdm1_mo"]) - 2 * o) < 1e-9
        fr.free()
    assert skipped == 0


def _factor_fragment(n, seed, naux, scale, gap=2.0):
    """helpers.synthetic_fragment_factor without the n^4 tensor: (h, B (naux, n, n) symmetric), the same draws in the same order"""
    rng = np.random.default_rng(seed)
    B = scale * rng.standard_normal((naux, n, n))
    B = 0.5 * (B + B.transpose(0, 2, 1))
    A = rng.standard_normal((n, n))
    return np.diag(gap * np.arange(n)) + 0.3 * 0.5 * (A + A.T), B


def test_benchmark_fragment_on_its_factor_matches_numpy_from_the_factor(qlib):
    """n = 220, o = 20, naux = 660 at the benchmark's amplitude: NumPy evaluates everything from the factor (ovov = Lov^T Lov, the n_f site rows only)"""
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    n, o, naux, nf, cen, w = 220, 20, 660, 8, [1, 2, 5], 0.75
    v = n - o
    h, B = _factor_fragment(n, 2026, naux, 0.03)
    il = np.tril_indices(n)
    Bp = np.ascontiguousarray(B[:, il[0], il[1]])
    h1, veff0, veff = _energy_data(n, 2026)
    fr = DeviceFragment(n, nf)
    fr.set_df_only(Bp)
    fr.set_energy_data(h1, veff0, veff, w, cen)
    out = fr.solve_mp2(o, h, eeval=True, want_t2=True)
    bytes_after_first = fr.resident_bytes()
    assert bytes_after_first == 8 * (Bp.size + 4 * n * n + n)                       # the factor, orbitals, density, J, K: nothing of the MP2 solve is kept
    assert fr.mo_route_used() == (True, naux)
    Cm, eps = out["mo_coeff"], out["mo_energy"]
    Lh = B @ Cm                                                                     # [L][p][q']
    Lov = np.einsum("pi,Lpa->Lia", Cm[:, :o], Lh[:, :, o:]).reshape(naux, o * v)
    ovov = (Lov.T @ Lov).reshape(o, v, o, v)
    e_ref, t2 = mpn.kernel(ovov, eps, o)
    dm1 = mpn.make_rdm1(t2)
    rdm = Cm @ dm1 @ Cm.T * 0.5
    hf = Cm[:, :o] @ Cm[:, :o].T
    d = 2.0 * (rdm - hf)
    e1 = np.einsum("ij,ij->i", h1[:nf], d[:nf]); ec = np.einsum("ij,ij->i", veff0[:nf], d[:nf])
    # e2_P = 1/2 sum C[P,x] dm2[x,y,z,w] (P y|z w) over the ovov and vovo blocks of mp2.make_rdm2, both 2 G
    G2 = 2.0 * mpn.theta(t2).reshape(o * v, o * v)
    Y = (Lov @ G2).reshape(naux, o, v)
    Ls = Lh[:, :nf, :]                                                              # [L][P][q']
    Z1 = np.einsum("LPa,Lia->iP", Ls[:, :, o:], Y); Z2 = np.einsum("LPi,Lia->aP", Ls[:, :, :o], Y)
    e2 = 0.5 * (np.einsum("Pi,iP->P", Cm[:nf, :o], Z1) + np.einsum("Pa,aP->P", Cm[:nf, o:], Z2))
    e_frag = np.array([w * sum(x[c] for c in cen) for x in (e1, e2, ec)])
    errs = dict(e_corr=abs(out["e_corr_mo"] - e_ref), t2=np.abs(out["t2"] - t2).max(), rdm1_mo=np.abs(out["rdm1_mo"] - dm1).max(),
                rdm1_emb=np.abs(out["rdm1_emb"] - rdm).max(), e_frag=np.abs(out["e_frag"] - e_frag).max())
    print("n=220: E_MP2 = %.10f  " % e_ref + " ".join(f"{a}={b:.2e}" for a, b in errs.items()))
    assert e_ref < -1e-3 and max(errs.values()) < TOL, errs
    out2 = fr.solve_mp2(o, h, dm0=2.0 * hf, eeval=True)
    assert fr.resident_bytes() == bytes_after_first                                 # unchanged by a solve
    assert abs(out2["e_corr_mo"] - e_ref) < TOL
    fr.free()


@pytest.mark.parametrize("o,v", [(1, 1), (3, 5), (7, 33), (20, 200), (21, 21)])
def test_amplitude_kernel_matches_numpy(qlib, o, v):
    """dev_mp2_amplitudes alone: t2 and G elementwise 1e-13 relative (one division, one fused multiply-add per element), energy 1e-12 relative"""
    import ctypes as C
    from quemb_amd._lib import DeviceBuffer, check
    rng = np.random.default_rng(17 * o + v)
    ovov = rng.standard_normal((o, v, o, v))
    ovov = 0.5 * (ovov + ovov.transpose(2, 3, 0, 1))
    eo = np.sort(rng.uniform(-3.0, -0.5, o)); ev = np.sort(rng.uniform(0.5, 4.0, v))
    d_in, d_eo, d_ev = DeviceBuffer.from_numpy(ovov), DeviceBuffer.from_numpy(eo), DeviceBuffer.from_numpy(ev)
    d_t2, d_G = DeviceBuffer.from_numpy(np.full((o, o, v, v), np.nan)), DeviceBuffer.from_numpy(np.full((o, v, o, v), np.nan))
    e = C.c_double()
    check(qlib.qemb_op_mp2_amplitudes(o, v, d_in.ptr, d_eo.ptr, d_ev.ptr, d_t2.ptr, d_G.ptr, C.byref(e)), "qemb_op_mp2_amplitudes")
    t2, G = d_t2.numpy((o, o, v, v)), d_G.numpy((o, v, o, v))
    _, t2_ref = mpn.kernel(ovov, np.concatenate([eo, ev]), o)
    G_ref = mpn.theta(t2_ref)
    assert np.array_equal(d_in.numpy(ovov.shape), ovov)
    assert np.isfinite(t2).all() and np.isfinite(G).all()
    # the reference energy in extended precision: a plain sum of 16 million terms is itself only good to a few 1e-13
    e_ref = float(np.sum((t2_ref * (2.0 * ovov.transpose(0, 2, 1, 3) - ovov.transpose(0, 2, 3, 1))).astype(np.longdouble)))
    rel = lambda a, b: float((np.abs(a - b) / np.abs(b)).max())
    print(f"o={o} v={v}: t2 {rel(t2, t2_ref):.2e}  G {rel(G, G_ref):.2e}  E {abs(e.value - e_ref) / abs(e_ref):.2e} (relative)")
    assert (np.abs(t2 - t2_ref) <= 1e-13 * np.abs(t2_ref)).all()
    assert (np.abs(G - G_ref) <= 1e-13 * np.abs(G_ref)).all()
    assert abs(e.value - e_ref) <= 1e-12 * abs(e_ref)
    e2 = C.c_double()
    check(qlib.qemb_op_mp2_amplitudes(o, v, d_in.ptr, d_eo.ptr, d_ev.ptr, d_t2.ptr, d_G.ptr, C.byref(e2)), "qemb_op_mp2_amplitudes")
    assert e2.value == e.value and np.array_equal(d_t2.numpy((o, o, v, v)), t2)      # the same bits run to run


def _octane(**kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    mf = RHF(Mole(GOLDEN / "octane.xyz")); mf.kernel()
    return BE(mf, FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_octane_be2"), distribute=False, **kw)


def test_octane_be2_sweep_modes_are_identical_and_match_numpy(qlib):
    res = {}
    for name, kw in (("serial", dict(nstreams=1, lockstep=False)), ("streams", dict(nstreams=4, lockstep=False)), ("batch", dict(nstreams=1, lockstep=True))):
        be = _octane(**kw)
        e, comps = be.oneshot(solver="MP2")
        res[name] = (e, np.asarray(comps), [f._rdm1.copy() for f in be.Fobjs], [f.rdm1__.copy() for f in be.Fobjs], be)
    for name in ("streams", "batch"):
        assert res[name][0] == res["serial"][0] and np.array_equal(res[name][1], res["serial"][1]), name
        for k in (2, 3):
            assert all(np.array_equal(a, b) for a, b in zip(res[name][k], res["serial"][k])), name
    be = res["serial"][4]
    tot = np.zeros(3)
    for f in be.Fobjs:
        e1 = eri.restore_s1(f.dev.get_eri_s4(), f.nao)
        w, cen = f.weight_and_relAO_per_center
        tot += mpn.fragment_mp2(f.mo_coeffs, f.mo_energy, f.nsocc, e1, f.n_frag, w, cen, f.h1, f.veff0, f.veff)["e_frag"]
    print(f"octane BE2 one-shot MP2: E_corr = {res['serial'][0]:.10f}, NumPy sum {tot.sum():.10f}")
    assert abs(res["serial"][0] - tot.sum()) < TOL and np.abs(res["serial"][1] - tot).max() < TOL
    opt = be.optimize(solver="MP2", only_chem=True, conv_tol=1e-7)
    assert opt.err < 1e-7


_SHAPELOG_JOB = """
import sys
sys.path[:0] = [r"{root}", r"{root}/tests", r"{root}/oracle"]
import numpy as np
from helpers import synthetic_fragment_factor
from quemb_amd import _lib
from quemb_amd.fragsolver import DeviceFragment
_lib.init(0)
n, o = 96, 16
h, e1, Bp = synthetic_fragment_factor(n, o, 5)
fr = DeviceFragment(n, 6)
fr.set_df_only(Bp)
rng = np.random.default_rng(1)
s = lambda: (lambda a: a + a.T)(rng.standard_normal((n, n)))
fr.set_energy_data(s(), s(), s(), 1.0, [0, 1])
out = fr.solve_mp2(o, h, eeval=True)
assert fr.mo_route_used() == (True, Bp.shape[0]) and out["e_corr_mo"] < 0
"""


def test_factor_route_has_no_quartic_virtual_work(qlib, tmp_path):
    """no product of an MP2 solve on the factor has more than 2 naux (o v)^2 flops: ovov = Lov^T Lov and Y = Lov G are the largest (the bound is derived
    for (o v)^2 >= n^2 v, true here: n = 96, o = 16).  The shape log is opened at a process's first product, hence the child process."""
    log = tmp_path / "shapes.txt"
    env = dict(os.environ, QEMB_GEMM_SHAPELOG=str(log))
    r = subprocess.run([sys.executable, "-c", _SHAPELOG_JOB.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    n, o, naux = 96, 16, 288
    bound = 2.0 * naux * (o * (n - o)) ** 2
    flops = [2.0 * m * nn * k * b for m, nn, k, b in (tuple(int(x) for x in ln.split()[:4]) for ln in log.read_text().splitlines() if ln.strip())]
    assert len(flops) > 5 and max(flops) <= bound, (max(flops), bound)
    assert sum(f == bound for f in flops) == 2                                       # step 2 and step 5, nothing else of that size
