"""-m gpu: the fragment 2-RDM on the device (rdm2_ops.hip behind qemb_frag_rdm2 / qemb_op_rdm2_assemble) against the oracle's make_rdm2_urlx (CCSD) and
the NumPy restatement of PySCF's mp2.make_rdm2 (MP2).  1e-8 absolute is the project's figure for every fragment-vs-oracle comparison; the kernel on
handed-in amplitudes evaluates the reference's expression per element, so there a few ulp of the largest term (1e-12 at O(1) amplitudes) is asked."""
import numpy as np
import pytest

import mp2_numpy as mpn
from helpers import GOLDEN, synthetic_fragment_factor
from qemb_oracle import eri, rdm

pytestmark = pytest.mark.gpu
TOL = 1e-8

CASES = [(6, 2, 3), (12, 4, 4), (20, 6, 5), (7, 1, 2), (7, 6, 3), (5, 5, 2)]      # the sizes of tests/test_rdm2_hostlogic.py: ..., o = 1, v = 1, nsocc == n


def _fragment(residency, n, nf, e1, Bp):
    from quemb_amd.fragsolver import DeviceFragment
    fr = DeviceFragment(n, nf)
    if residency == "factor":
        fr.set_df_only(Bp)
    else:
        fr.set_eri_s4(eri.pack_s4(e1))
        if residency == "block+factor":
            fr.set_df_factor(Bp)
    return fr


@pytest.mark.parametrize("with_dm1", [True, False])
@pytest.mark.parametrize("n,o,nf", CASES)
def test_fragment_ccsd_rdm2_matches_oracle(qlib, n, o, nf, with_dm1):
    h, e1, Bp = synthetic_fragment_factor(n, o, 300 + n)
    fr = _fragment("block", n, nf, e1, Bp)
    out = fr.solve(o, h, eeval=False, want_t2=True)
    got = fr.make_rdm2("CCSD", with_dm1=with_dm1)
    ref = rdm.make_rdm2_urlx(out["t1"], out["t2"], with_dm1=with_dm1)
    err = np.abs(got - ref).max()
    print(f"CCSD n={n} o={o} with_dm1={with_dm1}: max |device - oracle| = {err:.2e}")
    assert err < TOL
    assert np.array_equal(got, fr.make_rdm2("CCSD", with_dm1=with_dm1))      # the same bits call to call
    fr.free()


@pytest.mark.parametrize("with_dm1", [True, False])
@pytest.mark.parametrize("residency", ["block", "block+factor", "factor"])
@pytest.mark.parametrize("n,o,nf", CASES)
def test_fragment_mp2_rdm2_matches_numpy(qlib, residency, n, o, nf, with_dm1):
    from quemb_amd.fragsolver import default_opts
    h, e1, Bp = synthetic_fragment_factor(n, o, 300 + n)
    fr = _fragment(residency, n, nf, e1, Bp)
    out = fr.solve_mp2(o, h, opts=default_opts(scf_conv_tol=1e-13, scf_conv_tol_grad=1e-9), eeval=False, want_t2=True)
    route, kept = fr.mo_route_used(), fr.resident_bytes()
    got = fr.make_rdm2("MP2", with_dm1=with_dm1)
    assert fr.mo_route_used() == route and fr.resident_bytes() == kept
    ref = mpn.make_rdm2(out["t2"]) if with_dm1 else mpn.dovov_part(out["t2"])
    err = np.abs(got - ref).max()
    print(f"MP2 {residency} n={n} o={o} with_dm1={with_dm1}: max |device - numpy| = {err:.2e}")
    assert err < TOL
    fr.free()


@pytest.mark.parametrize("kind", ["CCSD", "MP2"])
def test_kernel_at_n84_matches_the_reference_expression(qlib, kind):
    """n = 84 (o = 21, v = 63: rows that are no multiple of the workgroup width, 398 MB written) on amplitudes without any symmetry, both values of with_dm1"""
    from quemb_amd.fragsolver import rdm2_from_amplitudes
    o, v = 21, 63
    n = o + v
    rng = np.random.default_rng(84)
    t1 = rng.standard_normal((o, v))
    t2 = rng.standard_normal((o, o, v, v))
    dm1 = rng.standard_normal((n, n))
    got = rdm2_from_amplitudes(t1 if kind == "CCSD" else None, t2, kind=kind)
    ref = rdm.make_rdm2_urlx(t1, t2, with_dm1=False) if kind == "CCSD" else mpn.dovov_part(t2)
    err = np.abs(got - ref).max()
    print(f"{kind} n={n}: with_dm1=False max |device - reference expression| = {err:.2e} (largest element {np.abs(ref).max():.1f})")
    assert err < 1e-12 * max(1.0, np.abs(ref).max())
    assert np.count_nonzero(got) == 2 * (o * v) ** 2
    got1 = rdm2_from_amplitudes(t1 if kind == "CCSD" else None, t2, dm1=dm1, kind=kind)
    d = dm1.copy(); d[np.diag_indices(o)] -= 2.0      # the with_dm1 statements of the reference with a general (unsymmetric) matrix in the place of dm1 - 2 I_occ
    for i in range(o):
        ref[i, i, :, :] += d * 2
        ref[:, :, i, i] += d * 2
        ref[:, i, i, :] -= d
        ref[i, :, :, i] -= d.T
    for i in range(o):
        for j in range(o):
            ref[i, i, j, j] += 4
            ref[i, j, j, i] -= 2
    err1 = np.abs(got1 - ref).max()
    print(f"{kind} n={n}: with_dm1=True  max |device - reference expression| = {err1:.2e}")
    assert err1 < 1e-12 * max(1.0, np.abs(ref).max())


def test_golden_rdm2_from_amplitudes(qlib):
    from quemb_amd.fragsolver import rdm2_from_amplitudes
    g = np.load(GOLDEN / "rdm.npz")
    for case in (0, 1, 2):
        t1, t2 = g[f"t1_{case}"], g[f"t2_{case}"]
        assert np.abs(rdm2_from_amplitudes(t1, t2, dm1=rdm.make_rdm1_ccsd_t1(t1), kind="CCSD") - g[f"rdm2_dm1_{case}"]).max() < TOL
        assert np.abs(rdm2_from_amplitudes(t1, t2, kind="CCSD") - g[f"rdm2_cum_{case}"]).max() < TOL


def test_memory_guard_with_a_faked_free_memory_figure(qlib):
    from quemb_amd._lib import QEMB_ERR_ALLOC, QembError
    from quemb_amd.fragsolver import default_opts
    n, o, nf = 12, 4, 4
    h, e1, Bp = synthetic_fragment_factor(n, o, 312)
    fr = _fragment("block", n, nf, e1, Bp)
    fr.solve(o, h, eeval=False)
    fr.set_rdm2_mem_limit(8 * (n ** 4 + n * n) - 1)      # tensor + the 1-RDM of with_dm1
    try:
        with pytest.raises(QembError, match=f"n = {n}") as ei:
            fr.make_rdm2("CCSD")
        assert ei.value.status == QEMB_ERR_ALLOC
    finally:
        fr.set_rdm2_mem_limit(-1)
    assert fr.make_rdm2("CCSD").shape == (n,) * 4
    # MP2 forms t2 again: its three o^2 v^2 tensors and the integral work space count too, and the message still names n
    fr.solve_mp2(o, h, eeval=False)
    fr.set_rdm2_mem_limit(8 * (n ** 4 + n * n + 3 * (o * (n - o)) ** 2))
    with pytest.raises(QembError, match=f"n = {n}") as ei:
        fr.make_rdm2("MP2")
    assert ei.value.status == QEMB_ERR_ALLOC
    fr.set_rdm2_mem_limit(-1)
    assert fr.make_rdm2("MP2").shape == (n,) * 4
    fr.solve(o, h, opts=default_opts(relax_density=1), eeval=False)
    with pytest.raises(NotImplementedError, match="relaxed"):
        fr.make_rdm2("CCSD")
    fr.free()


def _octane(**kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    mf = RHF(Mole(GOLDEN / "octane.xyz")); mf.kernel()
    return BE(mf, FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_octane_be2"), distribute=False, **kw)


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_octane_be2_fragment_rdm2_batched_and_one_by_one_identical(qlib, solver):
    """Frags.make_rdm2 after a serial and after a batched one-shot sweep: the same bits, and e2 of get_frag_energy contracted with the dense tensors is the
    two-body energy the sweep evaluated in place"""
    be_s = _octane(nstreams=1, lockstep=False)
    ecorr, comps = be_s.oneshot(solver=solver)
    be_b = _octane(nstreams=1, lockstep=True)
    be_b.oneshot(solver=solver)
    e2 = 0.0
    for f, fb in zip(be_s.Fobjs, be_b.Fobjs):
        got = f.make_rdm2(with_dm1=False)
        assert np.array_equal(got, fb.make_rdm2(with_dm1=False))
        e1_ = eri.restore_s1(f.dev.get_eri_s4(), f.nao)
        w, cen = f.weight_and_relAO_per_center
        Cm = f.mo_coeffs
        r2 = np.einsum("ijkl,pi,qj,rk,sl->pqrs", 0.5 * got, Cm[cen], Cm, Cm, Cm, optimize=True)
        e2 += w * float(np.einsum("pjkl,pjkl->", r2, e1_[cen]))
    print(f"octane BE2 {solver}: Tr(V K) from the dense fragment 2-RDMs {e2:.12f}, from the sweep {comps[1]:.12f}")
    assert abs(e2 - comps[1]) < TOL


# ---- the full basis on the device: BE.compute_energy_full / rdm12_fullbasis against the NumPy restatement of mbe.py:488-838 (tests/rdm2_numpy.py)
def _h8(**kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    mf = RHF(Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])); mf.kernel()
    return BE(mf, FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2"), distribute=False, **kw)


@pytest.mark.parametrize("system", ["h8", "octane"])
def test_compute_energy_full_matches_restatement_batched_and_one_by_one_identical(qlib, system):
    """H8 BE2 and octane BE2 (N = 58, fragments of 42: several workgroups per row, sizes that are no multiple of a tile): the energies and both density matrices
    against the restatement at 1e-8, the full-basis expression against the sweep's fragment energy sum, and a serial and a batched sweep giving the same bits"""
    import rdm2_numpy as r2n
    make = _h8 if system == "h8" else _octane
    be = make(nstreams=1, lockstep=False)
    be.oneshot(solver="CCSD")
    ebe_oneshot = be.ebe_tot
    ref = r2n.energy_of(be, use_full_rdm=True)
    g, G = be.compute_energy_full(use_full_rdm=True)
    e = dict(be.e_full)
    for k in ("EKapprox", "EKtrue", "E2"):
        print(f"{system} BE2 {k}: device {e[k]:.12f} restatement {ref[k]:.12f}")
        assert abs(e[k] - ref[k]) < TOL
    assert np.abs(g - ref["rdm1"]).max() < TOL and np.abs(G - ref["RDM2_full"]).max() < TOL
    assert abs(e["EKapprox"] - ebe_oneshot) < TOL
    be_b = make(nstreams=1, lockstep=True)
    be_b.oneshot(solver="CCSD")
    gb, Gb = be_b.compute_energy_full(use_full_rdm=True)
    assert np.array_equal(G, Gb) and np.array_equal(g, gb)
    assert all(be_b.e_full[k] == e[k] for k in ("EKapprox", "EKtrue", "E2"))
    g2, G2 = be.compute_energy_full(use_full_rdm=True)      # and the same bits when asked again
    assert np.array_equal(G, G2) and be.e_full["EKtrue"] == e["EKtrue"]


def test_h8_mp2_full_basis_and_packed_integral_forms(qlib):
    """solver="MP2" through the same path; the N^4 contraction reads the 8-fold, the 4-fold and the unpacked integrals to the same value"""
    import ctypes as C
    import rdm2_numpy as r2n
    from quemb_amd import rdm_full
    from quemb_amd._lib import DeviceBuffer
    be = _h8()
    be.oneshot(solver="MP2")
    ref = r2n.energy_of(be)
    be.compute_energy_full()
    assert abs(be.e_full["EKapprox"] - ref["EKapprox"]) < TOL and abs(be.e_full["EKtrue"] - ref["EKtrue"]) < TOL
    N = be.C.shape[0]
    e1 = np.asarray(be.mf._eri).reshape((N,) * 4)
    K = be.rdm12_fullbasis(only_rdm2=True)
    Kd = DeviceBuffer.from_numpy(K)
    s4 = eri.pack_s4(e1)
    tri = np.tril_indices(s4.shape[0])
    want = float(np.einsum("pqrs,pqrs", e1, K))
    for form in (e1, s4, s4[tri]):
        ao = rdm_full.AOIntegrals(qlib, form, N)
        got = ao.dot(Kd)
        ao.free()
        assert abs(got - want) < 1e-10 * max(1.0, abs(want)), (ao.sym, got, want)
    Kd.free()


def test_full_basis_memory_guard_with_a_faked_free_memory_figure(qlib):
    from quemb_amd._lib import QEMB_ERR_ALLOC, QembError
    be = _h8()
    be.oneshot(solver="CCSD")
    N = be.C.shape[0]
    be.rdm2_mem_limit = 8 * N ** 4 + 8      # the accumulator fits, its workspace does not: nothing is allocated
    with pytest.raises(QembError, match=f"N = {N}") as ei:
        be.compute_energy_full()
    assert ei.value.status == QEMB_ERR_ALLOC
    be.rdm2_mem_limit = None
    assert be.compute_energy_full()[1].shape == (N,) * 4
