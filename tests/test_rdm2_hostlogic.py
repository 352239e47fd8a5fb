"""CPU: the fragment 2-RDM (qemb_frag_rdm2, qemb_op_rdm2_assemble) from the C ABI to Frags.make_rdm2 and the solver functions, with the device layer
replaced by the scalar mock (tests/hostcheck), against the oracle's make_rdm2_urlx (CCSD), the NumPy restatement of PySCF's mp2.make_rdm2 (MP2) and
the reference-generated arrays of tests/golden/rdm.npz.  Tolerance 1e-8 absolute: the project's figure for every fragment-vs-oracle comparison."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import mp2_numpy as mpn
from helpers import GOLDEN, synthetic_fragment_factor
from qemb_oracle import eri, rdm

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))
TOL = 1e-8

# the size cases of tests/test_mp2_hostlogic.py: ..., o = 1, v = 1, nsocc == n
CASES = [(6, 2, 3, [0, 1]), (12, 4, 4, [1, 2]), (20, 6, 5, [0]), (7, 1, 2, [0]), (7, 6, 3, [2]), (5, 5, 2, [0, 1])]


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


def _fragment(lib, residency, n, nf, e1, Bp):
    from quemb_amd.fragsolver import DeviceFragment
    fr = DeviceFragment(n, nf, lib=lib)
    if residency == "factor":
        fr.set_df_only(Bp)
    else:
        fr.set_eri_s4(eri.pack_s4(e1))
        if residency == "block+factor":
            fr.set_df_factor(Bp)
    return fr


def _symmetries(dm2):
    """what every spin-summed 2-RDM of real orbitals has: (pq|rs) <-> (rs|pq) and the simultaneous transposition of both pairs"""
    assert np.abs(dm2 - dm2.transpose(2, 3, 0, 1)).max() < 1e-12
    assert np.abs(dm2 - dm2.transpose(1, 0, 3, 2)).max() < 1e-12


@pytest.mark.parametrize("with_dm1", [True, False])
@pytest.mark.parametrize("n,o,nf,cen", CASES)
def test_fragment_ccsd_rdm2_matches_oracle(hlib, n, o, nf, cen, with_dm1):
    from quemb_amd.fragsolver import default_opts
    h, e1, Bp = synthetic_fragment_factor(n, o, 300 + n)
    fr = _fragment(hlib, "block", n, nf, e1, Bp)
    out = fr.solve(o, h, opts=default_opts(hlib), eeval=False, want_t2=True)
    got = fr.make_rdm2("CCSD", with_dm1=with_dm1)
    ref = rdm.make_rdm2_urlx(out["t1"], out["t2"].reshape(o, o, n - o, n - o), with_dm1=with_dm1)
    err = np.abs(got - ref).max()
    print(f"CCSD n={n} o={o} with_dm1={with_dm1}: max |device - oracle| = {err:.2e}")
    assert got.shape == (n,) * 4 and err < TOL
    _symmetries(got)
    if with_dm1:      # N (N - 1) electron pairs: the correlation 1-RDM of unrelaxed CCSD has no diagonal, so the determinant terms alone count
        assert abs(np.einsum("pprr->", got) - 2 * o * (2 * o - 1)) < 1e-9
    if o == n:
        hf = rdm.make_rdm2_urlx(np.zeros((o, 0)), np.zeros((o, o, 0, 0)), with_dm1=with_dm1)
        assert np.array_equal(got, hf)
    with pytest.raises(Exception, match="last solve of this fragment was CCSD"):
        fr.make_rdm2("MP2")
    fr.free()


@pytest.mark.parametrize("with_dm1", [True, False])
@pytest.mark.parametrize("residency", ["block", "block+factor", "factor"])
@pytest.mark.parametrize("n,o,nf,cen", CASES)
def test_fragment_mp2_rdm2_matches_numpy(hlib, residency, n, o, nf, cen, with_dm1):
    from quemb_amd.fragsolver import default_opts
    h, e1, Bp = synthetic_fragment_factor(n, o, 300 + n)
    fr = _fragment(hlib, residency, n, nf, e1, Bp)
    opts = default_opts(hlib, scf_conv_tol=1e-13, scf_conv_tol_grad=1e-9)
    out = fr.solve_mp2(o, h, opts=opts, eeval=False, want_t2=True)
    route = fr.mo_route_used()
    bytes_before = fr.resident_bytes()
    got = fr.make_rdm2("MP2", with_dm1=with_dm1)
    assert fr.mo_route_used() == route and fr.resident_bytes() == bytes_before      # forming t2 again leaves the fragment as the solve left it
    t2 = out["t2"].reshape(o, o, n - o, n - o)
    ref = mpn.make_rdm2(t2) if with_dm1 else mpn.dovov_part(t2)
    err = np.abs(got - ref).max()
    print(f"MP2 {residency} n={n} o={o} with_dm1={with_dm1}: max |device - numpy| = {err:.2e}")
    assert err < TOL
    _symmetries(got)
    fr.free()


@pytest.mark.parametrize("case", [0, 1, 2])
def test_golden_rdm2_from_amplitudes(hlib, case):
    """the reference-generated make_rdm2_urlx arrays (tests/golden/rdm.npz) from their t1 / t2 through the operation behind make_rdm2"""
    from quemb_amd.fragsolver import rdm2_from_amplitudes
    g = np.load(GOLDEN / "rdm.npz")
    t1, t2 = g[f"t1_{case}"], g[f"t2_{case}"]
    got_dm1 = rdm2_from_amplitudes(t1, t2, dm1=rdm.make_rdm1_ccsd_t1(t1), kind="CCSD", lib=hlib)
    got_cum = rdm2_from_amplitudes(t1, t2, kind="CCSD", lib=hlib)
    assert np.abs(got_dm1 - g[f"rdm2_dm1_{case}"]).max() < TOL
    assert np.abs(got_cum - g[f"rdm2_cum_{case}"]).max() < TOL
    # handed-in amplitudes need not have the symmetry t2[i,j,a,b] = t2[j,i,b,a] the solvers produce: the expressions are evaluated literally
    rng = np.random.default_rng(case)
    t2r = rng.standard_normal(t2.shape)
    assert np.abs(rdm2_from_amplitudes(t1, t2r, kind="CCSD", lib=hlib) - rdm.make_rdm2_urlx(t1, t2r, with_dm1=False)).max() < 1e-12
    assert np.abs(rdm2_from_amplitudes(None, t2r, kind="MP2", lib=hlib) - mpn.dovov_part(t2r)).max() < 1e-12
    dm1 = mpn.make_rdm1(t2)
    assert np.abs(rdm2_from_amplitudes(None, t2, dm1=dm1, kind="MP2", lib=hlib) - mpn.make_rdm2(t2)).max() < 1e-12
    with pytest.raises(ValueError):
        rdm2_from_amplitudes(t1.T, t2, kind="CCSD", lib=hlib)
    with pytest.raises(ValueError, match="Solver not implemented"):
        rdm2_from_amplitudes(t1, t2, kind="FCI", lib=hlib)


def test_solver_functions_return_the_tensor(hlib):
    from quemb_amd.solver import solve_ccsd, solve_mp2
    n, o = 9, 3
    h, e1, Bp = synthetic_fragment_factor(n, o, 21)
    s4 = eri.pack_s4(e1)
    t1, t2, dm1, dm2 = solve_ccsd(h, s4, o, rdm_return=True, rdm2_return=True, lib=hlib)                 # use_cumulant=True: with_dm1=False (solver.py:941)
    assert np.abs(dm2 - rdm.make_rdm2_urlx(t1, t2, with_dm1=False)).max() < TOL
    assert np.abs(dm1 - rdm.make_rdm1_ccsd_t1(t1)).max() < TOL
    t1b, t2b, dm2b = solve_ccsd(h, s4, o, rdm2_return=True, use_cumulant=False, lib=hlib)
    assert np.array_equal(t1b, t1) and np.abs(dm2b - rdm.make_rdm2_urlx(t1, t2, with_dm1=True)).max() < TOL
    assert len(solve_ccsd(h, s4, o, rdm_return=True, lib=hlib)) == 4 and len(solve_ccsd(h, s4, o, lib=hlib)) == 2
    e, t2m, dm1m, dm2m = solve_mp2(h, s4, o, rdm_return=True, rdm2_return=True, use_cumulant=False, lib=hlib)
    assert np.abs(dm2m - mpn.make_rdm2(t2m)).max() < TOL and np.abs(dm1m - mpn.make_rdm1(t2m)).max() < TOL
    e2, t2f, dm2f = solve_mp2(h, None, o, df_factor=Bp, rdm2_return=True, lib=hlib)
    assert abs(e2 - e) < TOL and np.abs(dm2f - mpn.dovov_part(t2f)).max() < TOL
    # the energy the 2-RDM carries: <eri, dm2> / 2 with the dovov part is 2 E_MP2 (tests/mp2_numpy.py)
    Cm = solve_mp2(h, s4, o, rdm_return=True, lib=hlib)[3]
    assert abs(0.5 * np.einsum("pqrs,pqrs->", mpn.mo_eri(e1, Cm), dm2f) - 2.0 * e) < 1e-8


def test_relaxed_fragments_are_refused(hlib):
    from quemb_amd.fragsolver import default_opts
    from quemb_amd.pfrag import Frags
    from quemb_amd.solver import solve_ccsd
    n, o, nf = 8, 3, 3
    h, e1, Bp = synthetic_fragment_factor(n, o, 77)
    fr = _fragment(hlib, "block", n, nf, e1, Bp)
    fr.solve(o, h, opts=default_opts(hlib, relax_density=1), eeval=False)
    with pytest.raises(NotImplementedError, match="relaxed"):
        fr.make_rdm2("CCSD")
    fr.solve(o, h, opts=default_opts(hlib), eeval=False)                    # an unrelaxed solve of the same fragment is served again
    assert np.isfinite(fr.make_rdm2("CCSD")).all()
    with pytest.raises(NotImplementedError, match="relaxed"):
        solve_ccsd(h, eri.pack_s4(e1), o, rdm2_return=True, relax=True, lib=hlib)
    f = Frags(list(range(nf)), 0, [], [], [], [], (1.0, [0]), [0], lib=hlib)
    f.dev = fr
    f.nao, f.nsocc, f.fock, f.heff, f.dm0 = n, o, h, np.zeros((n, n)), None
    with pytest.raises(RuntimeError, match="solve the fragment first"):
        f.make_rdm2()
    f.solve(eeval=False, relax_density=True)
    with pytest.raises(NotImplementedError, match="relaxed"):
        f.make_rdm2()
    assert f.rdm2__ is None


def test_no_solve_or_changed_integrals_are_refused(hlib):
    from quemb_amd._lib import QembError
    from quemb_amd.fragsolver import default_opts
    n, o, nf = 6, 2, 2
    h, e1, Bp = synthetic_fragment_factor(n, o, 5)
    fr = _fragment(hlib, "block", n, nf, e1, Bp)
    with pytest.raises(QembError, match="no solve has run"):
        fr.make_rdm2("CCSD")
    fr.solve_mp2(o, h, opts=default_opts(hlib), eeval=False)
    assert np.isfinite(fr.make_rdm2("MP2")).all()
    fr.scf(o, h)                                                            # new orbitals: the kept 1-RDM no longer belongs to them
    with pytest.raises(QembError, match="no solve has run"):
        fr.make_rdm2("MP2")
    fr.solve_mp2(o, h, opts=default_opts(hlib), eeval=False)
    fr.set_eri_s4(eri.pack_s4(e1))
    with pytest.raises(QembError, match="no solve has run"):
        fr.make_rdm2("MP2")
    with pytest.raises(ValueError, match="Solver not implemented"):
        fr.make_rdm2("FCI")
    fr.free()


def test_memory_guard_names_n(hlib):
    from quemb_amd._lib import QEMB_ERR_ALLOC, QembError
    from quemb_amd.fragsolver import default_opts
    n, o, nf = 6, 2, 2
    h, e1, Bp = synthetic_fragment_factor(n, o, 5)
    fr = _fragment(hlib, "block", n, nf, e1, Bp)
    fr.solve(o, h, opts=default_opts(hlib), eeval=False)
    fr.set_rdm2_mem_limit(8 * (n ** 4 + n * n) - 1)      # tensor + the 1-RDM of with_dm1
    try:
        with pytest.raises(QembError, match=f"n = {n}") as ei:
            fr.make_rdm2("CCSD")
        assert ei.value.status == QEMB_ERR_ALLOC
        fr.set_rdm2_mem_limit(8 * (n ** 4 + n * n))
        assert fr.make_rdm2("CCSD").shape == (n,) * 4
    finally:
        fr.set_rdm2_mem_limit(-1)
    # MP2 forms t2 again: its three o^2 v^2 tensors and the integral work space count too, and the message still names n
    fr.solve_mp2(o, h, opts=default_opts(hlib), eeval=False)
    fr.set_rdm2_mem_limit(8 * (n ** 4 + n * n + 3 * (o * (n - o)) ** 2))
    with pytest.raises(QembError, match=f"n = {n}") as ei:
        fr.make_rdm2("MP2")
    assert ei.value.status == QEMB_ERR_ALLOC
    fr.set_rdm2_mem_limit(-1)
    assert fr.make_rdm2("MP2").shape == (n,) * 4
    fr.free()


def _h8(lib, **kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    mol = Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
    mf = RHF(mol); mf.kernel()
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    return BE(mf, fobj, lib=lib, distribute=False, **kw)


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_h8_be2_fragment_rdm2_after_a_sweep(hlib, solver):
    """Frags.make_rdm2 after BE.oneshot: rdm2__ of every fragment against the reference expression of the amplitudes the sweep left, the same bits after a
    batched sweep, and the fragment energy sum from it: e2 of get_frag_energy contracted with the dense tensor equals what the sweep evaluated in place."""
    be = _h8(hlib, lockstep=False, nstreams=1)
    ecorr, comps = be.oneshot(solver=solver)
    be_b = _h8(hlib, lockstep=True)
    be_b.oneshot(solver=solver)
    e2 = 0.0
    for f, fb in zip(be.Fobjs, be_b.Fobjs):
        assert f.rdm2__ is None
        got = f.make_rdm2(with_dm1=False)
        assert got is f.rdm2__ and np.array_equal(got, fb.make_rdm2(with_dm1=False))
        o, n = f.nsocc, f.nao
        if solver == "CCSD":
            t2 = f.dev.solve(o, f.fock + f.heff, f.dm0, opts=be.opts, eeval=False, want_t2=True)["t2"]
            ref = rdm.make_rdm2_urlx(f.t1, t2, with_dm1=False)
            full = rdm.make_rdm2_urlx(f.t1, t2, with_dm1=True)
        else:
            t2 = f.dev.solve_mp2(o, f.fock + f.heff, f.dm0, opts=be.opts, eeval=False, want_t2=True)["t2"]
            ref, full = mpn.dovov_part(t2), mpn.make_rdm2(t2)
        assert np.abs(got - ref).max() < TOL
        assert np.abs(f.make_rdm2(with_dm1=True) - full).max() < TOL
        e1_ = eri.restore_s1(f.dev.get_eri_s4(), n)
        w, cen = f.weight_and_relAO_per_center
        r2 = np.einsum("ijkl,pi,qj,rk,sl->pqrs", 0.5 * got, f.mo_coeffs, f.mo_coeffs, f.mo_coeffs, f.mo_coeffs, optimize=True)
        e2 += w * sum(np.einsum("jkl,jkl->", r2[c], e1_[c]) for c in cen)
    assert abs(e2 - comps[1]) < TOL, (e2, comps[1])


# ---- the full basis: BE.rdm12_fullbasis / BE.compute_energy_full against the NumPy restatement of mbe.py:488-838 (tests/rdm2_numpy.py)
def test_restatement_identities():
    """the restatement pinned by identities of its own, on random fragments: the 1-RDM and the cumulant are symmetric under the full transposition, the MO / LO forms rotate back to the AO ones, and approx_cumulant=True / False return the RDM built on the cumulant they name"""
    import rdm2_numpy as r2n
    rng = np.random.default_rng(7)
    N, n = 5, 4
    A = rng.standard_normal((N, N)); S = A @ A.T + N * np.eye(N)
    w, U = np.linalg.eigh(S); W = (U / np.sqrt(w)) @ U.T
    C = W @ np.linalg.qr(rng.standard_normal((N, N)))[0]
    frags = []
    for k in range(2):
        d = rng.standard_normal((n, n)); x = rng.standard_normal((n,) * 4)
        frags.append(dict(rdm1=d + d.T, rdm2=x + x.transpose(2, 3, 0, 1), nsocc=2, mo_coeffs=np.linalg.qr(rng.standard_normal((n, n)))[0],
                          TA=rng.standard_normal((N, n)), cind=[k, k + 2]))
    g, K = r2n.rdm12_fullbasis(frags, S, W, C, return_RDM2=False)
    g2, G = r2n.rdm12_fullbasis(frags, S, W, C, return_RDM2=True)
    assert np.array_equal(g, g2) and np.abs(g - g.T).max() < 1e-12
    assert np.abs(K - K.T).max() < 1e-9      # (G carries nc_AO of the 1-RDM as accumulated, which is symmetric only as far as that matrix is)
    assert np.array_equal(r2n.rdm12_fullbasis(frags, S, W, C, only_rdm2=True), G)
    gm, Gm, gl, Gl = r2n.rdm12_fullbasis(frags, S, W, C, return_ao=False, return_lo=True)
    assert np.abs(C @ gm @ C.T - g).max() < 1e-10 and np.abs(np.einsum("ijkl,pi,qj,rk,sl->pqrs", Gl, W, W, W, W, optimize=True) - G).max() < 1e-9
    e = np.zeros((N,) * 4); z = np.zeros((N, N))
    ra = r2n.compute_energy_full(frags, S, W, C, z, z, z, e, 0.0, 0.0, approx_cumulant=True)
    rt = r2n.compute_energy_full(frags, S, W, C, z, z, z, e, 0.0, 0.0, approx_cumulant=False)
    assert np.abs(ra["RDM2_full"] - (r2n.non_connected(g) + K)).max() < 1e-12 and np.abs(rt["RDM2_full"] - (r2n.non_connected(g) + G)).max() < 1e-12
    assert "EKtrue" not in ra and rt["ebe_tot"] == rt["EKtrue"] and ra["ebe_tot"] == ra["EKapprox"]


@pytest.fixture(scope="module")
def h8_swept(hlib):
    """H8 / STO-3G BE2 after one-shot sweeps with both solvers, with the restatement's energies (computed once)"""
    import rdm2_numpy as r2n
    out = {}
    for solver in ("CCSD", "MP2"):
        be = _h8(hlib)
        be.oneshot(solver=solver)
        out[solver] = (be, be.ebe_tot, r2n.frags_of(be), r2n.energy_of(be, use_full_rdm=True))
    return out


def test_h8_be2_rdm12_fullbasis_matches_restatement_in_every_return_mode(h8_swept):
    import rdm2_numpy as r2n
    be, _, frags, _ = h8_swept["CCSD"]
    for return_ao in (True, False):
        for return_lo in (True, False):
            for return_RDM2 in (True, False):
                kw = dict(return_ao=return_ao, return_lo=return_lo, return_RDM2=return_RDM2)
                got = be.rdm12_fullbasis(**kw)
                ref = r2n.rdm12_fullbasis(frags, be.S, be.W, be.C, **kw)
                assert len(got) == len(ref) == (4 if return_lo else 2)
                for a, b in zip(got, ref):
                    err = np.abs(a - b).max()
                    print(f"H8 BE2 rdm12_fullbasis {kw}: max |device path - restatement| = {err:.2e}")
                    assert a.shape == b.shape and err < TOL
            got = be.rdm12_fullbasis(return_ao=return_ao, only_rdm2=True, return_lo=return_lo)
            assert np.abs(got - r2n.rdm12_fullbasis(frags, be.S, be.W, be.C, return_ao=return_ao, only_rdm2=True, return_lo=return_lo)).max() < TOL


def test_h8_be2_electron_count_once_the_centres_are_matched(hlib):
    """Tr(S gamma) of the full-basis 1-RDM: a one-shot sweep does not conserve the electron number, the optimised potentials (chemical potential and edge
    matching, converged well below the tolerance) do"""
    be = _h8(hlib)
    be.optimize(solver="MP2", conv_tol=1e-10)
    g, G = be.rdm12_fullbasis()
    nel = np.trace(be.S @ g)
    print(f"H8 BE2 MP2 optimised: Tr(S gamma) = {nel:.12f}")
    assert abs(nel - 8.0) < TOL
    K = be.rdm12_fullbasis(only_rdm2=True, return_RDM2=False)
    assert np.abs(K - K.T).max() < 1e-12


@pytest.mark.parametrize("solver", ["CCSD", "MP2"])
def test_h8_be2_compute_energy_full_matches_restatement_and_the_sweep(h8_swept, solver, capsys):
    be, ebe_oneshot, frags, ref = h8_swept[solver]
    g, G = be.compute_energy_full(approx_cumulant=False, use_full_rdm=True, return_rdm=True)
    e = be.e_full
    print(f"{solver}: EKapprox {e['EKapprox']:.12f} (restatement {ref['EKapprox']:.12f}), EKtrue {e['EKtrue']:.12f} ({ref['EKtrue']:.12f}), oneshot {ebe_oneshot:.12f}")
    assert abs(e["EKapprox"] - ref["EKapprox"]) < TOL and abs(e["EKtrue"] - ref["EKtrue"]) < TOL and abs(e["E2"] - ref["E2"]) < TOL
    assert be.ebe_tot == e["EKtrue"]
    assert np.abs(g - ref["rdm1"]).max() < TOL and np.abs(G - ref["RDM2_full"]).max() < TOL
    out = capsys.readouterr().out
    assert " E_BE = E_HF + Tr(F del g) + Tr(V K_approx)" in out and " Tr(V K_true)    :" in out and " E(g+G)          :" in out
    # the fragment energy sum of the sweep and the full-basis expression are the same quantity with centre weights 1
    assert abs(ref["EKapprox"] - ebe_oneshot) < TOL, (ref["EKapprox"], ebe_oneshot)
    assert abs(e["EKapprox"] - ebe_oneshot) < TOL
    assert be.compute_energy_full(approx_cumulant=True, return_rdm=False) is None
    assert be.ebe_tot == be.e_full["EKapprox"] and abs(be.ebe_tot - ref["EKapprox"]) < TOL


def test_be_level_entry_points_need_a_sweep_and_an_unrelaxed_solve(hlib):
    be = _h8(hlib)
    with pytest.raises(RuntimeError, match="run oneshot"):
        be.rdm12_fullbasis()
    with pytest.raises(RuntimeError, match="run oneshot"):
        be.compute_energy_full()
    from quemb_amd.fragsolver import default_opts
    for f in be.Fobjs:
        f.solve(opts=default_opts(hlib, relax_density=1), eeval=False, relax_density=True)
    with pytest.raises(NotImplementedError, match="relaxed"):
        be.rdm12_fullbasis()
    with pytest.raises(NotImplementedError, match="relaxed"):
        be.compute_energy_full()


def test_full_basis_memory_guard_names_N(h8_swept):
    from quemb_amd._lib import QEMB_ERR_ALLOC, QembError
    be = h8_swept["CCSD"][0]
    N = be.C.shape[0]
    be.rdm2_mem_limit = 8 * N ** 4 + 8      # the accumulator fits, its workspace does not
    try:
        with pytest.raises(QembError, match=f"N = {N}") as ei:
            be.rdm12_fullbasis()
        assert ei.value.status == QEMB_ERR_ALLOC
        with pytest.raises(QembError, match=f"N = {N}"):
            be.compute_energy_full()
    finally:
        be.rdm2_mem_limit = None
    assert be.rdm12_fullbasis()[1].shape == (N,) * 4


def _worker_full(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    root = Path(__file__).resolve().parent.parent
    for p in (root, root / "tests", root / "tests" / "hostcheck", root / "oracle"):
        sys.path.insert(0, str(p))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import build as hc_build
    from quemb_amd import _lib
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    mol = Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
    mf = RHF(mol); mf.kernel()
    be = BE(mf, FragPart.from_json(root / "tests" / "golden" / "fragmentation.json", "test_autogen_h_linear_be2"), lib=lib, distribute=True)
    assert be.world == world and len(be.my_frags) < len(be.Fobjs)
    be.oneshot(solver="CCSD")
    g, G = be.compute_energy_full(use_full_rdm=True)
    q.put((rank, dict(be.e_full), g, G))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_compute_energy_full_equals_single_process(h8_swept):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_full, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=500) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    be = h8_swept["CCSD"][0]
    g1, G1 = be.compute_energy_full(use_full_rdm=True)
    for rank, e, g, G in res:
        for k in ("EKapprox", "EKtrue", "E2"):
            assert abs(e[k] - be.e_full[k]) < 1e-11, (k, e[k], be.e_full[k])
        assert np.abs(g - g1).max() < 1e-11 and np.abs(G - G1).max() < 1e-11
