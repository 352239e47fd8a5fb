"""solver="FCI-hip" above the single fragment: refusals, the Frags / solver / BE layers on H4 and H8 / STO-3G and the reference's golden energies.  Shared by
tests/test_fci_hostlogic.py (mock device) and tests/test_gpu_fci.py (MI355X); every function takes the library to drive."""
import warnings

import numpy as np
import pytest

import fci_cases as fc
import fci_numpy as fnp
from helpers import GOLDEN
from qemb_oracle import be as obe
from qemb_oracle import eri

TOL = 1e-8
# tests/molbe_h8_test.py:54-78 of the reference (H8 chain, 1 Angstrom, STO-3G, solver="FCI"): ebe_tot - ebe_hf; its bar is np.isclose: 1e-8 + 1e-5 |value|
GOLDEN_H8 = {("be1", True): -0.12831444938462155, ("be2", True): -0.1343968038684169, ("be2", False): -0.1343036698277933,
             ("be3", True): -0.1332017928466369, ("be3", False): -0.1332017928466369}


def h_chain(lib, natom, key=None, fobj=None, **kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    mol = Mole([["H", (0.0, 0.0, float(i))] for i in range(natom)])
    mf = RHF(mol); mf.kernel()
    if fobj is None:
        fobj = FragPart.from_json(GOLDEN / "fragmentation.json", key, n_BE=int(key[-1]))
    return BE(mf, fobj, lib=lib, distribute=False, **kw)


def check_refusals(lib):
    from quemb_amd import _lib
    from quemb_amd._lib import FciOpts, QembError
    from quemb_amd.fragsolver import DeviceFragment, default_fci_opts, default_opts, rdm2_from_amplitudes
    from quemb_amd.pfrag import Frags
    from quemb_amd.solver import be_func, fragment_work_bytes, solve_fragments
    # n = 17: beyond the cap, before anything is allocated (no ERIs are needed to be told so)
    fr = DeviceFragment(17, 2, lib=lib)
    with pytest.raises(QembError, match="n = 17") as ei:
        fr.solve_fci(8, np.zeros((17, 17)), eeval=False)
    assert ei.value.status == _lib.QEMB_ERR_UNSUPPORTED
    fr.free()
    n, o = 6, 3
    h = fc.inputs(n, o)[0]
    # the memory limit
    fr = fc.fragment(lib, n, o)
    fr.set_fci_mem_limit(1 << 16)
    with pytest.raises(QembError, match=r"n = 6, nsocc = 3 .*N_det = 400") as ei:
        fr.solve_fci(o, h)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    fr.set_fci_mem_limit(-1)
    import ctypes as C
    nb = C.c_int64()
    assert lib.qemb_frag_fci_bytes(n, o, 12, C.byref(nb)) == 0
    assert nb.value >= 8 * (2 * 36 * 400 + 28 * 400) and nb.value == int(fragment_work_bytes(n, o, solver="FCI-hip"))
    assert lib.qemb_frag_fci_bytes(17, 8, 12, C.byref(nb)) == _lib.QEMB_ERR_UNSUPPORTED
    # one application of H is not enough on (6,3): an error under strict convergence, results and a warning otherwise
    one = default_fci_opts(lib, max_cycle=1)
    with pytest.raises(QembError, match="did not converge") as ei:
        fr.solve_fci(o, h, fci_opts=one)
    assert ei.value.status == _lib.QEMB_ERR_NOCONV
    with pytest.raises(QembError, match="no solve has run"):
        fr.make_rdm2("FCI-hip")                                     # the failed solve left nothing to form it from
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fr.solve_fci(o, h, opts=default_opts(lib, strict_convergence=0), fci_opts=one, want_civec=True)
    assert any(issubclass(w.category, _lib.ConvergenceWarning) for w in rec)
    assert out["n_iter"] == 1 and out["residual"] > 1e-9 and abs(np.linalg.norm(out["civec"]) - 1.0) < 1e-12 and np.isfinite(out["e_frag"]).all()
    # a struct of another size
    bad = default_fci_opts(lib)
    bad.struct_size = 8
    with pytest.raises(QembError, match="struct_size") as ei:
        fr.solve_fci(o, h, fci_opts=bad)
    assert ei.value.status == _lib.QEMB_ERR_ARG
    assert C.sizeof(FciOpts) == default_fci_opts(lib).struct_size
    # the 2-RDM of another kind of solve, or after new ERIs
    fr.solve(o, h, eeval=False)
    with pytest.raises(QembError, match="the last solve of this fragment was CCSD") as ei:
        fr.make_rdm2("FCI-hip")
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.solve_fci(o, h)
    with pytest.raises(QembError, match="the last solve of this fragment was FCI"):
        fr.make_rdm2("CCSD")
    assert fr.make_rdm2("FCI-hip").shape == (n,) * 4
    fr.set_eri_s4(eri.pack_s4(fc.inputs(n, o)[1]))
    with pytest.raises(QembError, match="no solve has run") as ei:
        fr.make_rdm2("FCI-hip")
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.free()
    # the bare literals stay refused everywhere
    f = Frags([0, 1], 0, [], [], [], [], (1.0, [0]), [0], lib=lib)
    for bad_name in ("FCI", "SCI", "mp2"):
        for call in (lambda: f.solve(solver=bad_name), lambda: be_func(None, [f], 1, bad_name, 0.0), lambda: solve_fragments(None, [f], solver=bad_name),
                     lambda: fragment_work_bytes(6, 3, solver=bad_name), lambda: fr.make_rdm2(bad_name),
                     lambda: rdm2_from_amplitudes(np.zeros((1, 1)), np.zeros((1, 1, 1, 1)), kind=bad_name)):
            with pytest.raises(ValueError, match="Solver not implemented"):
                call()
    with pytest.raises(ValueError, match="Solver not implemented"):
        rdm2_from_amplitudes(np.zeros((1, 1)), np.zeros((1, 1, 1, 1)), kind="FCI-hip")      # an FCI 2-RDM comes from a vector


def check_frags_energy(lib):
    """Frags.solve(solver="FCI-hip"): use_cumulant=True contracts the cumulant on the device, use_cumulant=False is the reference's literal expression with the
    full make_rdm2"""
    from quemb_amd.pfrag import Frags
    n, o = 5, 2
    h, e1, Bp, h1, veff0, veff = fc.inputs(n, o)
    nf, cen = fc.sites(n)
    f = Frags(list(range(nf)), 0, [], [], [], [], (fc.WEIGHT, cen), cen, lib=lib)
    f.dev = fc.fragment(lib, n, o)
    f.nao, f.nsocc, f.h1, f.veff0, f.veff, f.fock, f.heff, f.dm0 = n, o, h1, veff0, veff, h, np.zeros((n, n)), None
    for cumulant in (True, False):
        out = f.solve(eeval=True, use_cumulant=cumulant, want_t2=True, relax_density=True, solver="FCI-hip", opts=fc.scf_opts(lib))      # (relax_density is not read)
        C = out["mo_coeff"]
        dm1, dm2 = fnp.rdm12(out["civec"], n, o)
        r2 = dm2 - fnp.mean_field_part(dm1, o) if cumulant else dm2
        ref = obe.get_frag_energy(C, o, nf, (fc.WEIGHT, cen), np.zeros((n, n)), h1, dm1, r2, eri.pack_s4(e1), veff0, veff, cumulant)
        assert np.abs(np.asarray(out["e_frag"]) - np.asarray(ref)).max() < TOL, (cumulant, out["e_frag"], ref)
        assert f.t1 is None and f.t2 is None and f._rdm1 is out["rdm1_emb"] and f._solver == "FCI-hip"
        assert np.abs(f.make_rdm2(with_dm1=not cumulant) - r2).max() < TOL


def check_solve_fci_function(lib):
    from quemb_amd.solver import solve_fci
    n, o = 5, 3
    h, e1, Bp = fc.inputs(n, o)[:3]
    e_a, c_a, dm1, mo = solve_fci(h, eri.pack_s4(e1), o, rdm_return=True, lib=lib)
    e_b, c_b, dm2 = solve_fci(h, None, o, df_factor=Bp, rdm2_return=True, use_cumulant=False, lib=lib)
    E, c, _ = fnp.ground_state(mo.T @ h @ mo, fnp.mo_eri(e1, mo), o)
    assert abs(e_a - E) < TOL and abs(e_b - E) < TOL and np.abs(c_a - c).max() < 1e-7 and dm2.shape == (n,) * 4
    assert np.abs(dm1 - fnp.rdm12(c, n, o)[0]).max() < TOL


def check_h8_be1_equals_ccsd(lib):
    """H8 BE1: two-electron fragments with n = 2, where CCSD is exact.  The sweep's default CCSD density is the reference's unrelaxed approximant
    [[2 I, t1], [t1^T, 0]] (shared/external/ccsd_rdm.py:10-20), which is not the exact 1-RDM even for two electrons: there only the correlation energy of the
    embedding problem agrees.  The exact CCSD densities are the response ones (relax_density: Lambda equations), and with them both energies and every _rdm1
    agree with FCI-hip at the same bar."""
    from quemb_amd.fragsolver import default_opts
    from quemb_amd.solver import be_func, solve_fragments
    tight = default_opts(lib, cc_conv_tol=1e-12, cc_conv_tol_normt=1e-10, lambda_conv_tol=1e-10)
    be_f, be_c = h_chain(lib, 8, "test_autogen_h_linear_be1"), h_chain(lib, 8, "test_autogen_h_linear_be1", solver_opts=tight)
    ef, cf = be_f.oneshot(solver="FCI-hip")
    assert all(f.nao == 2 and f.nsocc == 1 for f in be_f.Fobjs)
    ec, cc = be_func(None, be_c.Fobjs, be_c.Nocc, "CCSD", be_c.enuc, eeval=True, relax_density=True, opts=tight)
    print(f"H8 BE1 oneshot: FCI-hip {ef:.12f} {np.asarray(cf)}, CCSD (response densities) {ec:.12f} {np.asarray(cc)}")
    assert abs(ef - ec) < TOL and np.abs(np.asarray(cf) - np.asarray(cc)).max() < TOL
    assert abs(be_f.ebe_hf - be_c.ebe_hf) < 1e-12
    for a, b in zip(be_f.Fobjs, be_c.Fobjs):
        assert np.abs(a._rdm1 - b._rdm1).max() < TOL
    fci = solve_fragments(None, be_f.Fobjs, eeval=True, solver="FCI-hip")
    ccsd = solve_fragments(None, be_c.Fobjs, eeval=True, solver="CCSD", opts=tight)      # unrelaxed: the energy of the embedding problem alone
    for a, b in zip(fci, ccsd):
        assert abs(a["e_corr_mo"] - b["e_corr_mo"]) < TOL


def check_h4_whole_system(lib):
    """H4 as one fragment that is the whole system: the BE correlation energy is the molecule's FCI correlation energy (36 determinants, brute force)"""
    from quemb_amd.fragpart import FragPart
    fobj = FragPart(AO_per_frag=[[0, 1, 2, 3]], AO_per_edge_per_frag=[[]], ref_frag_idx_per_edge_per_frag=[[]], relAO_per_origin_per_frag=[[0, 1, 2, 3]],
                    weight_and_relAO_per_center_per_frag=[(1.0, [0, 1, 2, 3])], n_BE=1)
    be = h_chain(lib, 4, fobj=fobj)
    ecorr, _ = be.oneshot(solver="FCI-hip")
    Cm = be.C
    E = fnp.ground_state(Cm.T @ be.hcore @ Cm, fnp.mo_eri(np.asarray(be.mf._eri).reshape((4,) * 4), Cm), 2)[0]
    ref = E + be.enuc - be.hf_etot
    print(f"H4 whole system: BE E_corr = {ecorr:.12f}, molecular FCI E_corr = {ref:.12f}")
    assert abs(ecorr - ref) < TOL and ref < -1e-3


def check_h8_be2(lib):
    import rdm2_numpy as r2n
    from quemb_amd.solver import be_func
    be = h_chain(lib, 8, "test_autogen_h_linear_be2")
    ecorr, comps = be.oneshot(solver="FCI-hip")
    assert ecorr < 0 and abs(be.ebe_tot - (ecorr + be.ebe_hf)) < 1e-14 and all(f._solver == "FCI-hip" and f.t1 is None for f in be.Fobjs)
    # the fragment energies of the sweep against the oracle's get_frag_energy fed with the reference RDMs of the returned orbitals
    tot = np.zeros(3)
    for f in be.Fobjs:
        e1 = eri.restore_s1(f.dev.get_eri_s4(), f.nao)
        C = f.mo_coeffs
        _, c, _ = fnp.ground_state(C.T @ (f.fock + f.heff) @ C, fnp.mo_eri(e1, C), f.nsocc)
        dm1, dm2 = fnp.rdm12(c, f.nao, f.nsocc)
        w, cen = f.weight_and_relAO_per_center
        tot += np.array(obe.get_frag_energy(C, f.nsocc, f.n_frag, (w, cen), f.TA, f.h1, dm1, dm2 - fnp.mean_field_part(dm1, f.nsocc), f.dev.get_eri_s4(), f.veff0, f.veff, True))
    assert np.abs(np.asarray(comps) - tot).max() < TOL, (comps, tot)
    # be_func returns the error vector; lockstep has no batched entry and gives the same numbers
    # (fresh objects: a fragment's second RHF starts its eigensolver from the orbitals of the first, so only equal histories give equal bits)
    ba, bb = h_chain(lib, 8, "test_autogen_h_linear_be2"), h_chain(lib, 8, "test_autogen_h_linear_be2")
    r1 = be_func(list(ba.pot), ba.Fobjs, ba.Nocc, "FCI-hip", ba.enuc, eeval=True, return_vec=True)
    r2 = be_func(list(bb.pot), bb.Fobjs, bb.Nocc, "FCI-hip", bb.enuc, eeval=True, return_vec=True, lockstep=True)
    assert len(r1[1]) == len(be.pot) and r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and abs(r1[2][0] - ecorr) < 1e-12
    # full-basis densities and energies from the fragments' 2-RDMs, as the CCSD cases
    frags, ref = r2n.frags_of(be), r2n.energy_of(be, use_full_rdm=True)
    got = be.rdm12_fullbasis()
    for a, b in zip(got, r2n.rdm12_fullbasis(frags, be.S, be.W, be.C)):
        assert a.shape == b.shape and np.abs(a - b).max() < TOL
    be.compute_energy_full(approx_cumulant=False, use_full_rdm=True, return_rdm=False)
    e = be.e_full
    assert abs(e["EKapprox"] - ref["EKapprox"]) < TOL and abs(e["EKtrue"] - ref["EKtrue"]) < TOL and abs(ref["EKapprox"] - (ecorr + be.ebe_hf)) < TOL
    # density matching converges; the numerical Jacobian is finite
    be2 = h_chain(lib, 8, "test_autogen_h_linear_be2")
    opt = be2.optimize(solver="FCI-hip", only_chem=False, conv_tol=1e-7)
    assert opt.err < 1e-7 and opt.iter < 20
    J = h_chain(lib, 8, "test_autogen_h_linear_be2").compute_numerical_jacobian("FCI-hip", False, 1, step_size=1e-4)
    assert J.shape == (len(be.pot), len(be.pot)) and np.isfinite(J).all() and np.abs(J).max() > 1e-3
    # ... and on BE1 (two-electron fragments: CCSD exact) it is the CCSD one, taken with the exact (response) CCSD densities -- see check_h8_be1_equals_ccsd --, up to
    # the step-size error of a central difference, O(step^2) = 1e-8 times third derivatives of O(1), plus the solvers' convergence (1e-8 in the densities)
    # divided by the step: 1e-4
    step = 1e-4
    Jf = h_chain(lib, 8, "test_autogen_h_linear_be1").compute_numerical_jacobian("FCI-hip", True, 1, step_size=step)
    bc = h_chain(lib, 8, "test_autogen_h_linear_be1")
    err = [be_func([s_ * step], bc.Fobjs, bc.Nocc, "CCSD", bc.enuc, only_chem=True, relax_density=True, return_vec=True)[1][0] for s_ in (+1.0, -1.0)]
    Jc = (err[0] - err[1]) / (2 * step)
    print(f"H8 BE1 d(err)/d(mu): FCI-hip {Jf[0, 0]:.8f}, CCSD with response densities {Jc:.8f}")
    assert Jf.shape == (1, 1) and abs(Jf[0, 0] - Jc) < 2e-4 * max(1.0, abs(Jc)), (Jf, Jc)
    for bad in ("FCI", "SCI", "mp2"):
        for call in (lambda: be.oneshot(solver=bad), lambda: be.optimize(solver=bad), lambda: be.compute_numerical_jacobian(bad)):
            with pytest.raises(ValueError, match="Solver not implemented"):
                call()


def golden_distance(lib, level, only_chem):
    be = h_chain(lib, 8, f"test_autogen_h_linear_{level}")
    be.optimize(solver="FCI-hip", only_chem=only_chem, conv_tol=1e-8 if only_chem else 1e-7)
    return be.ebe_tot - be.ebe_hf - GOLDEN_H8[(level, only_chem)]


def check_goldens(lib):
    """the reference's stored H8 / STO-3G correlation energies (tests/molbe_h8_test.py) at its own bar, np.isclose: 1e-8 + 1e-5 |value|.  BE1 fragments are one atom
    each under any fragmenter; the stored `autogen` fragmentations of BE2 and BE3 reproduce the reference's `chemgen` values too (measured distances: DESIGN.md),
    so all five are pinned."""
    for (level, only_chem), gold in GOLDEN_H8.items():
        d = golden_distance(lib, level, only_chem)
        print(f"H8 {level} only_chem={only_chem}: E_corr - golden = {d:.3e} (bar {1e-8 + 1e-5 * abs(gold):.2e})")
        assert abs(d) <= 1e-8 + 1e-5 * abs(gold), (level, only_chem, d)
