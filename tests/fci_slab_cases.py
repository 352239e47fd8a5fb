"""The cases of the slabbed solver="FCI-hip" (DeviceFragment.set_fci_slab: the work matrices D and G in slabs of `rows` alpha strings) that
tests/test_fci_slab_hostlogic.py (scalar mock device, CPU) and tests/test_gpu_fci_slab.py (MI355X) both run: every function takes the library to drive.
Inputs, the NumPy twin and the bars are those of tests/fci_cases.py for the unslabbed solver -- 1e-8 absolute for energies, densities and fragment energies,
1e-7 for the vector, 1e-11 relative for one application of H, 1e-12 for the RDMs of a handed-in vector -- and every slabbed result is held to them twice:
against the twin and against the unslabbed solve of the same fragment.  Slabbing changes the order of the additions into sigma, so the Davidson paths may differ in
the last bits: bit identity is asked only between two runs at one slab height."""
from functools import lru_cache
from math import comb

import numpy as np
import pytest

import fci_cases as fc
import fci_numpy as fnp
import fci_pipeline as fp
from qemb_oracle import be, eri

TOL = fc.TOL
# (n, nsocc): ns = 6; ns = 20; ns = 35, an odd count no slab height divides; ns = 70 (4900 determinants: more than one workgroup per slab); one electron per
# spin; nearly full (ns = 5, almost every link diagonal)
SHAPES = [(4, 2), (6, 3), (7, 3), (8, 4), (6, 1), (5, 4)]
DENSE_MAX = 1225      # determinants up to which the twin's brute-force matrix is diagonalised ((7,3), as tests/fci_cases.py); beyond: its operator form


def slab_heights(n, o):
    """1 and ns - 1 (an off-by-one in the range test or the column offset), 2 and 3 (a ragged last slab wherever they do not divide ns), ns and ns + 5 (one slab)"""
    ns = comb(n, o)
    return sorted({1, 2, 3, ns - 1, ns, ns + 5})


CASES = [(n, o, r) for n, o in SHAPES for r in slab_heights(n, o)]
# the collapse of the Davidson basis: unslabbed, two rows per slab, one slab of ns rows
COLLAPSE = [(n, o, r) for n, o in [(4, 2), (6, 3), (7, 3)] for r in (0, 2, comb(n, o))]


def solve(lib, n, o, rows, fci_opts=None):
    """the solve of fc.solved with the slab height set first; slab_used as reported after the solve and after each 2-RDM"""
    h = fc.inputs(n, o)[0]
    fr = fc.fragment(lib, n, o)
    fr.set_fci_slab(rows)
    out = fr.solve_fci(o, h, opts=fc.scf_opts(lib), fci_opts=fci_opts, eeval=True, want_civec=True)
    out["slab_used"] = fr.fci_slab_used()
    out["dm2"] = fr.make_rdm2("FCI-hip", with_dm1=True)
    out["slab_used_rdm2"] = fr.fci_slab_used()
    out["dm2_cumulant"] = fr.make_rdm2("FCI-hip", with_dm1=False)
    fr.free()
    return out


@lru_cache(maxsize=None)
def unslabbed(lib, n, o):
    """the unslabbed solve of the shape (computed once per library, shared with the cases of tests/fci_cases.py) and the twin's Hamiltonian in its orbitals"""
    out = fc.solved(lib, n, o)[0]
    h, e1 = fc.inputs(n, o)[:2]
    C = out["mo_coeff"]
    ref = dict(h=C.T @ h @ C, V=fnp.mo_eri(e1, C))
    if comb(n, o) ** 2 <= DENSE_MAX:
        ref["e"], ref["c"], _ = fnp.ground_state(ref["h"], ref["V"], o)
    return out, ref


def check_against_twin(out, ref, n, o):
    """the assertions of fc.check_solve on a slabbed result: residual, Rayleigh quotient, eigenpair (where the dense twin exists), densities, fragment energies"""
    h, e1, Bp, h1, veff0, veff = fc.inputs(n, o)
    nf, cen = fc.sites(n)
    C, c = out["mo_coeff"], out["civec"]
    errs = {}
    assert out["residual"] <= 1e-9, out["residual"]
    assert abs(np.linalg.norm(c) - 1.0) < 1e-12 and c.reshape(-1)[np.argmax(np.abs(c))] > 0
    sg = fnp.sigma(ref["h"], ref["V"], c, o)
    errs["residual_numpy"] = np.linalg.norm(sg - out["e_fci"] * c)
    assert errs["residual_numpy"] <= 1e-9 + 1e-11 * np.abs(sg).max(), errs
    errs["rayleigh"] = abs(float(np.vdot(c, sg)) - out["e_fci"])
    assert errs["rayleigh"] < TOL and out["e_fci"] < out["e_scf"]
    cref = ref.get("c", c)      # operator form only beyond DENSE_MAX: the densities of the returned vector, which the residual pins
    if "e" in ref:
        errs["e"], errs["civec"] = abs(out["e_fci"] - ref["e"]), np.abs(c - ref["c"]).max()
        assert errs["e"] < TOL and errs["civec"] < 1e-7, errs
    dm1, dm2 = fnp.rdm12(cref, n, o)
    cum = dm2 - fnp.mean_field_part(dm1, o)
    e_frag = np.array(be.get_frag_energy(C, o, nf, (fc.WEIGHT, cen), np.zeros((n, n)), h1, dm1, cum, eri.pack_s4(e1), veff0, veff, True))
    errs["dm1"] = np.abs(out["rdm1_mo"] - dm1).max()
    errs["dm2"] = np.abs(out["dm2"] - dm2).max()
    errs["dm2_cumulant"] = np.abs(out["dm2_cumulant"] - cum).max()
    errs["rdm1_emb"] = np.abs(out["rdm1_emb"] - 0.5 * C @ dm1 @ C.T).max()
    errs["e_frag"] = np.abs(out["e_frag"] - e_frag).max()
    errs["e_from_rdms"] = abs(fnp.energy_from_rdms(ref["h"], ref["V"], out["rdm1_mo"], out["dm2"]) - out["e_fci"])
    assert max(errs[k] for k in ("dm1", "dm2", "dm2_cumulant", "rdm1_emb", "e_frag", "e_from_rdms")) < TOL, errs
    assert abs(np.trace(out["rdm1_mo"]) - 2 * o) < 1e-10
    return errs


def check_against_unslabbed(out, base):
    errs = {k: float(np.abs(np.asarray(out[k]) - np.asarray(base[k])).max()) for k in ("e_fci", "civec", "rdm1_mo", "dm2", "dm2_cumulant", "e_frag")}
    assert errs["civec"] < 1e-7 and max(v for k, v in errs.items() if k != "civec") < TOL, errs
    return errs


def check_slab_equals_unslabbed_and_twin(lib, n, o, rows):
    base, ref = unslabbed(lib, n, o)
    out = solve(lib, n, o, rows)
    ns = comb(n, o)
    want = (min(rows, ns), -(-ns // min(rows, ns)))
    assert out["slab_used"] == want and out["slab_used_rdm2"] == want, (out["slab_used"], out["slab_used_rdm2"], want)
    assert np.array_equal(out["mo_coeff"], base["mo_coeff"])      # the fragment RHF is not touched: one twin Hamiltonian serves every slab height
    a = check_against_twin(out, ref, n, o)
    b = check_against_unslabbed(out, base)
    print(f"slab ({n},{o}) rows = {rows} ({want[1]} slabs): n_iter = {out['n_iter']} (unslabbed {base['n_iter']}) residual = {out['residual']:.2e}; twin: "
          + " ".join(f"{k}={v:.2e}" for k, v in a.items()) + "; unslabbed: " + " ".join(f"{k}={v:.2e}" for k, v in b.items()))


def check_collapse(lib, n, o, rows):
    """max_space = 2: the basis collapses to the Ritz vector (and its image) after every second application of H -- the default max_space = 12 never gets there,
    every solve of these files converges in 6 to 8 applications.  The collapsed solve is held to the twin and to the default-options solve at the bars above;
    n_iter > max_space says the collapse ran."""
    from quemb_amd.fragsolver import default_fci_opts
    base, ref = unslabbed(lib, n, o)
    fo = default_fci_opts(lib, max_space=2, max_cycle=400)
    out = solve(lib, n, o, rows, fci_opts=fo)      # (strict convergence is the default: a solve that did not converge raises)
    ns = comb(n, o)
    assert out["slab_used"] == ((rows, -(-ns // rows)) if rows else (0, 1))
    assert out["residual"] <= fo.conv_tol and fo.max_space < out["n_iter"] <= fo.max_cycle, (out["residual"], out["n_iter"])
    a = check_against_twin(out, ref, n, o)
    b = check_against_unslabbed(out, base)
    print(f"collapse ({n},{o}) rows = {rows}: n_iter = {out['n_iter']} (max_space = 12: {base['n_iter']}) residual = {out['residual']:.2e}; twin: "
          + " ".join(f"{k}={v:.2e}" for k, v in a.items()) + "; default options: " + " ".join(f"{k}={v:.2e}" for k, v in b.items()))


def check_ops(lib, n, o):
    """one application of H and the RDM build on handed-in data, slab by slab, at the bars of fc.check_sigma and fc.check_rdm_op; one slab (rows >= ns) is the
    whole space bit for bit: the same code"""
    from quemb_amd.fragsolver import fci_rdm12, fci_sigma
    h, e1 = fc.inputs(n, o)[:2]
    ns = comb(n, o)
    c = np.random.default_rng(n * 100 + o).standard_normal((ns, ns))
    ref = fnp.sigma(h, e1, c, o)
    cn = c / np.linalg.norm(c)
    r1, r2 = fnp.rdm12(cn, n, o)
    whole = fci_sigma(h, e1, c, o, lib=lib), fci_rdm12(cn, n, o, lib=lib), fci_rdm12(cn, n, o, cumulant=True, lib=lib)
    for rows in (ns, ns + 5):
        assert np.array_equal(fci_sigma(h, e1, c, o, lib=lib, slab_rows=rows), whole[0]), rows
        for cumulant in (False, True):
            dm1, dm2 = fci_rdm12(cn, n, o, cumulant=cumulant, lib=lib, slab_rows=rows)
            assert np.array_equal(dm1, whole[1 + cumulant][0]) and np.array_equal(dm2, whole[1 + cumulant][1]), (rows, cumulant)
    for rows in slab_heights(n, o):
        s = fci_sigma(h, e1, c, o, lib=lib, slab_rows=rows)
        print(f"sigma ({n},{o}) rows = {rows}: max |d| = {np.abs(s - ref).max():.2e}, max |sigma| = {np.abs(ref).max():.2e}")
        assert np.abs(s - ref).max() <= 1e-11 * np.abs(ref).max(), rows
        assert np.array_equal(s, fci_sigma(h, e1, c, o, lib=lib, slab_rows=rows))      # for one slab height two calls give the same bits
        dm1, dm2 = fci_rdm12(cn, n, o, lib=lib, slab_rows=rows)
        assert np.abs(dm1 - r1).max() < 1e-12 and np.abs(dm2 - r2).max() < 1e-12, rows
        _, cum = fci_rdm12(cn, n, o, cumulant=True, lib=lib, slab_rows=rows)
        assert np.abs(cum - (r2 - fnp.mean_field_part(r1, o))).max() < 1e-12, rows


def check_deterministic(lib):
    """two slabbed solves at (8, 4) with rows = 3 (23 slabs and a ragged last one): the same bits"""
    a, b = solve(lib, 8, 4, 3), solve(lib, 8, 4, 3)
    assert a["slab_used"] == (3, 24) and a["n_iter"] == b["n_iter"]
    for k in ("e_fci", "civec", "dm2", "dm2_cumulant", "rdm1_mo", "e_frag", "residual"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def check_guard(lib):
    import ctypes as C

    from quemb_amd import _lib
    from quemb_amd._lib import QembError
    from quemb_amd.solver import fragment_work_bytes
    n, o = 6, 3
    ns = comb(n, o)
    h = fc.inputs(n, o)[0]
    nb = C.c_int64()

    def slab_bytes(rows, n=n, o=o):
        assert lib.qemb_frag_fci_bytes_slab(n, o, 12, rows, C.byref(nb)) == 0
        return nb.value
    assert lib.qemb_frag_fci_bytes(n, o, 12, C.byref(nb)) == 0
    whole = nb.value
    one_row = slab_bytes(1)
    # the figure: D and G at 2 x 8 n^2 rows ns, everything else as qemb_frag_fci_bytes; rows = 0 and rows >= ns are the whole space
    assert slab_bytes(0) == whole == slab_bytes(ns) == slab_bytes(ns + 5) and one_row < slab_bytes(2) < whole
    assert whole - one_row == 16 * n * n * ns * (ns - 1)
    for nn, oo in [(6, 3), (7, 3), (12, 6), (16, 8)]:
        for rows in (0, 1, 2, 7, comb(nn, oo) - 1, comb(nn, oo), comb(nn, oo) + 5):
            assert slab_bytes(rows, nn, oo) == int(fragment_work_bytes(nn, oo, solver="FCI-hip", slab_rows=rows)), (nn, oo, rows)
    assert slab_bytes(1, 16, 8) < 100e9 < slab_bytes(0, 16, 8)      # what the slabs are for: (16, 8) no longer needs 678 GB of D and G
    assert lib.qemb_frag_fci_bytes_slab(17, 8, 12, 1, C.byref(nb)) == _lib.QEMB_ERR_UNSUPPORTED
    assert lib.qemb_frag_fci_bytes_slab(n, o, 12, -1, C.byref(nb)) == _lib.QEMB_ERR_ARG
    base = unslabbed(lib, n, o)[0]
    fr = fc.fragment(lib, n, o)
    assert fr.fci_slab_used() == (0, 1)
    # a limit between the one-row figure and the whole: off refuses as before, automatic solves in slabs
    fr.set_fci_mem_limit((one_row + whole) // 2)
    with pytest.raises(QembError, match=r"n = 6, nsocc = 3 .*N_det = 400") as ei:
        fr.solve_fci(o, h)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC and "rows" not in str(ei.value)
    fr.set_fci_slab(-1)
    out = fr.solve_fci(o, h, opts=fc.scf_opts(lib), want_civec=True)
    rows, n_slab = fr.fci_slab_used()
    assert n_slab > 1 and 1 <= rows < ns and n_slab == -(-ns // rows)
    assert slab_bytes(rows) <= (one_row + whole) // 2 < slab_bytes(rows + 1)      # the largest height that fits
    assert abs(out["e_fci"] - base["e_fci"]) < TOL and np.abs(out["civec"] - base["civec"]).max() < 1e-7 and np.abs(out["e_frag"] - base["e_frag"]).max() < TOL
    # below the one-row figure nothing fits
    fr.set_fci_mem_limit(one_row - 1)
    with pytest.raises(QembError, match=r"n = 6, nsocc = 3 .*N_det = 400 .*rows = 1 .*20 slabs") as ei:
        fr.solve_fci(o, h)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    # a given height is held to the same limit; with room, automatic is the unslabbed path
    fr.set_fci_mem_limit(slab_bytes(4) - 1)
    fr.set_fci_slab(4)
    with pytest.raises(QembError, match=r"rows = 4 .*5 slabs") as ei:
        fr.solve_fci(o, h)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    fr.set_fci_slab(3)
    fr.solve_fci(o, h)
    assert fr.fci_slab_used() == (3, 7)
    fr.set_fci_mem_limit(-1)
    fr.set_fci_slab(-1)
    out = fr.solve_fci(o, h, opts=fc.scf_opts(lib), want_civec=True)
    assert fr.fci_slab_used() == (0, 1) and np.array_equal(out["civec"], base["civec"]) and out["e_fci"] == base["e_fci"]
    # any other negative value
    with pytest.raises(QembError, match="rows = -2") as ei:
        fr.set_fci_slab(-2)
    assert ei.value.status == _lib.QEMB_ERR_ARG
    assert fr.fci_slab_used() == (0, 1)
    # n > 16 stays unsupported whatever the slab height
    fr.free()
    from quemb_amd.fragsolver import DeviceFragment
    fr = DeviceFragment(17, 2, lib=lib)
    fr.set_fci_slab(1)
    with pytest.raises(QembError, match="n = 17") as ei:
        fr.solve_fci(8, np.zeros((17, 17)), eeval=False)
    assert ei.value.status == _lib.QEMB_ERR_UNSUPPORTED
    fr.free()


def check_solve_fci_function(lib):
    from quemb_amd.solver import solve_fci
    n, o = 5, 3
    h, e1 = fc.inputs(n, o)[:2]
    e_a, c_a, dm1_a, dm2_a = solve_fci(h, eri.pack_s4(e1), o, rdm_return=True, rdm2_return=True, lib=lib)
    e_b, c_b, dm1_b, dm2_b = solve_fci(h, eri.pack_s4(e1), o, rdm_return=True, rdm2_return=True, lib=lib, slab_rows=3)
    assert abs(e_a - e_b) < TOL and np.abs(c_a - c_b).max() < 1e-7 and np.abs(dm1_a - dm1_b).max() < TOL and np.abs(dm2_a - dm2_b).max() < TOL
    with pytest.raises(ValueError, match="Solver not implemented"):
        from quemb_amd.solver import fragment_work_bytes
        fragment_work_bytes(6, 3, solver="FCI", slab_rows=2)      # the bare literal stays refused


def check_driver(lib):
    """H8 / STO-3G BE2 (fragments of six embedding orbitals, ns = 20): BE(fci_slab_rows=2) -- ten slabs per application of H -- against the default to 1e-10 Eh,
    the project's bar between equivalent routes; the full-basis energies run on it; the other solvers do not read the setting"""
    key = "test_autogen_h_linear_be2"
    a, b = fp.h_chain(lib, 8, key), fp.h_chain(lib, 8, key, fci_slab_rows=2)
    ea, ca = a.oneshot(solver="FCI-hip")
    eb, cb = b.oneshot(solver="FCI-hip")
    used_a, used_b = [f.dev.fci_slab_used() for f in a.Fobjs], [f.dev.fci_slab_used() for f in b.Fobjs]
    print(f"H8 BE2 oneshot: default {ea:.12f}, fci_slab_rows = 2 {eb:.12f} (slabs used {used_b})")
    assert all(u == (0, 1) for u in used_a) and all(u[0] == 2 and u[1] == -(-comb(f.nao, f.nsocc) // 2) and u[1] > 1 for u, f in zip(used_b, b.Fobjs))
    assert abs(ea - eb) < 1e-10 and np.abs(np.asarray(ca) - np.asarray(cb)).max() < 1e-10
    a.compute_energy_full(approx_cumulant=False, use_full_rdm=True, return_rdm=False)
    b.compute_energy_full(approx_cumulant=False, use_full_rdm=True, return_rdm=False)
    assert all(f.dev.fci_slab_used()[0] == 2 for f in b.Fobjs)      # the fragments' 2-RDMs went slab by slab too
    for k in ("EKapprox", "EKtrue"):
        assert abs(a.e_full[k] - b.e_full[k]) < 1e-10, (k, a.e_full[k], b.e_full[k])
    for x, y in zip(a.rdm12_fullbasis(), b.rdm12_fullbasis()):
        assert np.abs(x - y).max() < TOL
    a2, b2 = fp.h_chain(lib, 8, key), fp.h_chain(lib, 8, key, fci_slab_rows=2)
    oa = a2.optimize(solver="FCI-hip", only_chem=False, conv_tol=1e-7)
    ob = b2.optimize(solver="FCI-hip", only_chem=False, conv_tol=1e-7)
    print(f"H8 BE2 optimize: default {a2.ebe_tot:.12f} in {oa.iter} iterations, fci_slab_rows = 2 {b2.ebe_tot:.12f} in {ob.iter}")
    assert oa.err < 1e-7 and ob.err < 1e-7 and abs(a2.ebe_tot - b2.ebe_tot) < 1e-10
    J = fp.h_chain(lib, 8, key, fci_slab_rows=2).compute_numerical_jacobian("FCI-hip", False, 1, step_size=1e-4)
    assert J.shape == (len(a.pot), len(a.pot)) and np.isfinite(J).all() and np.abs(J).max() > 1e-3
    c = fp.h_chain(lib, 8, key, fci_slab_rows=2)
    ec, _ = c.oneshot(solver="CCSD")
    ed, _ = fp.h_chain(lib, 8, key).oneshot(solver="CCSD")
    assert ec == ed
    with pytest.raises(ValueError, match="fci_slab_rows"):
        fp.h_chain(lib, 8, key, fci_slab_rows=-2)
    with pytest.raises(ValueError, match="Solver not implemented"):
        b.oneshot(solver="FCI")
