"""The cases of solver="FCI-hip" that tests/test_fci_hostlogic.py (scalar mock device, CPU) and tests/test_gpu_fci.py (MI355X) both run: every function takes
the library to drive.  Inputs are helpers.synthetic_fragment_factor (gap ~ 2: the error of a converged vector stays near its residual); the reference is
tests/fci_numpy.py, evaluated in the fragment-MO basis of the orbitals the device solve returned.  Bars: 1e-8 absolute for energies, densities and fragment
energies (the project's figure for fragment-vs-oracle comparisons), 1e-7 for the vector, 1e-11 relative for one application of H."""
from functools import lru_cache

import numpy as np

import fci_numpy as fnp
from helpers import synthetic_fragment_factor
from qemb_oracle import be, eri

TOL = 1e-8
# (n, nsocc): no sign changes / two electrons; first signs; particle-hole asymmetry; 400 determinants; many virtuals; a single determinant;
# 1225 determinants (ns = 35 is no multiple of 64, more than one workgroup); 63 504 determinants (the H8 BE3 size, operator form only)
DENSE = [(2, 1), (3, 1), (4, 2), (5, 2), (5, 3), (6, 3), (6, 1), (7, 3)]
SHAPES = DENSE + [(4, 4), (10, 5)]
WEIGHT = 0.75


def sites(n):
    nf = min(n, 3)
    return nf, ([0, nf - 1] if nf > 1 else [0])


@lru_cache(maxsize=None)
def inputs(n, o):
    h, e1, Bp = synthetic_fragment_factor(n, o, 700 + 10 * n + o)
    rng = np.random.default_rng(700 + 10 * n + o + 1)
    sym = lambda: (lambda a: a + a.T)(rng.standard_normal((n, n)))
    return h, e1, Bp, sym(), sym(), sym()


def fragment(lib, n, o, residency="block"):
    from quemb_amd.fragsolver import DeviceFragment
    h, e1, Bp, h1, veff0, veff = inputs(n, o)
    nf, cen = sites(n)
    fr = DeviceFragment(n, nf, lib=lib)
    if residency == "factor":
        fr.set_df_only(Bp)
    else:
        fr.set_eri_s4(eri.pack_s4(e1))
    fr.set_energy_data(h1, veff0, veff, WEIGHT, cen)
    return fr


def scf_opts(lib, **kw):
    from quemb_amd.fragsolver import default_opts
    return default_opts(lib, scf_conv_tol=1e-13, scf_conv_tol_grad=1e-9, **kw)


@lru_cache(maxsize=None)
def solved(lib, n, o):
    """the device solve of a shape (packed block resident) with both 2-RDMs, and its reference in the basis of the returned orbitals; computed once per library"""
    h, e1, Bp, h1, veff0, veff = inputs(n, o)
    nf, cen = sites(n)
    fr = fragment(lib, n, o)
    out = fr.solve_fci(o, h, opts=scf_opts(lib), eeval=True, want_civec=True)
    out["dm2"] = fr.make_rdm2("FCI-hip", with_dm1=True)
    out["dm2_cumulant"] = fr.make_rdm2("FCI-hip", with_dm1=False)
    fr.free()
    C = out["mo_coeff"]
    ref = dict(h=C.T @ h @ C, V=fnp.mo_eri(e1, C))
    if (n, o) in DENSE:
        ref["e"], ref["c"], ref["H"] = fnp.ground_state(ref["h"], ref["V"], o)
    elif o < n:      # operator form only: the reference densities are those of the returned vector, which the residual check pins
        ref["c"] = out["civec"]
    if o < n:
        ref["dm1"], ref["dm2"] = fnp.rdm12(ref["c"], n, o)
    else:
        ref["dm1"] = 2.0 * np.eye(n)
        ref["dm2"] = 4.0 * np.einsum("pq,rs->pqrs", np.eye(n), np.eye(n)) - 2.0 * np.einsum("ps,qr->pqrs", np.eye(n), np.eye(n))
    ref["cum"] = ref["dm2"] - fnp.mean_field_part(ref["dm1"], o)
    ref["e_frag"] = np.array(be.get_frag_energy(C, o, nf, (WEIGHT, cen), np.zeros((n, n)), h1, ref["dm1"], ref["cum"], eri.pack_s4(e1), veff0, veff, True))
    return out, ref


def check_sigma(lib, n, o):
    """one application of H on handed-in integrals against the operator form (and the brute-force matrix where it fits): max |d sigma| <= 1e-11 max |sigma| --
    ten times the accumulated rounding of ~n^4 terms (1.1e-12 at n = 10)"""
    from quemb_amd.fragsolver import fci_sigma
    h, e1 = inputs(n, o)[:2]
    ns = len(fnp.strings(n, o))
    c = np.random.default_rng(n * 100 + o).standard_normal((ns, ns))
    s = fci_sigma(h, e1, c, o, lib=lib)
    ref = fnp.sigma(h, e1, c, o)
    print(f"sigma ({n},{o}): max |d| = {np.abs(s - ref).max():.2e}, max |sigma| = {np.abs(ref).max():.2e}")
    assert np.abs(s - ref).max() <= 1e-11 * np.abs(ref).max()
    if n <= 5:
        assert np.abs(fnp.hamiltonian_matrix(h, e1, o) @ c.reshape(-1) - s.reshape(-1)).max() <= 1e-11 * np.abs(ref).max()


def check_rdm_op(lib, n, o):
    """the RDM build from a handed-in (random, normalised) vector against the operator form"""
    from quemb_amd.fragsolver import fci_rdm12
    ns = len(fnp.strings(n, o))
    c = np.random.default_rng(n * 100 + o + 7).standard_normal((ns, ns))
    c /= np.linalg.norm(c)
    dm1, dm2 = fci_rdm12(c, n, o, lib=lib)
    r1, r2 = fnp.rdm12(c, n, o)
    assert np.abs(dm1 - r1).max() < 1e-12 and np.abs(dm2 - r2).max() < 1e-12
    _, cum = fci_rdm12(c, n, o, cumulant=True, lib=lib)
    assert np.abs(cum - (r2 - fnp.mean_field_part(r1, o))).max() < 1e-12


def check_solve(lib, n, o):
    out, ref = solved(lib, n, o)
    errs = {}
    if o == n:      # a single determinant: the mean-field results
        assert out["e_corr_mo"] == 0.0 and out["e_fci"] == out["e_scf"] and out["n_iter"] == 0 and out["civec"].shape == (1, 1) and out["civec"][0, 0] == 1.0
        assert np.abs(out["rdm1_mo"] - 2.0 * np.eye(n)).max() == 0.0
    else:
        assert out["residual"] <= 1e-9, out["residual"]
        c = out["civec"]
        assert abs(np.linalg.norm(c) - 1.0) < 1e-12 and c.reshape(-1)[np.argmax(np.abs(c))] > 0
        sg = fnp.sigma(ref["h"], ref["V"], c, o)
        errs["residual_numpy"] = np.linalg.norm(sg - out["e_fci"] * c)
        assert errs["residual_numpy"] <= 1e-9 + 1e-11 * np.abs(sg).max()
        errs["rayleigh"] = abs(float(np.vdot(c, sg)) - out["e_fci"])
        assert errs["rayleigh"] < TOL
        assert out["e_fci"] < out["e_scf"]
        if "e" in ref:
            errs["e"] = abs(out["e_fci"] - ref["e"])
            errs["civec"] = np.abs(c - ref["c"]).max()
            assert errs["e"] < TOL and errs["civec"] < 1e-7, errs
    errs["dm1"] = np.abs(out["rdm1_mo"] - ref["dm1"]).max()
    errs["dm2"] = np.abs(out["dm2"] - ref["dm2"]).max()
    errs["dm2_cumulant"] = np.abs(out["dm2_cumulant"] - ref["cum"]).max()
    C = out["mo_coeff"]
    errs["rdm1_emb"] = np.abs(out["rdm1_emb"] - 0.5 * C @ ref["dm1"] @ C.T).max()
    errs["e_frag"] = np.abs(out["e_frag"] - ref["e_frag"]).max()
    errs["e_from_rdms"] = abs(fnp.energy_from_rdms(ref["h"], ref["V"], out["rdm1_mo"], out["dm2"]) - out["e_fci"])
    print(f"solve ({n},{o}): n_iter = {out['n_iter']} residual = {out['residual']:.2e} " + " ".join(f"{a}={b:.2e}" for a, b in errs.items()))
    assert max(errs[k] for k in ("dm1", "dm2", "dm2_cumulant", "rdm1_emb", "e_frag", "e_from_rdms")) < TOL, errs
    assert abs(np.trace(out["rdm1_mo"]) - 2 * o) < 1e-10
    assert out["t1"] is None and out["t2"] is None


def check_repeatable_and_residencies(lib, n, o):
    """two calls return identical bits; the packed block and the 3-index factor agree to 1e-10 in everything that does not depend on the choice of the fragment
    orbitals (the two fragment RHFs agree to their own convergence only): the eigenvalue, the embedding-basis 1-RDM, the fragment energies.  The vector error
    is residual / gap, so this comparison converges the residual to 1e-12."""
    from quemb_amd.fragsolver import default_fci_opts
    h = inputs(n, o)[0]
    runs = []
    for residency in ("block", "block", "factor"):
        fr = fragment(lib, n, o, residency)
        runs.append(fr.solve_fci(o, h, opts=scf_opts(lib), fci_opts=default_fci_opts(lib, conv_tol=1e-12), eeval=True, want_civec=True))
        fr.free()
    for k in ("e_fci", "civec", "rdm1_mo", "rdm1_emb", "e_frag", "mo_coeff", "residual"):
        assert np.array_equal(np.asarray(runs[0][k]), np.asarray(runs[1][k])), k
    for k in ("e_fci", "rdm1_emb", "e_frag"):
        assert np.abs(np.asarray(runs[0][k]) - np.asarray(runs[2][k])).max() < 1e-10, k
    assert runs[0]["n_iter"] == runs[1]["n_iter"] and runs[0]["residual"] <= 1e-12
