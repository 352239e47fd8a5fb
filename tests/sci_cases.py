"""The cases of solver="SCI-hip" that tests/test_sci_hostlogic.py (scalar mock device, CPU) and tests/test_gpu_sci.py (MI355X) both run: every function takes the
library to drive.  The reference is the twin tests/sci_numpy.py (Slater-Condon rules on Python integers, dict-of-keys matrix, numpy.linalg.eigh), evaluated in
the fragment-MO basis; the full-space references come from tests/fci_numpy.py.  Determinant sets are compared exactly, which is meaningful only while no
decision of the rule sits at the threshold: every comparison first asserts the twin's margin = min |crit / eps - 1| >= 1e-6.
Bars: 1e-8 absolute for energies, densities and fragment energies (the project's fragment-vs-oracle figure), 1e-7 for the vector (residual 1e-9 over a gap of
order 1e-2 at the least), 1e-11 relative for one application of H, 1e-12 for two runs of the atomically accumulated RDMs."""
import warnings
from functools import lru_cache

import numpy as np
import pytest

import fci_numpy as fnp
import sci_numpy as snp
from helpers import GOLDEN, synthetic_fragment_factor
from qemb_oracle import be as obe
from qemb_oracle import eri, scf

TOL = 1e-8
MARGIN = 1e-6
WEIGHT = 0.75
FAMILY = {"default": {}, "strong": dict(scale=0.25, gap=0.5)}      # strong: correlation energy of order 0.4 Eh at (6, 3), RHF still converges
# (n, o, family, eps): fewer determinants than a wavefront; 22 < 64; several workgroups with ragged rows; (7, 3); orbitals on both sides of bit 31 / 32; bit 63
OPS = [(4, 2, "default", 1e-3), (6, 3, "default", 1e-2), (6, 3, "strong", 1e-2), (7, 3, "default", 1e-3)]
WIDE = [(34, 2, "default", 1e-3), (64, 1, "default", 1e-3)]
SOLVE = [(2, 1, "default"), (4, 2, "default"), (5, 2, "default"), (6, 3, "default"), (6, 3, "strong"), (6, 1, "default"), (7, 3, "default"), (10, 5, "default")]
SEED = {}      # (n, o, family) -> seed where 900 + 10 n + o leaves a decision inside the band


def seed_of(n, o, family):
    return SEED.get((n, o, family), 900 + 10 * n + o)


def sites(n):
    nf = min(n, 3)
    return nf, ([0, nf - 1] if nf > 1 else [0])


@lru_cache(maxsize=None)
def inputs(n, o, family="default"):
    s = seed_of(n, o, family)
    h, e1, Bp = synthetic_fragment_factor(n, o, s, **FAMILY[family])
    rng = np.random.default_rng(s + 1)
    sym = lambda: (lambda a: a + a.T)(rng.standard_normal((n, n)))
    return h, e1, Bp, sym(), sym(), sym()


def fragment(lib, n, o, family="default", residency="block"):
    from quemb_amd.fragsolver import DeviceFragment
    h, e1, Bp, h1, veff0, veff = inputs(n, o, family)
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


def words(dets):
    return (np.array([d[0] for d in dets], dtype=np.uint64), np.array([d[1] for d in dets], dtype=np.uint64))


def pairs(alpha, beta):
    return [(int(a), int(b)) for a, b in zip(alpha, beta)]


# ---------------------------------------------------------------- the operations on their own, on states of the twin
@lru_cache(maxsize=None)
def twin_state(n, o, family, eps, max_round=30):
    """(h, V) in the RHF orbitals of the oracle and the twin's run on them; computed once and left unchanged"""
    h, e1 = inputs(n, o, family)[:2]
    C = scf.rhf(h, e1, o, conv_tol=1e-13, conv_tol_grad=1e-10)["mo_coeff"]
    hm, Vm = C.T @ h @ C, fnp.mo_eri(e1, C)
    r = snp.select(hm, Vm, o, eps, max_round=max_round)
    print(f"twin ({n},{o}) {family} eps={eps:g}: {len(r['dets'])} determinants, {r['rounds']} rounds, margin {r['margin']:.3e}")
    return hm, Vm, r


@lru_cache(maxsize=None)
def wide_state(n, o, family, eps):
    """the wide words: two rounds of the twin with its rules evaluated on arrays (snp.hij_many, pinned to hij by test_sci_hostlogic.py) and the lowest eigenpair of
    the second space from scipy's Lanczos -- thousands of determinants, where the Python-integer loops would take minutes.  history[1] is a state with occupied
    orbitals on both sides of bit 31 / 32 (at bit 63) and a vector that is no unit vector."""
    import scipy.sparse.linalg as sl      # (scipy: as tests/test_hostlogic_be.py and tests/test_integrals.py already need it)
    h, e1 = inputs(n, o, family)[:2]
    C = scf.rhf(h, e1, o, conv_tol=1e-13, conv_tol_grad=1e-10)["mo_coeff"]
    hm, Vm = C.T @ h @ C, fnp.mo_eri(e1, C)
    hf = (1 << o) - 1
    joined, margin = snp.candidates_many(hm, Vm, n, [(hf, hf)], np.ones(1), eps)
    dets = sorted([(hf, hf)] + joined)
    H = snp.hamiltonian_many(hm, Vm, dets)
    w, U = sl.eigsh(H, k=1, which="SA", tol=1e-13)
    c = snp.fix_sign(U[:, 0])
    assert np.linalg.norm(H @ c - w[0] * c) < 1e-10
    joined2, margin2 = snp.candidates_many(hm, Vm, n, dets, c, eps)
    print(f"twin ({n},{o}) {family} eps={eps:g}: {len(joined)} determinants join the HF determinant, then {len(joined2)}; margin {min(margin, margin2):.3e}")
    return hm, Vm, dict(margin=min(margin, margin2), H=H, history=[([(hf, hf)], np.ones(1), joined), (dets, c, joined2)])


def check_screen_and_merge(lib, n, o, family, eps, state=twin_state):
    """every round of the twin: the keys the screen emits are the determinants that joined, for the default slabs and for slabs of three determinants with the
    smallest candidate buffer allowed (several passes, the halving path); the merge gives the next space with the vector padded"""
    from quemb_amd.fragsolver import sci_merge, sci_screen
    hm, Vm, r = state(n, o, family, eps)
    assert r["margin"] >= MARGIN, r["margin"]
    v = n - o
    nexc = 2 * o * v + 2 * (o * (o - 1) // 2) * (v * (v - 1) // 2) + (o * v) ** 2
    cap = 2
    while cap < 2 * nexc:
        cap <<= 1
    for dets, c, joined in r["history"]:
        a, b = words(dets)
        for kw in (dict(), dict(slab=3, cap=cap)):
            ja, jb = sci_screen(hm, Vm, o, a, b, c, eps, lib=lib, **kw)
            assert pairs(ja, jb) == joined, (len(ja), len(joined), kw)
        if joined:
            ma, mb, mc = sci_merge(a, b, c, *words(joined), lib=lib)
            want = sorted(dets + joined)
            assert pairs(ma, mb) == want
            pos = {d: k for k, d in enumerate(dets)}
            assert np.array_equal(mc, np.array([c[pos[d]] if d in pos else 0.0 for d in want]))


def final_space(n, o, family, eps, state=twin_state):
    hm, Vm, r = state(n, o, family, eps)
    if state is wide_state:      # the space of the second round
        return hm, Vm, r["history"][1][0], r["history"][1][1]
    return hm, Vm, r["dets"], r["c"]


def check_matrix(lib, n, o, family, eps, state=twin_state):
    """the CSR matrix equals hij on every stored and every absent pair: stored are exactly the pairs at most two excitations apart, columns ascending"""
    from quemb_amd.fragsolver import sci_matrix
    hm, Vm, dets, _ = final_space(n, o, family, eps, state)
    N = len(dets)
    rp, col, val = sci_matrix(hm, Vm, *words(dets), lib=lib)
    assert rp[0] == 0 and rp[-1] == len(col) == len(val)
    H = np.zeros((N, N))
    stored = np.zeros((N, N), dtype=bool)
    for r_ in range(N):
        cs = col[rp[r_]:rp[r_ + 1]]
        assert np.all(np.diff(cs) > 0) and r_ in cs
        H[r_, cs] = val[rp[r_]:rp[r_ + 1]]
        stored[r_, cs] = True
    assert np.array_equal(stored, snp.near_pairs(dets))
    scale = max(1.0, np.abs(H).max())
    if state is twin_state:
        assert np.abs(H - snp.hamiltonian(hm, Vm, dets)).max() <= 1e-12 * scale
        return H
    # the wide words (thousands of determinants, millions of connected pairs): every value against the twin's rules evaluated on arrays, which 24 rows spread over
    # the space (first and last included) tie to hij itself here; two electrons also against the closed form H[(p,q),(r,s)] = h_pr d_qs + d_pr h_qs + (pr|qs)
    ref = state(n, o, family, eps)[2]["H"]
    assert np.abs(H - ref).max() <= 1e-12 * scale
    rows = sorted(set(np.linspace(0, N - 1, 24).astype(int).tolist()))
    assert np.abs(ref[rows] - snp.hamiltonian(hm, Vm, dets, rows=rows)[rows]).max() <= 1e-12 * scale
    if o == 1:
        p = np.array([snp.bits(d[0])[0] for d in dets])
        q = np.array([snp.bits(d[1])[0] for d in dets])
        H2 = hm[p[:, None], p[None, :]] * (q[:, None] == q[None, :]) + (p[:, None] == p[None, :]) * hm[q[:, None], q[None, :]] + Vm[p[:, None], p[None, :], q[:, None], q[None, :]]
        assert np.abs(H - H2).max() <= 1e-12 * scale
    return H


def check_spmv(lib, n, o, family, eps):
    from quemb_amd.fragsolver import sci_spmv
    hm, Vm, dets, _ = final_space(n, o, family, eps)
    x = np.random.default_rng(n * 100 + o).standard_normal(len(dets))
    ref = snp.hamiltonian(hm, Vm, dets) @ x
    y = sci_spmv(hm, Vm, *words(dets), x, lib=lib)
    print(f"spmv ({n},{o}) {family}: max |d| = {np.abs(y - ref).max():.2e}, max |y| = {np.abs(ref).max():.2e}")
    assert np.abs(y - ref).max() <= 1e-11 * np.abs(ref).max()


def check_rdm_op(lib, n, o, family, eps):
    from quemb_amd.fragsolver import sci_rdm12
    hm, Vm, dets, c = final_space(n, o, family, eps)
    r1, r2 = fnp.rdm12(snp.full_vector(dets, c, n, o), n, o)
    dm1, dm2 = sci_rdm12(hm, Vm, o, *words(dets), c, lib=lib)
    assert np.abs(dm1 - r1).max() < TOL and np.abs(dm2 - r2).max() < TOL
    _, cum = sci_rdm12(hm, Vm, o, *words(dets), c, cumulant=True, lib=lib)
    assert np.abs(cum - (r2 - fnp.mean_field_part(r1, o))).max() < TOL


# ---------------------------------------------------------------- the solve
@lru_cache(maxsize=None)
def solved(lib, n, o, family, eps=1e-3):
    from quemb_amd.fragsolver import default_sci_opts
    h, e1, Bp, h1, veff0, veff = inputs(n, o, family)
    nf, cen = sites(n)
    fr = fragment(lib, n, o, family)
    out = fr.solve_sci(o, h, opts=scf_opts(lib), sci_opts=default_sci_opts(lib, eps_var=eps), eeval=True, want_dets=True)
    out["dm2"] = fr.make_rdm2("SCI-hip", with_dm1=True)
    out["dm2_cumulant"] = fr.make_rdm2("SCI-hip", with_dm1=False)
    fr.free()
    C = out["mo_coeff"]
    ref = dict(h=C.T @ h @ C, V=fnp.mo_eri(e1, C))
    if o < n:
        ref["twin"] = snp.select(ref["h"], ref["V"], o, eps)
        ref["dm1"], ref["dm2"] = snp.rdm12(ref["twin"]["dets"], ref["twin"]["c"], n)
    else:
        ref["dm1"] = 2.0 * np.eye(n)
        ref["dm2"] = 4.0 * np.einsum("pq,rs->pqrs", np.eye(n), np.eye(n)) - 2.0 * np.einsum("ps,qr->pqrs", np.eye(n), np.eye(n))
    ref["cum"] = ref["dm2"] - fnp.mean_field_part(ref["dm1"], o)
    args = (C, o, nf, (WEIGHT, cen), np.zeros((n, n)), h1, ref["dm1"])
    ref["e_frag"] = np.array(obe.get_frag_energy(*args, ref["cum"], eri.pack_s4(e1), veff0, veff, True))
    ref["e_frag_full"] = np.array(obe.get_frag_energy(*args, ref["dm2"], eri.pack_s4(e1), veff0, veff, False))
    return out, ref


def check_solve(lib, n, o, family):
    out, ref = solved(lib, n, o, family)
    assert out["t1"] is None and out["t2"] is None
    if o == n:      # a single determinant: the mean-field results
        assert out["e_corr_mo"] == 0.0 and out["e_sci"] == out["e_scf"] and out["ndet"] == 1 and out["rounds"] == 0
        a, b, c = out["dets"]
        assert int(a[0]) == int(b[0]) == (1 << n) - 1 and c[0] == 1.0
        assert np.abs(out["rdm1_mo"] - 2.0 * np.eye(n)).max() == 0.0
    else:
        tw = ref["twin"]
        print(f"solve ({n},{o}) {family}: ndet = {out['ndet']} rounds = {out['rounds']} nnz = {out['nnz']} residual = {out['residual']:.2e}; twin margin = {tw['margin']:.3e}")
        assert tw["margin"] >= MARGIN, tw["margin"]      # no decision of the rule inside the band: the sets are comparable
        a, b, c = out["dets"]
        assert pairs(a, b) == tw["dets"] and out["ndet"] == len(tw["dets"]) and out["rounds"] == tw["rounds"] and tw["converged"]
        assert out["residual"] <= 1e-9 and abs(np.linalg.norm(c) - 1.0) < 1e-12 and c[np.argmax(np.abs(c))] > 0
        assert abs(out["e_sci"] - tw["e"]) < TOL and out["e_sci"] <= out["e_scf"] + 1e-12
        assert np.abs(c - tw["c"]).max() < 1e-7
    errs = dict(dm1=np.abs(out["rdm1_mo"] - ref["dm1"]).max(), dm2=np.abs(out["dm2"] - ref["dm2"]).max(), cum=np.abs(out["dm2_cumulant"] - ref["cum"]).max(),
                e_frag=np.abs(out["e_frag"] - ref["e_frag"]).max())
    C = out["mo_coeff"]
    errs["rdm1_emb"] = np.abs(out["rdm1_emb"] - 0.5 * C @ ref["dm1"] @ C.T).max()
    errs["e_from_rdms"] = abs(fnp.energy_from_rdms(ref["h"], ref["V"], out["rdm1_mo"], out["dm2"]) - out["e_sci"])
    print("   " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs
    assert abs(np.trace(out["rdm1_mo"]) - 2 * o) < 1e-10


def check_collapse(lib, n=10, o=5, family="default", max_space=2):
    """max_space = 2: the Davidson basis of every diagonalisation collapses to the Ritz vector after its second application of H, which the default max_space = 12
    never reaches.  The same determinants and rounds as the default-options solve of `solved`, energy, vector, densities and fragment energies at the bars above;
    more than max_space applications per round on average says that a collapse ran."""
    from quemb_amd.fragsolver import default_sci_opts
    base = solved(lib, n, o, family)[0]
    so = default_sci_opts(lib, eps_var=1e-3, max_space=max_space, max_cycle=400)
    fr = fragment(lib, n, o, family)
    out = fr.solve_sci(o, inputs(n, o, family)[0], opts=scf_opts(lib), sci_opts=so, eeval=True, want_dets=True)      # (strict: raises unless every diagonalisation converged)
    out["dm2"] = fr.make_rdm2("SCI-hip", with_dm1=True)
    out["dm2_cumulant"] = fr.make_rdm2("SCI-hip", with_dm1=False)
    fr.free()
    assert all(np.array_equal(x, y) for x, y in zip(out["dets"][:2], base["dets"][:2])) and out["rounds"] == base["rounds"] and out["nnz"] == base["nnz"]
    assert out["residual"] <= so.conv_tol and out["n_iter"] > max_space * out["rounds"], (out["residual"], out["n_iter"], out["rounds"])
    errs = {k: float(np.abs(np.asarray(out[k]) - np.asarray(base[k])).max()) for k in ("e_sci", "rdm1_mo", "rdm1_emb", "dm2", "dm2_cumulant", "e_frag")}
    errs["c"] = float(np.abs(out["dets"][2] - base["dets"][2]).max())
    print(f"collapse ({n},{o}) {family}: n_iter = {out['n_iter']} in {out['rounds']} rounds (max_space = 12: {base['n_iter']}) residual = {out['residual']:.2e} "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["c"] < 1e-7 and max(v for k, v in errs.items() if k != "c") < TOL, errs


def check_frags_energy(lib, n=5, o=2):
    """Frags.solve(solver="SCI-hip") for both values of use_cumulant against the oracle's get_frag_energy fed with the twin's RDMs"""
    from quemb_amd.pfrag import Frags
    from quemb_amd.solver import SHCI_ArgsUser
    h, e1, Bp, h1, veff0, veff = inputs(n, o)
    nf, cen = sites(n)
    f = Frags(list(range(nf)), 0, [], [], [], [], (WEIGHT, cen), cen, lib=lib)
    f.dev = fragment(lib, n, o)
    f.nao, f.nsocc, f.h1, f.veff0, f.veff, f.fock, f.heff, f.dm0 = n, o, h1, veff0, veff, h, np.zeros((n, n)), None
    for cumulant in (True, False):
        out = f.solve(eeval=True, use_cumulant=cumulant, want_t2=True, solver="SCI-hip", solver_args=SHCI_ArgsUser(hci_cutoff=1e-3), opts=scf_opts(lib))
        C = out["mo_coeff"]
        tw = snp.select(C.T @ h @ C, fnp.mo_eri(e1, C), o, 1e-3)
        assert tw["margin"] >= MARGIN and pairs(*out["dets"][:2]) == tw["dets"]
        dm1, dm2 = snp.rdm12(tw["dets"], tw["c"], n)
        r2 = dm2 - fnp.mean_field_part(dm1, o) if cumulant else dm2
        ref = obe.get_frag_energy(C, o, nf, (WEIGHT, cen), np.zeros((n, n)), h1, dm1, r2, eri.pack_s4(e1), veff0, veff, cumulant)
        assert np.abs(np.asarray(out["e_frag"]) - np.asarray(ref)).max() < TOL, (cumulant, out["e_frag"], ref)
        assert f._solver == "SCI-hip" and np.abs(f.make_rdm2(with_dm1=not cumulant) - r2).max() < TOL


def check_full_space_is_fci(lib, n, o):
    """eps -> 0: the selected space is the full one and everything equals the FCI-hip solve of the same fragment"""
    from quemb_amd.fragsolver import default_sci_opts
    from math import comb
    h = inputs(n, o)[0]
    fs, ff = fragment(lib, n, o), fragment(lib, n, o)
    s = fs.solve_sci(o, h, opts=scf_opts(lib), sci_opts=default_sci_opts(lib, eps_var=1e-12), eeval=True, want_dets=True)
    f = ff.solve_fci(o, h, opts=scf_opts(lib), eeval=True)
    errs = dict(e=abs(s["e_sci"] - f["e_fci"]), dm1=np.abs(s["rdm1_mo"] - f["rdm1_mo"]).max(), e_frag=np.abs(s["e_frag"] - f["e_frag"]).max())
    for with_dm1 in (True, False):
        errs[f"dm2_{int(with_dm1)}"] = np.abs(fs.make_rdm2("SCI-hip", with_dm1) - ff.make_rdm2("FCI-hip", with_dm1)).max()
    fs.free(); ff.free()
    print(f"eps -> 0 ({n},{o}): ndet = {s['ndet']} of {comb(n, o) ** 2}, rounds = {s['rounds']} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs
    if comb(n, o) ** 2 <= 1300:      # where the twin's dense eigenproblem fits: the count it reaches
        C = s["mo_coeff"]
        tw = snp.select(C.T @ h @ C, fnp.mo_eri(inputs(n, o)[1], C), o, 1e-12)
        assert tw["margin"] >= MARGIN and s["ndet"] == len(tw["dets"])
    else:      # (10, 5): the twin's run is recorded (tests/golden/make_sci_full_space.py; 63 504 determinants are beyond the twin's Python loops within a test)
        g = recorded_full_space()
        assert (n, o) == (int(g["n"]), int(g["o"])) and float(g["margin"]) >= MARGIN, float(g["margin"])
        assert s["ndet"] == int(g["counts"][-1]) and s["rounds"] == int(g["rounds"])
        left_out = set(pairs(g["outside"][:, 0], g["outside"][:, 1])) if len(g["outside"]) else set()
        st = [int(x) for x in fnp.strings(n, o)]
        assert pairs(*s["dets"][:2]) == [(x, y) for x in st for y in st if (x, y) not in left_out]
        assert abs(s["e_sci"] - float(g["e"])) < TOL
    return s


@lru_cache(maxsize=None)
def recorded_full_space():
    g = dict(np.load(GOLDEN / "sci_full_space_10_5.npz"))
    assert int(g["seed"]) == seed_of(int(g["n"]), int(g["o"]), "default") and float(g["eps"]) == 1e-12
    return g


def check_recorded_state_ops(lib):
    """(10, 5) at eps = 1e-12 by its single operations, on the twin's recorded state before the second screen (826 determinants, 20 300 join): the screen, the
    merge, and the product on the space that results, whose recorded eigenpair it must reproduce"""
    from quemb_amd.fragsolver import sci_merge, sci_screen, sci_spmv
    g = recorded_full_space()
    n, o = int(g["n"]), int(g["o"])
    h, e1 = inputs(n, o)[:2]
    hm, Vm = g["C"].T @ h @ g["C"], fnp.mo_eri(e1, g["C"])
    a, b, c = g["r1_keys"][:, 0].copy(), g["r1_keys"][:, 1].copy(), g["r1_c"]
    ja, jb = sci_screen(hm, Vm, o, a, b, c, 1e-12, lib=lib)
    assert float(g["margin"]) >= MARGIN and np.array_equal(ja, g["r2_joined"][:, 0]) and np.array_equal(jb, g["r2_joined"][:, 1])
    ma, mb, mc = sci_merge(a, b, c, ja, jb, lib=lib)
    assert len(ma) == int(g["counts"][2]) and np.count_nonzero(mc) <= len(a)
    y = sci_spmv(hm, Vm, ma, mb, g["r2_c"], lib=lib)
    resid = np.linalg.norm(y - float(g["r2_e"]) * g["r2_c"])
    print(f"(10,5) recorded state: {len(ja)} join {len(a)}, ||H c - E c|| = {resid:.2e} on {len(ma)} determinants")
    assert resid < TOL


def check_two_electrons_by_operations(lib, n=64):
    """two electrons in 64 orbitals at eps = 1e-12 by the single operations -- screen, merge, matrix, with scipy's Lanczos for the eigenpair -- against the oracle's
    CCSD, which is exact for two electrons: the widest word where a whole solve (the n^6 integral transformation) is beyond the scalar mock"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    from qemb_oracle import ccsd
    from quemb_amd.fragsolver import sci_matrix, sci_merge, sci_screen
    o = 1
    h, e1 = inputs(n, o)[:2]
    mf = scf.rhf(h, e1, o, conv_tol=1e-13, conv_tol_grad=1e-10)
    C = mf["mo_coeff"]
    ecc = ccsd.solve_ccsd(h, e1, o, C, mf["mo_energy"])[2]
    hm, Vm = C.T @ h @ C, fnp.mo_eri(e1, C)
    a, b, c = np.array([1], dtype=np.uint64), np.array([1], dtype=np.uint64), np.ones(1)
    e_hf = e = snp.hij(hm, Vm, (1, 1), (1, 1))
    for _ in range(30):
        ja, jb = sci_screen(hm, Vm, o, a, b, c, 1e-12, lib=lib)
        if len(ja) == 0:
            break
        a, b, c = sci_merge(a, b, c, ja, jb, lib=lib)
        rp, col, val = sci_matrix(hm, Vm, a, b, lib=lib)
        w, U = sl.eigsh(sp.csr_matrix((val, col, rp), shape=(len(a),) * 2), k=1, which="SA", v0=c + 1e-3, tol=1e-13)
        e, c = float(w[0]), snp.fix_sign(U[:, 0])
        if len(a) == n * n:      # the full space: nothing is left to join (and a screen of 4096 determinants takes the scalar mock 14 s)
            break
    print(f"({n},1) by operations: {len(a)} determinants, e_corr = {e - e_hf:.12f}, CCSD = {ecc:.12f}")
    assert abs((e - e_hf) - ecc) < TOL and int(a.max()) == 1 << (n - 1)


def check_two_electrons_in_64_orbitals(lib):
    """(64, 1) at eps = 1e-12 against CCSD, which is exact for two electrons: the widest word without any twin"""
    from quemb_amd.fragsolver import default_opts, default_sci_opts
    n, o = 64, 1
    h = inputs(n, o)[0]
    fr = fragment(lib, n, o)
    tight = scf_opts(lib, cc_conv_tol=1e-12, cc_conv_tol_normt=1e-10)
    s = fr.solve_sci(o, h, opts=tight, sci_opts=default_sci_opts(lib, eps_var=1e-12), eeval=False, want_dets=True)
    cc = fr.solve(o, h, opts=tight, eeval=False)
    fr.free()
    print(f"(64,1): ndet = {s['ndet']} e_corr SCI = {s['e_corr_mo']:.12f} CCSD = {cc['e_corr_mo']:.12f}")
    assert abs(s["e_corr_mo"] - cc["e_corr_mo"]) < TOL and s["ndet"] <= 64 * 64 and int(s["dets"][0].max()) == 1 << 63


def check_repeatable_and_residencies(lib, n, o, family="default"):
    """two calls: the same determinants, CSR arrays and vector bit for bit, the atomically accumulated RDMs to 1e-12; block and factor residency agree to 1e-10 in
    what does not depend on the choice of the fragment orbitals"""
    from quemb_amd.fragsolver import default_sci_opts, sci_matrix
    h = inputs(n, o, family)[0]
    so = default_sci_opts(lib, eps_var=1e-3, conv_tol=1e-12)
    runs, mats = [], []
    for residency in ("block", "block", "factor"):
        fr = fragment(lib, n, o, family, residency)
        runs.append(fr.solve_sci(o, h, opts=scf_opts(lib), sci_opts=so, eeval=True, want_dets=True))
        runs[-1]["dm2"] = fr.make_rdm2("SCI-hip")
        fr.free()
        C = runs[-1]["mo_coeff"]
        if residency == "block":
            mats.append(sci_matrix(C.T @ h @ C, fnp.mo_eri(inputs(n, o, family)[1], C), *runs[-1]["dets"][:2], lib=lib))
    for k in ("e_sci", "mo_coeff", "residual", "ndet", "nnz", "rounds", "n_iter"):
        assert np.array_equal(np.asarray(runs[0][k]), np.asarray(runs[1][k])), k
    for x, y in zip(runs[0]["dets"] + mats[0], runs[1]["dets"] + mats[1]):
        assert np.array_equal(x, y)
    assert len(mats[0][1]) == runs[0]["nnz"]
    for k in ("rdm1_mo", "rdm1_emb", "e_frag", "dm2"):
        assert np.abs(np.asarray(runs[0][k]) - np.asarray(runs[1][k])).max() < 1e-12, k
    for k in ("e_sci", "rdm1_emb", "e_frag"):
        assert np.abs(np.asarray(runs[0][k]) - np.asarray(runs[2][k])).max() < 1e-10, k
    assert runs[0]["ndet"] == runs[2]["ndet"] and runs[0]["residual"] <= 1e-12


def check_refusals(lib):
    import ctypes as C
    from quemb_amd import _lib
    from quemb_amd._lib import QembError, SciOpts
    from quemb_amd.fragsolver import DeviceFragment, default_opts, default_sci_opts
    from quemb_amd.pfrag import Frags
    from quemb_amd.solver import SHCI_ArgsUser, be_func, fragment_work_bytes, sci_opts_from_args
    fr = DeviceFragment(65, 2, lib=lib)      # beyond the word, before anything is allocated
    with pytest.raises(QembError, match="at most 64") as ei:
        fr.solve_sci(8, np.zeros((65, 65)), eeval=False)
    assert ei.value.status == _lib.QEMB_ERR_UNSUPPORTED
    fr.free()
    n, o = 6, 3
    h = inputs(n, o, "strong")[0]
    fr = fragment(lib, n, o, "strong")
    with pytest.raises(QembError, match="eps_var") as ei:
        fr.solve_sci(o, h, sci_opts=default_sci_opts(lib, eps_var=0.0))
    assert ei.value.status == _lib.QEMB_ERR_ARG
    bad = default_sci_opts(lib)
    bad.struct_size = 8
    with pytest.raises(QembError, match="struct_size") as ei:
        fr.solve_sci(o, h, sci_opts=bad)
    assert ei.value.status == _lib.QEMB_ERR_ARG and C.sizeof(SciOpts) == default_sci_opts(lib).struct_size
    d = default_sci_opts(lib)
    assert (d.eps_var, d.conv_tol, d.max_cycle, d.max_space, d.max_round, d.max_det) == (1e-3, 1e-9, 100, 12, 30, 1 << 20)
    # max_det below what the second round reaches: n, eps and the count are named
    with pytest.raises(QembError, match=r"n = 6, eps_var = 0\.001.* in round \d+: \d+ determinants, energy so far .*max_det = 20") as ei:
        fr.solve_sci(o, h, sci_opts=default_sci_opts(lib, max_det=20))
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    # one round is not enough
    one = default_sci_opts(lib, max_round=1)
    with pytest.raises(QembError, match="still adding determinants after max_round") as ei:
        fr.solve_sci(o, h, sci_opts=one)
    assert ei.value.status == _lib.QEMB_ERR_NOCONV
    with pytest.raises(QembError, match="no solve has run"):
        fr.make_rdm2("SCI-hip")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fr.solve_sci(o, h, opts=default_opts(lib, strict_convergence=0), sci_opts=one, want_dets=True)
    assert any(issubclass(w.category, _lib.ConvergenceWarning) for w in rec)
    assert out["rounds"] == 1 and out["ndet"] > 1 and np.isfinite(out["e_frag"]).all() and abs(np.linalg.norm(out["dets"][2]) - 1.0) < 1e-12
    # the memory limit, against the formula the library reports
    nb = C.c_int64()
    assert lib.qemb_frag_sci_bytes(n, o, 1 << 20, 12, C.byref(nb)) == 0 and nb.value == int(fragment_work_bytes(n, o, solver="SCI-hip")) and nb.value > 24 << 20
    assert lib.qemb_frag_sci_bytes(65, 8, 1 << 20, 12, C.byref(nb)) == _lib.QEMB_ERR_UNSUPPORTED
    fr.set_sci_mem_limit(1 << 16)
    with pytest.raises(QembError, match=r"n = 6, eps_var = 0\.001.*bytes") as ei:
        fr.solve_sci(o, h)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    fr.set_sci_mem_limit(-1)
    # the 2-RDM of another kind of solve
    fr.solve(o, h, eeval=False)
    with pytest.raises(QembError, match="the last solve of this fragment was CCSD") as ei:
        fr.make_rdm2("SCI-hip")
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.solve_sci(o, h)
    with pytest.raises(QembError, match="the last solve of this fragment was SCI"):
        fr.make_rdm2("CCSD")
    assert fr.make_rdm2("SCI-hip").shape == (n,) * 4
    fr.set_eri_s4(eri.pack_s4(inputs(n, o, "strong")[1]))
    with pytest.raises(QembError, match="no solve has run"):
        fr.make_rdm2("SCI-hip")
    fr.free()
    # the arguments of the reference that are not built, a wrong type, and the bare literal
    f = Frags([0, 1], 0, [], [], [], [], (1.0, [0]), [0], lib=lib)
    with pytest.raises(NotImplementedError, match="hci_pt"):
        be_func(None, [f], 1, "SCI-hip", 0.0, solver_args=SHCI_ArgsUser(hci_pt=True))
    with pytest.raises(NotImplementedError, match="return_frag_data"):
        be_func(None, [f], 1, "SCI-hip", 0.0, solver_args=SHCI_ArgsUser(return_frag_data=True))
    with pytest.raises(TypeError, match="SHCI_ArgsUser"):
        be_func(None, [f], 1, "SCI-hip", 0.0, solver_args=dict(hci_cutoff=1e-3))
    assert sci_opts_from_args("CCSD", dict(anything=1), lib) is None and sci_opts_from_args("SCI-hip", None, lib) is None
    assert sci_opts_from_args("SCI-hip", SHCI_ArgsUser(hci_cutoff=1e-4), lib).eps_var == 1e-4 and SHCI_ArgsUser() == SHCI_ArgsUser(0.001, False, False)
    with pytest.raises(Exception):
        SHCI_ArgsUser().hci_cutoff = 1.0      # frozen
    with pytest.raises(ValueError, match="Solver not implemented"):
        be_func(None, [f], 1, "SCI", 0.0)


def check_solve_sci_function(lib):
    from quemb_amd.fragsolver import default_sci_opts
    from quemb_amd.solver import solve_sci
    n, o = 5, 3
    h, e1, Bp = inputs(n, o)[:3]
    so = default_sci_opts(lib, eps_var=1e-12)
    e_a, dets, dm1, mo = solve_sci(h, eri.pack_s4(e1), o, rdm_return=True, sci_opts=so, lib=lib)
    e_b, _, dm2 = solve_sci(h, None, o, df_factor=Bp, rdm2_return=True, use_cumulant=False, sci_opts=so, lib=lib)
    E, c, _ = fnp.ground_state(mo.T @ h @ mo, fnp.mo_eri(e1, mo), o)
    assert abs(e_a - E) < TOL and abs(e_b - E) < TOL and dm2.shape == (n,) * 4
    assert np.abs(snp.full_vector(pairs(*dets[:2]), dets[2], n, o) - c).max() < 1e-7 and np.abs(dm1 - fnp.rdm12(c, n, o)[0]).max() < TOL


# ---------------------------------------------------------------- the BE driver: H8 / STO-3G with the stored fragment lists
def h_chain(lib, natom, key, **kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    mol = Mole([["H", (0.0, 0.0, float(i))] for i in range(natom)])
    mf = RHF(mol); mf.kernel()
    return BE(mf, FragPart.from_json(GOLDEN / "fragmentation.json", key, n_BE=int(key[-1])), lib=lib, distribute=False, **kw)


def check_h8_be2(lib):
    import rdm2_numpy as r2n
    from quemb_amd.be_parallel import be_func_parallel
    from quemb_amd.solver import SHCI_ArgsUser, be_func
    key = "test_autogen_h_linear_be2"
    full, loose = SHCI_ArgsUser(hci_cutoff=1e-12), SHCI_ArgsUser(hci_cutoff=1e-2)
    bf, bs = h_chain(lib, 8, key), h_chain(lib, 8, key)
    e_fci, _ = bf.oneshot(solver="FCI-hip")
    e_sci, comps = bs.oneshot(solver="SCI-hip", solver_args=full)
    print(f"H8 BE2 oneshot: FCI-hip {e_fci:.12f}, SCI-hip at 1e-12 {e_sci:.12f}")
    assert abs(e_sci - e_fci) < TOL and all(f._solver == "SCI-hip" for f in bs.Fobjs)
    # full-basis densities and energies through the 2-RDM handling of the FCI branch
    got, want = bs.rdm12_fullbasis(), bf.rdm12_fullbasis()
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.abs(a - b).max() < TOL
    bs.compute_energy_full(approx_cumulant=False, use_full_rdm=True, return_rdm=False)
    bf.compute_energy_full(approx_cumulant=False, use_full_rdm=True, return_rdm=False)
    assert abs(bs.e_full["EKapprox"] - bf.e_full["EKapprox"]) < TOL and abs(bs.e_full["EKtrue"] - bf.e_full["EKtrue"]) < TOL
    # a loose cutoff lies above and equals the sum of the oracle's fragment energies over the twin's solutions
    bl = h_chain(lib, 8, key)
    e_loose, comps = bl.oneshot(solver="SCI-hip", solver_args=loose)
    tot = np.zeros(3)
    for f in bl.Fobjs:
        e1 = eri.restore_s1(f.dev.get_eri_s4(), f.nao)
        C = f.mo_coeffs
        tw = snp.select(C.T @ (f.fock + f.heff) @ C, fnp.mo_eri(e1, C), f.nsocc, 1e-2)
        assert tw["margin"] >= MARGIN, tw["margin"]
        dm1, dm2 = snp.rdm12(tw["dets"], tw["c"], f.nao)
        w, cen = f.weight_and_relAO_per_center
        tot += np.array(obe.get_frag_energy(C, f.nsocc, f.n_frag, (w, cen), f.TA, f.h1, dm1, dm2 - fnp.mean_field_part(dm1, f.nsocc), f.dev.get_eri_s4(), f.veff0, f.veff, True))
    print(f"H8 BE2 oneshot at 1e-2: {e_loose:.12f} (FCI {e_fci:.12f})")
    assert e_loose > e_fci and np.abs(np.asarray(comps) - tot).max() < TOL, (comps, tot)
    # be_func_parallel (one rank) and the lock-step request give the serial numbers
    ba, bb, bc = h_chain(lib, 8, key), h_chain(lib, 8, key), h_chain(lib, 8, key)
    r1 = be_func(list(ba.pot), ba.Fobjs, ba.Nocc, "SCI-hip", ba.enuc, solver_args=loose, eeval=True, return_vec=True)
    r2 = be_func(list(bb.pot), bb.Fobjs, bb.Nocc, "SCI-hip", bb.enuc, solver_args=loose, eeval=True, return_vec=True, lockstep=True)
    r3 = be_func_parallel(list(bc.pot), bc.Fobjs, bc.Nocc, "SCI-hip", bc.enuc, solver_args=loose, eeval=True, return_vec=True)
    # (the densities come from atomic adds: equal to rounding, not to the bit)
    assert np.abs(r1[1] - r2[1]).max() < 1e-12 and np.abs(r1[1] - r3[1]).max() < 1e-12 and abs(r1[2][0] - e_loose) < 1e-10 and abs(r3[2][0] - e_loose) < 1e-10
    # chemical-potential matching converges to the FCI run; the numerical Jacobian agrees with the FCI one
    of = h_chain(lib, 8, key).optimize(solver="FCI-hip", only_chem=True, conv_tol=1e-7)
    os_ = h_chain(lib, 8, key).optimize(solver="SCI-hip", only_chem=True, conv_tol=1e-7, solver_args=full)
    assert os_.err < 1e-7 and abs(os_.Ebe[0] - of.Ebe[0]) < 1e-7, (os_.Ebe[0], of.Ebe[0])
    Js = h_chain(lib, 8, key).compute_numerical_jacobian("SCI-hip", False, 1, step_size=1e-4, solver_args=full)
    Jf = h_chain(lib, 8, key).compute_numerical_jacobian("FCI-hip", False, 1, step_size=1e-4)
    assert Js.shape == Jf.shape and np.abs(Js - Jf).max() < 1e-8 / 1e-4      # densities to 1e-8, divided by the step
