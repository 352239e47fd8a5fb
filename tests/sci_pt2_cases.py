"""The cases of the second-order correction of solver="SCI-hip" (DeviceFragment.sci_pt2, BE.sci_pt2) that tests/test_sci_pt2_hostlogic.py (scalar mock device, CPU)
and tests/test_gpu_sci_pt2.py (MI355X) both run: every function takes the library to drive.  The reference is the twin tests/sci_pt2_numpy.py on the states of
tests/sci_cases.py (same seeds and families); one case is independent of the Slater-Condon twin (the operator-form sigma of tests/fci_numpy.py).
Which determinants count is decided at a threshold, so every comparison first asserts the twin's margin = min | |H_ai c_i| / eps_pt - 1 | >= sci_cases.MARGIN.
Bars: 1e-11 * sum_a |contribution_a| for the energy (the project's figure for one application of H), 1e-12 of the same sum between two orders of the ranges,
sci_cases.TOL (1e-8) at the fragment level, where the device's own orbitals, vector and e_sci go into the twin."""
from functools import lru_cache

import numpy as np
import pytest

import fci_numpy as fnp
import sci_cases as sc
import sci_numpy as snp
import sci_pt2_numpy as ptn

# (n, o, family, eps_var, eps_pt) on the final space of sc.twin_state, with the n_ext the issue records for it
OPS = [(4, 2, "default", 1e-3, 1e-6, 17), (6, 3, "default", 1e-2, 1e-4, 102), (6, 3, "default", 1e-2, 1e-6, 359), (6, 3, "strong", 1e-2, 1e-4, 131),
       (6, 3, "strong", 1e-2, 1e-6, 131), (7, 3, "default", 1e-3, 1e-4, 102), (7, 3, "default", 1e-3, 1e-6, 904)]
ROWS = [(6, 3, "default", 1e-2), (6, 3, "strong", 1e-2), (7, 3, "default", 1e-3)]      # rows 2-4 of that table
FRAGMENTS = [(6, 3, "strong", 1e-2), (7, 3, "default", 1e-3)]      # ((6, 3) strong at 1e-3 selects the whole space: nothing is left outside)
# sc.wide_state history[1]: orbitals on both sides of bit 31 / 32, and bit 63; (eps_pt, passing products).  (34, 2) at 1e-5 or 3e-6 has margins below 1e-7.
WIDE = [(34, 2, "default", 1e-3, 1e-4, 63820), (64, 1, "default", 1e-3, 1e-5, 82690)]


def smallest_cap(n, o):
    v = n - o
    nexc = 2 * o * v + 2 * (o * (o - 1) // 2) * (v * (v - 1) // 2) + (o * v) ** 2
    cap = 2
    while cap < 2 * nexc:
        cap <<= 1
    return cap


@lru_cache(maxsize=None)
def state(n, o, family, eps_var):
    """(h, V, dets, c, e_var) of the twin's converged selection"""
    hm, Vm, r = sc.twin_state(n, o, family, eps_var)
    return hm, Vm, r["dets"], r["c"], r["e"]


@lru_cache(maxsize=None)
def wide(n, o, family, eps_var):
    """the second space of sc.wide_state with e_var = c.H.c from its stored matrix"""
    hm, Vm, r = sc.wide_state(n, o, family, eps_var)
    dets, c = r["history"][1][:2]
    return hm, Vm, dets, c, float(c @ (r["H"] @ c))


@lru_cache(maxsize=None)
def twin(n, o, family, eps_var, eps_pt):
    hm, Vm, dets, c, e = state(n, o, family, eps_var)
    r = ptn.pt2(hm, Vm, n, dets, c, e, eps_pt)
    print(f"pt2 twin ({n},{o}) {family} eps_var={eps_var:g} eps_pt={eps_pt:g}: N = {len(dets)} n_ext = {r['n_ext']} products = {r['products']} e_pt2 = {r['e_pt2']:.12f} "
          f"margin = {r['margin']:.3e}")
    return r


@lru_cache(maxsize=None)
def twin_wide(n, o, family, eps_var, eps_pt):
    """about 25 s of NumPy at (34, 2): once per session"""
    hm, Vm, dets, c, e = wide(n, o, family, eps_var)
    r = ptn.pt2_many(hm, Vm, n, dets, c, e, eps_pt)
    print(f"pt2 twin ({n},{o}) wide eps_pt={eps_pt:g}: N = {len(dets)} n_ext = {r['n_ext']} products = {r['products']} e_pt2 = {r['e_pt2']:.12f} margin = {r['margin']:.3e}")
    return r


def run_op(lib, st, o, eps_pt, **kw):
    from quemb_amd.fragsolver import sci_pt2
    hm, Vm, dets, c, e = st
    return sci_pt2(hm, Vm, o, *sc.words(dets), c, e, eps_pt, lib=lib, **kw)


def compare(got, ref, bar=1e-11):
    assert ref["margin"] >= sc.MARGIN, ref["margin"]
    err = abs(got["e_pt2"] - ref["e_pt2"])
    print(f"   e_pt2 = {got['e_pt2']:.14f} (twin {ref['e_pt2']:.14f}) |d| = {err:.2e}, bar {bar * ref['abs_sum']:.2e}; n_ext = {got['n_ext']} batches = {got['batches']}")
    assert got["n_ext"] == ref["n_ext"], (got["n_ext"], ref["n_ext"])
    assert err <= bar * ref["abs_sum"], (err, bar * ref["abs_sum"])


# ---------------------------------------------------------------- the operation
def check_op_against_twin(lib, n, o, family, eps_var, eps_pt, n_ext):
    """the twin's own (dets, c, E): n_ext equal, the energy to 1e-11 sum |contribution|; default slabs, and slabs of three determinants with the smallest buffer"""
    ref = twin(n, o, family, eps_var, eps_pt)
    assert ref["n_ext"] == n_ext, (ref["n_ext"], n_ext)      # (the twin against the recorded count)
    for kw in (dict(), dict(slab=3, cap=smallest_cap(n, o))):
        got = run_op(lib, state(n, o, family, eps_var), o, eps_pt, **kw)
        compare(got, ref)
        assert got["batches"] == 1


def check_independent_of_the_twin(lib, n, o, family, eps_var, eps_pt=1e-14):
    """eps_pt -> 0 against sum_{a outside V} sigma_a^2 / (E - H_aa) with sigma = H c in the operator form of tests/fci_numpy.py and the diagonal of its brute-force
    matrix: nothing of the Slater-Condon twin but the position of the determinants in the full space"""
    hm, Vm, dets, c, e = state(n, o, family, eps_var)
    full = snp.full_vector(dets, c, n, o)
    sig = fnp.sigma(hm, Vm, full, o)
    diag = np.diag(fnp.hamiltonian_matrix(hm, Vm, o)).reshape(sig.shape)
    outside = snp.full_vector(dets, np.ones(len(dets)), n, o) == 0.0
    contrib = sig[outside] ** 2 / (e - diag[outside])
    got = run_op(lib, state(n, o, family, eps_var), o, eps_pt)
    err = abs(got["e_pt2"] - contrib.sum())
    print(f"pt2 ({n},{o}) {family} at eps_pt = {eps_pt:g}: {got['e_pt2']:.14f}, operator form {contrib.sum():.14f}, |d| = {err:.2e}, bar {1e-11 * np.abs(contrib).sum():.2e}")
    assert err <= 1e-11 * np.abs(contrib).sum()
    assert got["n_ext"] <= int(outside.sum())


def check_wide_words(lib, n, o, family, eps_var, eps_pt, products):
    ref = twin_wide(n, o, family, eps_var, eps_pt)
    assert ref["products"] == products, (ref["products"], products)
    compare(run_op(lib, wide(n, o, family, eps_var), o, eps_pt), ref)


def check_batches(lib, wide_max_ext=4096):
    """ranges of the alpha word: (7, 3) at 1e-6 in ranges of at most 64 (at least 15 of them for 904 externals), (34, 2) in ranges of at most 4096 (the scalar
    mock, where every range is another screen of 4901 determinants in scalar loops, takes 16384); the same
    count, the energy to 1e-12 sum |contribution| of the one-range run (the ranges are summed one after another: another order of additions).  A bound that a
    single alpha word exceeds is refused."""
    from quemb_amd import _lib
    from quemb_amd._lib import QembError
    for st, ref, o, eps_pt, max_ext, least in ((state(7, 3, "default", 1e-3), twin(7, 3, "default", 1e-3, 1e-6), 3, 1e-6, 64, 15),
                                               (wide(34, 2, "default", 1e-3), twin_wide(34, 2, "default", 1e-3, 1e-4), 2, 1e-4, wide_max_ext, 2)):
        assert ref["margin"] >= sc.MARGIN
        one = run_op(lib, st, o, eps_pt)
        many = run_op(lib, st, o, eps_pt, max_ext=max_ext)
        print(f"pt2 batches: max_ext = {max_ext}: {many['batches']} ranges, n_ext = {many['n_ext']}, |d| = {abs(many['e_pt2'] - one['e_pt2']):.2e}")
        assert one["batches"] == 1 and many["batches"] >= least and many["batches"] > 1
        assert many["n_ext"] == one["n_ext"] == ref["n_ext"] and ref["n_ext"] > max_ext
        assert abs(many["e_pt2"] - one["e_pt2"]) <= 1e-12 * ref["abs_sum"]
    with pytest.raises(QembError, match="max_ext") as ei:
        run_op(lib, state(6, 3, "default", 1e-2), 3, 1e-4, max_ext=1)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC


def check_same_bits(lib):
    """no atomics, one order of additions: the same call twice returns the identical double, on the operation (one range and several) and on the fragment"""
    st = state(7, 3, "default", 1e-3)
    for kw in (dict(), dict(max_ext=64)):
        a, b = run_op(lib, st, 3, 1e-6, **kw), run_op(lib, st, 3, 1e-6, **kw)
        assert a == b and a["e_pt2"] != 0.0, (a, b)
    fr, _ = solved_fragment(lib, 6, 3, "strong", "block", 1e-2)
    x, y = fr.sci_pt2(1e-6), fr.sci_pt2(1e-6)
    assert x["e_pt2"] == y["e_pt2"] and x["n_ext"] == y["n_ext"] and x["e_pt2"] != 0.0


def check_is_the_second_order_correction(lib, n, o, family, eps_var):
    """at eps_pt = 1e-9 the corrected energy lies at least four times nearer to FCI than the variational one (the twin: ratios 0.004, 0.10, 0.009)"""
    hm, Vm, dets, c, e = state(n, o, family, eps_var)
    e_fci = fnp.ground_state(hm, Vm, o)[0]
    got = run_op(lib, state(n, o, family, eps_var), o, 1e-9)
    ratio = abs(e + got["e_pt2"] - e_fci) / abs(e - e_fci)
    print(f"pt2 ({n},{o}) {family}: e_var - e_fci = {e - e_fci:.3e}, e_var + e_pt2 - e_fci = {e + got['e_pt2'] - e_fci:.3e}, ratio {ratio:.4f}")
    assert got["e_pt2"] < 0.0 and abs(e + got["e_pt2"] - e_fci) <= 0.25 * abs(e - e_fci)


# ---------------------------------------------------------------- the fragment
_FRAGMENTS = {}


def solved_fragment(lib, n, o, family, residency, eps_var):
    """(fragment after solve_sci, its outputs); kept for the session, the solve left unchanged"""
    from quemb_amd.fragsolver import default_sci_opts
    key = (id(lib), n, o, family, residency, eps_var)
    if key not in _FRAGMENTS:
        fr = sc.fragment(lib, n, o, family, residency)
        out = fr.solve_sci(o, sc.inputs(n, o, family)[0], opts=sc.scf_opts(lib), sci_opts=default_sci_opts(lib, eps_var=eps_var), eeval=True, want_dets=True)
        _FRAGMENTS[key] = (fr, out)
    return _FRAGMENTS[key]


def check_exact_zero(lib, n=6, o=3, family="strong", eps_var=1e-2):
    """after a converged selection the last screen used this same vector and found nothing: eps_pt = eps_var gives exactly zero"""
    fr, out = solved_fragment(lib, n, o, family, "block", eps_var)
    r = fr.sci_pt2(eps_var)
    assert r["e_pt2"] == 0.0 and r["n_ext"] == 0 and r["e_var"] == out["e_sci"], r
    assert fr.sci_pt2(10 * eps_var)["e_pt2"] == 0.0


def check_fragment(lib, n, o, family, eps_var, residency, eps_pt=1e-6):
    """DeviceFragment.solve_sci, then sci_pt2, against the twin on the device's own determinants, vector, e_sci and orbitals; solve_sci(pt2_eps=...) appends it"""
    from math import comb
    from quemb_amd.fragsolver import default_sci_opts
    from quemb_amd.solver import solve_sci
    from qemb_oracle import eri
    h, e1, Bp = sc.inputs(n, o, family)[:3]
    fr, out = solved_fragment(lib, n, o, family, residency, eps_var)
    C = out["mo_coeff"]
    a, b, c = out["dets"]
    ref = ptn.pt2(C.T @ h @ C, fnp.mo_eri(e1, C), n, sc.pairs(a, b), c, out["e_sci"], eps_pt)
    got = fr.sci_pt2(eps_pt)
    print(f"pt2 fragment ({n},{o}) {family} eps_var={eps_var:g} {residency}: ndet = {out['ndet']} e_pt2 = {got['e_pt2']:.12f} twin {ref['e_pt2']:.12f} n_ext = {got['n_ext']} margin = {ref['margin']:.3e} "
          f"ms = {got['ms']}")
    assert ref["margin"] >= sc.MARGIN, ref["margin"]
    assert got["n_ext"] == ref["n_ext"] and got["batches"] == 1 and got["e_var"] == out["e_sci"] and set(got["ms"]) == {"screen", "merge", "rows"}
    assert abs(got["e_pt2"] - ref["e_pt2"]) < sc.TOL and got["e_pt2"] < 0.0
    ns = comb(n, o)      # (no alpha word has more externals than there are beta strings: this bound is never refused)
    few = fr.sci_pt2(eps_pt, max_ext=ns)
    assert few["batches"] > 1 and got["n_ext"] > ns and few["n_ext"] == got["n_ext"] and abs(few["e_pt2"] - got["e_pt2"]) <= 1e-12 * ref["abs_sum"]
    so = default_sci_opts(lib, eps_var=eps_var)
    kw = dict(df_factor=Bp) if residency == "factor" else {}
    plain = solve_sci(h, None if residency == "factor" else eri.pack_s4(e1), o, opts=sc.scf_opts(lib), sci_opts=so, lib=lib, **kw)
    with_pt = solve_sci(h, None if residency == "factor" else eri.pack_s4(e1), o, opts=sc.scf_opts(lib), sci_opts=so, lib=lib, pt2_eps=eps_pt, **kw)
    assert len(plain) == 2 and len(with_pt) == 3 and with_pt[0] == plain[0]
    assert abs(with_pt[-1] - got["e_pt2"]) <= 1e-12      # (another fragment object on the same inputs: the same solve to the rounding of its mean field)


def check_single_determinant(lib):
    fr, out = solved_fragment(lib, 4, 4, "default", "block", 1e-3)
    r = fr.sci_pt2(1e-6)
    assert r["e_pt2"] == 0.0 and r["n_ext"] == 0 and r["e_var"] == out["e_sci"]


def check_refusals(lib):
    import ctypes as C
    from quemb_amd import _lib
    from quemb_amd._lib import QembError
    from quemb_amd.pfrag import Frags
    from quemb_amd.solver import SHCI_ArgsUser, be_func
    n, o = 6, 3
    h = sc.inputs(n, o, "strong")[0]
    fr = sc.fragment(lib, n, o, "strong")
    with pytest.raises(QembError, match="no solve has run") as ei:
        fr.sci_pt2(1e-6)
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.solve(o, h, eeval=False)
    with pytest.raises(QembError, match="the last solve of this fragment was CCSD") as ei:
        fr.sci_pt2(1e-6)
    assert ei.value.status == _lib.QEMB_ERR_ARG
    out = fr.solve_sci(o, h, opts=sc.scf_opts(lib))
    for bad in (0.0, -1e-6):
        with pytest.raises(QembError, match="eps_pt") as ei:
            fr.sci_pt2(bad)
        assert ei.value.status == _lib.QEMB_ERR_ARG
    ok = fr.sci_pt2(1e-6, max_ext=1000)
    # the memory limit, against the formula the library reports: one byte under it is refused, the figure itself is not
    nb = C.c_int64()
    assert lib.qemb_frag_sci_pt2_bytes(n, o, out["ndet"], 1000, C.byref(nb)) == 0 and nb.value > 0
    fr.set_sci_mem_limit(nb.value - 1)
    with pytest.raises(QembError, match=r"n = 6, eps_pt = 1e-06.*bytes") as ei:
        fr.sci_pt2(1e-6, max_ext=1000)
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    fr.set_sci_mem_limit(nb.value)
    assert fr.sci_pt2(1e-6, max_ext=1000)["e_pt2"] == ok["e_pt2"]
    auto = fr.sci_pt2(1e-6)      # max_ext = 0 under the same limit: the largest count that fits
    assert auto["n_ext"] == ok["n_ext"] and abs(auto["e_pt2"] - ok["e_pt2"]) <= 1e-12 * abs(ok["e_pt2"])
    fr.set_sci_mem_limit(-1)
    assert lib.qemb_frag_sci_pt2_bytes(65, 8, 10, 10, C.byref(nb)) == _lib.QEMB_ERR_UNSUPPORTED
    # new ERIs: the kept solve is gone
    from qemb_oracle import eri
    fr.set_eri_s4(eri.pack_s4(sc.inputs(n, o, "strong")[1]))
    with pytest.raises(QembError, match="no solve has run"):
        fr.sci_pt2(1e-6)
    fr.free()
    # hci_pt inside a sweep stays refused
    f = Frags([0, 1], 0, [], [], [], [], (1.0, [0]), [0], lib=lib)
    with pytest.raises(NotImplementedError, match="hci_pt"):
        be_func(None, [f], 1, "SCI-hip", 0.0, solver_args=SHCI_ArgsUser(hci_pt=True))
    with pytest.raises(RuntimeError, match="SCI-hip"):
        f.sci_pt2(1e-6)


# ---------------------------------------------------------------- the BE driver
def check_h8_be2(lib):
    key = "test_autogen_h_linear_be2"
    b = sc.h_chain(lib, 8, key)
    with pytest.raises(RuntimeError, match="SCI-hip"):
        b.sci_pt2(1e-6)
    e_corr, comps = b.oneshot(solver="SCI-hip")
    before = (b.ebe_tot, b.e_corr, np.array(b.e_components, dtype=float).copy())
    res = b.sci_pt2(1e-6)
    assert len(res) == len(b.Fobjs) and all(set(r) == {"e_var", "e_pt2", "n_ext", "batches", "ms"} for r in res)
    for f, r in zip(b.Fobjs, res):
        one = f.sci_pt2(1e-6)
        print(f"H8 BE2 fragment {b.Fobjs.index(f)}: e_var = {r['e_var']:.10f} e_pt2 = {r['e_pt2']:.3e} n_ext = {r['n_ext']}")
        assert r["e_pt2"] <= 0.0 and r["e_pt2"] == one["e_pt2"] == f.e_pt2 and r["n_ext"] == one["n_ext"]
    assert any(r["e_pt2"] < 0.0 for r in res)
    assert (b.ebe_tot, b.e_corr) == before[:2] and np.array_equal(np.array(b.e_components, dtype=float), before[2]) and e_corr == b.e_corr
    c = sc.h_chain(lib, 8, key)
    c.oneshot(solver="CCSD")
    with pytest.raises(RuntimeError, match="SCI-hip"):
        c.sci_pt2(1e-6)
