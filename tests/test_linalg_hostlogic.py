"""CPU: the cases and assertions of tests/linalg_cases.py rehearsed before anything runs on a GPU.  With NumPy as the solver every case and every bar (the bars can be
met, the builders build what they say); with the hostcheck mock the eigh, eigh-in-basis, Cholesky, inverse, refusal and non-finite cases (the C ABI, the status
codes and the messages).  The mock's SVD is eigh(G^T G) by design -- it squares the condition number -- and is exempt from the SVD accuracy cases."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import linalg_cases as lc

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))

MOCK_SIZES = (1, 2, 3, 80, 97)                           # the mock has one path: small, even, odd


@pytest.fixture(scope="module")
def mock():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    s = lc.LibSolver(lib)
    s.name = "mock"
    return s


@pytest.fixture(scope="module")
def lapack():
    return lc.NumpySolver()


def _solver(request, which):
    return request.getfixturevalue(which)


# ---- the builders
def test_builders_build_what_they_say():
    for n in (1, 2, 3, 80, 97, 300):
        for family in lc.EIGH_FAMILIES:
            A = lc.eigh_matrix(family, n)
            assert A.shape == (n, n) and np.array_equal(A, A.T) and np.isfinite(A).all()
            assert np.array_equal(lc.eigh_matrix(family, n, 40), A * 2.0 ** 40)
    w = lc.eigh_reference("graded", 300)[0]
    assert w.min() < -0.99 and w.max() > 0.99 and np.abs(w).min() < 1e-13                       # fourteen decades, both signs
    w = lc.eigh_reference("projector", 97)[0]
    assert ((w > 1e-10) & (w < 1 - 1e-10)).sum() == 6 and (np.abs(w) < 1e-10).sum() > 20 and (np.abs(w - 1) < 1e-10).sum() > 20
    w = lc.eigh_reference("kron", 96)[0]
    assert np.abs(w[0::2] - w[1::2]).max() < 1e-13                                              # double degeneracy (LAPACK splits it by a few eps ||A||)
    w = lc.eigh_reference("pairs", 80)[0]
    assert np.abs(w + w[::-1]).max() < 1e-13
    w = lc.eigh_reference("clusters", 129)[0]
    assert len(set(np.round(w, 6))) == 3 and np.ptp(w[np.round(w, 6) == 2.0]) > 1e-10
    assert np.array_equal(lc.eigh_matrix("diagonal", 80), np.diag(np.diag(lc.eigh_matrix("diagonal", 80)))) and len(set(np.diag(lc.eigh_matrix("diagonal", 80)))) < 8
    assert lc.eigh_reference("negdef", 81)[0].max() < 0.0
    for (m, n) in lc.SVD_SHAPES:
        for family in lc.SVD_FAMILIES:
            assert lc.svd_matrix(family, m, n).shape == (m, n)
    assert (lc.svd_reference("lowrank", 150, 40) > 1e-10 * lc.svd_reference("lowrank", 150, 40)[0]).sum() == 3
    assert np.abs(lc.svd_reference("orthonormal", 500, 64) - 1.0).max() < 1e-14
    s = lc.svd_reference("gradedsv", 300, 40)
    assert abs(s[0] - 1.0) < 1e-12 and abs(s[-1] / 1e-12 - 1.0) < 1e-3
    s = lc.svd_reference("schmidt", 100, 70)
    assert s.max() <= 0.5 + 1e-12 and (s < 1e-10).sum() >= 70 - 56                              # sigma^2 = lambda (1 - lambda); rank <= nocc = 56
    for n in lc.CHOL_SIZES:
        for k in lc.CHOL_DECADES:
            w = np.linalg.eigvalsh(lc.spd_matrix(n, k))
            assert w[0] > 0.0 and (n == 1 or abs(np.log10(w[-1] / w[0]) - k) < 0.01 + 1e-3 * k)
    M = lc.octane_metric()
    assert M.shape[0] > 64 and np.linalg.eigvalsh(M)[0] > 0.0
    assert lc.plant(np.zeros((4, 4)), np.inf, "offdiagonal", True)[3, 1] == np.inf
    assert abs(lc.gamma(301) / (301 * 2.0 ** -53) - 1.0) < 1e-12


# ---- NumPy through every case
@pytest.mark.parametrize("family", lc.EIGH_FAMILIES)
def test_numpy_eigh_families(lapack, family):
    worst = 0.0
    for n in sorted(lc.EIGH_SIZES):
        r = lc.check_eigh(lapack, family, n)
        worst = max(worst, r["w"])
    for n in lc.EIGH_SCALED_SIZES:
        for e in (40, -40):
            worst = max(worst, lc.check_eigh(lapack, family, n, e)["w"])
    assert worst < 0.1                                   # the reference is reproducible far inside the bar
    for n in lc.IN_BASIS_SIZES:
        lc.check_eigh_in_basis(lapack, family, n)


@pytest.mark.parametrize("family", lc.SVD_FAMILIES)
def test_numpy_svd_families(lapack, family):
    for (m, n) in sorted(lc.SVD_SHAPES):
        lc.check_svd(lapack, family, m, n)


@pytest.mark.parametrize("which", ["lapack", "mock"])
def test_cholesky_and_inverse(request, which):
    solver = _solver(request, which)
    worst = 0.0
    for n in lc.CHOL_SIZES:
        for k in lc.CHOL_DECADES:
            worst = max(worst, lc.check_cholesky(solver, lc.spd_matrix(n, k), f"kappa=1e{k}")["backward"])
            lc.check_tri_inverse(solver, lc.spd_matrix(n, k), f"kappa=1e{k}")
    lc.check_cholesky(solver, lc.octane_metric(), "octane12 metric")
    lc.check_tri_inverse(solver, lc.octane_metric(), "octane12 metric")
    assert worst < 1.0 / 8.0                             # an unblocked factorisation is inside the bare bound; the factor 8 is for the blocked panel step


@pytest.mark.parametrize("which", ["lapack", "mock"])
def test_cholesky_refusals(request, which):
    solver = _solver(request, which)
    for label, A in lc.refusal_cases():
        lc.check_cholesky_refuses(solver, A, label)


@pytest.mark.parametrize("which", ["lapack", "mock"])
def test_nonfinite_input_is_refused(request, which):
    solver = _solver(request, which)
    for value in lc.NONFINITE_VALUES:
        for place in lc.NONFINITE_PLACES:
            for n in (40, 90):
                lc.check_nonfinite(solver, "eigh", n, value, place)
            lc.check_nonfinite(solver, "eigh_in_basis", 40, value, place)
            for shape in ((96, 64), (300, 22)):
                lc.check_nonfinite(solver, "svd", shape, value, place)
            for n in lc.NONFINITE_CHOL_SIZES:
                lc.check_nonfinite(solver, "cholesky", n, value, place)


# ---- the mock through the eigen cases
@pytest.mark.parametrize("family", lc.EIGH_FAMILIES)
def test_mock_eigh_families(mock, family):
    for n in MOCK_SIZES:
        lc.check_eigh(mock, family, n)
    for e in (40, -40):
        lc.check_eigh(mock, family, 80, e)
    for n in (1, 2, 3, 80):
        lc.check_eigh_in_basis(mock, family, n)


def test_a_wrong_answer_is_seen(lapack):
    """the checks themselves: a perturbed eigenvalue, a swapped pair, a dropped tie rule, an element above the Cholesky bound"""
    A = lc.eigh_matrix("graded", 80)
    w_ref, V_ref = lc.eigh_reference("graded", 80)
    good = lc.eigh_ratios(A, w_ref, V_ref, w_ref)
    assert max(good.values()) < 0.1
    w_bad = w_ref.copy(); w_bad[40] += 3e-12 * lc.row_scale(A)
    assert lc.eigh_ratios(A, w_bad, V_ref, w_ref)["w"] > 1.0
    V_bad = V_ref.copy(); V_bad[:, [0, 1]] = V_bad[:, [1, 0]]
    assert lc.eigh_ratios(A, w_ref, V_bad, w_ref)["resid"] > 1.0
    V_tie = np.eye(4); V_tie[:, 1] = V_tie[:, 0]                                                # two tied eigenvalues ranked to the same column
    assert lc.eigh_ratios(-0.75 * np.eye(4), np.full(4, -0.75), V_tie, np.full(4, -0.75))["orth"] > 1.0
    S = lc.spd_matrix(65, 8)
    L = np.linalg.cholesky(S)
    assert lc.cholesky_ratios(S, L)["backward"] < 1.0
    L[64, 3] *= 1.0 + 1e-12
    assert lc.cholesky_ratios(S, L)["backward"] > 1.0
