"""CPU: the localisation cases of tests/loc_cases.py on the hostcheck mock (the C ABI, the sweep driver, both variants' orders of summation in their scalar
restatement), the NumPy twin against independent answers, and the host pieces of quemb_amd.lo and of the BE keywords."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import loc_cases as lc
import loc_numpy as ln

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def mock():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


# ---- the twin itself
def test_twin_pair_order_is_a_tournament():
    for m in (2, 3, 4, 7, 10):
        np_ = m + (m & 1)
        seen = set()
        for r in range(np_ - 1):
            row = [ln.rr_pair(np_, r, j) for j in range(np_ // 2)]
            assert sorted(x for pq in row for x in pq) == list(range(np_))      # the rotations of a round are disjoint
            seen.update(row)
        assert len(seen) == np_ * (np_ - 1) // 2                                 # a sweep meets every pair once


def test_twin_angle_rule_maximises_the_pair_functional():
    """the algebra of the angle rule, checked by brute force: no angle on a fine grid does better than the rule's, and the gain is hypot - (sum d^2 - sum a^2)"""
    r = np.random.default_rng(3)
    for _ in range(20):
        Q = lc.random_stack(4, 2, int(r.integers(1 << 30)))
        th = ln.pair_angle(Q, 0, 1, (Q ** 2).sum())
        assert -np.pi / 4 < th <= np.pi / 4

        def f(t):
            G = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
            return ln.functional(np.einsum("ip,kij,jq->kpq", G, Q, G))
        grid = np.linspace(-np.pi / 4, np.pi / 4, 2001)
        assert f(th) >= max(f(t) for t in grid) - 1e-12 * (Q ** 2).sum()
        a, d = Q[:, 0, 1], 0.5 * (Q[:, 0, 0] - Q[:, 1, 1])
        x, y = d @ d - a @ a, 2 * a @ d
        assert abs((f(th) - f(0.0)) - (np.hypot(x, y) - x)) <= 1e-12 * (Q ** 2).sum()


def test_twin_leaves_a_pairwise_saddle():
    Q = np.array([[[0.0, 1.0], [1.0, 0.0]]])      # d = 0, a = 1: sum a d = 0 and sum d^2 < sum a^2
    assert abs(ln.pair_angle(Q, 0, 1, 2.0) - np.pi / 4) < 1e-15
    Qr, U, sw, f, cv = ln.joint_diag(Q)
    assert cv and abs(f - 2.0) < 1e-14


# ---- the kernel cases on the mock
def test_trivial_sizes(mock):
    lc.check_trivial(mock)
    lc.check_no_sweeps(mock)
    lc.check_max_sweeps(mock)
    lc.check_diagonal_stack(mock)


@pytest.mark.parametrize("m", [2, 3, 6, 59, 60])
def test_one_matrix_is_the_eigenproblem(mock, m):
    lc.check_eigen(mock, m, 11 + m)


@pytest.mark.parametrize("K,m", [(3, 3), (3, 12), (3, 45), (17, 21)])
def test_commuting_stack_is_diagonalised(mock, K, m):
    lc.check_commuting(mock, K, m, 21 + m)


@pytest.mark.parametrize("kind,K,m", lc.RANDOM)
def test_random_stack_against_the_twin(mock, kind, K, m):
    lc.check_random(mock, kind, K, m)


@pytest.mark.parametrize("m", [511, 512])
def test_rounds_variant_at_its_largest_m(mock, m):
    lc.check_rounds_limit(mock, m)


def test_guard_and_refusals(mock):
    lc.check_guard(mock)
    lc.check_refusals(mock)


# ---- dipole integrals (host source) against the quadrature
import int1e_cases as ic


@pytest.mark.parametrize("la,lb", ic.PAIR_CLASSES)
def test_dipole_host_against_quadrature(la, lb):
    lc.check_dipole_class(la, lb)


@pytest.mark.parametrize("la,lb", ic.PAIR_CLASSES)
def test_dipole_mock_against_quadrature_and_host(mock, la, lb):
    lc.check_dipole_class(la, lb, backend="hip", lib=mock)


def test_dipole_host_and_mock_agree_on_the_systems(mock):
    lc.check_dipole_backends(mock)


# ---- get_loc on the mock
def test_cholesky_mos():
    lc.check_cholesky_mos()


@pytest.mark.parametrize("name", ["h8", "h8-dz", "octane"])
@pytest.mark.parametrize("method,pop", [("boys", None), ("PM", None), ("PM", "mulliken"), ("cholesky", None)])
def test_get_loc(mock, name, method, pop):
    lc.check_get_loc(mock, name, method, pop)


@pytest.mark.parametrize("name,kind", [("h8", "cholesky"), ("h8", "fitted"), ("h8-dz", "cholesky"), ("octane", "cholesky")])
def test_get_loc_er(mock, name, kind):
    lc.check_get_loc(mock, name, "ER", df=lc.dense_context(mock, name, kind))


def test_get_loc_refusals(mock):
    lc.check_get_loc_refusals(mock)


# ---- the BE keywords on the mock (H8 BE2; octane runs on the device)
@pytest.mark.parametrize("method", ["cholesky", "ER", "PM", "boys"])
def test_be_bath_localisation_h8(mock, method):
    lc.check_be_bath(mock, "h8", method)


@pytest.mark.parametrize("method", ["boys", "PM"])
def test_be_lo_method_h8(mock, method):
    lc.check_be_lo_method(mock, "h8", method)


def test_be_lo_method_pm_mulliken_and_er_h8(mock):
    be = lc.check_be_lo_method(mock, "h8", "PM", pop_method="mulliken")
    assert be.lo_stats["W"]["f_after"] > be.lo_stats["W"]["f_before"] * (1.0 + 1e-6)
    lc.check_be_lo_method(mock, "h8", "ER", hf_bar=1e-6, **lc.CHOLESKY_ROUTE)
    lc.check_be_lo_method(mock, "h8", "ER", hf_bar=1e-3, int_transform="int-direct-DF-hip", auxbasis="etb")      # fitted: HF-in-HF to the fitting error


def test_be_defaults_and_refusals(mock):
    lc.check_be_defaults(mock, "h8")
    lc.check_be_refusals(mock)
