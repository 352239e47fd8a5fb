"""GPU: the localisation cases of tests/loc_cases.py on the device kernels (csrc/loc_ops.hip), both variants, and get_loc / the BE keywords on the device."""
import numpy as np
import pytest

import loc_cases as lc

pytestmark = pytest.mark.gpu


def test_trivial_sizes(qlib):
    lc.check_trivial(qlib)
    lc.check_no_sweeps(qlib)
    lc.check_max_sweeps(qlib)
    lc.check_diagonal_stack(qlib)


@pytest.mark.parametrize("m", [2, 3, 6, 59, 60])
def test_one_matrix_is_the_eigenproblem(qlib, m):
    lc.check_eigen(qlib, m, 11 + m)


@pytest.mark.parametrize("K,m", [(3, 3), (3, 12), (3, 45), (17, 21)])
def test_commuting_stack_is_diagonalised(qlib, K, m):
    lc.check_commuting(qlib, K, m, 21 + m)


@pytest.mark.parametrize("kind,K,m", lc.RANDOM)
def test_random_stack_against_the_twin(qlib, kind, K, m):
    lc.check_random(qlib, kind, K, m)


@pytest.mark.parametrize("m", [511, 512])
def test_rounds_variant_at_its_largest_m(qlib, m):
    lc.check_rounds_limit(qlib, m)


def test_guard_and_refusals(qlib):
    lc.check_guard(qlib)
    lc.check_refusals(qlib)


# ---- dipole integrals on the device
import int1e_cases as ic


@pytest.mark.parametrize("la,lb", ic.PAIR_CLASSES)
def test_dipole_device_against_quadrature_and_host(qlib, la, lb):
    lc.check_dipole_class(la, lb, backend="hip", lib=qlib)


def test_dipole_host_and_device_agree_on_the_systems(qlib):
    lc.check_dipole_backends(qlib)


# ---- get_loc on the device
@pytest.mark.parametrize("name", ["h8", "h8-dz", "octane"])
@pytest.mark.parametrize("method,pop", [("boys", None), ("PM", None), ("PM", "mulliken"), ("cholesky", None)])
def test_get_loc(qlib, name, method, pop):
    lc.check_get_loc(qlib, name, method, pop)


@pytest.mark.parametrize("name,kind", [("h8", "cholesky"), ("h8", "fitted"), ("h8-dz", "cholesky"), ("octane", "cholesky")])
def test_get_loc_er(qlib, name, kind):
    lc.check_get_loc(qlib, name, "ER", df=lc.dense_context(qlib, name, kind))


def test_get_loc_refusals(qlib):
    lc.check_get_loc_refusals(qlib)


# ---- the BE keywords on the device
@pytest.mark.parametrize("name", ["h8", "octane"])
@pytest.mark.parametrize("method", ["cholesky", "ER", "PM", "boys"])
def test_be_bath_localisation(qlib, name, method):
    lc.check_be_bath(qlib, name, method)


@pytest.mark.parametrize("name", ["h8", "octane"])
@pytest.mark.parametrize("method", ["boys", "PM"])
def test_be_lo_method(qlib, name, method):
    lc.check_be_lo_method(qlib, name, method)


@pytest.mark.parametrize("name", ["h8", "octane"])
def test_be_lo_method_pm_mulliken_rotates(qlib, name):
    be = lc.check_be_lo_method(qlib, name, "PM", pop_method="mulliken")
    assert be.lo_stats["W"]["f_after"] > be.lo_stats["W"]["f_before"] * (1.0 + 1e-6)


@pytest.mark.parametrize("name", ["h8", "octane"])
def test_be_lo_method_er_on_the_cholesky_route(qlib, name):
    # the factor holds the integrals to cd_tol = 1e-8 element by element: HF-in-HF against the exact mean field within 1e-6 (a sum over N^2 density elements)
    lc.check_be_lo_method(qlib, name, "ER", hf_bar=1e-6, **lc.CHOLESKY_ROUTE)


def test_be_lo_method_frozen_core(qlib):
    lc.check_be_lo_method(qlib, "octane", "PM", frozen=True)
    lc.check_be_lo_method(qlib, "octane", "boys", frozen=True)


@pytest.mark.parametrize("name", ["h8", "octane"])
def test_be_defaults_are_bit_identical(qlib, name):
    lc.check_be_defaults(qlib, name)


def test_be_refusals(qlib):
    lc.check_be_refusals(qlib)
