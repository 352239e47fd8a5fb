"""The integral-direct AO -> fragment transform on the device (csrc/int4c_ops.hip: the kTile form of int4c_class_kernel, int4c_pairprod_kernel,
int4c_addt_kernel; driver csrc/int4c.cpp: int4c_ao2mo_direct): tiles against the stored integrals, the identity transform, the stored route, many fragments in
one pass, tile-size independence, the memory guard, screening, BE end to end and the refusals.  The cases are those of ao2mo_direct_cases.py, shared with the
scalar-twin tests."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import ao2mo_direct_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tile_pairs", [1, 7, 40, 1000])
def test_tiles_are_the_stored_integrals(qlib, tile_pairs):
    n_transposed, n_big = cases.check_tiles(qlib, "spd3", tile_pairs)
    if tile_pairs <= 7:
        assert n_transposed > 0 and n_big >= 6      # the d-d shell pairs (15 or 25 AO pairs) are slabs of their own
    if tile_pairs == 1000:
        assert (n_transposed, n_big) == (0, 0)      # npair = 378: one slab, one R = S tile


@pytest.mark.parametrize("name", ["h4_ccpvdz", "h8_sto3g"])
def test_tiles_of_the_other_molecules(qlib, name):
    cases.check_tiles(qlib, name, 7)


@pytest.mark.parametrize("name", ["spd3", "h4_ccpvdz", "h8_sto3g"])
def test_identity_transform(qlib, name):
    cases.check_identity(qlib, name)


@pytest.mark.parametrize("name", ["spd3", "h4_ccpvdz"])
def test_against_the_stored_route(qlib, name):
    cases.check_random(qlib, name)


def test_h8_be2_fragments(qlib):
    cases.check_h8_fragments(qlib)


def test_many_fragments_one_pass(qlib):
    cases.check_many(qlib)


def test_tile_size_independence_and_reproducibility(qlib):
    cases.check_tile_independence(qlib)


def test_memory_guard(qlib):
    cases.check_memory(qlib)


def test_footprint_does_not_follow_npair_squared(qlib):
    cases.check_bytes_do_not_follow_npair_squared(qlib)


def test_screening_of_quartets_and_tiles(qlib):
    cases.check_screening(qlib)


@pytest.mark.parametrize("solver", ["MP2", "CCSD"])
def test_be_end_to_end_h8(qlib, solver):
    cases.check_end_to_end_h8(qlib, solver)


def test_be_end_to_end_octane(qlib):
    cases.check_end_to_end_octane(qlib)


def test_refusals(qlib):
    cases.check_refusals(qlib)
