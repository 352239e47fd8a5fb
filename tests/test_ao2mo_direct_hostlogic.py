"""The integral-direct AO -> fragment transform (csrc/int4c.cpp: int4c_ao2mo_direct) through the scalar twin of the mock library: the tile form of the quartet
items (int4c_core.h: kTile), the slabs and the tile loop of the driver, the pair-product and add-transpose passes, screening of quartets and tiles, the memory
guard, the refusals and the Python surface up to BE(int_transform="int-direct-hip"), without a device."""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck")); sys.path.insert(0, str(ROOT / "tests"))

import ao2mo_direct_cases as cases
from quemb_amd import _lib


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    return _lib.declare(C.CDLL(str(hc_build.build())))


@pytest.mark.parametrize("tile_pairs", [1, 7, 40, 1000])
def test_tiles_are_the_stored_integrals(hlib, tile_pairs):
    n_transposed, n_big = cases.check_tiles(hlib, "spd3", tile_pairs)
    if tile_pairs <= 7:
        assert n_transposed > 0 and n_big >= 6      # the d-d shell pairs (15 or 25 AO pairs) are slabs of their own
    if tile_pairs == 1000:
        assert (n_transposed, n_big) == (0, 0)      # npair = 378: one slab, one R = S tile


@pytest.mark.parametrize("name", ["h4_ccpvdz", "h8_sto3g"])
def test_tiles_of_the_other_molecules(hlib, name):
    cases.check_tiles(hlib, name, 7)


@pytest.mark.parametrize("name", ["spd3", "h4_ccpvdz", "h8_sto3g"])
def test_identity_transform(hlib, name):
    cases.check_identity(hlib, name)


@pytest.mark.parametrize("name", ["spd3", "h4_ccpvdz"])
def test_against_the_stored_route(hlib, name):
    cases.check_random(hlib, name)


def test_h8_be2_fragments(hlib):
    cases.check_h8_fragments(hlib)


def test_many_fragments_one_pass(hlib):
    cases.check_many(hlib)


def test_tile_size_independence_and_reproducibility(hlib):
    cases.check_tile_independence(hlib)


def test_memory_guard(hlib):
    cases.check_memory(hlib)


def test_footprint_does_not_follow_npair_squared(hlib):
    cases.check_bytes_do_not_follow_npair_squared(hlib)


def test_screening_of_quartets_and_tiles(hlib):
    cases.check_screening(hlib)


def test_be_end_to_end(hlib):
    cases.check_end_to_end_h8(hlib)


def test_refusals(hlib):
    cases.check_refusals(hlib)
