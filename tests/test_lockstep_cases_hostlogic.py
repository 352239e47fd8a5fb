"""The case table of the mid-size lock-step tests (tests/lockstep_cases.py) without a device: the table covers what it was written to cover, what it expects
the solver to choose is what the solver's own plan functions say, and the two small batches run through the batch driver of the mock library (which does not
tape: the merge itself is the GPU tests' business)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hostcheck"))

import lockstep_cases as lc  # noqa: E402
from helpers import GOLDEN, synthetic_scale  # noqa: E402


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


def _all():
    return [(name, o, v, seed) for name, b in lc.BATCHES.items() for o, v, seed in b["frags"]]


def test_table_covers_the_required_items():
    """every item the mid-size lock-step tests exist for appears in the table at least once: a later retuning that moves a border shows here, not as a case
    that silently checks something else"""
    ex = {(o, v): lc.expect(o, v) for _, o, v, _ in _all()}
    nov = lambda name: [o * v for o, v, _ in lc.BATCHES[name]["frags"]]
    assert set(lc.REQUIRED) == {"ring_borders", "workspace_border", "regime_edge", "golden_84", "golden_84_relaxed", "degenerate_mix", "sixteen_members", "forced_passes"}
    assert set(lc.BATCHES) == set(lc.REQUIRED) | {"unmarked_recording"} and set(lc.POSITION_MERGED) <= set(lc.BATCHES)
    assert all(2 <= len(b["frags"]) <= 8 for b in lc.BATCHES.values())
    # ring tiles on both sides of each border, inside one batch; every tile inside a tape
    assert nov("ring_borders") == [448, 896, 897, 1008, 1024]
    assert [ex[(o, v)]["ring"] for o, v, _ in lc.BATCHES["ring_borders"]["frags"]] == ["dispatcher", "dispatcher", "64x64", "64x64", "96x96k2"]
    assert {e["ring"] for e in ex.values() if e["replay"]} == {"dispatcher", "64x64", "96x96k2", "128x256"}
    # the Xw split (and the hole-hole ladder's own tile) on both sides of v = 63 / 64 at one n_occ
    assert (ex[(16, 63)]["xw_split"], ex[(16, 64)]["xw_split"]) == (False, True) and (ex[(16, 63)]["hh_tile"], ex[(16, 64)]["hh_tile"]) == (False, True)
    # region workspace below and above the 64 MB floor, and the last shape of the regime
    assert nov("workspace_border") == [1440, 1464, 1500, 2048]
    ws = [ex[(o, v)]["region_ws"] for o, v, _ in lc.BATCHES["workspace_border"]["frags"]]
    assert 0 < ws[0] <= lc.GWS_FLOOR < ws[1] < ws[2] < ws[3] and ws[:3] == [32 * x * x for x in (1440, 1464, 1500)] and ws[3] == 96 * 2048 * 2048
    assert all(ex[(o, v)]["replay"] for o, v, _ in lc.BATCHES["workspace_border"]["frags"]) and 2048 * 2048 == lc.REPLAY_LIMIT
    assert lc.expect(181, 8)["region_ws"] <= lc.GWS_FLOOR < lc.expect(23, 63)["region_ws"]      # (o v = 1448 / 1449: the border itself)
    # a batch in which one fragment is not taped at all
    assert [ex[(o, v)]["replay"] for o, v, _ in lc.BATCHES["regime_edge"]["frags"]] == [True, False, True] and len(lc.taped("regime_edge")) == 2
    assert all(len(lc.taped(name)) == len(b["frags"]) for name, b in lc.BATCHES.items() if name != "regime_edge")
    # the stored fragments
    assert lc.BATCHES["golden_84"]["frags"][:2] == [lc.FRAG84, lc.FRAG84] and lc.BATCHES["golden_84_relaxed"]["frags"][0] == lc.FRAG84
    assert lc.BATCHES["golden_84_relaxed"]["opts"]["relax_density"] == 1 and lc.BATCHES["golden_84_relaxed"]["frags"][1][:2] == (16, 56)
    assert lc.BATCHES["workspace_border"]["frags"][:2] == [(12, 120, lc.GOLDEN_SEED), (24, 61, lc.GOLDEN_SEED)]
    for fname, (o, v, seed) in (("frag84.npz", lc.FRAG84), ("frag84_relaxed.npz", lc.FRAG84), ("frag132.npz", (12, 120, lc.GOLDEN_SEED)), ("frag85_lockstep.npz", (24, 61, lc.GOLDEN_SEED))):
        g = np.load(GOLDEN / fname)
        assert (int(g["n"]), int(g["o"]), int(g["seed"])) == (o + v, o, seed), fname
        if "scale" in g.files:
            assert float(g["scale"]) == synthetic_scale(o + v), fname
    assert sorted(np.load(GOLDEN / "frag85_lockstep.npz").files) == sorted(["n", "o", "seed", "scale", "e_scf", "mo_energy", "e_corr", "n_iter", "rdm1_emb"])
    # tapes of unequal structure: one occupied orbital (no (-) chain), one virtual orbital (empty antisymmetric blocks), next to ordinary peers
    deg = lc.BATCHES["degenerate_mix"]["frags"]
    assert [(o, v) for o, v, _ in deg] == [(1, 11), (4, 8), (5, 1), (1, 1), (6, 10)] and all(o + v <= 20 for o, v, _ in deg)
    # more members of a two-chain region than one grouped launch takes -- and only there
    six = lc.BATCHES["sixteen_members"]["frags"]
    assert sorted(o + v for o, v, _ in six) == list(range(9, 17)) and all(3 <= o <= 6 for o, v, _ in six)
    assert lc.members_per_step("sixteen_members") == 16 > lc.GROUP_MAX
    assert all(lc.members_per_step(name) <= lc.GROUP_MAX for name in lc.BATCHES if name != "sixteen_members")
    # the one-pass kernels forced into tapes: n_occ on both sides of their 32-row limit
    fp = lc.BATCHES["forced_passes"]
    assert fp["env"] == dict(QEMB_OVVV_PASS="1", QEMB_RING_PREP="1") and [(o, v) for o, v, _ in fp["frags"]] == [(6, 40), (33, 20), (12, 30)]
    assert all("env" not in b for name, b in lc.BATCHES.items() if name not in ("forced_passes", "unmarked_recording"))
    # the recording without region marks: a cap on the slices of a region that the (24, 61) ring region exceeds and its peer's regions do not
    um = lc.BATCHES["unmarked_recording"]
    cap = int(um["env"]["QEMB_REGION_WS_MB"]) << 20
    assert [ex[(o, v)]["region_ws"] > cap for o, v, _ in um["frags"]] == [True, False] and ex[(24, 61)]["region_ws"] // 2 <= cap
    # seeds are written down, one fragment one seed
    assert all(isinstance(seed, int) for *_, seed in _all())
    assert set(lc.FEWER_ITERATIONS) <= {(o, v, seed) for _, o, v, seed in _all()} and all(o * v <= 1 for o, v, _ in lc.FEWER_ITERATIONS)


def test_expectations_are_the_solvers_own_plans(hlib):
    """what the table expects is what CcsdSolver plans: ccsd_ring_plan (tile, K split and region workspace of the ring products), the replay rule and the Xw plan
    of ccsd_gemm_plans -- for every fragment of the table and along the borders"""
    tiles = {-1: "dispatcher"}
    for index in range(200):
        out = [C.c_int() for _ in range(7)]
        if hlib.qemb_gemm_tile_table(index, *[C.byref(x) for x in out]) != 0:
            break
        tiles[out[0].value] = f"{out[1].value}x{out[2].value}"
    shapes = {(o, v) for _, o, v, _ in _all()} | {(1, x) for x in (255, 256, 896, 897, 1023, 1024, 1448, 1449, 2047, 2048, 2049)} | {(181, 8), (23, 63), (45, 45), (46, 45)}
    for o, v in sorted(shapes):
        e = lc.expect(o, v)
        r = (C.c_int64 * 4)()
        assert hlib.qemb_ccsd_ring_plan(o, v, r) == 0
        assert bool(r[0]) == e["replay"], (o, v)
        assert tiles[r[1]] + ("k2" if r[2] == 2 else "") == e["ring"], (o, v, tuple(r))
        assert r[2] in (0, 2)
        if e["replay"]:
            assert r[3] == e["region_ws"], (o, v, r[3], e["region_ws"])
        p = (C.c_int64 * 54)()
        assert hlib.qemb_ccsd_gemm_plans(o, v, p) == 0
        xw_p = tuple(p[6 * 5:6 * 5 + 6])      # (M, N, K, cfg, ksplit, slabs) of Xw(+)
        assert (xw_p[3] >= 0) == e["xw_split"], (o, v, xw_p)
        if e["xw_split"]:
            assert tiles[xw_p[3]] == "64x64" and xw_p[5] > 1


@pytest.mark.parametrize("name", lc.MOCK_BATCHES)
def test_small_batches_on_the_mock(hlib, name):
    """the batch driver on the two small batches: one by one == the batch == the batch over the same handles in reversed order, bit for bit, and the
    conditions on the inputs (iteration counts)"""
    from quemb_amd.fragsolver import default_opts
    handles, refs, outs, _ = lc.solve_both_ways(name, lib=hlib)
    lc.check_input_conditions(name, refs, default_opts(hlib).cc_max_cycle)
    lc.assert_bit_identical(name, refs, outs)
    order = list(range(len(refs)))[::-1]
    _, _, outs_r, _ = lc.solve_both_ways(name, lib=hlib, order=order, refs=refs, frags=handles)
    lc.assert_bit_identical(name, refs, outs_r)
    for fr in handles[0]:
        fr.free()
