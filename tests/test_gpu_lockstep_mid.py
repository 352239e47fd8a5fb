"""-m gpu: the lock-step CCSD sweep (qemb_frag_solve_batch: tapes, parallel regions, grouped launches) held to the one-by-one solve at mid sizes, up to the
edge of the replay regime (o v = 2048) -- the batches of tests/lockstep_cases.py.  The criterion is the project's own: bit identity with the one-by-one solve
(csrc/ccsd.cpp, ccsd_kernel_lockstep), and the stored oracle results where a fragment has them.

Every batch is solved one by one, then in lock step, then once more over the same handles in reversed order: every handle (but the middle one of an odd batch)
then sits on another execution context, whose address is part of the key of a kept tape, so it must record afresh (qemb_tape_cache_counters)."""
import ctypes as C
import time

import numpy as np
import pytest

import lockstep_cases as lc
from helpers import GOLDEN
from quemb_amd.fragsolver import default_opts

pytestmark = pytest.mark.gpu

TOL_E = 1e-8       # (tests/test_gpu_fragment.py: both solvers converged to |dE| < 1e-11, |dt| < 1e-9)
TOL_RDM = 1e-8


def _counters(qlib, reset=0):
    reused, recorded = C.c_int64(), C.c_int64()
    qlib.qemb_tape_cache_counters(C.byref(reused), C.byref(recorded), reset)
    return reused.value, recorded.value


def _check_taped(name, refs, stats):
    """the batch really ran from merged tapes: every in-regime fragment in the merged runs, grouped launches issued"""
    specs = lc.BATCHES[name]["frags"]
    T = len(lc.taped(name))
    assert stats["merged_runs"] > 0 and stats["max_group"] == T, (name, stats)
    # every iteration of a taped fragment runs from its tape: the merged runs are the iterations of the slowest taped fragment
    iters = sorted(r["n_iter"] for s, r in zip(specs, refs) if lc.expect(s[0], s[1])["replay"])
    assert stats["merged_runs"] == iters[-1], (name, stats, iters)
    if name in lc.POSITION_MERGED:
        # tapes of unequal structure are merged position by position (build_plan): whatever else lines up, position 0 of every tape is the layout pass at the top
        # of update_amps (dev_ccsd_ph_layouts / _ring: one kernel, one block shape, for every o and v), so every merged run of two or more tapes -- the
        # iterations of the second slowest fragment -- holds at least that grouped launch
        assert stats["grouped_launches"] >= iters[-2] > 0, (name, stats, iters)
    else:
        assert stats["grouped_launches"] > 0 and stats["launches"] < stats["operations"], (name, stats)


def _run(qlib, name, extra=None):
    """steps 1-5 for one batch; returns the one-by-one results, the lock-step results (fragment order) and the counters of the first lock-step sweep.
    extra(handles, refs): further runs over the same handles"""
    F = len(lc.BATCHES[name]["frags"])
    t0 = time.time()
    handles, refs, outs, stats = None, None, None, None
    try:
        specs, okw, env = lc.batch(name)
        opts = default_opts(**okw)
        with lc.forced_env(env):
            made = [lc.make_fragment(*s) for s in specs]
            handles = ([m[0] for m in made], [m[1] for m in made])
            t1 = time.time()
            refs = [fr.solve(s[0], h, None, opts=opts, eeval=True, want_t2=True) for fr, h, s in zip(*handles, specs)]
        t2 = time.time()
        print(f"{name}: set-up {t1 - t0:.2f} s, one by one {t2 - t1:.2f} s, n_iter {[r['n_iter'] for r in refs]}, lambda_iters {[r['lambda_iters'] for r in refs]}")
        lc.check_input_conditions(name, refs, opts.cc_max_cycle)
        _counters(qlib, reset=1)
        _, _, outs, stats = lc.solve_both_ways(name, refs=refs, frags=handles)
        t3 = time.time()
        print(f"{name}: lock step {t3 - t2:.2f} s, {stats}, tapes (reused, recorded) {_counters(qlib)}")
        lc.assert_bit_identical(name, refs, outs)
        _check_taped(name, refs, stats)
        assert _counters(qlib) == (0, F)                      # fresh handles keep no tape
        order = list(range(F))[::-1]
        _, _, outs_r, stats_r = lc.solve_both_ways(name, order=order, refs=refs, frags=handles)
        print(f"{name}: reversed {time.time() - t3:.2f} s, {stats_r}, tapes (reused, recorded) {_counters(qlib)}")
        lc.assert_bit_identical(name, refs, outs_r)
        _check_taped(name, refs, stats_r)
        reused, recorded = _counters(qlib)
        assert reused + recorded == 2 * F and reused <= F % 2, (name, reused, recorded)      # a handle moved to another context records afresh
        if extra:
            extra(handles, refs)
    finally:
        if handles:
            for fr in handles[0]:
                fr.free()
    return refs, outs, stats


def _against_stored(out, fname, iter_slack):
    """a converged solve against the oracle's stored results, at the tolerances of the one-by-one golden tests (test_gpu_fragment.py)"""
    g = np.load(GOLDEN / fname)
    print(f"{fname}: dE_scf {out['e_scf'] - float(g['e_scf']):.2e}  dE_corr {out['e_corr_mo'] - float(g['e_corr']):.2e}  n_iter {out['n_iter']} / {int(g['n_iter'])}"
          f"  max |d rdm1| {np.abs(out['rdm1_emb'] - g['rdm1_emb']).max():.2e}")
    assert abs(out["e_scf"] - float(g["e_scf"])) < TOL_E * max(1.0, abs(float(g["e_scf"])) if "scale" in g.files else 1.0)
    assert abs(out["e_corr_mo"] - float(g["e_corr"])) < TOL_E, (out["e_corr_mo"], float(g["e_corr"]))
    assert abs(out["n_iter"] - int(g["n_iter"])) <= iter_slack, (out["n_iter"], int(g["n_iter"]))
    assert np.abs(out["rdm1_emb"] - g["rdm1_emb"]).max() < TOL_RDM


def test_ring_borders(qlib):
    """the ring tile rule on both sides of each border (o v = 448, 896 | 897, 1008 | 1024) and the Xw split border v = 63 | 64, in one merged run"""
    _run(qlib, "ring_borders")


def test_workspace_border(qlib):
    """Region slices of the two-slice ring products below (o v = 1440) and above the workspace's 64 MB floor (1464, 1500), and o v = 2048, the last shape of the
    regime, in explicit lock step: completes, taped, bit for bit; the two stored fragments against the oracle.  Then four more sweeps in the places of the
    second: the buffer layout settles and the tapes are kept (qemb_tape_cache_counters: every solve either reuses or records, and at least one full sweep of
    reuse) -- the workspace is sized before the key of a tape is taken, so a kept tape names the workspace that is there.  (QEMB_TAPE_CACHE_CHECK=1 cannot
    serve here: dev_tape_equal compares the arguments of groupable kernels only, and the tiled pair packing of n_virt >= 32 is not one.)"""
    def kept_tapes(handles, refs):
        F = len(refs)
        _counters(qlib, reset=1)
        for sweep in (3, 4, 5, 6):
            _, _, outs_k, stats_k = lc.solve_both_ways("workspace_border", order=list(range(F))[::-1], refs=refs, frags=handles)
            print(f"workspace_border: sweep {sweep} {stats_k}, tapes (reused, recorded) {_counters(qlib)}")
            lc.assert_bit_identical("workspace_border", refs, outs_k)
            _check_taped("workspace_border", refs, stats_k)
        reused, recorded = _counters(qlib)
        assert reused + recorded == 4 * F and reused >= F, (reused, recorded)

    refs, outs, _ = _run(qlib, "workspace_border", extra=kept_tapes)
    assert [lc.expect(o, v)["region_ws"] > lc.GWS_FLOOR for o, v, _ in lc.BATCHES["workspace_border"]["frags"]] == [False, True, True, True]
    _against_stored(outs[0], "frag132.npz", 1)
    _against_stored(outs[1], "frag85_lockstep.npz", 1)


def test_regime_edge(qlib):
    """a batch in which one fragment, (32, 65), is outside the replay regime and iterates eagerly beside the merged tapes of the other two"""
    refs, outs, _ = _run(qlib, "regime_edge")
    specs = lc.BATCHES["regime_edge"]["frags"]
    k = [i for i, s in enumerate(specs) if not lc.expect(s[0], s[1])["replay"]]
    assert k == [1]
    for key in lc.BIT_KEYS_SCALAR:
        assert outs[1][key] == refs[1][key], key
    for key in lc.BIT_KEYS_ARRAY:
        assert np.array_equal(outs[1][key], refs[1][key]), key


def test_golden_84(qlib):
    """two handles on the stored (20, 64) fragment (and a (16, 56) peer): an oracle pin inside a mid-ring tape"""
    refs, outs, _ = _run(qlib, "golden_84")
    for k in (0, 1):
        _against_stored(outs[k], "frag84.npz", 0)


def test_golden_84_relaxed(qlib):
    """Lambda equations and response densities behind a lock-step solve: the stored relaxed (20, 64) fragment with a (16, 56) peer, relax_density = 1"""
    refs, outs, _ = _run(qlib, "golden_84_relaxed")
    g = np.load(GOLDEN / "frag84_relaxed.npz")
    out = outs[0]
    print(f"frag84_relaxed: dE_corr {out['e_corr_mo'] - float(g['e_corr']):.2e}  lambda_iters {out['lambda_iters']} / {int(g['lambda_iters'])}"
          f"  max |d rdm1| {np.abs(out['rdm1_emb'] - g['rdm1_emb']).max():.2e}  max |d e_frag| {np.abs(np.array(out['e_frag']) - g['e_frag']).max():.2e}")
    assert abs(out["e_corr_mo"] - float(g["e_corr"])) < TOL_E, (out["e_corr_mo"], float(g["e_corr"]))
    assert abs(out["lambda_iters"] - int(g["lambda_iters"])) <= 2
    assert np.abs(out["rdm1_emb"] - g["rdm1_emb"]).max() < TOL_RDM
    assert np.abs(np.array(out["e_frag"]) - g["e_frag"]).max() < TOL_E, (out["e_frag"], g["e_frag"])
    assert out["lambda_iters"] == refs[0]["lambda_iters"] and outs[1]["lambda_iters"] == refs[1]["lambda_iters"]


def test_degenerate_mix(qlib):
    """one occupied orbital (no (-) chain: one chain where the peers have two), one virtual orbital (empty antisymmetric blocks), both: the tapes differ in
    structure and are merged position by position"""
    _run(qlib, "degenerate_mix")


def test_sixteen_members(qlib):
    """eight fragments x two chains = 16 members of one step: more than one grouped launch takes (GROUP_MAX = 12), split into several"""
    _run(qlib, "sixteen_members")


def test_forced_passes(qlib):
    """QEMB_OVVV_PASS=1 and QEMB_RING_PREP=1 for the set-up: the one-pass kernels inside tapes, n_occ = 33 beside n_occ <= 32 (tapes of unequal structure again)"""
    import os
    before = (os.environ.get("QEMB_OVVV_PASS"), os.environ.get("QEMB_RING_PREP"))
    with lc.forced_env(lc.BATCHES["forced_passes"]["env"]):
        assert qlib.qemb_op_ccsd_ring_prep_rule(6, 40, 1) == 1 and qlib.qemb_op_ccsd_ring_prep_rule(12, 30, 1) == 1
    _run(qlib, "forced_passes")
    assert (os.environ.get("QEMB_OVVV_PASS"), os.environ.get("QEMB_RING_PREP")) == before


def test_unmarked_recording(qlib):
    """Beyond the required batches: a region whose split-K slices do not fit is recorded without region marks instead of failing (CcsdSolver::prepare_tape).  With
    the slices of a region capped at the workspace's 64 MB floor (QEMB_REGION_WS_MB, read at every slice) the ring region of the stored (24, 61) fragment does not
    fit: its tape carries no marks, the batch is merged position by position -- bit for bit all the same, and in more launches than the same batch on fresh
    handles without the cap, where the two chains of a region share their launches."""
    refs, outs, capped = _run(qlib, "unmarked_recording")
    _against_stored(outs[0], "frag85_lockstep.npz", 1)
    handles = None
    try:
        handles, _, outs_m, marked = lc.solve_both_ways("unmarked_recording", refs=refs, env={})
        print(f"unmarked_recording: with marks {marked}")
        lc.assert_bit_identical("unmarked_recording", refs, outs_m)
        assert marked["merged_runs"] == capped["merged_runs"] and marked["operations"] == capped["operations"]
        assert marked["launches"] < capped["launches"], (marked, capped)
    finally:
        if handles:
            for fr in handles[0]:
                fr.free()
