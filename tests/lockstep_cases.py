"""Case table of the lock-step CCSD sweeps at mid sizes (tests/test_gpu_lockstep_mid.py on the device, tests/test_lockstep_cases_hostlogic.py for the table itself
and the small batches on the mock).

A batch is a list of fragments (o, v, seed); n = o + v.  Fragments of n <= 20 are helpers.synthetic_fragment with the 4-fold block resident; larger ones live on
their DF factor alone (make_golden_frag220.bench_fragment at helpers.synthetic_scale(n), set_df_only): no host array beyond the factor.  Three fragments are the
oracle's stored ones: (20, 64, 584) on the block is tests/golden/frag84.npz (and frag84_relaxed.npz), (12, 120, 20260803) is frag132.npz and (24, 61, 20260803) is
frag85_lockstep.npz (make_golden_frag220.py 85:24:lockstep).

Every fragment also states what the solver is expected to choose for it, from the rules in csrc/ccsd.cpp (expect()):
  replay     o^2 v^2 <= 2^22: the update is recorded (CcsdSolver::replay_regime);
  ring       the tile of the (ov)^3 ring products: "dispatcher" below 200 tiles of 64 x 64 (o v < 897), "64x64" up to o v = 1023, "96x96k2" (K in two slices) for
             1024 <= o v < 2048, "128x256" from o v = 2048 (ccsd_ring_plan);
  xw_split   the Xw(+) product keeps K slabs on 64 x 64 tiles: ldp = npair(v) rounded up to even >= 2048, i.e. v >= 64 (pick_xw_split); the hole-hole ladder picks
             its own row tile under the same condition (npair(v) >= 2048);
  region_ws  bytes of split-K workspace the parallel region of the last two ring products takes inside a tape, a slice per product: 32 (ov)^2 for the two slices
             of the mid-size tiles; at o v = 2048, the last shape of the regime, the 16 x 8 tiles of 128 x 256 are cut into six slices by dev_gemm itself
             (gemm_auto_ksplit): 96 (ov)^2 = 403 MB; else 0.  The workspace's floor is 64 MB: the border is o v = 1448 / 1449.

Conditions on the inputs (checked by the tests that solve the batches): every fragment converges one by one within the default cc_max_cycle in at least
MIN_ITER = 6 iterations, and the iteration counts of a batch are not all equal.  Two remarks:
  * the (1, 1) fragment has one singles and one doubles amplitude; of the seeds 7600 ... 7899 none takes more than five iterations (two to four for all but one),
    so it is listed in FEWER_ITERATIONS with the seed that takes five;
  * golden_84 holds a (16, 56) peer next to the two handles on the one stored fragment: two handles on one fragment alone converge together.
"""
import functools
import sys

import numpy as np

from helpers import GOLDEN, synthetic_fragment, synthetic_scale

REPLAY_LIMIT = 1 << 22
GWS_FLOOR = 64 << 20
GROUP_MAX = 12            # grouped_launch.h
GOLDEN_SEED = 20260803    # make_golden_frag220.SEED: the DF family's stored fragments
FRAG84 = (20, 64, 584)    # make_golden_frag84: (O, N - O, SEED) on the 4-fold block, 30 fragment sites, centres 0..9

TIGHT = dict(cc_conv_tol=1e-11, cc_conv_tol_normt=1e-9, scf_conv_tol=1e-12, scf_conv_tol_grad=1e-8)                 # what the oracle's stored solves were converged to
TIGHT_RELAXED = dict(cc_conv_tol=1e-12, cc_conv_tol_normt=1e-10, scf_conv_tol=1e-12, scf_conv_tol_grad=1e-8, relax_density=1, lambda_conv_tol=1e-10)

# id -> fragments (o, v, seed), solver options, environment of the set-up
BATCHES = {
    "ring_borders": dict(frags=[(14, 32, 7101), (16, 56, 7102), (23, 39, 7103), (16, 63, 7104), (16, 64, 7105)]),
    "workspace_border": dict(frags=[(12, 120, GOLDEN_SEED), (24, 61, GOLDEN_SEED), (30, 50, 7204), (32, 64, 7207)], opts=TIGHT),
    "regime_edge": dict(frags=[(32, 64, 7301), (32, 65, 7302), (20, 64, 7303)]),
    "golden_84": dict(frags=[FRAG84, FRAG84, (16, 56, 7403)], opts=TIGHT),
    "golden_84_relaxed": dict(frags=[FRAG84, (16, 56, 7502)], opts=TIGHT_RELAXED),
    "degenerate_mix": dict(frags=[(1, 11, 7636), (4, 8, 7605), (5, 1, 7822), (1, 1, 7793), (6, 10, 7605)]),
    "sixteen_members": dict(frags=[(3, 6, 7701), (4, 6, 7702), (5, 6, 7703), (6, 6, 7704), (3, 10, 7705), (4, 10, 7706), (5, 10, 7707), (6, 10, 7708)]),
    "forced_passes": dict(frags=[(6, 40, 7801), (33, 20, 7802), (12, 30, 7803)], env=dict(QEMB_OVVV_PASS="1", QEMB_RING_PREP="1")),
    # beyond the required list: the slices of a region held to the 64 MB floor, so that the (24, 61) fragment's ring region does not fit and its update is
    # recorded without region marks (CcsdSolver::prepare_tape) -- next to a peer that keeps its marks
    "unmarked_recording": dict(frags=[(24, 61, GOLDEN_SEED), (16, 56, 7102)], env=dict(QEMB_REGION_WS_MB="64")),
}
REQUIRED = ("ring_borders", "workspace_border", "regime_edge", "golden_84", "golden_84_relaxed", "degenerate_mix", "sixteen_members", "forced_passes")
POSITION_MERGED = ("degenerate_mix", "forced_passes", "unmarked_recording")      # tapes of unequal structure: merged position by position (build_plan)
MOCK_BATCHES = ("degenerate_mix", "sixteen_members")      # small enough for the scalar mock
MIN_ITER = 6
FEWER_ITERATIONS = {(1, 1, 7793): 5}      # (module docstring)


def check_input_conditions(name, refs, max_cycle):
    """the conditions of the module docstring on the one-by-one solves of a batch"""
    specs = BATCHES[name]["frags"]
    for s, r in zip(specs, refs):
        assert FEWER_ITERATIONS.get(s, MIN_ITER) <= r["n_iter"] <= max_cycle, (name, s, r["n_iter"])
    assert len({r["n_iter"] for r in refs}) > 1, (name, [r["n_iter"] for r in refs])


def _slab_count(K, ks):      # gemm_slab_count (dev_ops.h)
    if ks <= 1 or K <= 0:
        return 1
    chunk = (-(-K // ks) + 31) // 32 * 32
    return max(1, -(-K // chunk))


def _auto_ksplit(tiles, K):      # gemm_auto_ksplit (dev_ops.h)
    if tiles >= 256 or K < 1024:
        return 0
    S = min(-(-768 // tiles), K // 256)
    return S if S > 1 else 0


def expect(o, v):
    """what the solver is expected to choose for a fragment of o occupied and v virtual orbitals (module docstring)"""
    nov = o * v
    replay = nov * nov <= REPLAY_LIMIT
    if nov >= 2048:
        ring, S = "128x256", _slab_count(nov, _auto_ksplit(-(-nov // 128) * -(-nov // 256), nov))
    elif nov >= 1024:
        ring, S = "96x96k2", _slab_count(nov, 2)
    elif nov >= 256 and (-(-nov // 64)) ** 2 >= 200:
        ring, S = "64x64", 1
    else:
        ring, S = "dispatcher", 1
    npv = v * (v + 1) // 2
    region_ws = 2 * ((8 * S * nov * nov + 255) // 256 * 256) if (replay and S > 1) else 0
    return dict(replay=replay, ring=ring, xw_split=npv + (npv & 1) >= 2048, hh_tile=npv >= 2048, region_ws=region_ws)


def batch(name):
    b = BATCHES[name]
    return b["frags"], dict(b.get("opts", {})), dict(b.get("env", {}))


def taped(name):
    """the fragments of the batch that are recorded: the size of the merged runs"""
    return [f for f in BATCHES[name]["frags"] if expect(f[0], f[1])["replay"]]


def members_per_step(name):
    """chains x fragments of a two-chain region of the batch: a fragment with one occupied orbital has no (-) chain"""
    return sum(2 if o > 1 else 1 for o, v, _ in taped(name))


def n_sites(n):
    return max(1, min(n // 3, 6))


def energy_data(n, seed):
    rng = np.random.default_rng(seed + 1)
    mats = []
    for _ in range(3):
        a = rng.standard_normal((n, n)); mats.append(a + a.T)
    return mats


def _golden_scripts():
    if str(GOLDEN) not in sys.path:
        sys.path.insert(0, str(GOLDEN))
    import make_golden_frag84 as m84
    import make_golden_frag220 as m220
    return m84, m220


@functools.lru_cache(maxsize=None)
def problem(o, v, seed):
    """(h, kind, payload, nf, cen, (h1, veff0, veff)) of one fragment, built once per process and never modified:
    kind "block": payload is the 4-fold packed ERI block (set_eri_s4); kind "factor": the packed 3-index factor (set_df_only)"""
    from qemb_oracle import eri
    m84, m220 = _golden_scripts()
    n = o + v
    if (o, v, seed) == FRAG84:
        # the stored fragment of make_golden_frag84.py: helpers.synthetic_fragment(84, 20, 584) -- its block as the pair product of its factor (the n^4 tensor is
        # 400 MB and its einsum seconds; the two differ in rounding only, nine orders below the tolerances of the stored results)
        assert (m84.N, m84.O, m84.SEED) == (n, o, seed)
        h, B = m220.bench_fragment(n, seed, synthetic_scale(n))
        il = np.tril_indices(n)
        Bp = np.ascontiguousarray(B[:, il[0], il[1]])
        return h, "block", Bp.T @ Bp, m84.NF, list(m84.CEN), tuple(m84.energy_data(n, n))
    nf = n_sites(n)
    if n <= 20:
        h, e1 = synthetic_fragment(n, o, seed)
        return h, "block", eri.pack_s4(e1), nf, [0], tuple(energy_data(n, seed))
    h, B = m220.bench_fragment(n, seed, synthetic_scale(n))
    il = np.tril_indices(n)
    return h, "factor", np.ascontiguousarray(B[:, il[0], il[1]]), nf, [0], tuple(energy_data(n, seed))


def make_fragment(o, v, seed, lib=None):
    """a fresh device handle on the fragment and its one-body Hamiltonian"""
    from quemb_amd.fragsolver import DeviceFragment
    h, kind, payload, nf, cen, (h1, veff0, veff) = problem(o, v, seed)
    fr = DeviceFragment(o + v, nf, lib=lib)
    if kind == "block":
        fr.set_eri_s4(payload)
    else:
        fr.set_df_only(payload)
    fr.set_energy_data(h1, veff0, veff, 1.0, cen)
    return fr, h


class forced_env:
    """the environment of a batch's set-up, restored afterwards (the switches are read at every solver set-up)"""

    def __init__(self, env):
        self.env, self.saved = env, {}

    def __enter__(self):
        import os
        for k, val in self.env.items():
            self.saved[k] = os.environ.get(k)
            os.environ[k] = val

    def __exit__(self, *exc):
        import os
        for k, old in self.saved.items():
            if old is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old
        return False


BIT_KEYS_SCALAR = ("n_iter", "scf_cycles", "e_corr_mo", "e_scf")
BIT_KEYS_ARRAY = ("e_frag", "rdm1_emb", "rdm1_mo", "t1", "t2")


def solve_both_ways(name, lib=None, order=None, refs=None, frags=None, env=None):
    """one by one (unless `refs` are given), then the batch in lock step over the same handles in `order`: ((handles, hs), refs, outs in fragment order, stats);
    env: another environment than the table's"""
    from quemb_amd.fragsolver import default_opts, solve_batch
    specs, okw, table_env = batch(name)
    env = table_env if env is None else env
    opts = default_opts(lib, **okw)
    with forced_env(env):
        if frags is None:
            made = [make_fragment(*s, lib=lib) for s in specs]
            frags, hs = [m[0] for m in made], [m[1] for m in made]
        else:
            frags, hs = frags
        if refs is None:
            refs = [fr.solve(s[0], h, None, opts=opts, eeval=True, want_t2=True) for fr, h, s in zip(frags, hs, specs)]
        order = list(range(len(specs))) if order is None else list(order)
        stats = {}
        got = solve_batch([frags[k] for k in order], [specs[k][0] for k in order], [hs[k] for k in order], None, opts=opts, eeval=True, want_t2=True, stats=stats)
    outs = [None] * len(specs)
    for k, out in zip(order, got):
        outs[k] = out
    return (frags, hs), refs, outs, stats


def assert_bit_identical(name, refs, outs):
    for f, (a, b) in enumerate(zip(outs, refs)):
        for key in BIT_KEYS_SCALAR:
            assert a[key] == b[key], (name, f, key, a[key], b[key])
        for key in BIT_KEYS_ARRAY:
            assert np.array_equal(a[key], b[key]), (name, f, key)
