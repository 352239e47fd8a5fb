"""The cases of the perturbative triples correction E_(T) (fragsolver.ccsd_t, DeviceFragment.ccsd_t, Frags.ccsd_t, BE.ccsd_t, solve_ccsd(triples=True)) that
tests/test_ccsd_t_hostlogic.py (scalar mock device, CPU) and tests/test_gpu_ccsd_t.py (MI355X) both run: every function takes the library to drive.  The
reference is the full-tensor twin of tests/ccsd_t_numpy.py, which the CPU file first pins to the brute-force determinant evaluation, and its slab-wise form,
pinned to the full one there, at the shapes production runs (stored in tests/golden/ccsd_t_pins.npz where it needs more than a moment).
Bars: 1e-10 * sum |W r3(V) / D| / 3 from the twin at the operation level (the project's relative figure for kernel-level checks), 1e-8 absolute at the
fragment level, where the device's own amplitudes, orbitals and orbital energies go into the twin (the project's fragment-vs-oracle figure)."""
from functools import lru_cache

import numpy as np
import pytest

import ccsd_t_numpy as tn
import mp2_numpy as mpn
from helpers import GOLDEN, synthetic_fragment_factor
from qemb_oracle import eri

TOL = 1e-8
REL = 1e-10
TILES = (1, 2, 4, 8)
LDS_CAP = 20      # the largest occupied count of the kernel's LDS form (ccsd_t_core.h: kCcsdTLdsMaxOcc)


def op_shapes():
    """(o, v): v in {1, 2, 3, Tv - 1, Tv, Tv + 1, 2 Tv + 3} for Tv in TILES -- with v = 2 Tv + 3 every kind of tile triple (A = B = C, A = B > C, A > B = C,
    A > B > C) and a ragged last tile --, o in {1, 2, 5}; then one o just below and one just above the LDS cap of the kernel with v = 4"""
    vs = sorted({v for T in TILES for v in (1, 2, 3, T - 1, T, T + 1, 2 * T + 3) if v >= 1})
    return [(o, v) for o in (1, 2, 5) for v in vs] + [(LDS_CAP, 4), (LDS_CAP + 1, 4)]


@lru_cache(maxsize=None)
def system(o, v):
    """(t1, t2, ovvv, ovoo, ovov, eo, ev) of the random symmetric family and the twin's dict(e_t, abs_sum): computed once per shape"""
    n = o + v
    h, e4, t1, t2, eo, ev = tn.random_system(n, o, 1000 * o + v, scale=0.1)
    args = (t1, t2, *tn.blocks(e4, o), eo, ev)
    return args, tn.full(*args)


def run_op(lib, o, v, tile):
    from quemb_amd.fragsolver import ccsd_t
    return ccsd_t(*system(o, v)[0], tile=tile, lib=lib)


# ---------------------------------------------------------------- the shapes production runs, against stored values of the slab-wise twin
# (o, v, forced tile).  The twin needs seconds to minutes there: tests/golden/make_golden_ccsd_t.py stores it in ccsd_t_pins.npz.
#   tile 16, the default: v = 2 * 16 + 3 every kind of tile triple and a ragged tile of 3, v = 17 / 33 a ragged tile of 1, v = 16 / 32 the exact fits;
#     o = 5: N = tz * 25 odd for odd tz; o = 10: the largest o at which production picks 16
#   the block sizes between one wave and sixteen: nth = 64 (every lane exactly 8 elements), 128, 192, 320, 512, 896; three tiles, the last ragged
#   both sides of the LDS cap with several ragged tiles; (21, 19, 4) is the global form at the tile production gives it
TILE16_CASES = [(2, 35, 16), (5, 16, 16), (5, 17, 16), (5, 32, 16), (5, 33, 16), (5, 35, 16), (10, 35, 16)]
WAVE_CASES = [(o, 5, 2) for o in (8, 9, 11, 13, 16, 19)]
CAP_CASES = [(LDS_CAP, 19, 8), (LDS_CAP + 1, 19, 8), (LDS_CAP + 1, 19, 4)]
PIN_CASES = TILE16_CASES + WAVE_CASES + CAP_CASES
PRODUCTION_PIN = (20, 64, 8)      # the benchmark's n_occ with a realistic v: 120 tile triples, the 16-wave LDS form at its limit, K = 84 (device only)


def pinned_shapes():
    """(o, v) of every stored reference, in the order of the file"""
    return list(dict.fromkeys((o, v) for o, v, _ in PIN_CASES + [PRODUCTION_PIN]))


def pin_inputs(o, v):
    """(t1, t2, ovvv, ovoo, ovov, eo, ev) of the family of `system`; not kept: the n^4 tensor is 400 MB at (20, 64)"""
    h, e4, t1, t2, eo, ev = tn.random_system(o + v, o, 1000 * o + v, scale=0.1)
    return (t1, t2, *tn.blocks(e4, o), eo, ev)


@lru_cache(maxsize=None)
def stored_pins():
    """{(o, v): dict(e_t, abs_sum)} of tests/golden/ccsd_t_pins.npz"""
    g = np.load(GOLDEN / "ccsd_t_pins.npz")
    return {(int(o), int(v)): dict(e_t=float(e), abs_sum=float(s)) for o, v, e, s in zip(g["o"], g["v"], g["e_t"], g["abs_sum"])}


_pin_seen = {}      # (o, v) -> {tile: e_t} of the pinned cases that ran: shapes with two tiles are compared with each other


def check_op_against_pin(lib, o, v, tile):
    """one forced tile against the stored twin within the bar; the same call twice: the same bits; a shape that ran at another tile: the two within the bar.
    Returns |d| / abs_sum."""
    from quemb_amd.fragsolver import ccsd_t
    ref = stored_pins()[(o, v)]
    bar = REL * ref["abs_sum"]
    args = pin_inputs(o, v)
    got = ccsd_t(*args, tile=tile, lib=lib)
    again = ccsd_t(*args, tile=tile, lib=lib)
    err = abs(got - ref["e_t"])
    print(f"ccsd_t pin o={o} v={v} tile={tile}: e_t = {got:.14e} (stored twin {ref['e_t']:.14e}) |d| / abs_sum = {err / ref['abs_sum']:.2e}, bar {REL:.0e}")
    assert ref["e_t"] != 0.0 and ref["abs_sum"] > 0.0
    assert np.isfinite(got) and err <= bar, (o, v, tile, err, bar)
    assert again == got, (o, v, tile)
    for other, val in _pin_seen.setdefault((o, v), {}).items():
        print(f"   tile {other} gave {val:.14e}: |d| / abs_sum = {abs(val - got) / ref['abs_sum']:.2e}")
        assert abs(val - got) <= bar, (o, v, tile, other, val, got, bar)
    _pin_seen[(o, v)][tile] = got
    return err / ref["abs_sum"]


# ---------------------------------------------------------------- the operation
def check_op_against_twin(lib, o, v):
    """every forced tile against the twin within the bar, hence all tiles the same value within it; the same tile twice: the same bits"""
    args, ref = system(o, v)
    bar = REL * ref["abs_sum"]
    seen = []
    for T in TILES:
        got = run_op(lib, o, v, T)
        seen.append(got)
        err = abs(got - ref["e_t"])
        print(f"ccsd_t op o={o} v={v} tile={T}: e_t = {got:.14e} (twin {ref['e_t']:.14e}) |d| = {err:.2e}, bar {bar:.2e}")
        assert np.isfinite(got) and err <= bar, (o, v, T, err, bar)
        assert run_op(lib, o, v, T) == got, (o, v, T)
    assert max(seen) - min(seen) <= bar, (o, v, seen, bar)
    if o >= 2 and v >= 2:
        assert ref["e_t"] != 0.0 and ref["abs_sum"] > 0.0


def check_empty_and_bad_arguments(lib):
    from quemb_amd.fragsolver import ccsd_t
    z = np.zeros
    assert ccsd_t(z((3, 0)), z((3, 3, 0, 0)), z((3, 0, 0, 0)), z((3, 0, 3, 3)), z((3, 0, 3, 0)), z(3), z(0), lib=lib) == 0.0
    assert ccsd_t(z((0, 3)), z((0, 0, 3, 3)), z((0, 3, 3, 3)), z((0, 3, 0, 0)), z((0, 3, 0, 3)), z(0), z(3), lib=lib) == 0.0
    args = system(2, 3)[0]
    with pytest.raises(ValueError, match="tile"):
        ccsd_t(*args, tile=0, lib=lib)
    with pytest.raises(ValueError, match="ovvv"):
        ccsd_t(args[0], args[1], args[2][:, :, :, :2], *args[3:], lib=lib)


# ---------------------------------------------------------------- the fragment
FRAGMENTS = [(6, 2), (12, 4), (20, 6), (7, 1), (7, 6), (5, 5)]      # the size cases of tests/test_rdm2_hostlogic.py
RESIDENCIES = ("block", "block+factor", "factor")
# both sides of the borders of the automatic tile (ccsd_t.h: kCcsdTBufferBytes), o = 10 | 11 (16 | 8) and o = 20 | 21 (8 | 4, and the LDS | global form):
# (n, o, residency); tile / tile triples (27, 10): 16 / 4, (30, 11): 8 / 10, (40, 20): 8 / 10, (40, 21): 4 / 35
CAP_FRAGMENTS = [(27, 10, "block"), (30, 11, "block"), (30, 11, "factor"), (40, 20, "block"), (40, 21, "block")]
CAP_TILES = {(27, 10): (16, 4), (30, 11): (8, 10), (40, 20): (8, 10), (40, 21): (4, 35)}


def expected_tile(o, v):
    """the automatic tile with room for it, restated from ccsd_t.h / ccsd_t_pick_tile: the first T of (16, 8, 4, 2, 1), cut to v, with T == 1 or the six
    buffers 8 * 6 * T^3 * o^3 within 192 MiB"""
    for t in (16, 8, 4, 2, 1):
        T = min(t, v)
        if T == 1 or 48 * T ** 3 * o ** 3 <= 192 * 2 ** 20:
            return T


def fragment(lib, n, o, residency, nf=2):
    from quemb_amd.fragsolver import DeviceFragment
    h, e1, Bp = synthetic_fragment_factor(n, o, 300 + n)
    fr = DeviceFragment(n, nf, lib=lib)
    if residency == "factor":
        fr.set_df_only(Bp)
    else:
        fr.set_eri_s4(eri.pack_s4(e1))
        if residency == "block+factor":
            fr.set_df_factor(Bp)
    return fr, h, e1


def opts(lib, **kw):
    from quemb_amd.fragsolver import default_opts
    return default_opts(lib, scf_conv_tol=1e-13, scf_conv_tol_grad=1e-9, **kw)


def twin_of_solve(out, e1, o):
    """the twin on what a solve returned: t1, t2, the MO integrals from mo_coeff and the orbital energies"""
    n = out["mo_coeff"].shape[0]
    v = n - o
    mo = mpn.mo_eri(e1, out["mo_coeff"])
    return tn.slabbed(out["t1"].reshape(o, v), out["t2"].reshape(o, o, v, v), *tn.blocks(mo, o), out["mo_energy"][:o], out["mo_energy"][o:])


def check_fragment(lib, n, o, residency):
    """solve CCSD, then ccsd_t: against the twin, bit-equal on a second call and after a relaxed solve of the same fragment, the fragment left as the solve left it"""
    fr, h, e1 = fragment(lib, n, o, residency)
    out = fr.solve(o, h, opts=opts(lib), eeval=False, want_t2=True)
    route, kept = fr.mo_route_used(), fr.resident_bytes()
    got = fr.ccsd_t()
    assert fr.mo_route_used() == route and fr.resident_bytes() == kept
    assert set(got) == {"e_t", "tile", "n_tile_triples", "bytes", "ms"} and set(got["ms"]) == {"images", "gemm", "assemble", "integrals"}
    if o < 2 or n - o < 2:      # no triples (no virtual orbitals at all at o == n)
        assert got["e_t"] == 0.0 and got["n_tile_triples"] == 0 and got["tile"] == 0
        assert o == n or twin_of_solve(out, e1, o)["e_t"] == 0.0
        fr.free()
        return
    ref = twin_of_solve(out, e1, o)
    err = abs(got["e_t"] - ref["e_t"])
    print(f"ccsd_t fragment ({n},{o}) {residency}: e_t = {got['e_t']:.12e} twin {ref['e_t']:.12e} |d| = {err:.2e} tile = {got['tile']} triples = {got['n_tile_triples']} "
          f"bytes = {got['bytes']} e_corr = {out['e_corr_mo']:.6e}")
    assert err < TOL
    v = n - o
    nt = -(-v // got["tile"])
    assert got["tile"] == expected_tile(o, v) and got["n_tile_triples"] == nt * (nt + 1) * (nt + 2) // 6 and got["bytes"] == fr.ccsd_t_bytes(o, got["tile"]) > 0
    assert got["e_t"] < 0.0 and abs(got["e_t"]) < abs(out["e_corr_mo"])
    assert fr.ccsd_t()["e_t"] == got["e_t"]
    # a relaxed solve keeps the same t1 / t2: the same correction
    fr.solve(o, h, opts=opts(lib, relax_density=1), eeval=False)
    relaxed = fr.ccsd_t()
    print(f"   after a relaxed solve: |d| = {abs(relaxed['e_t'] - got['e_t']):.2e}")
    assert relaxed["e_t"] == got["e_t"]
    fr.free()


_cap_twin = {}      # (n, o) -> the twin of the first solve of that fragment (seconds of host time at (40, 21)): shared by its residencies


def check_cap_fragment(lib, n, o, residency):
    """a fragment at a border of the automatic tile: solve CCSD, then ccsd_t with the tile left to the library -- the tile and the tile triples as derived
    from the constants, e_t against the twin, bit-equal on a second call.  Returns |d|."""
    fr, h, e1 = fragment(lib, n, o, residency)
    out = fr.solve(o, h, opts=opts(lib), eeval=False, want_t2=True)
    got = fr.ccsd_t()
    if (n, o) not in _cap_twin:
        _cap_twin[(n, o)] = twin_of_solve(out, e1, o)
    ref = _cap_twin[(n, o)]
    err = abs(got["e_t"] - ref["e_t"])
    print(f"ccsd_t fragment ({n},{o}) {residency}: e_t = {got['e_t']:.12e} twin {ref['e_t']:.12e} |d| = {err:.2e} abs_sum = {ref['abs_sum']:.2e} tile = {got['tile']} "
          f"triples = {got['n_tile_triples']} bytes = {got['bytes']} iterations = {out['n_iter']} ms = {got['ms']}")
    assert (got["tile"], got["n_tile_triples"]) == CAP_TILES[(n, o)] and got["tile"] == expected_tile(o, n - o)
    assert got["bytes"] == fr.ccsd_t_bytes(o, got["tile"]) > 0
    assert err < TOL
    assert got["e_t"] < 0.0 and abs(got["e_t"]) < abs(out["e_corr_mo"])
    assert fr.ccsd_t()["e_t"] == got["e_t"]
    fr.free()
    return err


def check_solver_function(lib):
    from quemb_amd.solver import solve_ccsd
    n, o = 9, 3
    h, e1, Bp = synthetic_fragment_factor(n, o, 21)
    s4 = eri.pack_s4(e1)
    plain = solve_ccsd(h, s4, o, rdm_return=True, opts=opts(lib), lib=lib)
    with_t = solve_ccsd(h, s4, o, rdm_return=True, opts=opts(lib), lib=lib, triples=True)
    assert len(plain) == 4 and len(with_t) == 5 and np.array_equal(plain[0], with_t[0]) and np.array_equal(plain[1], with_t[1])
    t1, t2, _, C, e_t = with_t
    eps = np.diag(C.T @ (h + _veff(e1, C, o)) @ C)
    ref = tn.full(t1, t2, *tn.blocks(mpn.mo_eri(e1, C), o), eps[:o], eps[o:])
    assert abs(e_t - ref["e_t"]) < TOL and e_t < 0.0
    assert len(solve_ccsd(h, s4, o, opts=opts(lib), lib=lib, triples=True)) == 3


def _veff(e1, C, o):
    P = 2.0 * C[:, :o] @ C[:, :o].T
    return np.einsum("pqrs,rs->pq", e1, P) - 0.5 * np.einsum("prqs,rs->pq", e1, P)


def check_refusals(lib):
    """no solve, another solver's solve, changed ERIs, amplitudes that were not kept"""
    from quemb_amd import _lib
    from quemb_amd._lib import QembError
    from quemb_amd.fragsolver import default_fci_opts
    n, o = 6, 2
    fr, h, e1 = fragment(lib, n, o, "block")
    with pytest.raises(QembError, match="no solve has run") as ei:
        fr.ccsd_t()
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.solve_mp2(o, h, opts=opts(lib), eeval=False)
    with pytest.raises(QembError, match="last solve of this fragment was MP2") as ei:
        fr.ccsd_t()
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.solve_fci(o, h, opts=opts(lib), fci_opts=default_fci_opts(lib), eeval=False)
    with pytest.raises(QembError, match="last solve of this fragment was FCI"):
        fr.ccsd_t()
    fr.solve(o, h, opts=opts(lib), eeval=False)
    assert fr.ccsd_t()["e_t"] < 0.0
    fr.set_eri_s4(eri.pack_s4(e1))
    with pytest.raises(QembError, match="no solve has run"):
        fr.ccsd_t()
    fr.solve(o, h, opts=opts(lib), eeval=False)
    kept = fr.resident_bytes()
    fr.drop_amplitudes()
    assert fr.resident_bytes() == kept - 8 * (o * (n - o) + (o * (n - o)) ** 2)
    with pytest.raises(QembError, match="amplitudes of the last CCSD solve were not kept") as ei:
        fr.ccsd_t()
    assert ei.value.status == _lib.QEMB_ERR_ARG
    fr.free()


def check_memory_guard(lib):
    """one byte under the working set of tile 1 is refused and names n; a limit that admits only a smaller tile than the default gives the same energy within
    the kernel-level bar, and the dict reports that tile"""
    from quemb_amd import _lib
    from quemb_amd._lib import QembError
    n, o = 12, 4
    fr, h, e1 = fragment(lib, n, o, "block")
    out = fr.solve(o, h, opts=opts(lib), eeval=False, want_t2=True)
    ref = twin_of_solve(out, e1, o)
    free = fr.ccsd_t()
    assert free["tile"] == 8
    least = fr.ccsd_t_bytes(o, 1)
    assert 0 < least <= fr.ccsd_t_bytes(o, 2) <= fr.ccsd_t_bytes(o, 4) < fr.ccsd_t_bytes(o, 8) == free["bytes"]
    fr.set_ccsd_t_mem_limit(least - 1)
    with pytest.raises(QembError, match=f"n = {n}") as ei:
        fr.ccsd_t()
    assert ei.value.status == _lib.QEMB_ERR_ALLOC
    for tile in (1, 4):
        fr.set_ccsd_t_mem_limit(fr.ccsd_t_bytes(o, tile))
        small = fr.ccsd_t()
        print(f"ccsd_t under a limit of {fr.ccsd_t_bytes(o, tile)} bytes: tile {small['tile']}, |d| = {abs(small['e_t'] - free['e_t']):.2e}, bar {REL * ref['abs_sum']:.2e}")
        fits = max(t for t in TILES if fr.ccsd_t_bytes(o, t) <= fr.ccsd_t_bytes(o, tile))      # (the transformation can be the larger part: tile 2 may cost what tile 1 costs)
        assert tile <= small["tile"] == fits < free["tile"] and small["bytes"] == fr.ccsd_t_bytes(o, fits)
        assert abs(small["e_t"] - free["e_t"]) <= REL * ref["abs_sum"]
    fr.set_ccsd_t_mem_limit(-1)
    assert fr.ccsd_t()["e_t"] == free["e_t"]
    fr.free()


# ---------------------------------------------------------------- the BE driver
def _be(lib, which, **kw):
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    if which == "h8":
        mol, key = Mole([["H", (0.0, 0.0, float(i))] for i in range(8)]), "test_autogen_h_linear_be2"
    else:
        mol, key = Mole(GOLDEN / "octane.xyz"), "test_autogen_octane_be2"
    mf = RHF(mol); mf.kernel()
    return BE(mf, FragPart.from_json(GOLDEN / "fragmentation.json", key), lib=lib, distribute=False, **kw)


def check_be(lib, which="h8"):
    b = _be(lib, which)
    with pytest.raises(ValueError, match="CCSD"):
        b.ccsd_t()
    e_corr, comps = b.oneshot(solver="CCSD")
    before = (b.ebe_tot, b.e_corr, np.array(b.e_components, dtype=float).copy())
    res = b.ccsd_t()
    assert len(res) == len(b.Fobjs) and all(set(r) == {"e_t", "tile", "n_tile_triples", "bytes", "ms"} for r in res)
    assert (b.ebe_tot, b.e_corr) == before[:2] and np.array_equal(np.array(b.e_components, dtype=float), before[2]) and e_corr == b.e_corr
    for k, (f, r) in enumerate(zip(b.Fobjs, res)):
        one = f.ccsd_t()
        assert np.isfinite(r["e_t"]) and r["e_t"] < 0.0 and r["e_t"] == one["e_t"] == f.e_t
        assert r["tile"] == expected_tile(f.nsocc, f.nao - f.nsocc), (k, f.nao, f.nsocc, r["tile"])
    for k, (f, r) in enumerate(zip(b.Fobjs, res)):      # (the correlation energy of the embedding problem: a one-by-one solve of the same inputs)
        e_mo = f.dev.solve(f.nsocc, f.fock + f.heff, f.dm0, opts=b.opts, eeval=False)["e_corr_mo"]
        print(f"{which} BE2 fragment {k}: n = {f.nao} o = {f.nsocc} e_corr_mo = {e_mo:.8f} e_t = {r['e_t']:.3e} tile = {r['tile']} ms = {r['ms']}")
        assert abs(r["e_t"]) < abs(e_mo)
    if which == "h8":
        c = _be(lib, which)
        c.oneshot(solver="MP2")
        with pytest.raises(ValueError, match="CCSD"):
            c.ccsd_t()
