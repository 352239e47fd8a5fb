"""-m gpu: dev_gemm on sub-matrix views (offset bases, padded leading dimensions, batch gaps) for every tile of gemm_tiles.h, bit for bit.

The cases, their exact-by-construction data and the expected full C buffer -- sentinels in every byte the product must not touch -- come from
tests/gemm_view_cases.py; tests/test_gemm_views_hostlogic.py rehearses the same cases on the hostcheck mock.  The tile ids are read from the library
(qemb_gemm_tile_table), so a tile added to the table is tested without an edit here, and every launch is checked through qemb_gemm_last_launch to have
run the variant its view class was built for.  No tolerance appears anywhere: np.array_equal over the whole buffer.

What these tests cannot see: an epilogue that takes the wide (16-byte pair) store path on a C that is only 8-byte aligned.  The hardware performs
the misaligned pair stores and the bytes written are the same, so all 130 cases stay green under that mutation of the kernel (tried once on an
MI355X); wide_c is the host's restatement of the predicate (gemm_wide_c, dev_ops.h), not a read-back from the kernel."""
import numpy as np
import pytest

import gemm_view_cases as gv

pytestmark = pytest.mark.gpu


def _collect_variants():
    """(table index, variant, label): every table entry as itself, as its classic-loop twin (+ 200) and as its ladder twin, where the table says they
    exist.  Read through the library at collection time (dlopen only, no device call); where that is not possible, indices 0..31 that skip past the end."""
    try:
        import torch  # noqa: F401  (before the library, as the qlib fixture does: both bring a HIP runtime and torch's has to be the one that is loaded)
        from quemb_amd import _lib
        table = gv.tile_table(_lib.load())
        assert table
    except Exception:
        return [(i, v, f"entry{i}-{v}") for i in range(32) for v in ("tile", "classic", "ladder")]
    out = []
    for i, t in enumerate(table):
        out.append((i, "tile", f"cfg{t['id']}"))
        if t["has_classic"]:
            out.append((i, "classic", f"cfg{t['id'] + gv.GEMM_CLASSIC}"))
        if t["ladder_twin"] >= 0:
            out.append((i, "ladder", f"cfg{t['ladder_twin']}"))
    return out


_VARIANTS = _collect_variants()


@pytest.fixture(scope="module")
def table(qlib):
    return gv.tile_table(qlib)


def _check(qlib, case, cfg, mode1, what="tile"):
    b = gv.build(case)
    got, rec = gv.run_case(qlib, b, cfg)
    assert gv.mismatch(got, b) == "", (cfg, rec)
    assert rec["vec2"] == case.expect_vec2(), (case.label(), cfg, rec)
    for k, v in case.must.items():
        if not (k == "wide_c" and rec["ksplit"] > 1):      # (under split-K the tile kernel writes workspace slabs: see _check_split)
            assert rec[k] == v, (case.label(), cfg, k, rec)
    if cfg >= 0:
        assert rec["cfg"] == cfg, (case.label(), cfg, rec)
        assert rec["mode"] == (mode1 if rec["vec2"] == 1 and what != "classic" else 0), (case.label(), cfg, rec)
    return rec


@pytest.mark.parametrize("a_kc,b_kc", gv.LAYOUTS)
@pytest.mark.parametrize("index,variant", [(i, v) for i, v, _ in _VARIANTS], ids=[label for _, _, label in _VARIANTS])
def test_every_tile_on_every_view(qlib, table, index, variant, a_kc, b_kc):
    if index >= len(table):
        pytest.skip("past the end of the tile table")
    t = table[index]
    if (variant == "classic" and not t["has_classic"]) or (variant == "ladder" and t["ladder_twin"] < 0):
        pytest.skip("the table has no such twin of this tile")
    cfg = {"tile": t["id"], "classic": t["id"] + gv.GEMM_CLASSIC, "ladder": t["ladder_twin"]}[variant]
    for case in gv.view_cases(t, a_kc, b_kc):
        rec = _check(qlib, case, cfg, t["mode1"], variant)
        assert rec["wide_c"] == case.expect_wide_c() and rec["ksplit"] == 1 and (rec["sb_m"], rec["sb_n"]) == (0, 0), (case.label(), cfg, rec)


def _check_split(qlib, case, cfg, mode1):
    rec = _check(qlib, case, cfg, mode1)
    assert rec["ksplit"] == gv.slab_count(case.K, case.ksplit) > 1, (case.label(), cfg, rec)
    assert rec["wide_c"] == int(case.N % 2 == 0), (case.label(), cfg, rec)      # of the workspace slabs [M][N] the slices write (ld = N, aligned)
    return rec


@pytest.mark.parametrize("tid", [1, 2, 13, 37, 38, -1])
def test_split_k_on_views(qlib, table, tid):
    """K = 200 in slices of 96, 96 and 8, and (automatic tile) the wave reduction of >= 128 slices into a misaligned window: alpha = 0.5 and beta = -2 are
    applied by the reduction kernels, so this is their ldc / strideC arithmetic."""
    t = next((x for x in table if x["id"] == tid), {"rows": 64, "cols": 64, "mode1": 0})
    ids = {x["id"] for x in table}
    for a_kc, b_kc in gv.LAYOUTS:
        for case in gv.split_k_cases(t["rows"], t["cols"], a_kc, b_kc):
            rec = _check_split(qlib, case, tid, t["mode1"])
            assert rec["cfg"] in ids
        if tid == -1:
            case = gv.wave_reduction_case(a_kc, b_kc)
            rec = _check_split(qlib, case, -1, 0)
            assert rec["ksplit"] >= 128 and case.M * case.N <= 65536 and case.expect_wide_c() == 0


@pytest.mark.parametrize("cfg,M,N", [(2, 512, 512), (2, 256 - 3, 1024), (2, 2048, 128 - 2), (1, 1024, 1024)])
def test_super_block_walk_writes_every_tile_once(qlib, table, cfg, M, N):
    """Grids of 16 x 16, 8 x 32 and 64 x 4 tiles of 32 x 32 and 16 x 16 tiles of 64 x 64 (a multiple of 256 tiles, one batch, no split): the tiles of an
    XCD's chunk are walked in super-blocks.  The product is a row gather of B[k, n] = k N + n on top of an integer C0: a walk that is not a bijection leaves
    tiles unwritten (C0 alone) or writes them twice (the gather added twice)."""
    t = next(x for x in table if x["id"] == cfg)
    tiles_m, tiles_n = -(-M // t["rows"]), -(-N // t["cols"])
    want = gv.super_block_rule(tiles_m, tiles_n, t["rows"], t["cols"])
    assert want[0] > 0                                        # these grids are chosen to take the walk
    b = gv.gather_case(M, N)
    got, rec = gv.run_case(qlib, b, cfg)
    assert (rec["sb_m"], rec["sb_n"]) == want and rec["cfg"] == cfg and rec["ksplit"] == 1 and rec["vec2"] == 1, rec
    assert gv.mismatch(got, b) == "", rec


@pytest.mark.parametrize("n", [193, 220, 224])
def test_quarter_lower_rows_windows(qlib, table, n):
    """The very windows gemm_quarter_lower_rows cuts (inner = 3, K = 40): A = C + s0 with lda = n, a result window of a wider matrix.  The upper part of the
    result (x' < s0 of every column block) keeps its sentinels bit for bit."""
    rows = {t["id"]: t["rows"] for t in table}
    q = gv.quarter_lower_case(n, 3, 40, rows)
    got, recs = gv.run_quarter_lower(qlib, q)
    bad = np.flatnonzero(~(got == q.expected))
    assert bad.size == 0, (n, q.windows, bad[:8], got[bad[:8]], q.expected[bad[:8]])
    by = {t["id"]: t for t in table}
    for (s0, s1, tid), rec in zip(q.windows, recs):
        vec2 = int(s0 % 2 == 0 and n % 2 == 0)
        assert rec["cfg"] == tid and rec["vec2"] == vec2 and rec["mode"] == (by[tid]["mode1"] if vec2 else 0), (n, s0, s1, rec)
        assert rec["wide_c"] == int(((s1 - s0) * 3) % 2 == 0 and (n * 3) % 2 == 0 and (s0 * n * 3 + s0 * 3) % 2 == 0), (n, s0, s1, rec)


def test_gemm_refuses_ld_below_extent(qlib):
    """The dispatcher's argument check (shared with the mock, where tests/test_gemm_views_hostlogic.py walks through it): refused before any launch."""
    from quemb_amd._lib import QEMB_ERR_ARG, DeviceBuffer
    d = DeviceBuffer.from_numpy(np.zeros(256))
    M, N, K = 6, 8, 10
    assert qlib.qemb_op_gemm(M, N, K, 1.0, d.ptr, K - 1, 1, 0, d.ptr, N, 0, 0, 0.0, d.ptr, N, 0, 1) == QEMB_ERR_ARG
    assert qlib.qemb_op_gemm(M, N, K, 1.0, d.ptr, K, 1, 0, d.ptr, N - 1, 0, 0, 0.0, d.ptr, N, 0, 1) == QEMB_ERR_ARG
    assert qlib.qemb_op_gemm(M, N, K, 1.0, d.ptr, K, 1, 0, d.ptr, N, 0, 0, 0.0, d.ptr, N - 1, 0, 1) == QEMB_ERR_ARG
    assert qlib.qemb_op_gemm(M, N, K, 1.0, d.ptr, K, 1, -1, d.ptr, N, 0, 0, 0.0, d.ptr, N, 0, 2) == QEMB_ERR_ARG
    d.free()
