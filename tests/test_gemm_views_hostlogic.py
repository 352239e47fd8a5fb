"""CPU: the sub-matrix view cases of tests/gemm_view_cases.py rehearsed on the hostcheck mock (whose dev_gemm honours ld and strides) before anything runs
on a GPU -- the builder, the offsets and the sentinel bookkeeping -- together with the proof that the data classes need no tolerance, the tile table the
GPU tests are parametrised from, and the argument checks of dev_gemm."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import gemm_view_cases as gv

sys.path.insert(0, str(Path(__file__).resolve().parent / "hostcheck"))


@pytest.fixture(scope="module")
def hlib():
    import build as hc_build
    from quemb_amd import _lib
    lib = _lib.declare(C.CDLL(str(hc_build.build())))
    assert lib.qemb_backend() == b"hostcheck"
    return lib


@pytest.fixture(scope="module")
def table(hlib):
    return gv.tile_table(hlib)


def test_tile_table_is_the_header_table(hlib, table):
    """The ids in the order gemm_tiles.h writes them (never renumbered), dimensions, classic-loop twins and ladder twins."""
    assert tuple(t["id"] for t in table) == gv.TABLE_IDS
    v = [C.c_int() for _ in range(7)]
    assert hlib.qemb_gemm_tile_table(len(table), *[C.byref(x) for x in v]) == -1          # QEMB_ERR_ARG past the end
    assert hlib.qemb_gemm_tile_table(-1, *[C.byref(x) for x in v]) == -1
    by = {t["id"]: t for t in table}
    assert (by[13]["rows"], by[13]["cols"]) == (224, 128) and (by[34]["rows"], by[34]["cols"]) == (128, 224) and (by[38]["rows"], by[38]["cols"]) == (48, 128)
    assert by[2]["bk"] == 32 and all(t["bk"] == 16 for t in table if t["id"] != 2)
    assert {t["id"]: t["ladder_twin"] for t in table if t["ladder_twin"] >= 0} == {13: 23, 15: 25}
    assert sorted(t["id"] for t in table if not t["has_classic"]) == [2, 10, 11, 12, 20, 21, 38]
    assert sorted(t["id"] for t in table if t["mode1"]) == [0, 1, 4, 13, 15, 33, 34, 35, 36, 37, 38]
    assert all(t["mode1"] for t in table if t["has_classic"])                               # only a MODE 1 tile has a classic loop to fall back to


def test_data_classes_are_exact_in_any_summation_order():
    """The largest case (K = 4100): FP64 products summed forward, reversed and pairwise all equal the int64 reference -- no tolerance is needed."""
    c = gv.wave_reduction_case(1, 0)
    A, r, s, C0 = gv.exact_data(np.random.default_rng(7), 1, c.M, c.N, c.K)
    ref = gv.exact_reference(A, r, s, np.zeros_like(C0), 1.0, 0.0)[0]
    B = r[0] + s[0] * 2.0 ** -30
    prod = A[0].astype(np.float64)[:, :, None] * B[None, :, :]                               # (M, K, N): every term exact
    fwd = np.zeros((c.M, c.N)); rev = np.zeros((c.M, c.N))
    for k in range(c.K):
        fwd += prod[:, k, :]
        rev += prod[:, c.K - 1 - k, :]
    pad = np.concatenate([prod, np.zeros((c.M, 4 * 1025 - c.K, c.N))], axis=1)
    pair = np.add.reduce(np.add.reduce(pad.reshape(c.M, 1025, 4, c.N), axis=2), axis=1)      # partial sums of four, then of those
    assert np.array_equal(fwd, ref) and np.array_equal(rev, ref) and np.array_equal(pair, ref)
    assert np.abs(ref).max() < 2.0 ** 21 and np.any(ref != np.round(ref))                    # ... and the low bits are in use
    assert not np.array_equal((A[0].astype(np.float32) @ B.astype(np.float32)).astype(np.float64), ref)      # a single-precision path is seen


def test_builder_places_windows_and_sentinels(table):
    """The bookkeeping itself: guard bands, ld - extent columns and batch gaps are NaN (A, B) or -(index + 0.25) (C); the windows hold the data."""
    t = next(x for x in table if x["id"] == 2)
    c = next(x for x in gv.view_cases(t, 0, 1) if x.cls == "batch_gap" and x.pb.stride != 0)
    b = gv.build(c)
    assert c.pc.ld > c.N and c.pc.stride > c.pc.ld * c.M and c.pa.off and c.batch == 3
    inside = np.zeros(b.bufC.size, dtype=bool)
    inside[gv._indices(c.pc, c.batch, c.M, c.N)] = True
    assert inside.sum() == 3 * c.M * c.N and not inside[:gv.GUARD + c.pc.off].any() and not inside[-gv.GUARD:].any() and inside[-gv.GUARD - 1]
    assert np.array_equal(b.bufC[~inside], gv.sentinels(b.bufC.size)[~inside]) and np.array_equal(b.expected[~inside], b.bufC[~inside])
    assert np.isfinite(b.expected).all() and np.isnan(b.bufA).sum() == b.bufA.size - 3 * c.M * c.K and np.isnan(b.bufB).sum() == b.bufB.size - 3 * c.K * c.N
    got = b.expected.copy(); got[gv.GUARD + c.pc.off + c.N] += 1.0                          # one element past N, in the padding of row 0
    assert "column %d" % c.N in gv.mismatch(got, b) and gv.mismatch(b.expected, b) == ""


def test_every_class_is_present_on_the_layouts_it_applies_to(table):
    for t in table:
        for a_kc, b_kc in gv.LAYOUTS:
            cases = gv.view_cases(t, a_kc, b_kc)
            want = {"tight", "padded_even", "c_odd_ld", "c_misaligned", "c_odd_n", "batch_gap"}
            want |= {"k8"} if (a_kc or b_kc) else set()
            want |= {"scalar_base", "scalar_ld"} if not (a_kc and b_kc) else set()
            assert {c.cls for c in cases} == want
            assert {c.K for c in cases} >= {2 * t["bk"] + 3, t["bk"] - 3} | ({5 * t["bk"]} if t["mode1"] else set())
            assert {t["rows"] + 3, t["rows"] - 1} <= {c.M for c in cases} and {t["cols"] + 6, t["cols"] + 5} <= {c.N for c in cases}
            assert any(c.batch == 3 and c.pb.stride == 0 for c in cases)
            assert max(c.M for c in cases) <= 260 and max(c.N for c in cases) <= 270 and max(c.K for c in cases) <= 163


def _check(hlib, case):
    b = gv.build(case)
    got, rec = gv.run_case(hlib, b)
    assert gv.mismatch(got, b) == ""
    assert rec["vec2"] == case.expect_vec2() and rec["wide_c"] == case.expect_wide_c(), (case.label(), rec)
    for k, v in case.must.items():
        assert rec[k] == v, (case.label(), k, rec)
    assert (rec["cfg"], rec["mode"], rec["ksplit"], rec["sb_m"], rec["sb_n"]) == (0, 0, 0, 0, 0)      # the mock chooses no tile, loop or split


@pytest.mark.parametrize("index", range(len(gv.TABLE_IDS)))
@pytest.mark.parametrize("a_kc,b_kc", gv.LAYOUTS)
def test_mock_every_tile_on_every_view(hlib, table, index, a_kc, b_kc):
    for case in gv.view_cases(table[index], a_kc, b_kc):
        _check(hlib, case)


@pytest.mark.parametrize("tid", [1, 2, 13, 37, 38, -1])
def test_mock_split_k_on_views(hlib, table, tid):
    rows, cols = next(((t["rows"], t["cols"]) for t in table if t["id"] == tid), (64, 64))
    for a_kc, b_kc in gv.LAYOUTS:
        for case in gv.split_k_cases(rows, cols, a_kc, b_kc):
            _check(hlib, case)
        if tid == -1:
            _check(hlib, gv.wave_reduction_case(a_kc, b_kc))


def test_super_block_rule_and_gather_case(hlib):
    """The rule of launch_cfg restated (the GPU test asserts the launch report against it), and the gather product through the mock."""
    assert gv.super_block_rule(16, 16, 32, 32) == (4, 8) and gv.super_block_rule(8, 32, 32, 32) == (4, 8) and gv.super_block_rule(64, 4, 32, 32) == (8, 4)
    assert gv.super_block_rule(16, 16, 64, 64) == (4, 8) and gv.super_block_rule(32, 16, 128, 256) == (8, 4)
    assert gv.super_block_rule(16, 15, 32, 32) == (0, 0) and gv.super_block_rule(4, 64, 32, 32) == (0, 0) and gv.super_block_rule(256, 1, 32, 32) == (0, 0)
    assert gv.super_block_rule(16, 16, 32, 32, batch=2) == (0, 0) and gv.super_block_rule(16, 16, 32, 32, ksplit=2) == (0, 0)
    assert gv.super_block_rule(64, 4, 16, 512) == (0, 0)                                     # 32 x 1 is cheapest: the m-fastest walk already
    b = gv.gather_case(256 - 3, 96)
    got, _ = gv.run_case(hlib, b)
    assert gv.mismatch(got, b) == ""
    assert b.expected[gv.GUARD + 5 * 96 + 7] == ((7 * 5 + 3) % 40) * 96 + 7 + b.bufC[gv.GUARD + 5 * 96 + 7]


@pytest.mark.parametrize("n", [193, 220, 224])
def test_mock_quarter_lower_rows_windows(hlib, table, n):
    rows = {t["id"]: t["rows"] for t in table}
    q = gv.quarter_lower_case(n, 3, 40, rows)
    assert q.windows[0][0] == 0 and q.windows[-1][1] == n and all(a[1] == b[0] for a, b in zip(q.windows, q.windows[1:]))
    assert all(n - s0 <= rows[tid] for s0, _, tid in q.windows)                              # every window fits one row tile
    if n == 193:
        assert q.windows[:2] == [(0, 1, 13), (1, 65, 15)]                                    # the second window starts at an odd element of C
    got, recs = gv.run_quarter_lower(hlib, q)
    assert np.array_equal(got, q.expected)
    view = got[gv.GUARD:gv.GUARD + n * n * 3].reshape(n, n * 3)
    sent = gv.sentinels(got.size)[gv.GUARD:gv.GUARD + n * n * 3].reshape(n, n * 3)
    upper = np.zeros((n, n * 3), dtype=bool)
    for s0, s1, _ in q.windows:
        upper[:s0, s0 * 3:s1 * 3] = True
    assert upper.sum() > 0 and np.array_equal(view[upper], sent[upper])                      # x' < s0 of every column block: untouched
    for (s0, s1, _), rec in zip(q.windows, recs):
        assert rec["vec2"] == int(s0 % 2 == 0 and n % 2 == 0) and rec["wide_c"] == int(((s1 - s0) * 3) % 2 == 0 and (n * 3) % 2 == 0 and (s0 * n * 3 + s0 * 3) % 2 == 0)


def test_gemm_refuses_ld_below_extent_and_negative_strides(hlib):
    from quemb_amd._lib import QEMB_ERR_ARG, DeviceBuffer
    M, N, K = 6, 8, 10
    bufs = [DeviceBuffer.from_numpy(np.zeros(4 * 64), lib=hlib) for _ in range(3)]
    dA, dB, dC = bufs

    def call(a_kc=1, b_kc=0, lda=None, ldb=None, ldc=None, sA=0, sB=0, sC=0, batch=1):
        lda = (K if a_kc else M) if lda is None else lda
        ldb = (K if b_kc else N) if ldb is None else ldb
        return hlib.qemb_op_gemm(M, N, K, 1.0, dA.ptr, lda, a_kc, sA, dB.ptr, ldb, b_kc, sB, 0.0, dC.ptr, N if ldc is None else ldc, sC, batch)

    assert call() == 0 and call(a_kc=0, b_kc=1) == 0
    assert call(lda=K - 1) == QEMB_ERR_ARG and b"lda" in hlib.qemb_last_error()
    assert call(a_kc=0, lda=M - 1) == QEMB_ERR_ARG
    assert call(a_kc=0, lda=M) == 0                                                          # K > M: the extent is M for an M-contiguous A
    assert call(ldb=N - 1) == QEMB_ERR_ARG and b"ldb" in hlib.qemb_last_error()
    assert call(b_kc=1, ldb=K - 1) == QEMB_ERR_ARG and call(b_kc=1, ldb=N) == QEMB_ERR_ARG and call(b_kc=1, ldb=K) == 0
    assert call(ldc=N - 1) == QEMB_ERR_ARG and b"ldc" in hlib.qemb_last_error()
    assert call(lda=0) == QEMB_ERR_ARG and call(ldc=-N) == QEMB_ERR_ARG
    for kw in ({"sA": -1}, {"sB": -2}, {"sC": -M * N}):
        assert call(batch=2, **kw) == QEMB_ERR_ARG and b"stride" in hlib.qemb_last_error()
    assert call(batch=2, sA=M * K, sB=0, sC=M * N) == 0                                      # one B for all: stride 0 stays legal
    for d in bufs:
        d.free()
