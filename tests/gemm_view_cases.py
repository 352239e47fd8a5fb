"""dev_gemm on sub-matrix views, bit for bit: the case builder shared by tests/test_gemm_views_hostlogic.py (the hostcheck mock, CPU) and
tests/test_gpu_gemm_views.py (the HIP kernels).

A case places A, B and C as windows inside larger buffers: GUARD elements in front of the window and GUARD behind it, a base offset, a
leading dimension >= the extent and a batch stride >= ld * rows.  Everything of the A and B buffers outside the windows is NaN (a load that
takes one element of padding poisons the product); everything of the C buffer outside the window is -(index + 0.25), distinct per element (a
store that spills is seen, and where it came from).  With beta = 0 the C window itself starts as NaN.

Data, exact by construction: A holds integers in [-4, 4], B holds r + s * 2**-30 with integers r, s in [-4, 4], C0 integers in [-4, 4],
alpha in {1, 0.5}, beta in {0, 1, -2}.  With K <= 2**16 every partial sum, in any order and with fused multiply-adds, is below 2**21 with
lowest bit 2**-31: 52 bits, exact in FP64 (and in no FP32 or split-precision path).  The reference is formed in int64 on values scaled by
2**31 and converted once; the comparison is np.array_equal over the WHOLE C buffer.  No tolerance anywhere
(tests/test_gemm_views_hostlogic.py::test_data_classes_are_exact_in_any_summation_order proves the claim on the host).
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

GUARD = 64
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]
TABLE_IDS = (0, 1, 2, 4, 10, 11, 12, 13, 15, 20, 21, 33, 34, 35, 36, 37, 38)      # gemm_tiles.h: never renumbered (checked against the library on the CPU)
GEMM_CLASSIC = 200


# ---- the two introspection hooks -----------------------------------------------------------------------------------------------------------
def tile_table(lib):
    """Every entry of qemb_gemm_tile_table, in the table's order."""
    out = []
    for index in range(1000):
        v = [C.c_int() for _ in range(7)]
        if lib.qemb_gemm_tile_table(index, *[C.byref(x) for x in v]) != 0:
            break
        out.append(dict(zip(("id", "rows", "cols", "bk", "mode1", "has_classic", "ladder_twin"), (x.value for x in v))))
    return out


def last_launch(lib):
    v = [C.c_int() for _ in range(7)]
    assert lib.qemb_gemm_last_launch(*[C.byref(x) for x in v]) == 0
    return dict(zip(("cfg", "vec2", "mode", "ksplit", "sb_m", "sb_n", "wide_c"), (x.value for x in v)))


def slab_count(K, ksplit):
    """The K slices dev_gemm cuts for an explicit ksplit (chunks rounded up to 32)."""
    if ksplit <= 1 or K <= 0:
        return 1
    chunk = (-(-K // ksplit) + 31) // 32 * 32
    return max(-(-K // chunk), 1)


# ---- a case -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Place:
    """A window: base = allocation + GUARD + off elements, rows of `ld` elements, matrices `stride` elements apart."""
    off: int
    ld: int
    stride: int


@dataclass
class ViewCase:
    cls: str
    M: int
    N: int
    K: int
    a_kc: int
    b_kc: int
    pa: Place
    pb: Place
    pc: Place
    batch: int = 1
    alpha: float = 1.0
    beta: float = 0.0
    ksplit: int = 0
    must: dict = field(default_factory=dict)      # what the class pins of the launch report: {"vec2": 0/1, "wide_c": 0/1}

    def extents(self):
        """(rows, contiguous extent) of the stored A, B, C."""
        return ((self.M, self.K) if self.a_kc else (self.K, self.M), (self.N, self.K) if self.b_kc else (self.K, self.N), (self.M, self.N))

    # the dispatch rules as DESIGN.md and the header state them, restated here from offsets (the allocations are 16-byte aligned: run_case checks)
    def expect_vec2(self):
        def ok(p, ext, kc):
            return True if kc else (p.off % 2 == 0 and p.ld % 2 == 0 and p.stride % 2 == 0 and ext % 2 == 0)
        (_, ea), (_, eb), _ = self.extents()
        return int(ok(self.pa, ea, self.a_kc) and ok(self.pb, eb, self.b_kc))

    def expect_wide_c(self):
        return int(self.pc.ld % 2 == 0 and self.N % 2 == 0 and self.pc.off % 2 == 0 and (self.batch == 1 or self.pc.stride % 2 == 0))

    def label(self):
        return f"{self.cls} M={self.M} N={self.N} K={self.K} a_kc={self.a_kc} b_kc={self.b_kc} batch={self.batch} alpha={self.alpha} beta={self.beta} ksplit={self.ksplit}"


def _seed(c):
    return [c.M, c.N, c.K, c.a_kc, c.b_kc, c.batch, c.pa.off, c.pb.off, c.pc.off, c.pa.ld, c.pb.ld, c.pc.ld, int(2 * c.alpha), int(c.beta) + 2]


def exact_data(rng, batch, M, N, K, shared_b=False):
    """Logical A (batch, M, K), the two integer parts r, s of B = r + s * 2**-30 (batch or 1, K, N), C0 (batch, M, N): all int64."""
    A = rng.integers(-4, 5, (batch, M, K))
    r = rng.integers(-4, 5, (1 if shared_b else batch, K, N))
    s = rng.integers(-4, 5, (1 if shared_b else batch, K, N))
    C0 = rng.integers(-4, 5, (batch, M, N))
    return A, r, s, C0


def exact_reference(A, r, s, C0, alpha, beta):
    """alpha * A (r + s 2**-30) + beta * C0 in int64 on values scaled by 2**31, converted once.  (The two integer products run through the FP64 matmul: their
    entries are integers below 2**21, exact in any order; everything after that is int64.)"""
    assert 2 * alpha == int(2 * alpha) and beta == int(beta) and A.shape[-1] <= 2 ** 16
    Af = A.astype(np.float64)
    pr = np.matmul(Af, r.astype(np.float64)).astype(np.int64)
    ps = np.matmul(Af, s.astype(np.float64)).astype(np.int64)
    scaled = int(2 * alpha) * (pr * 2 ** 30 + ps) + int(beta) * C0 * 2 ** 31
    assert np.abs(scaled).max(initial=0) < 2 ** 53
    return scaled.astype(np.float64) * 2.0 ** -31


def _indices(p, nmat, rows, ext):
    return (GUARD + p.off + np.arange(nmat)[:, None, None] * p.stride + np.arange(rows)[None, :, None] * p.ld + np.arange(ext)[None, None, :])


def _size(p, nmat, rows, ext):
    return GUARD + p.off + (nmat - 1) * p.stride + (rows - 1) * p.ld + ext + GUARD


def sentinels(n):
    return -(np.arange(n, dtype=np.float64) + 0.25)


@dataclass
class Built:
    case: ViewCase
    bufA: np.ndarray
    bufB: np.ndarray
    bufC: np.ndarray
    expected: np.ndarray      # the full C buffer after the product, sentinels included


def build(c, data=None):
    """Buffers, and the expected full C buffer, of one case.  data: (A, r, s, C0) as exact_data returns them (default: seeded from the case)."""
    (ra, ea), (rb, eb), (rc, ec) = c.extents()
    for p, rows, ext in ((c.pa, ra, ea), (c.pb, rb, eb), (c.pc, rc, ec)):
        assert p.ld >= ext and p.off >= 0 and (p.stride >= p.ld * rows or (p.stride == 0 and p is c.pb) or c.batch == 1), (c.label(), p)
    shared_b = c.batch > 1 and c.pb.stride == 0
    A, r, s, C0 = data if data is not None else exact_data(np.random.default_rng(_seed(c)), c.batch, c.M, c.N, c.K, shared_b)
    nb = 1 if shared_b else c.batch
    bufA = np.full(_size(c.pa, c.batch, ra, ea), np.nan)
    bufB = np.full(_size(c.pb, nb, rb, eb), np.nan)
    n_c = _size(c.pc, c.batch, rc, ec)
    bufC, expected = sentinels(n_c), sentinels(n_c)
    Bv = r.astype(np.float64) + s.astype(np.float64) * 2.0 ** -30
    bufA[_indices(c.pa, c.batch, ra, ea)] = A if c.a_kc else A.transpose(0, 2, 1)
    bufB[_indices(c.pb, nb, rb, eb)] = Bv.transpose(0, 2, 1) if c.b_kc else Bv
    ic = _indices(c.pc, c.batch, rc, ec)
    bufC[ic] = C0 if c.beta != 0.0 else np.nan
    expected[ic] = exact_reference(A, r, s, C0, c.alpha, c.beta)
    return Built(c, bufA, bufB, bufC, expected)


def run_case(lib, b, cfg=-1):
    """The case through qemb_op_gemm of `lib` (the HIP library or the hostcheck mock).  Returns the full C buffer and the launch report."""
    from quemb_amd._lib import DeviceBuffer, check
    c = b.case
    dA, dB, dC = (DeviceBuffer.from_numpy(x, lib=lib) for x in (b.bufA, b.bufB, b.bufC))
    assert dA.ptr % 16 == 0 and dB.ptr % 16 == 0 and dC.ptr % 16 == 0
    lib.qemb_set_gemm_config(cfg)
    lib.qemb_set_gemm_ksplit(c.ksplit)
    try:
        check(lib.qemb_op_gemm(c.M, c.N, c.K, c.alpha, dA.at(GUARD + c.pa.off), c.pa.ld, c.a_kc, c.pa.stride, dB.at(GUARD + c.pb.off), c.pb.ld, c.b_kc,
                               c.pb.stride, c.beta, dC.at(GUARD + c.pc.off), c.pc.ld, c.pc.stride, c.batch), "qemb_op_gemm: " + c.label(), lib)
        rec = last_launch(lib)
    finally:
        lib.qemb_set_gemm_config(-1)
        lib.qemb_set_gemm_ksplit(0)
    got = dC.numpy()
    for d in (dA, dB, dC):
        d.free()
    return got, rec


def mismatch(got, b):
    """'' when the whole C buffer is as expected bit for bit, else where the first difference sits."""
    if np.array_equal(got, b.expected):
        return ""
    bad = np.flatnonzero(~((got == b.expected)))
    i = int(bad[0])
    c = b.case
    rel = i - GUARD - c.pc.off
    where = "guard band in front of the C window" if rel < 0 else f"batch {rel // c.pc.stride if c.batch > 1 and c.pc.stride else 0}, row {(rel % c.pc.stride if c.batch > 1 and c.pc.stride else rel) // c.pc.ld}, column {(rel % c.pc.stride if c.batch > 1 and c.pc.stride else rel) % c.pc.ld} of ldc = {c.pc.ld} (N = {c.N})"
    return f"{c.label()}: {bad.size} elements of the C buffer differ; first at element {i} ({where}): got {got[i]!r}, expected {b.expected[i]!r}"


# ---- the view classes ---------------------------------------------------------------------------------------------------------------------
def _place(ext, rows, off=0, pad=0, gap=0):
    ld = ext + pad
    return Place(off, ld, ld * rows + gap)


def view_cases(tile, a_kc, b_kc):
    """The cases of one tile (an entry of tile_table) on one operand layout: every view class that applies to the layout, at the smallest shapes that reach
    every branch -- M in {rows + 3, rows - 1}, N in {cols + 6, cols + 5}, K = 2 bk + 3 (guarded prologue tile, one interior tile through the pointer-bump
    loader with clamped edge rows, guarded k-tail), K = bk - 3 (a single partial tile) and, for MODE 1 tiles, K = 5 bk (the steady state of the
    one-k-step-ahead loop, no tail).  A class that must report 16-byte loads takes the even neighbours (rows + 2 / rows - 2, cols + 6 / cols + 4) for an
    M/N-contiguous operand, whose extent has to be even; K-contiguous operands keep the odd sizes."""
    rows, cols, bk = tile["rows"], tile["cols"], tile["bk"]
    K3, K1, K5 = 2 * bk + 3, bk - 3, (5 * bk if tile["mode1"] else 2 * bk + 3)
    M_odd, N_any = (rows + 3, rows - 1), (cols + 6, cols + 5)
    M_v = M_odd if a_kc else (rows + 2, rows - 2)            # sizes at which A allows 16-byte loads
    N_v = N_any if b_kc else (cols + 6, cols + 4)            # ... and B
    out = []

    def add(cls, M, N, K, alpha, beta, a=(0, 0, 0), b=(0, 0, 0), c=(0, 0, 0), batch=1, shared_b=False, must=None):
        case = ViewCase(cls, M, N, K, a_kc, b_kc, None, None, None, batch=batch, alpha=alpha, beta=beta, must=dict(must or {}))
        (ra, ea), (rb, eb), (rc, ec) = case.extents()
        case.pa, case.pb, case.pc = _place(ea, ra, *a), _place(eb, rb, *b), _place(ec, rc, *c)
        if shared_b:
            case.pb.stride = 0
        for k, v in case.must.items():      # a class states what it is built to hit; the construction has to deliver it by the documented rule
            assert {"vec2": case.expect_vec2, "wide_c": case.expect_wide_c}[k]() == v, (case.label(), k, v)
        out.append(case)

    even = (2, 6, 10)                                         # (base offset, ld - extent, stride - ld * rows)
    # tight: today's layout
    add("tight", M_odd[0], N_any[0], K3, 1.0, 0.0)
    add("tight", M_odd[1], N_any[1], K1, 0.5, 1.0)
    add("tight", M_v[0], N_v[0], K5, 1.0, -2.0, must={"vec2": 1, "wide_c": 1})
    # padded_even: even offsets, ld = extent + 6, even strides
    add("padded_even", M_v[0], N_v[0], K3 + 1, 1.0, 1.0, even, even, even, must={"vec2": 1, "wide_c": 1})
    add("padded_even", M_v[1], N_v[1], K5, 0.5, 0.0, even, even, even, must={"vec2": 1, "wide_c": int(N_v[1] % 2 == 0)})
    # k8: K-contiguous operands at an odd element offset with odd ld and odd K -- 8-byte pair loads and the lone last element of every row
    if a_kc or b_kc:
        odd = (1, 2, 11)                                      # K odd: ld = K + 2 odd; odd stride
        add("k8", M_v[0], N_v[0], K3, 0.5, -2.0, odd if a_kc else even, odd if b_kc else even, must={"vec2": 1})
        add("k8", M_v[1], N_v[1], K1, 1.0, 0.0, odd if a_kc else even, odd if b_kc else even, even, must={"vec2": 1})
    # scalar_base / scalar_ld: an M/N-contiguous operand that forbids 16-byte loads
    if not (a_kc and b_kc):
        first_a = not a_kc                                    # the first M/N-contiguous operand takes the odd base, the last one the odd ld
        add("scalar_base", M_v[0], N_v[0], K3, 1.0, 1.0, (1, 6, 10) if first_a else even, even if first_a else (1, 6, 10), even, must={"vec2": 0})
        last_b = not b_kc
        add("scalar_ld", M_v[1], N_v[1], K3, 0.5, 0.0, even if last_b else (2, 5, 10), (2, 5, 10) if last_b else even, even, must={"vec2": 0})
    # the three ways C leaves the wide epilogue, on operands that keep the 16-byte loads
    add("c_odd_ld", M_v[0], N_v[0], K3 + 1, 0.5, 1.0, even, even, (2, 5, 10), must={"vec2": 1, "wide_c": 0})
    add("c_misaligned", M_v[1], N_v[0], K5, 1.0, -2.0, even, even, (1, 6, 10), must={"vec2": 1, "wide_c": 0})
    add("c_odd_n", M_v[0], cols + 5, K3, 1.0, 0.0, even, even, (2, 1, 10), must={"wide_c": 0})
    # batch_gap: three matrices further apart than they are long; once with one B for all
    gap = (2, 6, 14)
    add("batch_gap", M_v[1], N_v[0], K3 + 1, 0.5, 1.0, gap, gap, gap, batch=3, must={"vec2": 1, "wide_c": 1})
    add("batch_gap", M_odd[0], N_any[1], K1, 1.0, 0.0, gap, gap, (1, 6, 15), batch=3, shared_b=True, must={"wide_c": 0})
    return out


def split_k_cases(rows, cols, a_kc, b_kc):
    """K = 200 under ksplit = 3: chunks of 96, 96 and 8 -- the last slice is shorter than one k-tile.  alpha = 0.5, beta = -2 are applied by the reduction
    kernel, through the ldc / strideC of the view."""
    assert slab_count(200, 3) == 3
    M, N, K = rows + 3 if a_kc else rows + 2, cols + 6, 200
    out = []
    for cls, cpl, batch in (("padded_even", (2, 6, 10), 1), ("c_odd_ld", (2, 5, 10), 1), ("batch_gap", (2, 6, 14), 3)):
        c = ViewCase(cls, M, N, K, a_kc, b_kc, None, None, None, batch=batch, alpha=0.5, beta=-2.0, ksplit=3)
        (ra, ea), (rb, eb), (rc, ec) = c.extents()
        pad = (2, 6, 14 if batch > 1 else 10)
        c.pa, c.pb, c.pc = _place(ea, ra, *pad), _place(eb, rb, *pad), _place(ec, rc, *cpl)
        c.must = {"vec2": 1}
        assert c.expect_vec2() == 1
        out.append(c)
    return out


def wave_reduction_case(a_kc, b_kc):
    """>= 128 slices at M N <= 65536: the one-wave-per-element reduction kernel, writing a c_misaligned window."""
    M, N, K, ks = 21, 19, 4100, 200
    assert slab_count(K, ks) >= 128 and M * N <= 65536 and K <= 2 ** 16
    c = ViewCase("c_misaligned", M, N, K, a_kc, b_kc, None, None, None, alpha=0.5, beta=-2.0, ksplit=ks)
    (ra, ea), (rb, eb), (rc, ec) = c.extents()
    c.pa, c.pb, c.pc = _place(ea, ra, 2, 6, 10), _place(eb, rb, 2, 6, 10), _place(ec, rc, 1, 7, 10)
    return c


# ---- the super-block walk -----------------------------------------------------------------------------------------------------------------
def super_block_rule(tiles_m, tiles_n, bm, bn, batch=1, ksplit=1):
    """(sb_m, sb_n) as launch_cfg chooses them: super-blocks of 32 tiles, the shape that moves the fewest operand bytes per k-step among those that divide
    the grid; (0, 0): the m-fastest walk."""
    if not (batch == 1 and ksplit <= 1 and tiles_m >= 8 and tiles_n >= 4 and (tiles_m * tiles_n) % 256 == 0):
        return 0, 0
    best, pick = None, (0, 0)
    for sm in (1, 2, 4, 8, 16, 32):
        sn = 32 // sm
        if tiles_m % sm or tiles_n % sn:
            continue
        cost = sm * bm + sn * bn
        if best is None or cost < best:
            best, pick = cost, (sm, sn)
    return (0, 0) if pick[0] == 32 else pick


def gather_case(M, N, K=40):
    """A has a single 1 per row, so the product is a row gather of the asymmetric integer B[k, n] = k N + n: a misplaced tile shows as wrong values, not as
    noise; beta = 1 on an integer C0 makes a tile written twice wrong too.  Tight views, A K-contiguous, B N-contiguous."""
    c = ViewCase("tight", M, N, K, 1, 0, Place(0, K, M * K), Place(0, N, K * N), Place(0, N, M * N), alpha=1.0, beta=1.0)
    rng = np.random.default_rng([M, N, K])
    src = (7 * np.arange(M) + 3) % K
    A = np.zeros((1, M, K), dtype=np.int64)
    A[0, np.arange(M), src] = 1
    Bm = (np.arange(K)[:, None] * N + np.arange(N)[None, :]).astype(np.float64)
    C0 = rng.integers(-4, 5, (1, M, N))
    bufA = np.full(_size(c.pa, 1, M, K), np.nan)
    bufB = np.full(_size(c.pb, 1, K, N), np.nan)
    bufC, expected = sentinels(_size(c.pc, 1, M, N)), sentinels(_size(c.pc, 1, M, N))
    bufA[_indices(c.pa, 1, M, K)] = A
    bufB[_indices(c.pb, 1, K, N)] = Bm[None]
    ic = _indices(c.pc, 1, M, N)
    bufC[ic] = C0
    expected[ic] = Bm[src][None] + C0          # integers below 2**53: exact
    return Built(c, bufA, bufB, bufC, expected)


# ---- the windows gemm_quarter_lower_rows cuts ---------------------------------------------------------------------------------------------
QUARTER_TILES = (13, 15, 4, 33, 12)      # tensor_utils.h: 224-, 192-, 128-, 112- and 64-row tiles, tallest first


def quarter_lower_windows(n, tile_rows):
    """(s0, s1, tile id) of every product gemm_quarter_lower_rows issues for 193 <= n <= 224: column block [s0, s1) of the result is computed for the rows
    x' >= s0 only, on the smallest tile that holds n - s0 rows."""
    out, s0 = [], 0
    for t, tid in enumerate(QUARTER_TILES):
        if s0 >= n:
            break
        s1 = min(n, max(s0, n - tile_rows[QUARTER_TILES[t + 1]])) if t + 1 < len(QUARTER_TILES) else n
        if s1 > s0:
            out.append((s0, s1, tid))
        s0 = s1
    return out


@dataclass
class QuarterLower:
    n: int
    inner: int
    K: int
    windows: list
    bufA: np.ndarray          # C[k][x'] (K x n) between guard bands
    bufB: np.ndarray          # In[(y', i)][k] (n inner x K) between guard bands
    bufC: np.ndarray          # Out[x'][(y', i)] (n x n inner): NaN where a window will be written, sentinels everywhere else
    expected: np.ndarray


def quarter_lower_case(n, inner, K, tile_rows):
    """Out[x', (y', i)] = sum_k C[k, x'] In[(y', i), k] for the windows only, into ONE result buffer: whatever lies in no window -- the guard bands and the
    upper part x' < s0 of every column block -- keeps its sentinels."""
    ncol = n * inner
    rng = np.random.default_rng([n, inner, K])
    A, r, s, _ = exact_data(rng, 1, n, ncol, K)
    bufA = np.full(GUARD + K * n + GUARD, np.nan)
    bufB = np.full(GUARD + ncol * K + GUARD, np.nan)
    bufA[GUARD:GUARD + K * n] = A[0].T.reshape(-1)
    bufB[GUARD:GUARD + ncol * K] = (r[0] + s[0] * 2.0 ** -30).T.reshape(-1)
    full = exact_reference(A, r, s, np.zeros((1, n, ncol), dtype=np.int64), 1.0, 0.0)[0]
    bufC, expected = sentinels(GUARD + n * ncol + GUARD), sentinels(GUARD + n * ncol + GUARD)
    wins = quarter_lower_windows(n, tile_rows)
    vC, vE = bufC[GUARD:GUARD + n * ncol].reshape(n, ncol), expected[GUARD:GUARD + n * ncol].reshape(n, ncol)
    for s0, s1, _ in wins:
        vC[s0:, s0 * inner:s1 * inner] = np.nan
        vE[s0:, s0 * inner:s1 * inner] = full[s0:, s0 * inner:s1 * inner]
    return QuarterLower(n, inner, K, wins, bufA, bufB, bufC, expected)


def run_quarter_lower(lib, q):
    """The windows of q through qemb_op_gemm with the very arguments gemm_quarter_lower_rows passes.  Returns the result buffer and the launch reports."""
    from quemb_amd._lib import DeviceBuffer, check
    n, inner, K, ncol = q.n, q.inner, q.K, q.n * q.inner
    dA, dB, dC = (DeviceBuffer.from_numpy(x, lib=lib) for x in (q.bufA, q.bufB, q.bufC))
    recs = []
    try:
        for s0, s1, tid in q.windows:
            lib.qemb_set_gemm_config(tid)
            check(lib.qemb_op_gemm(n - s0, (s1 - s0) * inner, K, 1.0, dA.at(GUARD + s0), n, 0, 0, dB.at(GUARD + s0 * inner * K), K, 1, 0, 0.0,
                                   dC.at(GUARD + s0 * ncol + s0 * inner), ncol, 0, 1), f"quarter window n={n} s0={s0} s1={s1} tile={tid}", lib)
            recs.append(last_launch(lib))
    finally:
        lib.qemb_set_gemm_config(-1)
    got = dC.numpy()
    for d in (dA, dB, dC):
        d.free()
    return got, recs
