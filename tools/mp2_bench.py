"""Time the MP2 solve of a fragment that lives on its 3-index factor against the CCSD solve of the same fragment in the same process.

    python tools/mp2_bench.py [out.jsonl]        (default profiles/mp2_bench.jsonl; sizes: the benchmark's n = 220 / n_occ = 20 / naux = 660, and n = 42, 96, 132)

Per size one JSON line: wall time of a warm MP2 solve with energies (qemb_frag_solve_mp2: fragment RHF + products with the factor + the amplitude pass +
densities + energies), and of a warm CCSD solve with its phases from the device timers -- `ccsd_outside_iterations_ms` is the CCSD wall time minus the device
time of its iterations, i.e. fragment RHF + MO integrals + set-up (+ the short end phase): what an MP2 solve, which does a strict subset of that work, has to
stay under.  The amplitude pass (dev_mp2_amplitudes) is timed on its own and priced as an HBM pass: 3 x 8 o^2 v^2 bytes against 8 TB/s."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from quemb_amd import _lib                                               # noqa: E402
from quemb_amd._lib import DeviceBuffer, check                            # noqa: E402
from quemb_amd.fragsolver import DeviceFragment, default_opts             # noqa: E402

HBM_PEAK = 8.0e12
SIZES = [(220, 20, 660), (42, 21, 126), (96, 9, 288), (132, 12, 396)]
SLOT = 9


def factor_fragment(n, seed, naux, gap=2.0):
    rng = np.random.default_rng(seed)
    scale = 0.06 * min(1.0, (55.0 / n) ** 0.5)
    B = scale * rng.standard_normal((naux, n, n))
    B = 0.5 * (B + B.transpose(0, 2, 1))
    il = np.tril_indices(n)
    A = rng.standard_normal((n, n))
    return np.diag(gap * np.arange(n)) + 0.3 * 0.5 * (A + A.T), np.ascontiguousarray(B[:, il[0], il[1]])


def timer(lib, slot):
    ms = C.c_double(); cnt = C.c_int64()
    lib.qemb_timer_read(slot, C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def amplitude_pass(lib, o, v, reps=20):
    rng = np.random.default_rng(3)
    d_in = DeviceBuffer.from_numpy(rng.standard_normal(o * v * o * v))
    d_eo, d_ev = DeviceBuffer.from_numpy(-1.0 - np.arange(o, dtype=float)), DeviceBuffer.from_numpy(1.0 + np.arange(v, dtype=float))
    d_t2, d_G = DeviceBuffer(o * o * v * v), DeviceBuffer(o * o * v * v)
    e = C.c_double()
    for _ in range(3):
        check(lib.qemb_op_mp2_amplitudes(o, v, d_in.ptr, d_eo.ptr, d_ev.ptr, d_t2.ptr, d_G.ptr, C.byref(e)))
    best = None
    for _ in range(reps):
        lib.qemb_timer_reset(SLOT)
        lib.qemb_timer_begin(SLOT)
        check(lib.qemb_op_mp2_amplitudes(o, v, d_in.ptr, d_eo.ptr, d_ev.ptr, d_t2.ptr, d_G.ptr, C.byref(e)))
        lib.qemb_timer_end(SLOT)
        ms = timer(lib, SLOT)[0]
        best = ms if best is None else min(best, ms)
    for d in (d_in, d_eo, d_ev, d_t2, d_G):
        d.free()
    return best


def one_size(lib, n, o, naux):
    v = n - o
    h, Bp = factor_fragment(n, 20260803, naux)
    fr = DeviceFragment(n, min(22, n // 2))
    fr.set_df_only(Bp)
    rng = np.random.default_rng(1)
    V = rng.standard_normal((n, n))
    fr.set_energy_data(h, 0.05 * (V + V.T), None, 1.0, list(range(4)))
    h2 = h.copy(); h2[:4, :4] += 1e-3                                   # as in a BE sweep: the one-body matrix moved a little, dm0 is the previous density
    res = dict(n=n, o=o, naux=naux)
    out = fr.solve_mp2(o, h, eeval=True)                                # cold: allocations
    dm0 = 2.0 * out["mo_coeff"][:, :o] @ out["mo_coeff"][:, :o].T
    walls = []
    for _ in range(5):
        lib.qemb_sync(); t0 = time.perf_counter()
        out = fr.solve_mp2(o, h2, dm0=dm0, eeval=True)
        lib.qemb_sync(); walls.append(1e3 * (time.perf_counter() - t0))
    res.update(mp2_wall_ms=min(walls), mp2_wall_ms_all=walls, e_mp2=out["e_corr_mo"], scf_cycles=out["scf_cycles"], mo_route_factor=fr.mo_route_used()[0])
    fr.solve(o, h, opts=default_opts(), eeval=True)                      # cold CCSD
    best = None
    for _ in range(3):
        for s in range(8):
            lib.qemb_timer_reset(s)
        lib.qemb_sync(); t0 = time.perf_counter()
        cc = fr.solve(o, h2, dm0=dm0, opts=default_opts(), eeval=True)
        lib.qemb_sync(); wall = 1e3 * (time.perf_counter() - t0)
        it_ms, it_n = timer(lib, 2)
        row = dict(ccsd_wall_ms=wall, ccsd_iterations=cc["n_iter"], ccsd_iterations_ms=it_ms, ccsd_outside_iterations_ms=wall - it_ms,
                   ccsd_scf_ms=timer(lib, 4)[0], ccsd_mo_integrals_ms=timer(lib, 3)[0], e_ccsd=cc["e_corr_mo"])
        if best is None or row["ccsd_outside_iterations_ms"] < best["ccsd_outside_iterations_ms"]:
            best = row
    res.update(best)
    res["mp2_within_ccsd_prephase"] = bool(res["mp2_wall_ms"] <= res["ccsd_outside_iterations_ms"])
    ms = amplitude_pass(lib, o, v)
    nbytes = 3.0 * 8.0 * (o * v) ** 2
    res.update(amplitude_pass_ms=ms, amplitude_pass_bytes=nbytes, amplitude_pass_tb_s=nbytes / (ms * 1e-3) / 1e12, amplitude_pass_fraction_of_8tb_s=nbytes / (ms * 1e-3) / HBM_PEAK)
    fr.free()
    return res


if __name__ == "__main__":
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mp2_bench.jsonl"
    lib = _lib.init(0)
    rows = []
    for n, o, naux in SIZES:
        rows.append(one_size(lib, n, o, naux))
        print(json.dumps(rows[-1]), flush=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("".join(json.dumps(r) + "\n" for r in rows))
