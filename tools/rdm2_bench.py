"""Time the assembly of the fragment 2-RDM on the device (rdm2_ops.hip, qemb_op_rdm2_assemble) against the reference's literal NumPy expression on the host.

    python tools/rdm2_bench.py [out.jsonl]        (default profiles/rdm2_bench.jsonl)

Then the full basis: BE.compute_energy_full on octane / STO-3G BE2 and BE3 against the reference's literal einsum expressions (tests/rdm2_numpy.py), and the three
memory-bound passes of csrc/rdm2_ops.hip (add_nc, symmetrize, eri_dot) on a synthetic N = 96 tensor as HBM passes.

Sizes: n = 42 / n_occ = 21 and n = 55 / 27 (the fragments of octane / STO-3G BE2 and BE3), n = 84 / 21, and a synthetic n = 96 / 9.  Per size, kind (CCSD, MP2)
and with_dm1 one JSON line:
  * `max_abs_err`: device result against the host expression (oracle make_rdm2_urlx, tests/mp2_numpy.make_rdm2 statements), on amplitudes of O(1);
  * `host_ms`: the host expression, `device_ms`: the kernel alone (device timer, best of 20), `device_with_download_ms`: plus the n^4 download;
  * the kernel as an HBM pass: 8 n^4 bytes written (the amplitudes, 8 o^2 v^2 read, are counted too) against 8 TB/s, next to the figures the tracked per-kernel
    roofline (profiles/r05_kernel_roofline.jsonl) holds for the write-heavy passes of the CCSD iteration (`comparable_passes`)."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))
import mp2_numpy as mpn                                                   # noqa: E402
from qemb_oracle import rdm                                               # noqa: E402
from quemb_amd import _lib                                                # noqa: E402
from quemb_amd._lib import DeviceBuffer, check                            # noqa: E402
from quemb_amd.fragsolver import RDM2_KINDS                               # noqa: E402

HBM_PEAK = 8.0e12
SIZES = [(42, 21), (55, 27), (84, 21), (96, 9)]
COMPARABLE = ("unpack_tril_tiled_kernel", "ladder_pack_vvvv_pf_kernel", "ccsd_ph_layouts_kernel", "ccsd_finish_t2_rings_kernel")
SLOT = 9


def comparable_passes():
    out = {}
    f = ROOT / "profiles" / "r05_kernel_roofline.jsonl"
    for ln in f.read_text().splitlines():
        if ln.strip().startswith("{"):
            d = json.loads(ln)
            if d.get("kernel") in COMPARABLE and "frac_of_8_TBps" in d:
                out[d["kernel"]] = dict(algorithmic_GB=d["algorithmic_GB"], frac_of_8_TBps=d["frac_of_8_TBps"])
    return out


def timer(lib):
    ms = C.c_double(); cnt = C.c_int64()
    lib.qemb_timer_read(SLOT, C.byref(ms), C.byref(cnt))
    return ms.value


def host_expression(kind, t1, t2, dm1):
    if kind == "CCSD":
        if dm1 is None:
            return rdm.make_rdm2_urlx(t1, t2, with_dm1=False)
        return rdm.add_dm1_terms(rdm.make_rdm2_urlx(t1, t2, with_dm1=False), dm1, t1.shape[0])
    dm2 = mpn.dovov_part(t2)
    return dm2 if dm1 is None else rdm.add_dm1_terms(dm2, dm1, t2.shape[0])      # (dm1 symmetric: PySCF's transposed statements are the same)


def one_case(lib, n, o, kind, with_dm1, comp, reps=20):
    v = n - o
    rng = np.random.default_rng(n)
    t1, t2 = rng.standard_normal((o, v)), rng.standard_normal((o, o, v, v))
    dm1 = None
    if with_dm1:
        A = rng.standard_normal((n, n)); dm1 = 0.1 * (A + A.T); dm1[np.diag_indices(o)] += 2.0
    t0 = time.perf_counter()
    ref = host_expression(kind, t1, t2, dm1)
    host_ms = 1e3 * (time.perf_counter() - t0)
    d_t1, d_t2, d_out = DeviceBuffer.from_numpy(t1), DeviceBuffer.from_numpy(t2), DeviceBuffer(n ** 4)
    d_d = None
    if with_dm1:
        d = dm1.copy(); d[np.diag_indices(o)] -= 2.0
        d_d = DeviceBuffer.from_numpy(d)
    call = lambda: check(lib.qemb_op_rdm2_assemble(RDM2_KINDS[kind], o, v, d_t1.ptr if kind == "CCSD" else None, d_t2.ptr, d_d.ptr if d_d else None, d_out.ptr))
    for _ in range(3):
        call()
    best = None
    for _ in range(reps):
        lib.qemb_timer_reset(SLOT); lib.qemb_timer_begin(SLOT)
        call()
        lib.qemb_timer_end(SLOT)
        ms = timer(lib)
        best = ms if best is None else min(best, ms)
    lib.qemb_sync(); t0 = time.perf_counter()
    call(); got = d_out.numpy((n, n, n, n))
    with_download_ms = 1e3 * (time.perf_counter() - t0)
    err = float(np.abs(got - ref).max())
    nbytes = 8.0 * (n ** 4 + (o * v) ** 2 + (o * v if kind == "CCSD" else 0) + (n * n if with_dm1 else 0))
    for b in (d_t1, d_t2, d_out, d_d):
        if b is not None:
            b.free()
    return dict(n=n, o=o, kind=kind, with_dm1=with_dm1, max_abs_err=err, equals_host_expression=bool(err < 1e-12 * max(1.0, float(np.abs(ref).max()))),
                host_ms=host_ms, device_ms=best, device_with_download_ms=with_download_ms, host_over_device=host_ms / best,
                algorithmic_bytes=nbytes, TBps=nbytes / (best * 1e-3) / 1e12, frac_of_8_TBps=nbytes / (best * 1e-3) / HBM_PEAK, comparable_passes=comp)


def timed(lib, call, reps=10):
    for _ in range(2):
        call()
    best = None
    for _ in range(reps):
        lib.qemb_timer_reset(SLOT); lib.qemb_timer_begin(SLOT)
        call()
        lib.qemb_timer_end(SLOT)
        ms = timer(lib)
        best = ms if best is None else min(best, ms)
    return best


def full_basis_kernels(lib, N, comp):
    """the three memory-bound passes of the full basis on a synthetic [N]^4 tensor: result against NumPy, device time, bytes against 8 TB/s"""
    import rdm2_numpy as r2n
    from quemb_amd import rdm_full
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N,) * 4); g = rng.standard_normal((N, N)); e1 = rng.standard_normal((N,) * 4)
    Xd, gd = DeviceBuffer.from_numpy(X), DeviceBuffer.from_numpy(g)
    rows = []
    def row(kernel, err, ms, nbytes):
        rows.append(dict(case=f"synthetic N={N}", kernel=kernel, max_abs_err=err, equals_host_expression=bool(err < 1e-9), device_ms=ms, algorithmic_bytes=nbytes,
                         TBps=nbytes / (ms * 1e-3) / 1e12, frac_of_8_TBps=nbytes / (ms * 1e-3) / HBM_PEAK, comparable_passes=comp))
    check(lib.qemb_op_rdm2_add_nc(N, gd.ptr, -1.0, Xd.ptr))
    err = float(np.abs(Xd.numpy((N,) * 4) - (X - r2n.non_connected(g))).max())
    row("rdm2_add_nc_kernel", err, timed(lib, lambda: check(lib.qemb_op_rdm2_add_nc(N, gd.ptr, -1.0, Xd.ptr))), 16.0 * N ** 4)
    Xd.upload(X)
    check(lib.qemb_op_rdm2_symmetrize(N, gd.ptr, Xd.ptr))
    err = float(np.abs(Xd.numpy((N,) * 4) - ((X + X.T) / 2 + r2n.non_connected(g))).max())
    row("rdm2_symmetrize_kernel", err, timed(lib, lambda: check(lib.qemb_op_rdm2_symmetrize(N, None, Xd.ptr))), 16.0 * N ** 4)
    Xd.upload(X)
    s4 = np.ascontiguousarray(rdm_pack_s4(e1))
    for form, name in ((e1, "s1"), (s4, "s4")):
        ao = rdm_full.AOIntegrals(lib, form, N)
        want = float(np.einsum("pqrs,pqrs", rdm_restore(form, N), X))
        err = abs(ao.dot(Xd) - want) / max(1.0, abs(want))
        row(f"rdm2_eri_dot_kernel[{name}]", err, timed(lib, lambda: ao.dot(Xd)), 8.0 * (N ** 4 + form.size))
        ao.free()
    Xd.free(); gd.free()
    return rows


def rdm_pack_s4(e1):
    from qemb_oracle import eri
    n = e1.shape[0]
    e = e1 + e1.transpose(1, 0, 2, 3); e = e + e.transpose(0, 1, 3, 2); e = e + e.transpose(2, 3, 0, 1)      # any tensor -> one with the 8-fold symmetry
    return eri.pack_s4(e / 8.0)


def rdm_restore(form, n):
    from qemb_oracle import eri
    return form if form.ndim == 4 else eri.restore_s1(form, n)


def full_basis_system(key):
    """octane / STO-3G: BE.compute_energy_full (device) against the reference's literal einsum expressions on the host (tests/rdm2_numpy.py)"""
    import rdm2_numpy as r2n
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    golden = ROOT / "tests" / "golden"
    mf = RHF(Mole(golden / "octane.xyz")); mf.kernel()
    be = BE(mf, FragPart.from_json(golden / "fragmentation.json", key, n_BE=int(key[-1])), distribute=False)
    be.oneshot(solver="CCSD")
    frags = r2n.frags_of(be)
    t0 = time.perf_counter(); ref = r2n.energy_of(be, use_full_rdm=True); host_s = time.perf_counter() - t0
    be.compute_energy_full(use_full_rdm=True)
    t0 = time.perf_counter(); g, G = be.compute_energy_full(use_full_rdm=True); dev_s = time.perf_counter() - t0
    errs = {k: abs(be.e_full[k] - ref[k]) for k in ("EKapprox", "EKtrue", "E2")}
    err2 = float(np.abs(G - ref["RDM2_full"]).max())
    return dict(case=key, N=int(be.C.shape[0]), n_frag=len(frags), n_max=max(f["TA"].shape[1] for f in frags), energy_abs_err=errs, rdm2_max_abs_err=err2,
                equals_host_expression=bool(err2 < 1e-8 and max(errs.values()) < 1e-8), host_einsum_s=host_s, device_path_s=dev_s, host_over_device=host_s / dev_s,
                note="host_einsum_s includes assembling the fragment tensors for the restatement; device_path_s includes the two N^4 downloads")


if __name__ == "__main__":
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "rdm2_bench.jsonl"
    lib = _lib.init(0)
    comp = comparable_passes()
    rows = []
    for n, o in SIZES:
        for kind in ("CCSD", "MP2"):
            for with_dm1 in (False, True):
                rows.append(one_case(lib, n, o, kind, with_dm1, comp))
                print(json.dumps({k: v for k, v in rows[-1].items() if k != "comparable_passes"}), flush=True)
    for key in ("test_autogen_octane_be2", "test_autogen_octane_be3"):
        rows.append(full_basis_system(key))
        print(json.dumps(rows[-1]), flush=True)
    for r in full_basis_kernels(lib, 96, comp):
        rows.append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "comparable_passes"}), flush=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("".join(json.dumps(r) + "\n" for r in rows))
