#!/usr/bin/env python
"""bench.py -- fragment-sweep throughput of the MI355X hot path.

    python bench.py --gpus N --steps K --warmup W
N > 1 without WORLD_SIZE in the environment: this process only LAUNCHES -- it starts N fresh rank processes (RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT set, one per GPU) before touching the GPU itself, forwards rank 0's JSON line and fails if any rank fails; the
reference starts its own worker pool the same way (molbe/be_parallel.py:484-513).  Under an external launcher
(python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...) the ranks are already there and --gpus must equal
WORLD_SIZE.  The ranks talk through the library's own RCCL communicator (qemb_comm_*, quemb_amd/comm.py); QEMB_DIST_BACKEND=nccl|gloo selects a
torch.distributed process group instead (gloo: rehearsal of several ranks on one card / on the CPU mock).

Workload (BASELINE.json configs[2], the one the metric's n_occ/n_virt and the 1/2/4/8-GPU scaling are quoted on;
configs[1] -- octane BE2 -- is a parity case in tests/): F synthetic fragments PER GPU (weak scaling), each
n = 220 embedding orbitals, n_occ = 20, n_virt = 200, DF-factorised 8-fold-symmetric ERIs (SURVEY.md 8d family,
seed 20260803 + global fragment index; ERI scale 0.03 instead of 0.06), ERIs resident in HBM before timing.

One STEP = one objective evaluation of the density-matching loop through the PRODUCT sweep -- quemb_amd.solver.be_func
(1 GPU) / quemb_amd.be_parallel.be_func_parallel (N GPUs), the mirrors of molbe/solver.py:244 and
molbe/be_parallel.py:413 -- over `Frags` objects that are matched in a ring (edge AOs of fragment I against centre AOs
of fragment I+1), so the residual buffer that is all-reduced is the real ErrorMap one.  Per fragment: update_heff ->
fragment RHF -> embedding->MO integral transform -> RCCSD to convergence -> 1-RDM -> fragment energy; then ONE
all-reduce (RCCL) of [edge values, centre values, sum centre diag, e1, e2, ec, n_iter, failure flag].  Nothing is cached
between steps (amplitudes restart from MP2 exactly like the reference).
value = CCSD iterations completed by all ranks in the K timed steps / wall time (max over ranks).

A plain run sets up, warms up, times the K steps and prints the line.  Everything else the benchmark measures or checks -- the
single-stream roofline pass and the clock / MFMA probes, the four-index route, the oracle parity probes, the octane / H8 / DF / k-point
figures, the fragment-size sweep and the CPU baselines -- runs only under --full (its --no-* options still apply there).
--dump-outputs DIR writes what the last timed step returned on rank 0 (residual norm and vector, correlation energies, the 1-RDMs of
the rank's fragments) as DIR/<name>.npy in float64, so that two builds can be compared output for output.
"""
import os as _os
# BLAS / OpenMP pools inside the CPU share of this process, before NumPy starts them (quemb_amd/hostthreads.py: on a box that shows 256 cores
# to a 16-CPU container an unbounded OpenBLAS pool gets the whole process throttled for most of a 100 ms period now and then)
if not _os.environ.get("QEMB_KEEP_BLAS_THREADS"):
    try:
        _q, _p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        _n = len(_os.sched_getaffinity(0))
        if _q != "max":
            _n = min(_n, max(1, int(float(_q) / float(_p) + 0.5)))
    except Exception:  # noqa: BLE001
        _n = _os.cpu_count() or 1
    try:
        _lw = max(1, int(_os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))      # the ranks of one node share its CPU quota
    except ValueError:
        _lw = 1
    _cap, _auto = max(1, _n // (2 * _lw)), []
    for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        try:
            _have = int(_os.environ.get(_v, "0") or 0)
        except ValueError:
            _have = 0
        if _have <= 0 or _have > _cap:            # unset, or larger than this process's share (a value inherited from a process with a larger share): lower it
            _os.environ[_v] = str(_cap); _auto.append(_v)
    _os.environ["QEMB_BENCH_AUTO_THREAD_VARS"] = ",".join(_auto)      # launch_ranks drops these from the ranks' environment: each rank derives its own share
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
# the host driver of this pool only supports dmabuf IPC: RCCL needs this before the runtime starts (already exported on the boxes)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

PEAK_FP64_MFMA_TFLOPS = 78.6     # MI355X FP64 matrix peak (AMD spec; == the FP64 vector peak). The MI355X guide
                                 # lists no f64 row; see DESIGN.md "Roofline".
SEED0 = 20260803
N_EDGE = 6                       # matched AOs per fragment of the synthetic ring (edge [0..5] <-> centre [6..11] of the next one)
PMC_FILE = "profiles/r05_pmc_ladder.json"
MIN_GAP = 0.2                    # Eh: fragments of the synthetic family with a smaller fragment-RHF gap are redrawn (make_ring)
REDRAWN = []                     # ... and listed here

T_START = time.perf_counter()


def log(msg):
    """progress on stderr (the JSON line is the only thing on stdout)"""
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also run every figure beside the headline (roofline pass and probes, four-index route, parity probes, octane / H8 / DF / k-point "
                         "figures, size sweep, CPU baselines); a plain run only times the steps")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write what the last timed step computed (rank 0) as DIR/<name>.npy in float64")
    ap.add_argument("--frags-per-gpu", type=int, default=8)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (the driver's contract): --frags-per-gpu fragments on every GPU; strong: --frags-total fragments shared out over the GPUs")
    ap.add_argument("--frags-total", type=int, default=64, help="fragments of the whole job under --scaling strong (BASELINE configs[2]: 64)")
    ap.add_argument("--cu-split", type=int, default=2, help="execution contexts on this many interleaved sets of compute units (qemb_ctx_partition; 0: whole chip each)")
    ap.add_argument("--nstreams", type=int, default=4, help="fragments in flight per GPU (separate HIP streams, be_func(..., nstreams=k)); "
                    "under --full the roofline of the ladder kernel is measured in a separate single-stream pass after the timed region")
    ap.add_argument("--mo-route", choices=("factor", "four-index"), default="factor",
                    help="how a solve forms its MO integrals: from the fragment's 3-index DF factor (qemb_frag_set_df_factor; the synthetic family IS DF-factorised) "
                         "or by the four quarter transformations of the 4-fold packed block")
    ap.add_argument("--resident", choices=("factor", "block"), default="factor",
                    help="what each fragment keeps in HBM between sweeps: 'factor' = its 3-index DF factor alone (8 naux npair bytes; J / K, MO integrals and energies from it), "
                         "'block' = the 4-fold packed ERI block and the factor (rounds 1-4: 8 npair^2 bytes more)")
    ap.add_argument("--no-size-sweep", action="store_true", help="skip the fragment-size sweep (n = 42 ... 300) beside the headline")
    ap.add_argument("--n", type=int, default=220)
    ap.add_argument("--nocc", type=int, default=20)
    ap.add_argument("--scale", type=float, default=0.03)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-octane", action="store_true", help="skip the small-fragment figure (octane BE2 sweep) beside the headline")
    ap.add_argument("--cpu-iters", type=int, default=2, help="amplitude updates per worker timed by the CPU baseline")
    ap.add_argument("--cpu-ompnum", type=int, default=4, help="BLAS threads per CPU worker (the reference's `ompnum`)")
    ap.add_argument("--full-n", type=int, default=FULL_N, help="fragment size of the full-solve CPU baseline sample")
    ap.add_argument("--full-nocc", type=int, default=FULL_O)
    ap.add_argument("--cpu-worker", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-mode", type=str, default="updates", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-nproc", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--roofline-iters", type=int, default=8, help="single-stream CCSD iterations of the roofline pass")
    ap.add_argument("--master-port", type=int, default=0, help="rendezvous port handed to the ranks this process launches (0: a free one)")
    ap.add_argument("--lib", type=str, default=None, help=argparse.SUPPRESS)   # tests only: run the host logic on tests/hostcheck's mock library
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------ launcher
def launch_ranks(args):
    """--gpus N > 1 and no WORLD_SIZE: start N fresh rank processes of this script and wait for them.  Nothing in this process has
    touched the GPU (no torch, no library call), and it never execs: the ranks are children (subprocess), each with its own device.
    Rank 0's stdout (the JSON line) is forwarded; a failing rank ends the others and makes this process fail."""
    import shutil
    import socket
    import subprocess
    import tempfile
    n = args.gpus
    port = args.master_port
    if not port:
        sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    rdv_dir = tempfile.mkdtemp(prefix="qemb_rdv_")
    base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                QEMB_RDV_FILE=os.path.join(rdv_dir, "comm_id"), HSA_ENABLE_IPC_MODE_LEGACY="0")
    # thread-count variables THIS process derived for itself (whole-node share) must not reach the ranks, which share the node N ways: each rank derives its own
    # from LOCAL_WORLD_SIZE at import (the header of this file, and quemb_amd/hostthreads.py)
    for var in filter(None, base.pop("QEMB_BENCH_AUTO_THREAD_VARS", "").split(",")):
        base.pop(var, None)
    cmd = [sys.executable, str(Path(__file__).resolve())] + sys.argv[1:]
    procs = []
    try:
        for r in range(n):
            env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
            procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
        log(f"launched {n} ranks (pids {[p.pid for p in procs]}), rendezvous {base['QEMB_RDV_FILE']}")
        out0 = None
        failed = None
        pending = set(range(n))
        import threading
        box = {}
        t = threading.Thread(target=lambda: box.setdefault("out", procs[0].stdout.read()), daemon=True)
        t.start()
        while pending and failed is None:
            for r in sorted(pending):
                rc = procs[r].poll()
                if rc is None:
                    continue
                pending.discard(r)
                if rc != 0:
                    failed = (r, rc)
                    break
            time.sleep(0.05)
        if failed is not None:
            for r in pending:                     # the exact processes this launcher started, nothing else
                procs[r].terminate()
            for r in pending:
                try:
                    procs[r].wait(20)
                except subprocess.TimeoutExpired:
                    procs[r].kill()
            print(f"bench.py: rank {failed[0]} exited with status {failed[1]}; the other ranks were stopped", file=sys.stderr, flush=True)
            return 1
        t.join(10)
        out0 = box.get("out", "")
        sys.stdout.write(out0)
        sys.stdout.flush()
        if not any(ln.startswith("{") for ln in out0.splitlines()):
            print("bench.py: rank 0 printed no JSON line", file=sys.stderr, flush=True)
            return 1
        return 0
    finally:
        for p in procs:                           # interrupted launcher: do not leave ranks behind
            if p.poll() is None:
                p.terminate()
        shutil.rmtree(rdv_dir, ignore_errors=True)


# ------------------------------------------------------------------------------------------------------------ workload
def make_device_eris(lib, n, seed, scale, block=True):
    """h (host), the DF factor of the synthetic family on the device and -- unless block is False -- the 4-fold packed ERIs built from it ON THE DEVICE."""
    from quemb_amd._lib import DeviceBuffer, check
    rng = np.random.default_rng(seed)
    naux = 3 * n
    B = scale * rng.standard_normal((naux, n, n))
    B = 0.5 * (B + B.transpose(0, 2, 1))
    il = np.tril_indices(n)
    Bp = np.ascontiguousarray(B[:, il[0], il[1]])
    npair = Bp.shape[1]
    dB = DeviceBuffer.from_numpy(Bp, lib=lib)
    d4 = None
    if block:
        d4 = DeviceBuffer(npair * npair, lib=lib)
        check(lib.qemb_op_gemm(npair, npair, naux, 1.0, dB.ptr, npair, 0, 0, dB.ptr, npair, 0, 0, 0.0, d4.ptr, npair, 0, 1))
    A = rng.standard_normal((n, n))
    h = np.diag(2.0 * np.arange(n)) + 0.3 * 0.5 * (A + A.T)
    V = rng.standard_normal((n, n)); veff0 = 0.05 * (V + V.T)
    return h, veff0, d4, dB, naux


def make_ring(lib, n, o, nf, F_total, owner, rank, scale, opts, mo_route="factor", resident="factor"):
    """The fragment objects of the sweep: `quemb_amd.pfrag.Frags`, the mirror of molbe/pfrag.py:38.  Every rank holds the (light)
    host objects of all fragments -- be_func_parallel's contract -- and the device state (ERIs in HBM, Fock, dm0) of its own."""
    from quemb_amd.fragsolver import DeviceFragment
    from quemb_amd.pfrag import Frags
    edge, cen = list(range(N_EDGE)), list(range(N_EDGE, 2 * N_EDGE))
    frs = []
    for I in range(F_total):
        f = Frags(list(range(nf)), I, [edge], [(I + 1) % F_total], [edge], [cen], (1.0, cen), cen, lib=lib)
        f.nao, f.nsocc = n, o
        if owner[I] == rank:
            # A random draw of the family can come out with a nearly closed HOMO-LUMO gap of its fragment RHF (fragment 61 of the 64: 0.044 Eh at n = 220, where
            # the others have 0.3-1.6): RCCSD from the MP2 guess diverges on such a fragment for any solver.  The family therefore redraws a fragment whose gap
            # is below MIN_GAP with the seed moved by 1000 (deterministic, the same on every rank count); `redrawn` lists them in the bench line.
            for attempt in range(8):
                seed = SEED0 + I + 1000 * attempt
                h, veff0, d4, dB, naux = make_device_eris(lib, n, seed, scale, block=(resident == "block"))
                if f.dev is not None:
                    f.dev.free()
                f.dev = DeviceFragment(n, nf, lib=lib)
                if resident == "block":
                    f.dev.set_eri_s4_dev(d4.ptr); d4.free()
                    # the fragment keeps the 3-index factor its block was formed from, as one delivered by qemb_df_transform does (integral_direct_DF's bb)
                    f.dev.set_df_factor_dev(dB.ptr, naux); dB.free()
                else:
                    # the fragment lives on the factor alone, as one delivered by qemb_df_transform_factor does (round 5): no 4-fold packed block in HBM
                    f.dev.set_df_only_dev(dB.ptr, naux); dB.free()
                f.dev.set_mo_route(-1 if mo_route == "factor" else 0)
                r = f.dev.scf(o, h, None, opts=opts)        # BE.initialize does the same (Frags.scf(fs=True), mbe.py:1160)
                gap = float(r["mo_energy"][o] - r["mo_energy"][o - 1]) if o < n else MIN_GAP
                if gap >= MIN_GAP:
                    break
                REDRAWN.append(dict(fragment=I, seed=seed, gap=gap))
            f.seed = seed
            f.h1, f.veff0, f.veff, f.fock, f.heff = h, veff0, None, h, np.zeros((n, n))
            f._mo_coeffs = r["mo_coeff"]
            f.dm0 = 2.0 * r["mo_coeff"][:, :o] @ r["mo_coeff"][:, :o].T
        frs.append(f)
    c = 0
    for f in frs:
        f.udim = c
        c = f.set_udim(c)
    return frs, c + 1


DUMP_RDM_BYTES = 48 << 20        # --dump-outputs: the 1-RDMs of at most this many bytes (the first fragments of the rank, in ring order)


def dump_outputs(d, frs, mine, ernorm, ervec, ecorr, e_parts):
    """--dump-outputs: what the last timed step returned -- be_func's (ernorm, ervec, [Ecorr, total_e]) -- and the embedding-basis 1-RDMs it left
    on this rank's fragments (Frags._rdm1, what the density matching reads), as float64 .npy files"""
    os.makedirs(d, exist_ok=True)
    n2 = 8 * frs[mine[0]]._rdm1.size
    keep = mine[:max(1, DUMP_RDM_BYTES // n2)]
    outs = dict(residual_norm=[ernorm], residual_vec=ervec, e_corr=[ecorr], e_corr_parts=e_parts,
                rdm1_emb=np.stack([frs[i]._rdm1 for i in keep]), rdm1_fragments=keep)
    for name, a in outs.items():
        np.save(os.path.join(d, name + ".npy"), np.asarray(a, dtype=np.float64))
    return sorted(outs)


def read_timer(lib, slot, nctx=1, reset=0):
    """device timer `slot` summed over the execution contexts 0..nctx-1"""
    tot, n = 0.0, 0
    for k in range(nctx):
        ms = C.c_double(); cnt = C.c_int64()
        lib.qemb_ctx_timer_read(k, slot, C.byref(ms), C.byref(cnt), reset)
        tot += ms.value; n += cnt.value
    return tot, n


# ------------------------------------------------------------------------------------------------------------ CPU baseline
def usable_cores():
    """host cores this process may use: scheduler affinity, capped by the cgroup CPU quota when there is one"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(p) + 0.5)))
    except Exception:  # noqa: BLE001
        pass
    return n


FULL_N, FULL_O, FULL_NF = 132, 12, 22      # the fragment size of the FULL-SOLVE CPU baseline (a whole n = 220 solve takes minutes per CPU worker); --full-n / --full-nocc


def full_solve_fragment(i, scale):
    """inputs of one whole-fragment solve of the baseline sample: the synthetic family of the timed workload at n = 132, n_occ = 12
    (what the reference's pool worker receives, molbe/be_parallel.py:40-60)"""
    n = FULL_N
    rng = np.random.default_rng(SEED0 + 1000 + i)
    B = scale * (220.0 / n) ** 0.5 * rng.standard_normal((3 * n, n, n))      # same Coulomb strength per orbital as the n = 220 family
    B = 0.5 * (B + B.transpose(0, 2, 1))
    il = np.tril_indices(n)
    Bp = np.ascontiguousarray(B[:, il[0], il[1]])
    A = rng.standard_normal((n, n)); V = rng.standard_normal((n, n))
    return dict(h=np.diag(2.0 * np.arange(n)) + 0.15 * (A + A.T), veff0=0.05 * (V + V.T), s4=Bp.T @ Bp)


def cpu_pool_run(d, mode, nproc, ompnum, extra, timeout_s):
    """one timed run of the CPU pool in a child process (never touches the GPU); returns the child's JSON or an error string"""
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS=str(ompnum), OPENBLAS_NUM_THREADS=str(ompnum), MKL_NUM_THREADS=str(ompnum))
    try:
        p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--cpu-worker", d, "--cpu-mode", mode, "--cpu-nproc", str(nproc)] + extra,
                           env=env, capture_output=True, text=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return f"pool exceeded {timeout_s} s"
    if p.returncode != 0:
        return f"pool failed: {p.stderr[-400:]}"
    return json.loads(p.stdout.strip().splitlines()[-1])


def cpu_baseline(lib, fr, h, dm0, o, opts, iters, ompnum, scale, budget_s=150):
    """QuEmb's own CPU shape -- a pool of nproc worker processes with OMP_NUM_THREADS = ompnum each, one whole fragment per worker at a time
    (molbe/be_parallel.py:484-513; defaults nproc = 1, ompnum = 4, mbe.py:850-851) -- with the oracle ('port') as the per-fragment solver.

    (1) FULL SOLVES (cpu_baseline.value): every worker runs the reference worker's whole job on one fragment -- fragment RHF -> four-index
        transformation -> RCCSD with DIIS to |dE| < 1e-10 -> 1-RDM -> 2-RDM and fragment energies (oracle/qemb_oracle/worker.py =
        run_solver, be_parallel.py:40-307) -- at n = 132, n_occ = 12 (n = 220 takes minutes per worker: outside a default bench run), in two
        settings: the reference's defaults (1 worker x 4 threads) and every usable core (cores // 4 workers x 4 threads).  The GPU solves the
        SAME fragments through the product call (qemb_frag_solve) for the figure beside it, and the energies are compared.
    (2) AT THE BENCHMARKED SIZE: `iters` plain amplitude updates per worker on fragment 0 of the timed workload (n = 220), MO integrals
        exported from the device (the CPU number of rounds 1-2; also returns both energies for the full-size parity field)."""
    import shutil
    import tempfile
    from quemb_amd.fragsolver import DeviceFragment
    cores = usable_cores()
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    info = dict(unit="CCSD iterations/s", kind="port", os_cpu_count=os.cpu_count(), ompnum=ompnum, value=None, cores=None)
    # ---- (1) whole fragments
    nproc_all = max(1, cores // ompnum)
    d = tempfile.mkdtemp(prefix="qemb_bench_full_", dir=base)
    try:
        gpu = []
        cen = list(range(FULL_NF // 4, FULL_NF // 2))
        t_gpu = 0.0
        for i in range(nproc_all):
            f = full_solve_fragment(i, scale)
            np.savez(os.path.join(d, f"frag{i}.npz"), o=FULL_O, nf=FULL_NF, cen=np.array(cen), **f)
            dfr = DeviceFragment(FULL_N, FULL_NF, lib=lib)
            dfr.set_eri_s4(f["s4"])
            dfr.set_energy_data(f["h"], f["veff0"], None, 1.0, cen)
            if i == 0:
                dfr.solve(FULL_O, f["h"], None, opts=opts, eeval=True)           # warm-up (allocations, hipGraph instantiation)
            lib.qemb_sync(); t0 = time.perf_counter()
            out = dfr.solve(FULL_O, f["h"], None, opts=opts, eeval=True)
            lib.qemb_sync(); t_gpu += time.perf_counter() - t0
            gpu.append((out["n_iter"], out["e_corr_mo"], list(out["e_frag"])))
            dfr.free()
        log(f"cpu_baseline: {nproc_all} whole fragments (n={FULL_N}, n_occ={FULL_O}) on the GPU in {t_gpu:.2f} s; CPU pools next")
        full = dict(n=FULL_N, n_occ=FULL_O, n_virt=FULL_N - FULL_O,
                    work="fragment RHF -> 4-index transformation -> RCCSD (DIIS, |dE|<1e-10) -> 1-RDM -> 2-RDM + fragment energies, one whole fragment per worker "
                         "(oracle/qemb_oracle/worker.py = run_solver, molbe/be_parallel.py:40-307)",
                    gpu_same_fragments=dict(iterations_per_s=sum(g[0] for g in gpu) / t_gpu, fragments_per_s=len(gpu) / t_gpu, fragments=len(gpu),
                                            how="the same fragments through qemb_frag_solve (eeval), one at a time on one stream"))
        for key, nproc in (("reference_defaults_nproc1_ompnum4", 1), ("all_cores", nproc_all)):
            r = cpu_pool_run(d, "full", nproc, ompnum, [], budget_s)
            if isinstance(r, str):
                full[key] = dict(value=None, note=r, nproc=nproc, ompnum=ompnum)
                continue
            err = max(abs(e - gpu[i][1]) for i, e in enumerate(r["e_corr"]))
            erf = max(abs(a - b) for i, ef in enumerate(r["e_frag"]) for a, b in zip(ef, gpu[i][2]))
            full[key] = dict(iterations_per_s=r["iterations"] / r["pool_wall_s"], fragments_per_s=nproc / r["pool_wall_s"], nproc=nproc, ompnum=ompnum,
                             threads=nproc * ompnum, pool_wall_s=r["pool_wall_s"], iterations=r["iterations"], slowest_worker_s=r["slowest_worker_s"],
                             max_abs_e_corr_diff_vs_gpu_Eh=err, max_abs_e_frag_diff_vs_gpu_Eh=erf)
        info["full_solve"] = full
        best = full.get("all_cores", {})
        if best.get("iterations_per_s"):
            # the value is measured at n = FULL_N, not at the n = 220 of the headline (one iteration costs ~21x more there): the size is in the
            # unit, and the like-for-like ratio -- this GPU over all CPU cores on the SAME whole fragments -- is spelled out (advisor, round 3)
            info["unit"] = f"CCSD iterations/s at n={FULL_N} n_occ={FULL_O} (whole fragment solves; NOT comparable with the n=220 headline value)"
            info["like_for_like"] = dict(gpu_over_all_cores=full["gpu_same_fragments"]["iterations_per_s"] / best["iterations_per_s"],
                                         what=f"qemb_frag_solve on one stream / the all-cores CPU pool, both on the same {best['nproc']} whole fragments at n={FULL_N}")
            info.update(value=best["iterations_per_s"], cores=best["threads"], fragments_per_s=best["fragments_per_s"],
                        sample=f"{best['nproc']} whole synthetic fragments of the timed family at n={FULL_N}, n_occ={FULL_O} (a whole n=220 solve takes minutes per CPU "
                               f"worker), one per worker process, {ompnum} BLAS threads each: fragment RHF + 4-index transformation + RCCSD with DIIS to |dE|<1e-10 + "
                               "RDMs + fragment energies (oracle/qemb_oracle/worker.py); value = all CCSD iterations / pool wall time. "
                               "full_solve.reference_defaults_nproc1_ompnum4 = the reference's default pool; full_solve.gpu_same_fragments = this GPU on the same fragments; "
                               "n220_amplitude_updates = the CPU at the benchmarked size")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    # ---- (2) the benchmarked size: plain amplitude updates on the device-exported MO integrals of fragment 0
    n = fr.n
    v = n - o
    fr.prepare_ccsd(o, h, dm0, opts=opts)
    e_dev, _ = fr.ccsd_iterate(iters)          # plain Jacobi updates from the MP2 guess (no DIIS outside CcsdSolver::kernel)
    shapes = dict(oooo=(o, o, o, o), ovoo=(o, v, o, o), ovov=(o, v, o, v), ovvv=(o, v, v, v), Vl=(v, v, v, v),
                  W1base=(o, v, o, v), W2base=(o, v, o, v), eo=(o,), ev=(v,))
    d = tempfile.mkdtemp(prefix="qemb_bench_", dir=base)
    e_cpu = None
    try:
        for name, shp in shapes.items():
            np.save(os.path.join(d, name + ".npy"), fr.ccsd_export(name, shp))
        log(f"cpu_baseline: n={n} integrals exported to {d}; pool of {nproc_all} worker(s) x {ompnum} thread(s), {iters} amplitude update(s) each")
        r = cpu_pool_run(d, "updates", nproc_all, ompnum, ["--cpu-iters", str(iters), "--nocc", str(o)], budget_s)
        if isinstance(r, str):
            info["n220_amplitude_updates"] = dict(value=None, note=r)
        else:
            e_cpu = r["e_corr"]
            info["n220_amplitude_updates"] = dict(
                value=r["iterations_per_s"], unit="plain RCCSD amplitude updates/s", nproc=nproc_all, ompnum=ompnum, threads=nproc_all * ompnum,
                s_per_iteration_per_worker=r["s_per_iteration_per_worker"], pool_wall_s=r["pool_wall_s"], e_corr_after_sample=e_cpu,
                sample=f"fragment 0 of the timed workload (n_occ={o}, n_virt={v}), MO integrals exported from the device and shared; {nproc_all} worker processes x "
                       f"{iters} full RCCSD amplitude updates each from the MP2 guess (oracle/qemb_oracle/ccsd_lean.py, no RHF / transformation / DIIS / RDMs)")
            if info["value"] is None:      # the full-solve pools did not finish: fall back to the same-size figure, labelled as such
                info.update(value=r["iterations_per_s"], cores=nproc_all * ompnum, sample=info["n220_amplitude_updates"]["sample"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return info, e_dev, e_cpu


def _cpu_full_task(args):
    """one worker of the full-solve pool: the reference worker's whole job on one fragment"""
    d, i = args
    sys.path.insert(0, str(ROOT / "oracle"))
    from qemb_oracle import worker
    z = np.load(os.path.join(d, f"frag{i}.npz"))
    t0 = time.perf_counter()
    out = worker.run_solver(z["h"], None, z["s4"], int(z["o"]), int(z["nf"]), (1.0, [int(c) for c in z["cen"]]), z["h"], z["veff0"], eeval=True)
    return time.perf_counter() - t0, int(out["n_iter"]), float(out["e_corr"]), [float(x) for x in out["e_f"]], bool(out["converged"])


def _cpu_pool_task(args):
    """one worker of the CPU pool: `iters` amplitude updates of the exported fragment (blocks memory-mapped from /dev/shm)"""
    d, o, iters = args
    sys.path.insert(0, str(ROOT / "oracle"))
    from qemb_oracle import ccsd_lean
    ld = lambda nm: np.load(os.path.join(d, nm + ".npy"), mmap_mode="r")
    eo, ev = np.array(ld("eo")), np.array(ld("ev"))
    W1, W2 = ld("W1base"), ld("W2base")
    ovvo = np.ascontiguousarray(W1.transpose(2, 3, 1, 0))     # ovvo[k,c,a,i] = W1base[i,a,k,c]
    oovv = np.ascontiguousarray(W2.transpose(2, 0, 1, 3))     # oovv[k,i,a,c] = W2base[i,a,k,c]
    er = ccsd_lean.LeanEris.from_blocks(o, np.concatenate([eo, ev]), np.array(ld("oooo")), np.array(ld("ovoo")), np.array(ld("ovov")),
                                        oovv, ovvo, ld("ovvv"), ld("Vl"))
    t1, t2 = ccsd_lean.init_amps(er)
    t0 = time.perf_counter()
    for _ in range(iters):
        t1, t2 = ccsd_lean.update_amps(t1, t2, er)
    dt = time.perf_counter() - t0
    return dt, ccsd_lean.energy(t1, t2, er)


def cpu_worker(d, mode, o, iters, nproc):
    """child process of cpu_baseline (never touches the GPU): runs the worker pool and prints one JSON line"""
    import multiprocessing as mp
    if mode == "octane":          # `iters` carries the number of fragments: more tasks than workers, one fragment per task
        task, jobs = _cpu_octane_task, [(d, i) for i in range(iters)]
    else:
        task, jobs = (_cpu_full_task, [(d, i) for i in range(nproc)]) if mode == "full" else (_cpu_pool_task, [(d, o, iters)] * nproc)
    t0 = time.perf_counter()
    if nproc <= 1:
        res = [task(j) for j in jobs]
    else:
        with mp.get_context("spawn").Pool(nproc) as pool:
            res = pool.map(task, jobs, chunksize=1)
    wall = time.perf_counter() - t0
    slowest = max(r[0] for r in res)
    if mode in ("full", "octane"):
        assert all(r[4] for r in res), "a CPU fragment solve did not converge"
        print(json.dumps(dict(pool_wall_s=wall, slowest_worker_s=slowest, iterations=sum(r[1] for r in res), e_corr=[r[2] for r in res],
                              e_frag=[r[3] for r in res])), flush=True)
    else:
        print(json.dumps(dict(iterations_per_s=len(res) * iters / slowest, s_per_iteration_per_worker=slowest / iters, pool_wall_s=wall,
                              e_corr=res[0][1])), flush=True)


# ------------------------------------------------------------------------------------------------------------ probes
def parity_probe():
    """corr-E error vs the oracle on a small fragment of the same family (the full solve: SCF + CCSD to convergence)."""
    sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tests"))
    from helpers import synthetic_fragment
    from qemb_oracle import ccsd, eri, scf
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    n, o = 26, 6
    h, e1 = synthetic_fragment(n, o, SEED0)
    fr = DeviceFragment(n, 6); fr.set_eri_s4(eri.pack_s4(e1))
    out = fr.solve(o, h, opts=default_opts(), eeval=False)
    mf = scf.rhf(h, e1, o)
    _, _, ecc, _ = ccsd.solve_ccsd(h, e1, o, mf["mo_coeff"], mf["mo_energy"])
    fr.free()
    return abs(out["e_corr_mo"] - ecc)


def clock_probe(lib):
    """Sustained shader clock under the pp-ladder kernel: one launch of the ladder tile (224 x 128, one 8-wave workgroup per CU) on
    random operands with every workgroup recording its s_memtime ticks; sum(ticks) / (256 CUs x kernel time).  Outside the timed region."""
    from quemb_amd._lib import DeviceBuffer, check
    M, N, K = 210, 4096, 16384
    rng = np.random.default_rng(7)
    dA, dB, dC = DeviceBuffer.from_numpy(rng.standard_normal((M, K))), DeviceBuffer.from_numpy(rng.standard_normal((N, K))), DeviceBuffer(M * N)
    vals = []
    for _ in range(4):
        ms, ghz, wg = C.c_double(), C.c_double(), C.c_int64()
        check(lib.qemb_op_gemm_probe(M, N, K, dA.ptr, K, 1, dB.ptr, K, 1, dC.ptr, N, 13, 8, C.byref(ms), C.byref(ghz), C.byref(wg)), "qemb_op_gemm_probe", lib)
        vals.append((ghz.value, ms.value, wg.value))
    for b in (dA, dB, dC):
        b.free()
    ghz, ms, wg = sorted(vals[1:])[1]
    return dict(ghz=ghz, ms=ms, workgroups=wg, tflops=2.0 * M * N * K / (ms * 1e9))


def mfma_peak_probe(lib):
    """register-only v_mfma_f64_16x16x4_f64 loop, 16 independent accumulator chains per wave, 2 waves per SIMD (gemm_f64.hip)"""
    t = C.c_double()
    best = 0.0
    for _ in range(3):
        if lib.qemb_mfma_f64_peak(40000, 2, C.byref(t)) == 0:
            best = max(best, t.value)
    return best


def roofline_pass(lib, fr, h, dm0, o, opts, iters):
    """The dominant kernel on its own: one fragment, ONE stream, `iters` CCSD iterations with the ladder bracketed by HIP events on the
    stream it is launched on (QEMB_TIMER_LADDER).  Separate from the timed region, where several fragments share the device."""
    for s in (0, 1, 2):
        lib.qemb_ctx_timer_read(0, s, None, None, 1)
    fr.prepare_ccsd(o, h, dm0, opts=opts)
    fr.ccsd_iterate(2)
    for s in (0, 1, 2):
        lib.qemb_ctx_timer_read(0, s, None, None, 1)
    fr.ccsd_iterate(iters)
    lad = read_timer(lib, 0, 1); ring = read_timer(lib, 1, 1); it = read_timer(lib, 2, 1)
    return dict(ladder_ms=lad[0] / max(lad[1], 1), ladder_count=lad[1], rings_ms=ring[0] / max(ring[1], 1), iter_ms=it[0] / max(it[1], 1))


def _stats_ms(ts):
    """p50 / p95 / max / mean / min of a series of sweep times (ms) and the series itself"""
    xs = sorted(ts)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]
    return dict(p50_ms=q(0.5), p95_ms=q(0.95), max_ms=xs[-1], min_ms=xs[0], mean_ms=sum(xs) / len(xs), sweeps=len(xs), series_ms=[round(t, 2) for t in ts])


def timed_sweeps(lib, fn, reps):
    """`reps` sweeps, each bracketed by a device sync; Python's cyclic garbage collector is held off during the series (a generation-2
    collection in the middle of a 15 ms sweep is a host pause of tens of ms that has nothing to do with the device path) and run once before it"""
    import gc
    t_gc = time.perf_counter()
    gc.collect()
    timed_sweeps.last_full_gc_ms = (time.perf_counter() - t_gc) * 1e3      # what a generation-2 collection costs in THIS process, reported beside the series
    was = gc.isenabled()
    gc.disable()
    ts = []
    try:
        for _ in range(reps):
            lib.qemb_device_sync(); t0 = time.perf_counter()
            out = fn()
            lib.qemb_device_sync()
            ts.append((time.perf_counter() - t0) * 1e3)
    finally:
        if was:
            gc.enable()
    return ts, out


def _cpu_octane_task(args):
    """one worker of the octane CPU pool: the reference worker's whole job on one fragment of the octane BE2 sweep"""
    d, i = args
    sys.path.insert(0, str(ROOT / "oracle"))
    from qemb_oracle import worker
    z = np.load(os.path.join(d, f"oct{i}.npz"))
    t0 = time.perf_counter()
    out = worker.run_solver(z["h"], z["dm0"], z["s4"], int(z["o"]), int(z["nf"]), (float(z["w"]), [int(c) for c in z["cen"]]), z["h1"], z["veff0"], eeval=True)
    return time.perf_counter() - t0, int(out["n_iter"]), float(out["e_corr"]), [float(x) for x in out["e_f"]], bool(out["converged"])


def octane_cpu_baseline(be, e_gpu, ompnum=4, budget_s=120):
    """cpu_baseline for the small-fragment regime: the SAME six octane BE2 fragments (h = fock + heff, dm0, 4-fold packed ERIs read back from
    the device, centre weights) through the oracle's worker (oracle/qemb_oracle/worker.py = run_solver, be_parallel.py:40-307) in the
    reference's pool shape -- `cores // ompnum` worker processes with `ompnum` BLAS threads each, one fragment per task -- one sweep timed."""
    import shutil
    import tempfile
    cores = usable_cores()
    nproc = max(1, min(len(be.Fobjs), cores // ompnum))
    d = tempfile.mkdtemp(prefix="qemb_bench_oct_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        for i, f in enumerate(be.Fobjs):
            w, cen = f.weight_and_relAO_per_center
            np.savez(os.path.join(d, f"oct{i}.npz"), h=f.fock + f.heff, dm0=f.dm0, s4=f.dev.get_eri_s4(), o=f.nsocc, nf=f.n_frag, w=w, cen=np.array(cen),
                     h1=f.h1, veff0=f.veff0)
        r = cpu_pool_run(d, "octane", nproc, ompnum, ["--cpu-iters", str(len(be.Fobjs))], budget_s)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if isinstance(r, str):
        return dict(value=None, note=r, nproc=nproc, ompnum=ompnum)
    e_cpu = sum(sum(ef) for ef in r["e_frag"])
    return dict(sweep_ms=r["pool_wall_s"] * 1e3, unit="ms per octane BE2 sweep", kind="port", nproc=nproc, ompnum=ompnum, cores=nproc * ompnum,
                iterations=r["iterations"], slowest_fragment_s=r["slowest_worker_s"], e_corr=e_cpu, abs_e_corr_diff_vs_gpu_Eh=abs(e_cpu - e_gpu),
                sample="one sweep: the six fragments of the GPU sweep (same h, dm0, ERIs read back from the device), whole fragment solves by "
                       "oracle/qemb_oracle/worker.py, one fragment per pool task")


def octane_sweeps(lib, reps=24, cpu=True):
    """BASELINE configs[1] beside the headline: one octane/STO-3G BE2 sweep (six fragments of ~40 embedding orbitals; integrals, RHF and
    fragmentation from the in-tree source, tests/golden/) through the product -- fragment by fragment, six fragments in flight on separate
    streams, and all fragments in ONE lock-step batched call (qemb_frag_solve_batch: one grouped launch per operation of the CCSD update
    for all fragments).  The three sweeps return bit-identical energies.  Per mode: p50 / p95 / max over `reps` sweeps."""
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    G = ROOT / "tests" / "golden"
    mf = RHF(Mole(G / "octane.xyz")); mf.kernel()
    out = {}
    energies = []
    be = None
    for label, kw, n in (("serial", dict(nstreams=1), max(5, reps // 4)), ("streams6", dict(nstreams=6), reps), ("lockstep", dict(lockstep=True), reps)):
        be = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_octane_be2"), distribute=False, lib=lib, **kw)
        be.oneshot(); be.oneshot(); be.oneshot()      # (the first two sweeps of a new BE object carry one-off costs: see `outliers` below)
        be.stats.clear()
        ts, (e, _) = timed_sweeps(lib, be.oneshot, n)
        st = _stats_ms(ts)
        st["full_gc_before_series_ms"] = timed_sweeps.last_full_gc_ms
        st["ccsd_iterations_per_sweep"] = int(be.stats.get("ccsd_iterations", 0)) // max(len(ts), 1)
        out[label] = st
        out[label + "_ms"] = st["p50_ms"]
        energies.append(e)
        if label == "lockstep":
            out["lockstep_launch_stats"] = {k: int(v) for k, v in be.stats.items() if k in ("merged_runs", "launches", "grouped_launches", "operations", "max_group")}
    out["outliers"] = ("round 3 reported one 92 ms sweep among five (median 16).  Found in round 4 (tools/octane_idle_probe.py, profiles/r04_octane_idle_probe.log): "
                       "CPU-bandwidth throttling of the container.  The box shows 256 cores to a cgroup limited to 16 CPUs (cpu.max 1600000 / 100000); OpenBLAS starts a worker "
                       "per visible core and the workers spin after every NumPy call, so host work between sweeps (building a BE object, 0.3 s of NumPy) burns the quota of a "
                       "100 ms period in a few ms and the kernel freezes the whole process -- the threads that feed the GPU included -- until the period ends: the next sweep "
                       "or the one after takes 85-100 ms (nr_throttled in /sys/fs/cgroup/cpu.stat).  Not the GC (no collection inside a timed sweep), not the allocator "
                       "(0 driver allocations or frees in the slow sweeps, qemb_alloc_stats), not stream capture.  quemb_amd now caps the BLAS pool at half the usable cores "
                       "at import (quemb_amd/hostthreads.py; QEMB_KEEP_BLAS_THREADS=1 brings the stalls back) and bench.py sets the same before NumPy loads")
    out["e_corr"] = energies[0]
    out["bit_identical"] = bool(energies[0] == energies[1] == energies[2])
    # The sweeps above converge every fragment's CCSD to the product's defaults, |dE| < 1e-10 and |dt| < 1e-8 (what the 1e-8 Eh parity bar needs).
    # The reference runs PySCF's defaults, |dE| < 1e-7 and |dt| < 1e-5 (molbe/solver.py: cc.CCSD(...).kernel()): the same sweep at THOSE thresholds,
    # reported beside -- fewer iterations per fragment, same kernels.
    try:
        from quemb_amd.fragsolver import default_opts
        o_ref = default_opts(lib, cc_conv_tol=1e-7, cc_conv_tol_normt=1e-5)
        br = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_octane_be2"), distribute=False, lib=lib, lockstep=True, solver_opts=o_ref)
        br.oneshot(); br.oneshot(); br.oneshot()
        br.stats.clear()
        ts, (e_ref, _) = timed_sweeps(lib, br.oneshot, reps)
        st = _stats_ms(ts)
        st.update(cc_conv_tol=1e-7, cc_conv_tol_normt=1e-5, e_corr=float(e_ref), abs_e_corr_diff_vs_tight_Eh=abs(float(e_ref) - float(energies[2])),
                  ccsd_iterations_per_sweep=int(br.stats.get("ccsd_iterations", 0)) // max(len(ts), 1),
                  what="lock-step sweep with the CCSD thresholds of the reference (PySCF defaults) instead of the product's tighter defaults")
        out["lockstep_reference_thresholds"] = st
    except Exception as e:  # noqa: BLE001
        out["lockstep_reference_thresholds"] = dict(p50_ms=None, note=f"failed: {e}")
    out["fragments"] = 6
    out["what"] = "octane/STO-3G BE2 one-shot sweep (example/molbe_octane.py): fragment RHF + MO transformation + RCCSD + RDMs + energies for every fragment"
    # the reference's headline example end to end (example/molbe_octane.py: mybe.optimize(solver="CCSD")): density matching to convergence from a
    # fresh BE object -- HF Jacobian (CPHF on the device), quasi-Newton sweeps -- against the reference's own golden energy
    try:
        bo = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_octane_be2"), distribute=False, lib=lib)
        bo.stats.clear()
        lib.qemb_device_sync(); t0 = time.perf_counter()
        bo.optimize(solver="CCSD")
        lib.qemb_device_sync(); t_opt = time.perf_counter() - t0
        golden = -0.5499514850769742           # /root/reference/tests/molbe_octane_test.py:32-36 (PySCF conv_tol 1e-7)
        out["density_matching"] = dict(seconds=t_opt, e_corr=float(bo.e_corr), abs_diff_vs_reference_golden_Eh=abs(float(bo.e_corr) - golden),
                                       sweeps=int(bo.stats.get("fragments", 0)) // 6, ccsd_iterations=int(bo.stats.get("ccsd_iterations", 0)),
                                       what="BE2 density matching of octane/STO-3G to the reference's default conv_tol 1e-6, warm-started amplitudes between sweeps; "
                                            "golden -0.5499514850769742 (reference tolerance rtol 1e-5)")
    except Exception as e:  # noqa: BLE001
        out["density_matching"] = dict(seconds=None, note=f"failed: {e}")
    try:        # the reference's "expensive" test beside it: BE3 density matching of the same molecule (tests/molbe_octane_test.py:63-68)
        b3 = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_octane_be3"), distribute=False, lib=lib)
        lib.qemb_device_sync(); t0 = time.perf_counter()
        b3.optimize(solver="CCSD")
        lib.qemb_device_sync(); t_opt = time.perf_counter() - t0
        out["be3_density_matching"] = dict(seconds=t_opt, e_corr=float(b3.e_corr), abs_diff_vs_reference_golden_Eh=abs(float(b3.e_corr) + 0.5497021857717073),
                                           fragments=len(b3.Fobjs), n_emb=[int(f.nao) for f in b3.Fobjs], sweeps=int(b3.stats.get("fragments", 0)) // max(len(b3.Fobjs), 1))
    except Exception as e:  # noqa: BLE001
        out["be3_density_matching"] = dict(seconds=None, note=f"failed: {e}")
    try:        # BE3 one-shot sweeps (four fragments of 54-57 orbitals) at the product's thresholds and at the reference's
        from quemb_amd.fragsolver import default_opts
        b3s = {}
        for label, so in (("product_thresholds", None), ("reference_thresholds", default_opts(lib, cc_conv_tol=1e-7, cc_conv_tol_normt=1e-5))):
            bb3 = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_octane_be3"), distribute=False, lib=lib, solver_opts=so)
            bb3.oneshot(); bb3.oneshot(); bb3.oneshot()
            bb3.stats.clear()
            ts, (e3, _) = timed_sweeps(lib, bb3.oneshot, 10)
            st = _stats_ms(ts)
            st.update(e_corr=float(e3), ccsd_iterations_per_sweep=int(bb3.stats.get("ccsd_iterations", 0)) // max(len(ts), 1), nstreams=int(bb3.nstreams), lockstep=bool(bb3.lockstep))
            b3s[label] = st
        out["be3_sweeps"] = b3s
    except Exception as e:  # noqa: BLE001
        out["be3_sweeps"] = dict(note=f"failed: {e}")
    if cpu:
        try:
            out["cpu_baseline"] = octane_cpu_baseline(be, energies[0])
        except Exception as e:  # noqa: BLE001
            out["cpu_baseline"] = dict(value=None, note=f"failed: {e}")
    return out


def h8_be2(lib):
    """BASELINE configs[0] in the line as well: linear H8 / STO-3G BE2 (the reference's plumbing case; six fragments of <= 6 orbitals): HF-in-HF, the
    one-shot CCSD energy against the reference's golden and the density matching, timed."""
    from quemb_amd.fragpart import FragPart
    from quemb_amd.integrals import RHF, Mole
    from quemb_amd.mbe import BE
    G = ROOT / "tests" / "golden"
    mf = RHF(Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])); mf.kernel()
    be = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_h_linear_be2"), distribute=False, lib=lib)
    e1, _ = be.oneshot(); be.oneshot()
    ts, (e1, _) = timed_sweeps(lib, be.oneshot, 10)
    lib.qemb_device_sync(); t0 = time.perf_counter()
    be.optimize(solver="CCSD")
    lib.qemb_device_sync(); t_opt = time.perf_counter() - t0
    golden = -0.13198886164212092              # /root/reference/tests/_expected_data_for_fragmentation_test.py:983 (PySCF conv_tol 1e-7)
    return dict(sweep_ms=_stats_ms(ts)["p50_ms"], hf_in_hf_error_Eh=float(be.hf_err), e_corr_oneshot=float(e1), abs_diff_vs_reference_golden_Eh=abs(float(e1) - golden),
                density_matching_seconds=t_opt, e_corr_matched=float(be.e_corr), fragments=len(be.Fobjs), n_emb=[int(f.nao) for f in be.Fobjs])


def df_c4(lib, reps=5):
    """BASELINE configs[3] in the line: the density-fitted AO -> fragment transform at N_ao = 512, n_aux = 1000, n = 220, synthetic integrals, result
    resident in a device fragment.  Executed flops as in tools/transform_bench.py (two rotations, the product with L^-1, the block columns of bb^T bb at and below
    the diagonal); parity at this size: tests/test_gpu_be.py::test_transforms_at_survey_sizes."""
    from quemb_amd import eri_transform as et
    from quemb_amd.fragsolver import DeviceFragment
    rng = np.random.default_rng(SEED0)
    N, naux, n = 512, 1000, 220
    npair = N * (N + 1) // 2
    ints = 0.06 * rng.standard_normal((naux, npair))
    A = rng.standard_normal((naux, naux)) / np.sqrt(naux)
    j2c = A @ A.T + np.eye(naux)
    TA = np.linalg.qr(rng.standard_normal((N, N)))[0][:, :n].copy()
    t0 = time.perf_counter()
    df = et.DFContext(j2c=j2c, lib=lib); df.set_ints(ints, N, layout="packed"); lib.qemb_sync()
    t_setup = time.perf_counter() - t0
    fr = DeviceFragment(n, 22, lib=lib)
    df.transform(TA, frag=fr, want_host=False); lib.qemb_sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); df.transform(TA, frag=fr, want_host=False); lib.qemb_sync(); ts.append(time.perf_counter() - t0)
    dt = min(ts)
    npn = n * (n + 1) // 2
    nblk = 8 if npn >= 2048 else 1
    w = ((npn + nblk - 1) // nblk + 127) // 128 * 128
    syrk = sum(2.0 * (npn - c0) * min(w, npn - c0) * naux for c0 in range(0, npn, w))
    flop = 2.0 * naux * N * N * n + 2.0 * naux * N * n * n + 2.0 * naux * naux * npn + syrk
    df.free(); fr.free()
    return dict(N_ao=N, n_aux=naux, n=n, transform_ms=dt * 1e3, executed_GFLOP=flop / 1e9, tflops_executed=flop / dt / 1e12,
                frac_of_fp64_matrix_peak=flop / dt / 1e12 / PEAK_FP64_MFMA_TFLOPS, setup_s=t_setup,
                what="qemb_df_transform: (P|mu nu) -> (P|ij), L^-1, bb^T bb into the fragment's 4-fold packed block (molbe/eri_onthefly.py:45-145)")


def kbe_c5_sweeps(lib, reps=20):
    """BASELINE configs[4] at its own dimensions (kbe polyacetylene BE2: a C4H4 cell of 24 AOs and 28 electrons, 1 x 1 x 3 k-points) on the
    density-fitted model of that size (tests/kbe_model.build_chain; PySCF-PBC / libdmet integrals do not exist in this image): the supercell
    mean field by the device fragment RHF, `kbe_pbe.BE(int_transform="supercell-DF-hip")` -- k -> R Fourier step and SVD Schmidt per
    fragment, fragment ERIs from the supercell DF integrals through the device CC-GDF transform, k-averaged Fock, fragment RHF, HF-in-HF --
    then one-shot sweeps over the four fragments of the reference cell (36 embedding orbitals each)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import kbe_model
    from kbe_df_source import GammaSourceFromFactor
    from quemb_amd import kbe_pbe
    from quemb_amd.fragpart import FragPart
    from quemb_amd.fragsolver import DeviceFragment

    def device_rhf(hs, eri_s1, nocc):
        N = hs.shape[0]
        il = np.tril_indices(N)
        fr = DeviceFragment(N, N, lib=lib)
        fr.set_eri_s4(np.ascontiguousarray(eri_s1[il[0], il[1]][:, il[0], il[1]]))
        r = fr.scf(nocc, hs, None)
        if not r["converged"]:
            raise RuntimeError("the supercell RHF of the configs[4] model did not converge")
        C_ = r["mo_coeff"]
        dm = 2.0 * C_[:, :nocc] @ C_[:, :nocc].T
        J, K = fr.jk(dm)
        fr.free()
        veff = J - 0.5 * K
        return dict(mo_coeff=C_, mo_energy=r["mo_energy"], dm=dm, e_tot=0.5 * float(np.einsum("ij,ji->", 2.0 * hs + veff, dm)), veff=veff)

    t0 = time.perf_counter()
    m = kbe_model.build_chain(rhf=device_rhf)
    t_model = time.perf_counter() - t0
    kmf = kbe_pbe.KMeanField(a_vec=m["a_vec"], kpts=m["kpts"], kmesh=m["kmesh"], nelectron=2 * m["nocc_cell"], hcore=m["hk"], S=m["Sk"],
                             mo_coeff=m["Ck"], mo_energy=m["ek"], hf_veff=m["veffk"], e_tot=m["e_tot_cell"])
    src = GammaSourceFromFactor(m["B"])
    lib.qemb_device_sync(); t0 = time.perf_counter()
    be = kbe_pbe.BE(kmf, FragPart(**kbe_model.chain_be2_lists(m["n_units"], m["units_per_cell"], m["unit_size"])), lib=lib, distribute=False,
                    int_transform="supercell-DF-hip", df_source=src)
    lib.qemb_device_sync(); t_init = (time.perf_counter() - t0) * 1e3
    be.oneshot(); be.oneshot(); be.oneshot()
    ts, (e, _) = timed_sweeps(lib, be.oneshot, reps)
    st = _stats_ms(ts)
    return dict(sweep=st, sweep_ms=st["p50_ms"], fragments=len(be.Fobjs), n_emb=[int(f.nao) for f in be.Fobjs], n_occ=[int(f.nsocc) for f in be.Fobjs],
                aos_per_cell=m["nlo"], kpts=m["nk"], electrons_per_cell=2 * m["nocc_cell"], n_supercell=m["N"], naux_supercell=int(m["B"].shape[0]),
                initialize_ms=t_init, model_build_s=t_model, hf_in_hf_error_Eh=float(be.hf_err), e_corr_per_cell=float(e), nstreams=be.nstreams, lockstep=be.lockstep,
                what="kbe_pbe.BE one-shot sweep at the dimensions of BASELINE configs[4] (kbe/pbe.py:78-316, :502-716): 4 BE2 fragments of the reference cell, "
                     "fragment RHF + MO transformation + RCCSD + RDMs + energies each; initialize_ms = Schmidt (k -> R, SVD), supercell CC-GDF transform of all "
                     "fragments, k-averaged Fock, fragment RHF, HF-in-HF; synthetic DF model integrals (tests/kbe_model.build_chain), parity in "
                     "tests/test_gpu_be.py::test_c5_dimensions_kpoint_view_equals_supercell_view")


# ------------------------------------------------------------------------------------------------------------ main
def main():
    global FULL_N, FULL_O, FULL_NF
    args = parse()
    if os.environ.get("QEMB_BENCH_WATCHDOG_S"):      # diagnostics: the Python stacks of all threads to stderr every so many seconds (where does a silent run sit?)
        import faulthandler
        faulthandler.enable(file=sys.stderr, all_threads=True)
        faulthandler.dump_traceback_later(float(os.environ["QEMB_BENCH_WATCHDOG_S"]), repeat=True, file=sys.stderr)
    FULL_N, FULL_O = args.full_n, args.full_nocc
    FULL_NF = min(FULL_NF, FULL_N // 2)
    if args.cpu_worker:
        return cpu_worker(args.cpu_worker, args.cpu_mode, args.nocc, args.cpu_iters, args.cpu_nproc)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args)                 # this process stays off the GPU; the ranks are its children
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1")); lrank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: under an external launcher start exactly --gpus ranks "
                         "(or unset WORLD_SIZE and let bench.py launch them)")
    # Transport between the ranks: "rccl" = the library's own communicator (qemb_comm_*, no torch in the process);
    # "nccl" / "gloo" = a torch.distributed group (gloo + several ranks on one card is a rehearsal mode for 1-GPU boxes: RCCL refuses duplicate GPUs)
    backend = os.environ.get("QEMB_DIST_BACKEND", "rccl")
    if backend not in ("rccl", "nccl", "gloo"):
        raise SystemExit(f"QEMB_DIST_BACKEND={backend}: expected rccl, nccl or gloo")
    dist = torch = None
    if world > 1 and backend != "rccl":
        import torch                              # before libqemb_hip.so: see quemb_amd/be_parallel.py on the load order
        import torch.distributed as dist
        lrank = lrank % max(torch.cuda.device_count(), 1)
        if torch.cuda.is_available():
            torch.cuda.set_device(lrank)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", lrank))
        else:
            dist.init_process_group(backend="gloo")
    from quemb_amd import _lib, comm
    from quemb_amd.be_parallel import be_func_parallel, fragment_cost, partition_fragments
    from quemb_amd.fragsolver import default_opts
    from quemb_amd.solver import ErrorMap, be_func
    if args.lib:                                  # tests only (tests/test_bench_launcher.py): the drivers on the scalar mock device layer
        lib = _lib.declare(C.CDLL(args.lib))
        _lib.check(lib.qemb_init(0), "qemb_init", lib)
    else:
        lib = _lib.init(lrank)
    if world > 1 and backend == "rccl":
        try:
            if os.environ.get("QEMB_BENCH_FAIL_COMM_INIT"):       # tests only: exercise the fallback below
                raise RuntimeError("communicator start-up failure requested by QEMB_BENCH_FAIL_COMM_INIT")
            comm.init_from_env(lib)
            log(f"communicator up: {world} ranks ({lib.qemb_backend().decode()})")
        except Exception as e:  # noqa: BLE001
            # The library communicator did not come up (bounded: QEMB_COMM_TIMEOUT_S).  A start-up failure is global -- ncclCommInitRank is
            # collective -- so every rank gets here; rather than lose the whole N-GPU measurement the ranks fall back to a torch.distributed
            # gloo group for the one small all-reduce per sweep (host buffers, a few hundred bytes: latency of ~0.1 ms against a sweep of
            # seconds), and the JSON line says so in config.transport.  (torch after libqemb_hip.so is fine for CPU tensors.)
            print(f"bench.py rank {rank}: library communicator failed ({e}); falling back to torch.distributed gloo", file=sys.stderr, flush=True)
            backend = "gloo-fallback"
            try:
                comm.destroy(lib)            # (a communicator that came up half way must not be picked up by be_parallel.all_reduce_sum)
            except Exception:  # noqa: BLE001
                comm._active = None
            import datetime
            import torch
            import torch.distributed as dist
            dist.init_process_group(backend="gloo", timeout=datetime.timedelta(seconds=float(os.environ.get("QEMB_COMM_INIT_TIMEOUT_S") or os.environ.get("QEMB_COMM_TIMEOUT_S") or "300") + 60.0))

    def barrier():
        if world > 1:
            comm.barrier(lib) if backend == "rccl" else dist.barrier()

    def max_over_ranks(x):
        if world == 1:
            return x
        if backend == "rccl":
            return float(comm.all_reduce(lib, np.array([x]), comm.MAX)[0])
        tt = torch.tensor([x], dtype=torch.float64, device=torch.device("cuda", lrank) if backend == "nccl" else torch.device("cpu"))
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    def sync():
        """every stream of this rank's device idle (hipDeviceSynchronize: what torch.cuda.synchronize() does)"""
        _lib.check(lib.qemb_device_sync(), "qemb_device_sync", lib)
    n, o, F = args.n, args.nocc, args.frags_per_gpu
    v = n - o
    nf = min(22, n // 2)
    if nf < 2 * N_EDGE:
        raise SystemExit(f"--n {n}: the synthetic ring needs at least {2 * N_EDGE} fragment sites (n >= {4 * N_EDGE})")
    opts = default_opts(lib)
    F_total = F * world if args.scaling == "weak" else args.frags_total
    if F_total < world:
        raise SystemExit(f"--scaling strong: {F_total} fragments cannot occupy {world} ranks")
    owner = partition_fragments([fragment_cost(n, o)] * F_total, world)     # the product's LPT partition (equal costs: F per rank)
    F = max(owner.count(r) for r in range(world))
    if not args.lib:
        # resident per fragment: the 4-fold packed ERIs; beside them the pooled work space of the fragments in flight
        npair = n * (n + 1) // 2
        naux_syn = 3 * n
        # resident per fragment (factor, and the block with --resident block) + the work space of the fragments in flight (two n^2 x npair transform buffers and
        # ~1.5 more of that size in ladder operands / amplitudes, the unpacked and rotated factor images)
        need = F * 8.0 * (naux_syn * npair + (npair * npair if args.resident == "block" else 0)) + args.nstreams * 8.0 * (3.5 * n * n * npair + 3.5 * naux_syn * n * n)
        free_b, total_b = C.c_size_t(), C.c_size_t()
        if lib.qemb_mem_info(C.byref(free_b), C.byref(total_b)) == 0 and need > 0.97 * free_b.value:
            raise SystemExit(f"bench.py: {F} fragments of n={n} per GPU need ~{need / 1e9:.0f} GB, {free_b.value / 1e9:.0f} GB are free "
                             f"(--scaling {args.scaling}: lower --frags-{'per-gpu' if args.scaling == 'weak' else 'total'} or use more GPUs)")

    # ---- set-up (untimed): fragments resident in HBM, initial fragment SCF for dm0 (BE.initialize does the same)
    log(f"setting up {F} fragments per GPU (n={n}, n_occ={o}), {F_total} in the ring")
    frs, npot = make_ring(lib, n, o, nf, F_total, owner, rank, args.scale, opts, args.mo_route, args.resident)
    mine = [i for i in range(F_total) if owner[i] == rank]
    emap = ErrorMap(frs)
    pot = [0.0] * npot
    Nocc = float(F_total * N_EDGE) * 1.0
    if args.nstreams > 1 and args.cu_split > 1 and not args.lib:
        from quemb_amd.solver import set_cu_partition
        set_cu_partition(lib, args.cu_split)
    nctx = lib.qemb_ctx_count(args.nstreams + 1) if args.nstreams > 1 else 1
    stats = {}

    def sweep():
        """one objective evaluation through the product sweep; returns the residual norm and the energies"""
        if world > 1:
            return be_func_parallel(pot, frs, Nocc, "CCSD", 0.0, eeval=True, return_vec=True, owner=owner, opts=opts, stats=stats, emap=emap,
                                    nstreams=args.nstreams)
        return be_func(pot, frs, Nocc, "CCSD", 0.0, eeval=True, return_vec=True, opts=opts, stats=stats, nstreams=args.nstreams)

    log("fragments resident; warm-up sweeps")
    for _ in range(args.warmup):
        sweep()
    log("timed sweeps")
    for s in range(8):
        read_timer(lib, s, nctx, reset=1)
    stats.clear()
    barrier()
    sync()
    t0 = time.perf_counter()
    ecorr_sum = 0.0
    for _ in range(args.steps):
        ernorm, ervec, (ecorr, e_parts) = sweep()
        ecorr_sum += ecorr
    sync()
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    # stats["ccsd_iterations"] is summed over ranks inside the sweep's all-reduce when world > 1
    n_iter_total = float(stats.get("ccsd_iterations", 0)); n_frag_total = float(stats.get("fragments", 0))

    log(f"timed region done: {dt:.2f} s for {args.steps} step(s)")
    if rank == 0:
        it_ms, it_cnt = read_timer(lib, 2, nctx)
        ao_ms, ao_cnt = read_timer(lib, 3, nctx)
        scf_ms, scf_cnt = read_timer(lib, 4, nctx)
        ring_ms, ring_cnt = read_timer(lib, 1, nctx)
        lad_ms_c, lad_cnt_c = read_timer(lib, 0, nctx)
        fr0 = frs[mine[0]]
        h0, dm00 = fr0.fock, fr0.dm0
        if args.dump_outputs:
            names = dump_outputs(args.dump_outputs, frs, mine, ernorm, ervec, ecorr, e_parts)
            log(f"outputs of the last timed step written to {args.dump_outputs}: {', '.join(names)}")
        res = {
            "metric": "fragment CCSD iters/sec (full BE sweep over synthetic n_occ=20 n_virt=200 fragments); corr-E error vs oracle in parity_max_abs_err_Eh / parity_n220_abs_err_Eh",
            "value": n_iter_total / dt, "unit": "CCSD iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[2]: synthetic fragment sweep, {F} fragments per GPU ({F_total} total, {args.scaling} scaling), "
                                   f"n_occ={o} n_virt={v} (n={n}), DF-factorised ERIs naux={3 * n}, ERI scale={args.scale} (SURVEY 8d says 0.06: the oracle's "
                                   "own RHF/CCSD diverges there for n > ~100, DESIGN.md), one be_func / be_func_parallel sweep per step "
                                   "(update_heff + fragment RHF + MO-basis integrals + RCCSD to |dE|<1e-10 + 1-RDM + energies per fragment, solve_error, 1 all-reduce); "
                                   + ("MO-basis integrals from each fragment's 3-index DF factor (north_star's density-fitted 3-index route: the factor is rotated into the "
                                      "fragment's orbitals and multiplied with itself, 2 naux npair^2 flops; same integrals to rounding as the four-index transformation "
                                      "-- tests/test_gpu_fragment.py holds both routes to the oracle at n = 220 -- whose figure is `four_index_route`)"
                                      if args.mo_route == "factor" else "MO-basis integrals by the four quarter transformations of the 4-fold packed block"),
                       "mo_route": args.mo_route,
                       "redrawn_fragments_rank0": REDRAWN, "min_fragment_rhf_gap_Eh": MIN_GAP,
                       "resident": args.resident,
                       "resident_bytes_per_fragment": (fr0.dev.resident_bytes() if hasattr(fr0.dev, "resident_bytes") and not args.lib else None),
                       "resident_note": ("each fragment keeps its 3-index DF factor alone (qemb_frag_set_df_only: 8 naux npair bytes + orbitals, densities and kept amplitudes); "
                                         "J / K of the fragment RHF, MO integrals and energies come from it, no 4-fold packed block (8 npair^2 = 4.7 GB at n = 220) is formed"
                                         if args.resident == "factor" else "each fragment keeps the 4-fold packed ERI block and its 3-index factor (rounds 1-4)"),
                       "fragments_per_gpu": F, "n_occ": o, "n_virt": v, "fragments_in_flight_per_gpu": args.nstreams, "cu_partition": (args.cu_split if args.nstreams > 1 else 0),
                       "parallelism": f"fragments sharded over {world} GPU(s) by the LPT partition, 1 all-reduce per sweep",
                       "transport": None if world == 1 else {"rccl": "library communicator: ncclAllReduce on a persistent RCCL communicator (qemb_comm_allreduce)",
                                                             "nccl": "torch.distributed nccl (RCCL)", "gloo": "torch.distributed gloo (rehearsal)",
                                                             "gloo-fallback": "torch.distributed gloo -- FALLBACK: the library's RCCL communicator failed to start (stderr has the reason)"}[backend]
                                    + (" [hostcheck mock: shared-memory transport]" if args.lib else ""),
                       "fragments_per_rank": [owner.count(r) for r in range(world)],
                       "allreduce_bytes_per_sweep": stats.get("allreduce_bytes_per_sweep", 0 if world == 1 else None),
                       "residual_slots": int(2 * emap.n_match + 5)},
            "host": {"usable_cores": usable_cores(), "os_cpu_count": os.cpu_count(), "blas_threads": os.environ.get("OPENBLAS_NUM_THREADS"),
                     "note": "BLAS / OpenMP pools capped inside the container's CPU share (quemb_amd/hostthreads.py): an unbounded OpenBLAS pool gets the process "
                             "throttled by the cgroup for most of a 100 ms period now and then"},
            "fragments_per_s": n_frag_total / dt,
            "ccsd_iterations_per_fragment": n_iter_total / max(n_frag_total, 1),
            "mean_e_corr_per_sweep": ecorr_sum / args.steps,
            "residual_norm": float(ernorm),
            "device_time_ms_rank0": {"note": f"HIP-event brackets inside the timed region; with {args.nstreams} fragment(s) in flight the brackets of different streams overlap",
                                     "ccsd_iteration_avg": it_ms / max(it_cnt, 1), "ccsd_iterations": it_cnt, "rings_avg": ring_ms / max(ring_cnt, 1),
                                     "mo_transform_avg": ao_ms / max(ao_cnt, 1), "fragment_scf_avg": scf_ms / max(scf_cnt, 1)},
        }
        if args.full:
            log("roofline pass: one fragment, one stream")
            rp = roofline_pass(lib, fr0.dev, h0, dm00, o, opts, args.roofline_iters)
            lad_avg = rp["ladder_ms"] * 1e-3
            npair_o = o * (o + 1) // 2
            npv, nmv, nmo = v * (v + 1) // 2, v * (v - 1) // 2, o * (o - 1) // 2
            flop_ladder = 2.0 * npair_o * float(npv) ** 2 + 2.0 * nmo * float(nmv) ** 2   # executed: (+/-) pair-packed products
            flop_dense = 2.0 * o * o * float(v) ** 4                 # SURVEY 8(d) dense-equivalent figure
            achieved = flop_ladder / lad_avg / 1e12 if lad_avg > 0 else 0.0
            traffic, traffic_source = None, None                     # HBM bytes per launch from the separate --pmc passes
            for cand in (PMC_FILE, "profiles/r04_pmc_ladder.json", "profiles/r03_pmc_ladder.json", "profiles/r02_pmc_ladder.json"):
                pmc = ROOT / cand
                if pmc.exists():
                    try:
                        traffic = json.loads(pmc.read_text()).get("hbm_bytes_per_launch")
                        traffic_source = f"{cand}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over tools/frag_bench.py (tools/pmc_ladder.sh), NOT collected in this run"
                        break
                    except Exception:  # noqa: BLE001
                        traffic = None
            res["roofline"] = {"bound": "mfma", "kernel": "dgemm_mfma_kernel<7,2,2,4,16,true,true,2,1,1> (+ pairs, 224x128 tile) and <6,2,2,4,16,true,true,2,1,1> (- pairs, 192x128): pp-ladder over (+/-) packed pairs, M=npair(o) N=K=npair(v), split-K + slab reduce",
                               "achieved": achieved, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_FP64_MFMA_TFLOPS,
                               # one pp-ladder = TWO dispatches of this kernel ((+) and (-) pair blocks); per-dispatch averages:
                               "traffic": None if traffic is None else traffic / 2.0, "traffic_source": traffic_source,
                               "avg_launch_ms": lad_avg * 1e3 / 2.0, "launches": 2 * rp["ladder_count"],
                               "measured": f"HIP events on the launch stream around the two ladder dispatches (+ their slab reductions) in a separate single-stream pass of {args.roofline_iters} CCSD iterations on fragment 0 right after the timed region",
                               "flop_per_launch": flop_ladder / 2.0, "ladder_ms": lad_avg * 1e3,
                               "dense_equivalent_tflops": flop_dense / lad_avg / 1e12 if lad_avg > 0 else 0.0,
                               "algorithmic_bytes_per_launch": 4.0 * (float(npv) ** 2 + float(nmv) ** 2 + 2.0 * npair_o * npv + 2.0 * nmo * nmv),
                               "ladder_ms_in_timed_region": lad_ms_c / max(lad_cnt_c, 1),
                               "single_stream_iteration_ms": rp["iter_ms"], "single_stream_rings_ms": rp["rings_ms"]}
        if world == 1 and args.full:
            try:
                res["roofline"]["peak_measured"] = mfma_peak_probe(lib)
                res["roofline"]["peak_measured_how"] = "register-only v_mfma_f64_16x16x4_f64 loop, 16 independent accumulator chains per wave, 8 waves per CU (qemb_mfma_f64_peak)"
                cp = clock_probe(lib)
                clk = cp["ghz"]
                res["roofline"].update({"sustained_clock_ghz": clk, "peak_at_sustained_clock": PEAK_FP64_MFMA_TFLOPS * clk / 2.4,
                                        "frac_of_sustained_peak": achieved / (PEAK_FP64_MFMA_TFLOPS * clk / 2.4) if clk > 0 else None,
                                        "clock_probe_tflops": cp["tflops"],
                                        "clock_probe": "launches of the ladder tile (cfg 13 = the same code under the untagged kernel symbol, M=210 N=4096 K=16384, split-K 8 = 256 workgroups, random operands) "
                                                       "right after the timed region, GPU still hot: sum of per-workgroup s_memtime ticks / (256 CUs x kernel time)"})
            except Exception as e:  # noqa: BLE001
                res["roofline"]["sustained_clock_ghz"] = f"probe failed: {e}"
            if args.mo_route == "factor" and not args.lib:
                # the same sweep with the other route (the four quarter transformations of the packed block, as in rounds 1-3), one warm-up and one timed sweep
                try:
                    if args.resident == "factor":
                        # the four quarter transformations read the 4-fold packed block: give the fragments theirs for this leg (as --resident block keeps it),
                        # when 8 npair^2 bytes per fragment fit beside the work space; otherwise the leg is skipped (the block as a per-solve transient would be timed too)
                        npair_ = n * (n + 1) // 2
                        free_b, total_b = C.c_size_t(), C.c_size_t()
                        lib.qemb_trim_all(); lib.qemb_mem_info(C.byref(free_b), C.byref(total_b))
                        # (the work space of the fragments in flight is parked in the contexts' pools and is reused: only the blocks are new)
                        if len(mine) * 8.0 * npair_ * npair_ > 0.85 * free_b.value:
                            raise RuntimeError("skipped: the 4-fold packed blocks of this many fragments do not fit")
                        for I in mine:
                            _, _, d4, dB, naux_ = make_device_eris(lib, n, frs[I].seed, args.scale, block=True)
                            frs[I].dev.set_eri_s4_dev(d4.ptr); d4.free()
                            frs[I].dev.set_df_factor_dev(dB.ptr, naux_); dB.free()
                    for f in frs:
                        if getattr(f, "dev", None) is not None:
                            f.dev.set_mo_route(0)
                    sweep()
                    n0 = float(stats.get("ccsd_iterations", 0))
                    sync(); t1 = time.perf_counter()
                    sweep()
                    sync(); dt4 = time.perf_counter() - t1
                    res["four_index_route"] = {"value": (float(stats.get("ccsd_iterations", 0)) - n0) / dt4, "unit": "CCSD iterations/s", "ms_per_step": dt4 * 1e3,
                                               "mo_transform_avg_ms": None, "what": "one timed sweep of the same fragments with qemb_frag_mo_route(0)"}
                    for f in frs:
                        if getattr(f, "dev", None) is not None:
                            f.dev.set_mo_route(-1)
                except Exception as e:  # noqa: BLE001
                    res["four_index_route"] = f"failed: {e}"
            log("parity probe vs oracle")
            try:
                res["parity_max_abs_err_Eh"] = parity_probe()
            except Exception as e:  # noqa: BLE001
                res["parity_max_abs_err_Eh"] = f"probe failed: {e}"
            if not args.no_octane and not args.lib:
                log("small-fragment regime: octane BE2 sweeps")
                try:
                    import contextlib
                    if args.nstreams > 1 and args.cu_split > 1:
                        from quemb_amd.solver import set_cu_partition
                        set_cu_partition(lib, 0)          # small fragments: every context on the whole chip again
                    with contextlib.redirect_stdout(sys.stderr):      # the BE driver prints its energies: stdout carries the ONE JSON line only
                        oc = octane_sweeps(lib, cpu=not args.no_cpu_baseline)
                    res["octane_be2_sweep_ms"] = min(oc["streams6_ms"], oc["lockstep_ms"])
                    res["octane_be2"] = oc
                except Exception as e:  # noqa: BLE001
                    res["octane_be2_sweep_ms"] = f"failed: {e}"
                try:
                    res["df_c4"] = df_c4(lib)
                except Exception as e:  # noqa: BLE001
                    res["df_c4"] = f"failed: {e}"
                try:
                    with contextlib.redirect_stdout(sys.stderr):
                        res["h8_be2"] = h8_be2(lib)
                except Exception as e:  # noqa: BLE001
                    res["h8_be2"] = f"failed: {e}"
                log("periodic driver at the dimensions of configs[4]")
                try:
                    with contextlib.redirect_stdout(sys.stderr):
                        kc = kbe_c5_sweeps(lib)
                    res["kbe_c5_sweep_ms"] = kc["sweep_ms"]
                    res["kbe_c5"] = kc
                except Exception as e:  # noqa: BLE001
                    res["kbe_c5_sweep_ms"] = f"failed: {e}"
            if not args.no_size_sweep and not args.lib:
                log("fragment-size sweep")
                try:
                    for f in frs:                      # the headline fragments are done: their HBM goes to the sweep's (n = 300: 16 GB of work space per fragment in flight)
                        if getattr(f, "dev", None) is not None and f is not fr0:
                            f.dev.free()
                    lib.qemb_trim_all()                # (every context's parked work space: ~200 GB after the sections above)
                    sys.path.insert(0, str(ROOT / "tools"))
                    import size_sweep
                    import contextlib
                    with contextlib.redirect_stdout(sys.stderr):
                        res["size_sweep"] = size_sweep.run(lib, log=log)
                except Exception as e:  # noqa: BLE001
                    res["size_sweep"] = f"failed: {e}"
            if not args.no_cpu_baseline:
                info, e_dev, e_cpu = cpu_baseline(lib, fr0.dev, h0, dm00, o, opts, args.cpu_iters, args.cpu_ompnum, args.scale)
                res["cpu_baseline"] = info
                # full-size parity: the device and the oracle run the SAME args.cpu_iters plain amplitude updates on the same n = 220 fragment
                res["parity_n220_abs_err_Eh"] = None if e_cpu is None else abs(e_dev - e_cpu)
                res["parity_n220"] = dict(e_corr_device=e_dev, e_corr_oracle=e_cpu, updates=args.cpu_iters,
                                          what="E_corr after the same number of plain (no DIIS) RCCSD amplitude updates from the MP2 guess, fragment 0 (n=220): device vs oracle/qemb_oracle/ccsd_lean.py on the device-exported MO integrals")
        print(json.dumps(res), flush=True)
    barrier()
    if world > 1:
        comm.destroy(lib) if backend == "rccl" else dist.destroy_process_group()
    if backend == "gloo-fallback":
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(0)          # a rendezvous thread may still sit inside RCCL: leave without running its exit handlers
    return 0


if __name__ == "__main__":
    sys.exit(main())
