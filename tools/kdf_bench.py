"""Time the k-point density-fitted route of the periodic driver against the supercell route, and price its three passes as HBM passes.

    python tools/kdf_bench.py [out.jsonl]        (default profiles/kdf_bench.jsonl)

Meshes: 1 x 1 x nk with nk = 3, 5, 8 at the dimensions of tests/kbe_model.build_chain (BASELINE configs[4]: 24 orbitals and 32 auxiliary functions per cell, a
36-orbital BE2 fragment).  The factor is built by build_chain's recipe; no mean field is solved (at nk = 8 the dense supercell integrals are 10 GB) -- the
embedding orbitals are a random real orthonormal set in the supercell, Fourier transformed: time-reversal symmetric like the ones of a mean field.
Per mesh one JSON line: wall time of both routes for four fragments (set-up: upload of the tensor; transform: per fragment, warm), the resident bytes of
both, the largest difference of the two blocks, and per pass of kdf_ops.hip the device time (library timers) against its bytes at 8 TB/s."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from kbe_df_source import GammaSourceFromFactor                          # noqa: E402
from quemb_amd import _lib                                               # noqa: E402
from quemb_amd import eri_transform as et                                 # noqa: E402
from quemb_amd._lib import DeviceBuffer, check                            # noqa: E402
from quemb_amd.fragsolver import DeviceFragment                           # noqa: E402
from quemb_amd.kbe_eri_kpoint import KdfContext, KPointDFSource           # noqa: E402
from quemb_amd.kbe_pfrag import get_phase1                                # noqa: E402

HBM_PEAK = 8.0e12
SLOT = 9
U, u, NAUX_UNIT, NFRAG, N_EMB, A = 4, 6, 8, 4, 36, 4.91


def chain_factor(nk, seed=11, scale=0.12):
    """the DF factor of kbe_model.build_chain (auxiliary functions on three consecutive units), without the mean field"""
    rng = np.random.default_rng(seed)
    nun, N = nk * U, nk * U * u
    orb = lambda j: np.arange((j % nun) * u, (j % nun + 1) * u)
    decay = np.repeat([0.45, 1.0, 0.45], u)
    pats = []
    for t in range(U):
        pt = scale * rng.standard_normal((NAUX_UNIT, 3 * u, 3 * u))
        pats.append(0.5 * (pt + pt.transpose(0, 2, 1)) * decay[None, :, None] * decay[None, None, :])
    B = np.zeros((nun * NAUX_UNIT, N, N))
    for j in range(nun):
        idx = np.concatenate([orb(j - 1), orb(j), orb(j + 1)])
        for a_ in range(NAUX_UNIT):
            B[j * NAUX_UNIT + a_][np.ix_(idx, idx)] += pats[j % U][a_]
    return B


def timed(lib, fn, reps=3):
    fn()
    check(lib.qemb_device_sync(), lib=lib)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    check(lib.qemb_device_sync(), lib=lib)
    return (time.perf_counter() - t0) / reps * 1e3


def dev_ms(lib, fn, reps=5):
    fn()
    check(lib.qemb_timer_reset(SLOT), lib=lib)
    for _ in range(reps):
        check(lib.qemb_timer_begin(SLOT), lib=lib)
        fn()
        check(lib.qemb_timer_end(SLOT), lib=lib)
    ms, cnt = C.c_double(), C.c_int64()
    check(lib.qemb_timer_read(SLOT, C.byref(ms), C.byref(cnt)), lib=lib)
    return ms.value / max(cnt.value, 1)


def main():
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "kdf_bench.jsonl"
    lib = _lib.init()
    rows = []
    for nk in (3, 5, 8):
        nao, naux = U * u, U * NAUX_UNIT
        kpts = np.array([[0.0, 0.0, 2 * np.pi * m / (nk * A)] for m in range(nk)])
        a_vec, kmesh = np.diag([8.0, 8.0, A]), [1, 1, nk]
        B = chain_factor(nk)
        rng = np.random.default_rng(nk)
        TAs_R = [np.linalg.qr(rng.standard_normal((nk * nao, N_EMB)))[0] for _ in range(NFRAG)]
        ph1 = get_phase1(a_vec, kpts, kmesh)
        TAs_k = [np.einsum("Rmi,Rk->kmi", T.reshape(nk, nao, N_EMB), ph1) for T in TAs_R]      # the back transform of KFrags.sd (kbe/pfrag.py:192)
        # ---- supercell route: the whole factor resident, one real transform per fragment
        t0 = time.perf_counter()
        gsrc = GammaSourceFromFactor(B)
        df = et.DFContext.periodic(gsrc.j2c(), lib=lib)
        df.alloc_ints(gsrc.nao)
        F = np.asarray(gsrc.ft_aux_block(0, gsrc.n_planewaves)).conj().T
        df.add_pw_block(F, gsrc.pw_block(0, gsrc.n_planewaves))
        df.add_rs_block(0, gsrc.rs_block(0, gsrc.naux))
        check(lib.qemb_device_sync(), lib=lib)
        sup_setup = (time.perf_counter() - t0) * 1e3
        frs = [DeviceFragment(N_EMB, 18, lib=lib) for _ in range(NFRAG)]
        sup_ms = timed(lib, lambda: [df.transform(T, frag=d) for T, d in zip(TAs_R, frs)]) / NFRAG
        ref = [d.get_eri_s4() for d in frs]
        df.free()
        # ---- k-point route
        t0 = time.perf_counter()
        src = KPointDFSource.from_supercell_factor(B, nk, naux, a_vec, kpts, kmesh)
        fourier_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ctx = KdfContext(src, lib=lib)
        check(lib.qemb_device_sync(), lib=lib)
        k_setup = (time.perf_counter() - t0) * 1e3
        k_ms = timed(lib, lambda: [ctx.transform(T, frag=d, factor_only=False) for T, d in zip(TAs_k, frs)]) / NFRAG
        kf_ms = timed(lib, lambda: [ctx.transform(T, frag=d, factor_only=True) for T, d in zip(TAs_k, frs)]) / NFRAG
        err = max(np.abs(d.get_eri_s4() - r).max() for d, r in zip(frs, ref))
        ctx.free()
        # ---- the three passes on their own
        ld, n, np_ = (nao + 15) // 16 * 16, N_EMB, N_EMB * (N_EMB + 1) // 2
        z = DeviceBuffer.from_numpy(rng.standard_normal(naux * nao * nao * 2), lib=lib)
        pl = DeviceBuffer(naux * nao * 2 * ld, lib=lib)
        ta = DeviceBuffer.from_numpy(rng.standard_normal(nk * nao * n * 2), lib=lib)
        cs, dk = DeviceBuffer(nk * 4 * ld * n, lib=lib), DeviceBuffer(nk * 4 * nao * n, lib=lib)
        M = DeviceBuffer.from_numpy(rng.standard_normal(naux * 2 * n * n), lib=lib)
        Fb = DeviceBuffer(2 * naux * np_, lib=lib)
        o2 = (C.c_double * 2)()
        passes = {}
        for name, fn, nbytes in [
                ("split", lambda: check(lib.qemb_op_kdf_split(naux * nao, nao, z.ptr, pl.ptr), lib=lib), 8 * (naux * nao * nao * 2 + naux * nao * 2 * ld)),
                ("stack", lambda: check(lib.qemb_op_kdf_stack(nk, nao, n, ta.ptr, cs.ptr, dk.ptr), lib=lib), 8 * (nk * nao * n * 2 + nk * 4 * (ld + nao) * n)),
                ("pack", lambda: check(lib.qemb_op_kdf_pack(naux, n, M.ptr, 1, 0.5, Fb.ptr, np_, o2), lib=lib), 8 * (naux * 2 * n * n + 2 * naux * np_))]:
            ms = dev_ms(lib, fn)
            passes[name] = dict(device_ms=round(ms, 5), bytes=nbytes, floor_ms_at_8TBs=round(nbytes / HBM_PEAK * 1e3, 6), frac_of_hbm=round(nbytes / HBM_PEAK / (ms * 1e-3), 4))
        n_kept = sum(1 for q in range(nk) if src.kept(q))
        row = dict(nk=nk, nao=nao, naux=naux, n=n, fragments=NFRAG,
                   supercell=dict(setup_ms=round(sup_setup, 2), transform_ms_per_fragment=round(sup_ms, 3), resident_bytes=8 * nk * naux * (nk * nao) ** 2),
                   kpoint=dict(host_fourier_ms=round(fourier_ms, 2), setup_ms=round(k_setup, 2), transform_block_ms_per_fragment=round(k_ms, 3),
                               transform_factor_only_ms_per_fragment=round(kf_ms, 3), resident_bytes=8 * n_kept * nk * naux * nao * 2 * ld),
                   max_abs_diff_blocks=float(err), passes=passes)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
