"""Time the Cholesky-decomposed AO integrals (qemb_df_set_ints_from_cholesky plus one qemb_df_transform per fragment) against the stored and the
integral-direct route of the same process.

    python tools/cholesky_bench.py [out.jsonl]                     (default profiles/cholesky_bench.jsonl)

Cases: H8 / STO-3G, H8 / cc-pVDZ and octane / STO-3G with the embedding coefficients of their BE2 fragments, at tol = 1e-4, 1e-6, 1e-8.  Per case and
tolerance one JSON line; every time is the wall time around synchronous calls on a warm basis, two warm-up calls, min / median / max of 9 repetitions:
  cholesky_ms     the decomposition into a DF context and one transform per fragment (blocks back to the host, as on the other sides)
  decompose_ms    the decomposition alone
  stored_ms       qemb_aoeri_from_basis plus one qemb_ao2mo_dense per fragment ("in-core-hip")
  direct_ms       one qemb_ao2mo_direct call for all fragments ("int-direct-hip", its default tile)
with rank, panels, integral columns evaluated over npair, the device bytes of the decomposition (qemb_int_cholesky_bytes at max_rank = the rank found) against
the 8 npair^2 of the stored integrals, the largest deviation of the blocks from the stored route, and the one-shot BE2 MP2 correlation energy of
int_transform="cholesky-hip" minus that of "in-core-hip" from the geometry."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np                                                        # noqa: E402
from quemb_amd import eri_transform as et                                 # noqa: E402
from quemb_amd import integrals as I                                      # noqa: E402
import ao2mo_direct_bench as bd                                           # noqa: E402
import int4c_bench as b4                                                  # noqa: E402

TOLS = (1e-4, 1e-6, 1e-8)


def be_energy(name, mf, lib, route, **kw):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    key, rep = bd.FRAGS[name]
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", key)
    if rep > 1:
        fobj = fobj.replicate_sites(rep)
    be = BE(mf, fobj, lib=lib, distribute=False, int_transform=route, integral_backend="hip", **kw)
    return float(be.oneshot(solver="MP2")[0])


def main_cases(out):
    from quemb_amd import _lib
    lib = _lib.init()
    rows = []
    for name, mol in b4.cases():
        tas = bd.fragment_tas(name, mol, lib)
        ns = [t.shape[1] for t in tas]
        npair = mol.nao * (mol.nao + 1) // 2
        basis = I.DeviceBasis(mol, lib)

        def stored():
            ao = et.AOEri.from_basis(basis)
            try:
                return [ao.transform(t) for t in tas]
            finally:
                ao.free()

        ref = stored()
        t_stored = bd.timed(stored)
        t_direct = bd.timed(lambda: basis.ao2mo(tas))
        mf = I.RHF(mol, integral_backend="hip", lib=lib, direct=True)
        mf.kernel()
        e_ref = be_energy(name, mf, lib, "in-core-hip")
        for tol in TOLS:
            def cholesky(with_transforms=True):
                df = et.DFContext.from_cholesky(mol, tol=tol, basis=basis)
                try:
                    return ([df.transform(t) for t in tas] if with_transforms else None), df.cd_stats
                finally:
                    df.free()

            got, st = cholesky()
            dev = max(float(np.abs(g - r).max()) for g, r in zip(got, ref))
            row = dict(case=name, nao=mol.nao, npair=npair, n_frag=len(tas), n=ns, tol=tol, rank=st["rank"], panels=st["panels"], columns=st["columns"],
                       columns_over_npair=st["columns"] / npair, final_max_d=st["max_d"],
                       timing="wall time around synchronous calls on a warm basis, 2 warm-up calls, min / median / max in ms",
                       cholesky_ms=bd.timed(cholesky), decompose_ms=bd.timed(lambda: cholesky(False)), stored_ms=t_stored, direct_ms=t_direct,
                       cholesky_device_bytes=basis.cholesky_bytes(max_rank=st["rank"]), stored_integral_bytes=8 * npair * npair,
                       max_abs_deviation_from_stored_blocks=dev, e_corr_mp2_oneshot_minus_in_core_hip=be_energy(name, mf, lib, "cholesky-hip", cd_tol=tol) - e_ref)
            print(json.dumps(row), flush=True)
            rows.append(row)
        mf.free()
        basis.free()
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    a = sys.argv[1:]
    main_cases(Path(a[0]) if a else ROOT / "profiles" / "cholesky_bench.jsonl")
