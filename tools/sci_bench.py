"""Time solver="SCI-hip" per stage: screen, sort / merge, matrix build, Davidson, RDMs.

    python tools/sci_bench.py [--pt2] [out.jsonl] [budget_s] [rows]        (default profiles/sci_bench.jsonl, 600 s per row, rows = synthetic,octane,small)

Per row one JSON line: eps, ndet, rounds, nnz, the energy beside CCSD's, the time of the whole solve (host clock around DeviceFragment.solve_sci without energies,
which ends in a synchronisation) and per stage (qemb_frag_sci_stage_ms: host wall time with the device drained at each boundary -- screen: the count and emit
passes with their scans; merge: the slab sorts, the unique / difference passes and every merge; build: the CSR matrix; davidson; rdm).  Medians of 9 calls after
two warm-ups.  A row whose single solve is so long that eleven of them would pass the budget is measured with fewer calls; `warmups` and `repeats` say how many, so
that such a row is not mistaken for a median of nine.  max_det is 2^23 (the default 2^20 refuses the smaller cutoffs at (42, 21)); a row that the limits still
refuse (max_det, or the memory left for the matrix) is recorded with the library's message.
Rows: the default synthetic fragment at (n, o) = (42, 21) and the first fragment of octane BE2 / STO-3G (tests/golden) for eps = 1e-3, 3e-4, 1e-4; (12, 6) at
eps = 1e-12 beside "FCI-hip" on the same fragment.
--pt2: the second-order correction (DeviceFragment.sci_pt2) instead: per row of PT2_CUTOFFS one solve, then one call at eps_pt = eps / 100 and one at eps / 1000 (a
first call that takes under a tenth of the budget is repeated and the median of up to five taken).  New lines with kind = "pt2": e_pt2, n_ext, batches, the three
stage times (screen, merge, rows), the time of the call, the time of the solve of the same run and their ratio.  They stand beside the solve rows, which stay as
they are; an earlier pt2 line of the same (fragment, eps, eps_pt) is replaced."""
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "oracle"))
from quemb_amd import _lib                                                            # noqa: E402
from quemb_amd.fragsolver import DeviceFragment, default_opts, default_sci_opts     # noqa: E402

CUTOFFS = (1e-3, 3e-4, 1e-4)
WARM, REPS = 2, 9
MAX_DET = 1 << 23
PT2_CUTOFFS = {"synthetic(42,21)": (1e-3,), "octane": (1e-3, 3e-4), "synthetic(12,6)": (1e-12,)}      # by the start of the row's name


def timed(fn, budget):
    """(median ms, last result, warm-ups, repeats, stage medians) of REPS calls after WARM warm-ups -- fewer of either when (WARM + REPS) calls would pass the budget (s)"""
    t0 = time.perf_counter()
    res = fn()
    first = time.perf_counter() - t0
    afford = max(2, int(budget / max(first, 1e-9)))      # calls the budget holds, the first included
    warm = min(WARM, max(1, afford - REPS)) if afford >= 3 else 1
    for _ in range(warm - 1):
        res = fn()
    reps = max(1, min(REPS, afford - warm))
    ts, stages = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
        stages.append(res[1])
    med = {k: statistics.median(s[k] for s in stages) for k in stages[0]} if stages[0] else {}
    return statistics.median(ts), res[0], warm, reps, med


def fragments(lib, which):
    """(name, DeviceFragment, nsocc, h, dm0, cutoffs) of the rows asked for"""
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    def synthetic(n, o):
        h, e1 = synthetic_fragment(n, o, 900 + 10 * n + o)
        fr = DeviceFragment(n, min(n, 3), lib=lib)
        fr.set_eri_s4(eri.pack_s4(e1))
        return fr, o, h, None
    if "synthetic" in which:
        yield ("synthetic(42,21)", *synthetic(42, 21), CUTOFFS)
    if "octane" in which:
        from quemb_amd.fragpart import FragPart
        from quemb_amd.integrals import RHF, Mole
        from quemb_amd.mbe import BE
        G = ROOT / "tests" / "golden"
        mf = RHF(Mole(G / "octane.xyz")); mf.kernel()
        be = BE(mf, FragPart.from_json(G / "fragmentation.json", "test_autogen_octane_be2"), lib=lib, distribute=False)
        f = be.Fobjs[0]
        yield (f"octane BE2 fragment 0 ({f.nao},{f.nsocc})", f.dev, f.nsocc, f.fock + f.heff, f.dm0, CUTOFFS)
    if "small" in which:
        yield ("synthetic(12,6)", *synthetic(12, 6), (1e-12,))


def pt2_rows(lib, opts, which, budget):
    """the lines of --pt2"""
    rows = []
    for name, fr, o, h, dm0, _ in fragments(lib, which):
        for eps in next(v for k, v in PT2_CUTOFFS.items() if name.startswith(k)):
            so = default_sci_opts(lib, eps_var=eps, max_det=MAX_DET)
            fr.solve_sci(o, h, dm0, opts=opts, sci_opts=so, eeval=False)      # (warm-up: the pool and the code objects)
            t0 = time.perf_counter()
            r = fr.solve_sci(o, h, dm0, opts=opts, sci_opts=so, eeval=False)
            solve_ms = 1e3 * (time.perf_counter() - t0)
            for eps_pt in (eps / 100, eps / 1000):
                ts, res = [], None
                while len(ts) < 5 and (len(ts) < 1 or ts[0] < 100.0 * budget):
                    t0 = time.perf_counter()
                    res = fr.sci_pt2(eps_pt)
                    ts.append(1e3 * (time.perf_counter() - t0))
                ms = statistics.median(ts)
                rows.append(dict(kind="pt2", fragment=name, eps=eps, eps_pt=eps_pt, ndet=r["ndet"], e_corr_sci=r["e_corr_mo"], e_pt2=res["e_pt2"], n_ext=res["n_ext"],
                                 batches=res["batches"], pt2_ms=ms, stage_ms=res["ms"], solve_ms=solve_ms, pt2_over_solve=ms / solve_ms, repeats=len(ts)))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    argv = [a for a in sys.argv[1:] if a != "--pt2"]
    pt2 = "--pt2" in sys.argv[1:]
    out = Path(argv[0]) if len(argv) > 0 else ROOT / "profiles" / "sci_bench.jsonl"
    budget = float(argv[1]) if len(argv) > 1 else 600.0
    which = argv[2].split(",") if len(argv) > 2 else ["synthetic", "octane", "small"]
    lib = _lib.init()
    opts = default_opts(lib, strict_convergence=0)
    if pt2:
        rows = pt2_rows(lib, opts, which, budget)
        same = {(r["fragment"], r["eps"], r["eps_pt"]) for r in rows}
        lines = [ln for ln in (out.read_text().splitlines() if out.exists() else []) if ln.strip()]
        kept = [ln for ln in lines if not (json.loads(ln).get("kind") == "pt2" and (json.loads(ln)["fragment"], json.loads(ln)["eps"], json.loads(ln)["eps_pt"]) in same)]
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("".join(ln + "\n" for ln in kept) + "".join(json.dumps(r) + "\n" for r in rows))
        return
    rows = []
    for name, fr, o, h, dm0, cutoffs in fragments(lib, which):
        e_ccsd = fr.solve(o, h, dm0, opts=opts, eeval=False)["e_corr_mo"]
        for eps in cutoffs:
            so = default_sci_opts(lib, eps_var=eps, max_det=MAX_DET)

            def sci():
                r = fr.solve_sci(o, h, dm0, opts=opts, sci_opts=so, eeval=False)
                return r, fr.sci_stage_ms()
            try:
                ms, r, warm, reps, st = timed(sci, budget)
            except _lib.QembError as e:      # (a row the limits refuse is a result too)
                rows.append(dict(fragment=name, eps=eps, max_det=MAX_DET, e_corr_ccsd=e_ccsd, refused=str(e)))
                print(json.dumps(rows[-1]), flush=True)
                continue
            row = dict(fragment=name, eps=eps, max_det=MAX_DET, ndet=r["ndet"], rounds=r["rounds"], nnz=r["nnz"], e_corr_sci=r["e_corr_mo"], e_corr_ccsd=e_ccsd,
                       residual=r["residual"], applications_of_H=r["n_iter"], solve_ms=ms, stage_ms=st, dominant_stage=max(st, key=st.get), warmups=warm, repeats=reps)
            if fr.n <= 14:
                fms, fr_, fwarm, freps, _ = timed(lambda: (fr.solve_fci(o, h, opts=opts, eeval=False), {}), budget)
                row.update(fci_solve_ms=fms, e_corr_fci=fr_["e_corr_mo"], fci_repeats=freps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    # the groups of rows may come from separate runs: rows of the fragments measured now replace those the file had, the others stay
    kept = [ln for ln in (out.read_text().splitlines() if out.exists() else []) if ln.strip() and (json.loads(ln).get("kind") == "pt2" or json.loads(ln)["fragment"] not in {r["fragment"] for r in rows})]
    out.write_text("".join(ln + "\n" for ln in kept) + "".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
