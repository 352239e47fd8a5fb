"""be_func / solve_error / solve_ccsd -- host mirror of molbe/solver.py over the device fragment solver.

`be_func` keeps the reference's signature (molbe/solver.py:244-257) for solver == "CCSD", solver == "MP2"
(:313-317) and solver == "FCI-hip" -- the reference's FCI branch (:339-342, :507-528) as a determinant-space solver on
the device; every other solver string of the reference (the bare "FCI", SCI, DMRG, ...) raises
ValueError("Solver not implemented") exactly like the reference's final else (:490-491).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import SolverOpts
from .fragsolver import SOLVERS, DeviceFragment, default_opts


class ErrorMap:
    """Static index map of solve_error (molbe/solver.py:683-778): which (fragment, row, col) of the fragment 1-RDMs
    feed each slot of err_edge / err_cen.  Built once; evaluating the residual is then two gathers -- and in the
    multi-GPU sweep the same map tells each rank which slots of the all-reduce buffer it owns."""

    def __init__(self, Fobjs):
        ef, er, ec = [], [], []
        cf, cr, cc = [], [], []
        cenf, ceni = [], []
        for fidx, f in enumerate(Fobjs):
            for edge in f.relAO_per_edge:
                for j in range(len(edge)):
                    for k in range(j, len(edge)):
                        ef.append(fidx); er.append(edge[j]); ec.append(edge[k])
            for i in f.weight_and_relAO_per_center[1]:
                cenf.append(fidx); ceni.append(i)
        for f in Fobjs:
            for cidx, cens in enumerate(f.relAO_in_ref_per_edge):
                ref = f.ref_frag_idx_per_edge[cidx]
                for j in range(len(cens)):
                    for k in range(j, len(cens)):
                        cf.append(ref); cr.append(cens[j]); cc.append(cens[k])
        self.edge = (np.array(ef, dtype=int), np.array(er, dtype=int), np.array(ec, dtype=int))
        self.cen = (np.array(cf, dtype=int), np.array(cr, dtype=int), np.array(cc, dtype=int))
        self.diag = (np.array(cenf, dtype=int), np.array(ceni, dtype=int))
        if len(self.edge[0]) != len(self.cen[0]):
            raise ValueError("edge / centre matching lists have different lengths")
        self.n_match = len(self.edge[0])

    def fill(self, Fobjs, owned, edge_vals, cen_vals):
        """Add the contributions of the fragments in `owned` to the (zero-initialised) buffers; returns the
        centre-diagonal partial sum (the chemical-potential condition)."""
        owned = set(owned)
        tr = 0.0
        f, r, c = self.edge
        for s in range(self.n_match):
            if f[s] in owned:
                edge_vals[s] += Fobjs[f[s]]._rdm1[r[s], c[s]]
        f, r, c = self.cen
        for s in range(self.n_match):
            if f[s] in owned:
                cen_vals[s] += Fobjs[f[s]]._rdm1[r[s], c[s]]
        f, i = self.diag
        for s in range(len(f)):
            if f[s] in owned:
                tr += Fobjs[f[s]]._rdm1[i[s], i[s]]
        return tr


def solve_error(Fobjs, Nocc, only_chem=False, rdm1_list=None):
    """molbe/solver.py:683-778: (norm, err_vec).  err_vec = [edge elements ..., sum centre diag / nkpt] -
    [centre elements read from the reference fragments ..., Nocc]; norm = sqrt(mean(err^2))."""
    if rdm1_list is not None:
        class _V:  # lightweight view so that ErrorMap can index `._rdm1`
            def __init__(self, f, r):
                self.__dict__.update(f.__dict__); self._rdm1 = r
        Fobjs = [_V(f, r) for f, r in zip(Fobjs, rdm1_list)]
    emap = ErrorMap(Fobjs)
    edge = np.zeros(emap.n_match); cen = np.zeros(emap.n_match)
    tr = emap.fill(Fobjs, range(len(Fobjs)), edge, cen) / Fobjs[0].unitcell_nkpt
    if only_chem:
        err = tr - Nocc
        return abs(err), np.asarray([err])
    err_vec = np.append(edge, tr) - np.append(cen, Nocc)
    return float(np.mean(err_vec * err_vec) ** 0.5), err_vec


@dataclass(frozen=True)
class SHCI_ArgsUser:
    """the reference's user arguments of its selected-CI branch (molbe/solver.py), read by solver="SCI-hip": hci_cutoff is the threshold eps_var on |H_ai c_i|.
    hci_pt and return_frag_data are not built: NotImplementedError.  The perturbative correction is a call of its own after the sweep, BE.sci_pt2."""
    hci_cutoff: float = 0.001
    hci_pt: bool = False
    return_frag_data: bool = False


def sci_opts_from_args(solver, solver_args, lib=None):
    """qemb_sci_opts of a sweep with `solver_args`: None unless solver == "SCI-hip" (the other solvers do not read the argument) or when it is None (the library's
    defaults); a SHCI_ArgsUser gives eps_var = hci_cutoff; anything else is a TypeError.
    Without a library only the checks are made."""
    if solver != "SCI-hip" or solver_args is None:
        return None
    if not isinstance(solver_args, SHCI_ArgsUser):
        raise TypeError(f"solver_args of solver='SCI-hip' must be a SHCI_ArgsUser or None, not {type(solver_args).__name__}")
    if solver_args.hci_pt:
        raise NotImplementedError("SCI-hip: the perturbative correction inside a sweep (hci_pt) is not implemented; call BE.sci_pt2 after the sweep")
    if solver_args.return_frag_data:
        raise NotImplementedError("SCI-hip: return_frag_data is not implemented")
    if lib is None:      # (the checks alone: be_func refuses a bad argument before any fragment is solved)
        return None
    from .fragsolver import default_sci_opts
    return default_sci_opts(lib, eps_var=float(solver_args.hci_cutoff))


def _solve_fragment(name, solver, keys, h, eri_s4, nsocc, dm0, *, n_frag, rdm_return, rdm2_return, use_cumulant, opts, lib, df_factor=None, fci_opts=None, sci_opts=None,
                    slab_rows=0, pt2_eps=None, triples=False):
    """What solve_ccsd / solve_mp2 / solve_fci share: a fragment with its ERIs (or living on its 3-index factor) is created, solved without energies and freed.
    Returns (out[keys[0]], out[keys[1]]), then rdm1_mo and mo_coeff with rdm_return; rdm2_return: the 2-RDM of the solve takes the place of mo_coeff
    (solver.py:940-942), or is appended without rdm_return.  pt2_eps (read for "SCI-hip" alone): the second-order correction at that threshold is the last element;
    triples (read for "CCSD" alone): E_(T) is the last element."""
    fr = DeviceFragment(h.shape[0], n_frag, lib=lib)
    try:
        if eri_s4 is not None:
            fr.set_eri_s4(eri_s4)
            if df_factor is not None:
                fr.set_df_factor(df_factor)
        elif df_factor is not None:
            fr.set_df_only(df_factor)
        else:
            raise ValueError(f"{name} needs the fragment ERIs or their 3-index factor")
        if slab_rows:
            fr.set_fci_slab(slab_rows)
        out = fr.solve_as(solver, nsocc, h, dm0, opts=opts, eeval=False, want_amplitudes=True, fci_opts=fci_opts, sci_opts=sci_opts)
        rdm2 = fr.make_rdm2(solver, with_dm1=not use_cumulant) if rdm2_return else None
        tail = () if pt2_eps is None else (fr.sci_pt2(pt2_eps)["e_pt2"],)
        if triples:
            tail = (fr.ccsd_t()["e_t"],)
    finally:
        fr.free()
    head = (out[keys[0]], out[keys[1]])
    if rdm_return:
        return (*head, out["rdm1_mo"], rdm2 if rdm2_return else out["mo_coeff"], *tail)
    return (*head, rdm2, *tail) if rdm2_return else (*head, *tail)


def solve_ccsd(h, eri_s4, nsocc, dm0=None, *, n_frag=0, rdm_return=False, rdm2_return=False, relax=False, use_cumulant=True,
               opts=None, lib=None, triples=False):
    """Device counterpart of solve_ccsd (molbe/solver.py:829-946).  The reference takes a PySCF mean-field object;
    here the fragment RHF is part of the device call, so the inputs are what `get_scfObj` would have been given:
    h = fock + heff, the 4-fold packed fragment ERIs, nsocc and dm0.
    Returns (t1, t2) or (t1, t2, rdm1_mo, mo_coeff) with rdm_return.  rdm2_return: the fragment 2-RDM in the MO basis,
    make_rdm2_urlx(t1, t2, with_dm1=not use_cumulant), assembled on the device, takes the place of mo_coeff -- (t1, t2, rdm1_mo, rdm2) as
    solver.py:940-942 -- or is appended to (t1, t2) without rdm_return.  Unrelaxed only: with relax it raises NotImplementedError.  The energies of a sweep never need it: `Frags.solve` contracts it in place.
    triples: the perturbative triples correction E_(T) of the solve (DeviceFragment.ccsd_t) is appended as the last element -- the triples energy of this
    embedding problem, a diagnostic contained in none of the other results."""
    if relax:
        opts = SolverOpts.from_buffer_copy(opts) if opts is not None else default_opts(lib)
        opts.relax_density = 1
    return _solve_fragment("solve_ccsd", "CCSD", ("t1", "t2"), h, eri_s4, nsocc, dm0, n_frag=n_frag, rdm_return=rdm_return, rdm2_return=rdm2_return,
                           use_cumulant=use_cumulant, opts=opts, lib=lib, triples=triples)


def solve_mp2(h, eri_s4, nsocc, dm0=None, *, n_frag=0, rdm_return=False, rdm2_return=False, use_cumulant=True, df_factor=None, opts=None, lib=None):
    """Device counterpart of solve_mp2 (molbe/solver.py:781-826) with the inputs of `solve_ccsd` above: h = fock + heff, the 4-fold packed
    fragment ERIs (or None with `df_factor`, the 3-index factor (naux, npair(n)) the fragment then lives on), nsocc and dm0.
    Returns (e_corr, t2) or (e_corr, t2, rdm1_mo, mo_coeff) with rdm_return; rdm1_mo is PySCF's unrelaxed mp2.make_rdm1.  rdm2_return: the
    fragment 2-RDM in the MO basis (mp2.make_rdm2, or its dovov part alone with use_cumulant) in the place `solve_ccsd` gives it."""
    return _solve_fragment("solve_mp2", "MP2", ("e_corr_mo", "t2"), h, eri_s4, nsocc, dm0, n_frag=n_frag, rdm_return=rdm_return, rdm2_return=rdm2_return,
                           use_cumulant=use_cumulant, opts=opts, lib=lib, df_factor=df_factor)


def solve_fci(h, eri_s4, nsocc, dm0=None, *, n_frag=0, rdm_return=False, rdm2_return=False, use_cumulant=True, df_factor=None, opts=None, fci_opts=None, lib=None,
              slab_rows=0):
    """Device counterpart of the reference's FCI branch (molbe/solver.py:339-342: fci.FCI(mf, mo_coeff).kernel(), make_rdm1, make_rdm2) with the inputs of
    `solve_mp2` above.  Returns (e_fci, civec) -- the eigenvalue of h = fock + heff with the fragment ERIs and the (ns, ns) vector -- or
    (e_fci, civec, rdm1_mo, mo_coeff) with rdm_return; rdm2_return: make_rdm2 (minus its mean-field part with use_cumulant) in the place `solve_ccsd` gives it.
    slab_rows: the work matrices D and G in slabs of that many alpha strings (DeviceFragment.set_fci_slab: 0 off, -1 automatic)."""
    return _solve_fragment("solve_fci", "FCI-hip", ("e_fci", "civec"), h, eri_s4, nsocc, dm0, n_frag=n_frag, rdm_return=rdm_return, rdm2_return=rdm2_return,
                           use_cumulant=use_cumulant, opts=opts, lib=lib, df_factor=df_factor, fci_opts=fci_opts, slab_rows=slab_rows)


def solve_sci(h, eri_s4, nsocc, dm0=None, *, n_frag=0, rdm_return=False, rdm2_return=False, use_cumulant=True, df_factor=None, opts=None, sci_opts=None, lib=None,
              pt2_eps=None):
    """Device counterpart of the reference's selected-CI branch (molbe/solver.py:412-462) with the inputs of `solve_fci` above.  Returns (e_sci, dets) -- the
    eigenvalue in the selected space and (alpha, beta, c), the occupation words of the final space sorted by (alpha, beta) with the vector -- or
    (e_sci, dets, rdm1_mo, mo_coeff) with rdm_return; rdm2_return: the 2-RDM (minus its mean-field part with use_cumulant) in the place `solve_ccsd` gives it.
    pt2_eps: with a value, the screened Epstein-Nesbet second-order correction at that threshold (DeviceFragment.sci_pt2) is appended as the last element -- a
    diagnostic of the cutoff, contained in none of the other results."""
    return _solve_fragment("solve_sci", "SCI-hip", ("e_sci", "dets"), h, eri_s4, nsocc, dm0, n_frag=n_frag, rdm_return=rdm_return, rdm2_return=rdm2_return,
                           use_cumulant=use_cumulant, opts=opts, lib=lib, df_factor=df_factor, sci_opts=sci_opts, pt2_eps=pt2_eps)


def sci_work_bytes(n, o, max_det=1 << 20, max_space=12):
    """qemb_frag_sci_bytes restated: what max_det fixes of the working set of solver="SCI-hip" (the CSR arrays, 12 bytes per stored element, come on top)"""
    from math import comb
    v = n - o
    nexc = 2 * o * v + 2 * comb(o, 2) * comb(v, 2) + (o * v) ** 2
    cap = 1 << 20
    while cap < 2 * nexc:
        cap <<= 1
    return float(3 * 24 * max_det + cap * 28 + 4096 * 256 * 12 + 8 * (2 * max_space + 4) * max_det + 20 * max_det + 8 * (4 * n ** 4 + 2 * n * n))


def fragment_work_bytes(n, o=None, solver="CCSD", naux=None, slab_rows=0):
    """Device memory ONE fragment in flight takes beside its resident ERIs: the two n^2 x npair buffers of the
    embedding->MO transformation (rows at a stride of whole 128-byte lines), the (+/-) pair-packed ladder operands, the ovvv block with its
    packed images, and ~30 tensors of the size of t2.  Without n_occ the worst split (n_occ = n / 4) is assumed.
    solver="FCI-hip" (csrc/fci.cpp; qemb_frag_fci_bytes with the default max_space = 12): D and G (2 x 8 n^2 N_det), 28 vectors of N_det, the tables and the n^4
    pieces; without n_occ the worst split (n_occ = n / 2) is assumed.  slab_rows > 0 (read by this solver alone; qemb_frag_fci_bytes_slab): D and G at
    2 x 8 n^2 min(slab_rows, ns) ns.
    solver="MP2" (factor route, csrc/mp2.cpp): the unpacked factor and its half-rotated virtual columns while Lov is formed (naux n^2 + naux n v), then
    Lov, Y and its transpose (naux o v each) and three o^2 v^2 tensors (ovov, t2, G); naux = 3 n when not given."""
    if solver not in SOLVERS:
        raise ValueError("Solver not implemented")
    n = int(n)
    if solver == "SCI-hip":      # (csrc/sci.cpp; qemb_frag_sci_bytes with the default max_det = 2^20 and max_space = 12; without n_occ: n_occ = n / 2)
        return sci_work_bytes(n, max(1, n // 2) if o is None else int(o))
    if solver == "FCI-hip":
        from math import comb
        o = max(1, n // 2) if o is None else int(o)
        ns = comb(n, o)
        rows = ns if int(slab_rows) <= 0 else min(int(slab_rows), ns)
        return 8.0 * (2.0 * n * n * rows * ns + 28.0 * ns * ns + 8.0 * n ** 4) + 4.0 * ns * (o * (n - o + 1) + 1)
    o = max(1, n // 4) if o is None else int(o)
    v = max(n - o, 1)
    if solver == "MP2":
        naux = 3 * n if naux is None else int(naux)
        return 8.0 * (max(float(naux) * n * (n + v), 3.0 * (o * v) ** 2 + 2.0 * naux * o * v) + naux * o * v)
    ld = (n + 15) // 16 * 16
    npair = n * (n + 1) // 2
    pv, qv = v * (v + 1) // 2, v * (v - 1) // 2
    return 8.0 * (2.0 * n * ld * npair + pv * pv + qv * qv + 2.0 * o * v ** 3 + 30.0 * (o * v) ** 2)


def sweep_mode(frags, nstreams=None, lockstep=None, mem_free=None, solver="CCSD"):
    """How the fragments of a sweep share the GPU when the caller leaves it open (BE(..., nstreams=None, lockstep=None)):
    many small fragments (>= 4 of at most 64 embedding orbitals: launch bound) advance in lock step -- one grouped launch per
    operation for all of them;
    otherwise several fragments are in flight on separate streams: up to six small ones, up to four of at most 256 orbitals, two beyond --
    and never more than the device memory that is free (`mem_free` bytes; taken from the fragments' library when they are on a device)
    holds working sets of (fragment_work_bytes): a calculation that fits one fragment at a time keeps fitting with the default.
    Measured on octane/STO-3G: BE2 (six fragments of ~42 orbitals) 40 ms serial, 18.3 ms six streams, 16.7 ms lock step; BE3 (four of ~55) 41 / 28 / 29 ms.
    Every mode returns bit-identical results."""
    frags = list(frags)
    nmax = max((int(f.nao) for f in frags), default=0)
    if lockstep is None:          # (an explicit nstreams is a request for that many streams, not for the lock step)
        # (round 4: four fragments of 36 orbitals -- the periodic configs[4] cell -- run 6.8 ms in lock step against 9.5 ms on four streams;
        #  four of ~55, octane BE3, tie at 28-29 ms)
        # (round 5: with the update's parallel regions four fragments of ~55 orbitals -- octane BE3 -- run 26.5 ms in lock step against 28.7 ms on four streams)
        lockstep = nstreams is None and len(frags) >= 4 and nmax <= 64
    if nstreams is None:
        nstreams = 1 if len(frags) <= 1 else (min(6, len(frags)) if nmax <= 96 else min(4 if nmax <= 256 else 2, len(frags)))
        if nstreams > 1 and nmax > 96:
            if mem_free is None:
                mem_free = _device_free_bytes(frags)
            if mem_free is not None:
                work = max(fragment_work_bytes(f.nao, getattr(f, "nsocc", None), solver=solver) for f in frags)
                nstreams = max(1, min(nstreams, int(0.9 * mem_free // work)))
    return int(nstreams), bool(lockstep)


def _device_free_bytes(frags):
    """free device memory as the fragments' library reports it (qemb_mem_info) plus nothing else: blocks the library has parked count as used,
    so the bound errs on the side of fewer fragments in flight.  None when the fragments are not on a device (host-logic tests)."""
    import ctypes as C
    dev = next((getattr(f, "dev", None) for f in frags if getattr(f, "dev", None) is not None), None)
    lib = getattr(dev, "lib", None)
    if lib is None or not hasattr(lib, "qemb_mem_info"):
        return None
    free_b, total_b = C.c_size_t(), C.c_size_t()
    try:
        if hasattr(lib, "qemb_trim"):
            lib.qemb_trim()                      # parked work space of earlier sweeps is free for this decision
        if lib.qemb_mem_info(C.byref(free_b), C.byref(total_b)) != 0:
            return None
    except Exception:  # noqa: BLE001
        return None
    return float(free_b.value)


def set_cu_partition(lib, parts):
    """Spread the execution contexts that `map_fragments` creates from now on over `parts` disjoint, interleaved sets of compute units (qemb_ctx_partition; 0 or 1:
    every context on the whole chip).  Two parts with four large fragments in flight let the HBM-bound passes of one fragment run beside the MFMA-bound products of
    another: +0.7-2 % on the n = 220 sweep by box (small, launch-bound fragments lose: leave them on the whole chip).  Call it between sweeps: contexts that exist
    are drained and get new streams."""
    from ._lib import check
    check(lib.qemb_ctx_partition(int(parts)), "qemb_ctx_partition", lib)


def map_fragments(fn, frags, nstreams=1):
    """[fn(f) for f in frags], with up to `nstreams` fragments in flight at once: each worker thread is bound to its own
    execution context of the library (HIP stream + workspaces, qemb_ctx_bind), so fragments whose kernels are latency bound
    overlap on the device.  The reference overlaps fragments with a process pool (be_parallel.py:484-513)."""
    frags = list(frags)
    if nstreams <= 1 or len(frags) <= 1:
        return [fn(f) for f in frags]
    from concurrent.futures import ThreadPoolExecutor
    lib = frags[0].dev.lib
    have = lib.qemb_ctx_count(int(nstreams) + 1)          # context 0 stays with the calling thread
    if have < 0:
        from ._lib import check
        check(have, "qemb_ctx_count", lib)
    nwork = min(int(nstreams), have - 1, len(frags))
    if nwork <= 1:
        return [fn(f) for f in frags]
    # STATIC assignment of fragments to worker contexts (longest first, each to the least loaded worker; ties in fragment order): the same
    # fragment meets the same context in every sweep.  The caching allocator of a context hands blocks back by exact size, so a context
    # that gets a fragment of another size than last time misses its pool and goes to the driver (hipMalloc of a solve's ~10^3 buffers:
    # tens of ms) -- with a dynamic queue that happened now and then in any sweep (the 92 ms sweep of the round-3 octane figures,
    # tools/octane_sweep_series.py), with the static assignment only in the first one.
    def cost(f):
        n, o = int(getattr(f, "nao", 0) or 0), getattr(f, "nsocc", None)
        o = n // 2 if o is None else int(o)
        v = max(n - o, 0)
        return float(o * o) * float(v) ** 4 + 4.0 * float(o * v) ** 3
    order = sorted(range(len(frags)), key=lambda k: (-cost(frags[k]), k))
    load, mine = [0.0] * nwork, [[] for _ in range(nwork)]
    for k in order:
        w = min(range(nwork), key=lambda j: (load[j], j))
        mine[w].append(k); load[w] += max(cost(frags[k]), 1.0)

    from ._lib import QEMB_ERR_ALLOC, QembError, check
    res, retry = [None] * len(frags), []

    def work(w):
        check(lib.qemb_ctx_bind(w + 1), "qemb_ctx_bind", lib)
        out = []
        for k in mine[w]:
            try:
                out.append((k, fn(frags[k]), None))
            except QembError as e:
                if getattr(e, "status", None) != QEMB_ERR_ALLOC:
                    raise
                out.append((k, None, e))
        return out
    with ThreadPoolExecutor(max_workers=nwork) as pool:
        for part in pool.map(work, range(nwork)):
            for k, r, err in part:
                if err is not None:
                    retry.append(k)
                else:
                    res[k] = r
    if retry:
        # the working sets of `nwork` fragments did not fit together: what fits one fragment at a time must keep working (the serial sweep
        # is what nstreams = 1 runs); parked blocks of every context are released first
        import warnings
        warnings.warn(f"{len(retry)} fragment(s) ran out of device memory with {nwork} in flight; solving them one at a time", RuntimeWarning, stacklevel=2)
        if hasattr(lib, "qemb_trim"):
            lib.qemb_trim()
        for k in retry:
            res[k] = fn(frags[k])
    return res


def solve_fragments(pot, frags, only_chem=False, opts=None, eeval=False, use_cumulant=True, relax_density=False, nstreams=1, lockstep=False,
                    stats=None, solver="CCSD", solver_args=None):
    """The loop body of be_func (molbe/solver.py:301-547) for the fragments `frags`: update_heff, then the device solve of each.
    nstreams > 1: that many fragments in flight on separate streams (map_fragments).  lockstep: ALL fragments in one library call
    (qemb_frag_solve_batch) -- their CCSD iterations advance together, every operation one grouped launch; the small-fragment regime
    (octane BE2 / BE3), where a fragment alone is bound by its ~110 dependent launches per iteration.  Same results, bit for bit.
    solver="MP2": the MP2 branch of the loop body (solver.py:313-317); `lockstep` then takes qemb_frag_solve_mp2_batch and relax_density is not read.
    solver="FCI-hip": the FCI branch (solver.py:339-342); there is no batched entry -- with `lockstep` the fragments run one by one, or on `nstreams` streams;
    relax_density is not read.
    solver="SCI-hip": the selected-CI branch (solver.py:412-462) with `solver_args` (SHCI_ArgsUser or None); the fragments run as those of "FCI-hip" do."""
    if solver not in SOLVERS:
        raise ValueError("Solver not implemented")
    if solver != "CCSD":
        relax_density = False
    frags = list(frags)
    if lockstep and len(frags) > 1 and solver not in ("FCI-hip", "SCI-hip"):
        from .fragsolver import solve_batch
        o_list = []
        for f in frags:
            if pot is not None:
                f.update_heff(pot, only_chem=only_chem)
            assert f.fock is not None and f.heff is not None
            o_list.append(f._solve_inputs(opts, eeval, relax_density))
        # one options struct for the batch: the per-fragment ones differ at most by relax_density, which _solve_inputs set identically
        outs = solve_batch([f.dev for f in frags], [f.nsocc for f in frags], [f.fock + f.heff for f in frags], [f.dm0 for f in frags],
                           opts=o_list[0], eeval=eeval, stats=stats, solver=solver)
        return [f._solve_outputs(out, eeval, use_cumulant, solver) for f, out in zip(frags, outs)]

    def one(fobj):
        if pot is not None:
            fobj.update_heff(pot, only_chem=only_chem)
        assert fobj.fock is not None and fobj.heff is not None
        return fobj.solve(opts=opts, eeval=eeval, use_cumulant=use_cumulant, relax_density=relax_density, solver=solver, solver_args=solver_args)
    return map_fragments(one, frags, nstreams)


def be_func(pot, Fobjs, Nocc, solver, enuc, solver_args=None, scratch_dir=None, only_chem=False, eeval=False,
            relax_density=False, return_vec=False, use_cumulant=True, *, opts=None, stats=None, nstreams=1, lockstep=False):
    """molbe/solver.py:244-562 for solver == 'CCSD', 'MP2' and 'FCI-hip' (relax_density is ignored for MP2 and FCI-hip: those branches of the reference never read it).  `opts` (qemb_solver_opts), `stats` (dict collecting per-sweep
    counters), `nstreams` (fragments in flight at once, see map_fragments) and `lockstep` (all fragments in one batched call, see
    solve_fragments) are additions; everything else has the reference's meaning."""
    if solver not in SOLVERS:
        raise ValueError("Solver not implemented")
    sci_opts_from_args(solver, solver_args)      # (a wrong type or an option that is not built is refused before any fragment is solved; read by "SCI-hip" alone)
    total_e = [0.0, 0.0, 0.0]
    n_iter = 0
    for out in solve_fragments(pot, Fobjs, only_chem, opts, eeval, use_cumulant, relax_density, nstreams, lockstep, stats, solver, solver_args):
        n_iter += out["n_iter"]
        if eeval:
            total_e = [a + b for a, b in zip(total_e, out["e_frag"])]
    if stats is not None:
        stats["ccsd_iterations"] = stats.get("ccsd_iterations", 0) + n_iter
        stats["fragments"] = stats.get("fragments", 0) + len(Fobjs)
    Ecorr = sum(total_e)
    if eeval and not return_vec:
        return (Ecorr, total_e)
    ernorm, ervec = solve_error(Fobjs, Nocc, only_chem=only_chem)
    if eeval:
        return (ernorm, ervec, [Ecorr, total_e])
    if return_vec:
        return (ernorm, ervec, None)
    return ernorm
