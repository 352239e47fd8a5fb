"""Python handle on one device-resident fragment (C ABI qemb_frag_* in include/qemb_hip.h).

This is the object `quemb_amd.pfrag.Frags` keeps in place of the reference's HDF5 dataset name + PySCF
objects: fragment ERIs stay in HBM between sweeps (the reference re-reads `eri_file.h5` every call --
molbe/helper.py:182-189, :303-304) and one `solve()` is the body of be_func's loop (molbe/solver.py:301-547).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FciOpts, SciOpts, SolverOpts, c_vp, check


def _p(a):
    return None if a is None else a.ctypes.data


def default_opts(lib=None, **kw) -> SolverOpts:
    lib = lib or _lib.init()
    o = SolverOpts()
    lib.qemb_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown solver option {k!r}")
        setattr(o, k, v)
    return o


def default_fci_opts(lib=None, **kw) -> FciOpts:
    """qemb_fci_opts with the library's defaults (conv_tol 1e-9 on the residual, max_cycle 100, max_space 12, lindep 1e-14), single fields changed by keyword"""
    lib = lib or _lib.init()
    o = FciOpts()
    lib.qemb_default_fci_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown FCI option {k!r}")
        setattr(o, k, v)
    return o


def default_sci_opts(lib=None, **kw) -> SciOpts:
    """qemb_sci_opts with the library's defaults (eps_var 1e-3, conv_tol 1e-9, max_cycle 100, max_space 12, max_round 30, max_det 2^20), single fields changed by keyword"""
    lib = lib or _lib.init()
    o = SciOpts()
    lib.qemb_default_sci_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown SCI option {k!r}")
        setattr(o, k, v)
    return o


def fci_ndet(n, nsocc):
    """N_det = C(n, nsocc)^2 determinants of the M_s = 0 space"""
    from math import comb
    return comb(int(n), int(nsocc)) ** 2


class DeviceFragment:
    def __init__(self, n: int, n_f: int, lib=None):
        self.lib = lib or _lib.init()
        self.n, self.n_f = int(n), int(n_f)
        h = c_vp()
        check(self.lib.qemb_frag_create(self.n, self.n_f, C.byref(h)), "qemb_frag_create", self.lib)
        self.h = h

    # ---- data --------------------------------------------------------------------------------
    def set_eri_s4(self, eri_s4: np.ndarray):
        npair = self.n * (self.n + 1) // 2
        a = np.ascontiguousarray(eri_s4, dtype=np.float64)
        if a.shape != (npair, npair):
            raise ValueError(f"fragment ERIs must be 4-fold packed ({npair},{npair}), got {a.shape}")
        check(self.lib.qemb_frag_set_eri_s4(self.h, a.ctypes.data), "qemb_frag_set_eri_s4", self.lib)

    def set_eri_s4_dev(self, dev_ptr: int):
        check(self.lib.qemb_frag_set_eri_s4_dev(self.h, dev_ptr), "qemb_frag_set_eri_s4_dev", self.lib)

    def set_df_factor(self, B: np.ndarray):
        """the fitted 3-index factor B (naux, npair(n)) with eri_s4 = B.T @ B (`bb` of molbe/eri_onthefly.py:141-143): solves then form their MO integrals
        from it while that is the cheaper route (qemb_frag_mo_route).  Call after set_eri_s4 (new ERIs drop the factor)."""
        npair = self.n * (self.n + 1) // 2
        a = np.ascontiguousarray(B, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != npair:
            raise ValueError(f"the 3-index factor must be (naux, {npair}), got {a.shape}")
        check(self.lib.qemb_frag_set_df_factor(self.h, int(a.shape[0]), a.ctypes.data), "qemb_frag_set_df_factor", self.lib)

    def set_df_factor_dev(self, dev_ptr: int, naux: int):
        check(self.lib.qemb_frag_set_df_factor_dev(self.h, int(naux), dev_ptr), "qemb_frag_set_df_factor_dev", self.lib)

    def set_df_only(self, B: np.ndarray):
        """the fragment lives on its 3-index factor B (naux, npair(n)) alone -- no 4-fold packed block resident (qemb_frag_set_df_only): J / K, MO integrals,
        energies and responses come from B; `get_eri_s4` forms B.T @ B on demand"""
        npair = self.n * (self.n + 1) // 2
        a = np.ascontiguousarray(B, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != npair:
            raise ValueError(f"the 3-index factor must be (naux, {npair}), got {a.shape}")
        check(self.lib.qemb_frag_set_df_only(self.h, int(a.shape[0]), a.ctypes.data), "qemb_frag_set_df_only", self.lib)

    def set_df_only_dev(self, dev_ptr: int, naux: int):
        check(self.lib.qemb_frag_set_df_only_dev(self.h, int(naux), dev_ptr), "qemb_frag_set_df_only_dev", self.lib)

    def resident_bytes(self) -> int:
        b = C.c_int64()
        check(self.lib.qemb_frag_resident_bytes(self.h, C.byref(b)), "qemb_frag_resident_bytes", self.lib)
        return int(b.value)

    def set_mo_route(self, route: int):
        """-1: the cheaper route (default), 0: four-index transformation of the packed block, 1: the 3-index factor"""
        check(self.lib.qemb_frag_mo_route(self.h, int(route)), "qemb_frag_mo_route", self.lib)

    def mo_route_used(self):
        """(the last solve formed its MO integrals from the factor, naux of the factor held -- 0: none)"""
        used, naux = C.c_int(), C.c_int()
        check(self.lib.qemb_frag_mo_route_used(self.h, C.byref(used), C.byref(naux)), "qemb_frag_mo_route_used", self.lib)
        return bool(used.value), int(naux.value)

    def get_eri_s4(self) -> np.ndarray:
        npair = self.n * (self.n + 1) // 2
        out = np.empty((npair, npair))
        check(self.lib.qemb_frag_get_eri_s4(self.h, out.ctypes.data), "qemb_frag_get_eri_s4", self.lib)
        return out

    def set_energy_data(self, h1, veff0, veff, weight, centers):
        h1 = np.ascontiguousarray(h1, dtype=np.float64)
        veff0 = np.ascontiguousarray(veff0, dtype=np.float64)
        veff = None if veff is None else np.ascontiguousarray(veff, dtype=np.float64)
        cen = np.ascontiguousarray(centers, dtype=np.int32)
        check(self.lib.qemb_frag_set_energy_data(self.h, h1.ctypes.data, veff0.ctypes.data, _p(veff), float(weight),
                                                 cen.ctypes.data_as(C.POINTER(C.c_int)), len(cen)), "qemb_frag_set_energy_data", self.lib)

    def jk(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64)
        J = np.empty((self.n, self.n)); K = np.empty((self.n, self.n))
        check(self.lib.qemb_frag_jk(self.h, P.ctypes.data, J.ctypes.data, K.ctypes.data), "qemb_frag_jk", self.lib)
        return J, K

    # ---- the sweep body -------------------------------------------------------------------------
    def solve(self, nsocc, h, dm0=None, opts: SolverOpts | None = None, eeval=True, want_t2=False):
        c = _SolveCall([self], [nsocc], [h], [dm0], opts, eeval, batch=False, t1=True, t2=want_t2)
        c.call("qemb_frag_solve", ("t1", "t2"))
        return c.results(lambda_iters=True)[0]

    def solve_mp2(self, nsocc, h, dm0=None, opts: SolverOpts | None = None, eeval=True, want_t2=False):
        """solver == "MP2" of be_func (qemb_frag_solve_mp2): fragment RHF -> density-fitted MP2 -> unrelaxed MP2 1-RDM -> fragment energies.
        The dict `solve` returns, with t1 = None and n_iter = 0; of `opts` only scf_*, verbose and strict_convergence are read."""
        c = _SolveCall([self], [nsocc], [h], [dm0], opts, eeval, batch=False, t2=want_t2)
        c.call("qemb_frag_solve_mp2", ("t2",), n_iter=False)
        return c.results()[0]

    def solve_fci(self, nsocc, h, dm0=None, opts: SolverOpts | None = None, fci_opts: FciOpts | None = None, eeval=True, want_civec=False):
        """solver == "FCI-hip" of be_func (qemb_frag_solve_fci): fragment RHF -> determinant-space FCI on the device -> make_rdm1 -> fragment energies from the cumulant
        of make_rdm2.  The dict `solve` returns with t1 = t2 = None, plus e_fci (the eigenvalue; e_corr_mo = e_fci - e_scf), residual (||H c - E c||_2), n_iter (the
        applications of H) and civec ((ns, ns), row = alpha string; None unless want_civec).  Of `opts` only scf_*, verbose and strict_convergence are read;
        fci_opts None: the defaults of `default_fci_opts`."""
        from math import comb
        n, o = self.n, int(nsocc)
        ns = comb(n, o) if 0 < o <= n else 1
        c = _SolveCall([self], [nsocc], [h], [dm0], opts, eeval, batch=False)
        c.outs[0]["civec"] = np.empty((ns, ns)) if want_civec and n <= 16 else None
        c.call("qemb_frag_solve_fci", ("civec",), after_opts=(None if fci_opts is None else C.byref(fci_opts),))
        resid = C.c_double()
        check(self.lib.qemb_frag_fci_residual(self.h, C.byref(resid)), "qemb_frag_fci_residual", self.lib)
        out = c.results()[0]
        out.update(e_fci=c.e[0], e_corr_mo=c.e[0] - c.e_scf[0], residual=resid.value)      # (this entry reports the eigenvalue where the others report e_corr_mo)
        return out

    def solve_sci(self, nsocc, h, dm0=None, opts: SolverOpts | None = None, sci_opts: SciOpts | None = None, eeval=True, want_dets=False):
        """solver == "SCI-hip" of be_func (qemb_frag_solve_sci): fragment RHF -> heat-bath selected CI on the device -> 1-RDM -> fragment energies from the cumulant of
        the 2-RDM.  The dict `solve` returns with t1 = t2 = None, plus e_sci (the eigenvalue; e_corr_mo = e_sci - e_scf), ndet, rounds, nnz (stored elements of H),
        residual (||H c - E c||_2 of the last diagonalisation), n_iter (applications of H over all rounds) and, with want_dets, dets = (alpha, beta, c): the final
        space as uint64 occupation words sorted by (alpha, beta) and its vector.  sci_opts None: the defaults of `default_sci_opts`."""
        c = _SolveCall([self], [nsocc], [h], [dm0], opts, eeval, batch=False)
        c.call("qemb_frag_solve_sci", (), after_opts=(None if sci_opts is None else C.byref(sci_opts),))
        ndet, rounds, nnz, resid = C.c_int64(), C.c_int(), C.c_int64(), C.c_double()
        check(self.lib.qemb_frag_sci_stats(self.h, C.byref(ndet), C.byref(rounds), C.byref(nnz), C.byref(resid)), "qemb_frag_sci_stats", self.lib)
        out = c.results()[0]
        out.update(e_sci=c.e[0], e_corr_mo=c.e[0] - c.e_scf[0], ndet=int(ndet.value), rounds=int(rounds.value), nnz=int(nnz.value), residual=resid.value)
        self._sci_e_var = out["e_sci"]      # (what `sci_pt2` reports beside its correction; the library keeps its own copy)
        if want_dets:
            a, b, v = np.empty(out["ndet"], dtype=np.uint64), np.empty(out["ndet"], dtype=np.uint64), np.empty(out["ndet"])
            check(self.lib.qemb_frag_sci_dets(self.h, a.ctypes.data, b.ctypes.data, v.ctypes.data), "qemb_frag_sci_dets", self.lib)
            out["dets"] = (a, b, v)
        return out

    def sci_stage_ms(self):
        """host wall time (ms) of the stages of the last `solve_sci`: dict(screen, merge, build, davidson, rdm)"""
        ms = (C.c_double * 5)()
        check(self.lib.qemb_frag_sci_stage_ms(self.h, ms), "qemb_frag_sci_stage_ms", self.lib)
        return dict(zip(("screen", "merge", "build", "davidson", "rdm"), (float(x) for x in ms)))

    def set_sci_mem_limit(self, nbytes):
        """device bytes `solve_sci` of this fragment may take (qemb_frag_sci_mem_limit); negative: whatever is free"""
        check(self.lib.qemb_frag_sci_mem_limit(self.h, int(nbytes)), "qemb_frag_sci_mem_limit", self.lib)

    def sci_pt2(self, eps_pt, max_ext=0):
        """the screened Epstein-Nesbet second-order correction of the last `solve_sci` of this fragment (qemb_frag_sci_pt2), from the determinants, the vector and e_sci
        it left on the device:  S_a = sum of the products H_ai c_i with |H_ai c_i| >= eps_pt,  e_pt2 = sum_a S_a^2 / (e_var - H_aa)  over the n_ext determinants
        outside the space with a passing product and their spin partners; denominators are not guarded.  Returns dict(e_var, e_pt2, n_ext, batches, ms) -- batches: the
        ranges of at most max_ext externals the sum ran in (max_ext = 0: the largest count that fits the memory), ms: dict(screen, merge, rows) of host wall time.
        e_var + e_pt2 tells whether the cutoff of the solve was small enough; it is a diagnostic of the embedding problem and is added to no fragment or BE energy
        (those come from the variational RDMs, as in the reference)."""
        e, next_, nb, ms = C.c_double(), C.c_int64(), C.c_int(), (C.c_double * 3)()
        check(self.lib.qemb_frag_sci_pt2(self.h, float(eps_pt), int(max_ext), C.byref(e), C.byref(next_), C.byref(nb), ms), "qemb_frag_sci_pt2", self.lib)
        return dict(e_var=self._sci_e_var, e_pt2=e.value, n_ext=int(next_.value), batches=int(nb.value), ms=dict(zip(("screen", "merge", "rows"), (float(x) for x in ms))))

    def solve_as(self, solver, nsocc, h, dm0=None, opts=None, eeval=True, want_amplitudes=False, fci_opts=None, sci_opts=None):
        """the solve of be_func's solver literal (one of SOLVERS): `solve`, `solve_mp2`, `solve_fci` or `solve_sci`.  want_amplitudes asks for t2 (the CI vector of
        "FCI-hip", the determinants and vector of "SCI-hip"); fci_opts is read by "FCI-hip" alone, sci_opts by "SCI-hip" alone"""
        if solver not in SOLVERS:
            raise ValueError("Solver not implemented")
        if solver == "SCI-hip":
            return self.solve_sci(nsocc, h, dm0, opts=opts, sci_opts=sci_opts, eeval=eeval, want_dets=want_amplitudes)
        if solver == "FCI-hip":
            return self.solve_fci(nsocc, h, dm0, opts=opts, fci_opts=fci_opts, eeval=eeval, want_civec=want_amplitudes)
        return (self.solve_mp2 if solver == "MP2" else self.solve)(nsocc, h, dm0, opts=opts, eeval=eeval, want_t2=want_amplitudes)

    def set_fci_mem_limit(self, nbytes):
        """device bytes `solve_fci` of this fragment may take (qemb_frag_fci_mem_limit); negative: whatever is free"""
        check(self.lib.qemb_frag_fci_mem_limit(self.h, int(nbytes)), "qemb_frag_fci_mem_limit", self.lib)

    def set_fci_slab(self, rows):
        """the slab height of `solve_fci` and of make_rdm2("FCI-hip") of this fragment (qemb_frag_fci_slab): 0 (default) off, k > 0 the work matrices D and G in
        slabs of k alpha strings (k >= ns: one slab), -1 unslabbed when that fits the memory limit, else the largest height that does"""
        check(self.lib.qemb_frag_fci_slab(self.h, int(rows)), "qemb_frag_fci_slab", self.lib)

    def fci_slab_used(self):
        """(rows, n_slab) of the last FCI solve or FCI 2-RDM call of this fragment (qemb_frag_fci_slab_used); unslabbed: (0, 1)"""
        rows, n_slab = C.c_int64(), C.c_int64()
        check(self.lib.qemb_frag_fci_slab_used(self.h, C.byref(rows), C.byref(n_slab)), "qemb_frag_fci_slab_used", self.lib)
        return int(rows.value), int(n_slab.value)

    def make_rdm2(self, kind="CCSD", with_dm1=True):
        """Frags.rdm2__ (molbe/solver.py:528) of the last solve of this fragment in the fragment-MO basis, (n, n, n, n): qemb_frag_rdm2.
        kind="CCSD": make_rdm2_urlx(t1, t2, with_dm1) (shared/external/ccsd_rdm.py:23-55) from the amplitudes `solve` left on the device;
        kind="MP2": PySCF's mp2.make_rdm2 (with_dm1=False: its dovov part) after `solve_mp2`.  One kernel writes the n^4 tensor on the device.
        kind="FCI-hip": make_rdm2 of the vector `solve_fci` left on the device (with_dm1=False: minus the mean-field part of molbe/solver.py:513-527).
        kind="SCI-hip": the same of the selected vector `solve_sci` left on the device.
        Relaxed (Lambda) 2-RDMs are not implemented: after a solve with relax_density this raises NotImplementedError."""
        if kind not in RDM2_KINDS:
            raise ValueError("Solver not implemented")
        n = self.n
        out = np.empty((n, n, n, n))
        try:
            check(self.lib.qemb_frag_rdm2(self.h, RDM2_KINDS[kind], int(bool(with_dm1)), out.ctypes.data), "qemb_frag_rdm2", self.lib)
        except _lib.QembError as e:
            if e.status == _lib.QEMB_ERR_UNSUPPORTED:
                raise NotImplementedError(str(e)) from None
            raise
        return out

    def ccsd_t(self):
        """the perturbative triples correction E_(T) of the last `solve` (CCSD, relaxed or not) of this fragment (qemb_frag_ccsd_t), from the t1 / t2 it left on
        the device, the orbital energies, and (ia|bc), (ia|jk), (ia|jb) formed again from the resident factor or block.  Closed shell, Fock = diag(mo_energy):
            g[i,j,k,a,b,c] = sum_f (ia|fb) t2[k,j,c,f] - sum_m (ia|mj) t2[m,k,b,c];   W = the sum of g over the six simultaneous permutations of (i,a), (j,b), (k,c);
            V = W + t1[i,a] (jb|kc) + t1[j,b] (ia|kc) + t1[k,c] (ia|jb);   E_(T) = 1/3 sum W r3(V) / (e_i + e_j + e_k - e_a - e_b - e_c)   (not guarded).
        Returns dict(e_t, tile, n_tile_triples, bytes, ms) -- the tile of the virtual orbitals the call chose, the tile triples A >= B >= C it visited, the device
        bytes of its working set, ms: dict(images, gemm, assemble, integrals).  The same bits on every call.  E_(T) is the triples energy of the EMBEDDING problem
        of this fragment, a diagnostic of what CCSD leaves out: it is added to no fragment or BE energy, and a centre-projected BE-level (T) energy is not formed."""
        e, tile, ntt, ms = C.c_double(), C.c_int(), C.c_int64(), (C.c_double * 4)()
        check(self.lib.qemb_frag_ccsd_t(self.h, C.byref(e), C.byref(tile), C.byref(ntt), ms), "qemb_frag_ccsd_t", self.lib)
        nbytes = self.ccsd_t_bytes(0, tile.value) if tile.value > 0 else 0
        return dict(e_t=e.value, tile=int(tile.value), n_tile_triples=int(ntt.value), bytes=nbytes, ms=dict(zip(("images", "gemm", "assemble", "integrals"), (float(x) for x in ms))))

    def ccsd_t_bytes(self, nsocc, tile):
        """device bytes `ccsd_t` takes with nsocc occupied orbitals (0: as many as the last solve had) and that tile of the virtual orbitals
        (qemb_frag_ccsd_t_bytes): the larger of the integral transformation and of the kept MO blocks with the images, the six product buffers and the partial sums"""
        b = C.c_int64()
        check(self.lib.qemb_frag_ccsd_t_bytes(self.h, int(nsocc), int(tile), C.byref(b)), "qemb_frag_ccsd_t_bytes", self.lib)
        return int(b.value)

    def drop_amplitudes(self):
        """releases the t1 / t2 (and Lambda multipliers) kept from the last CCSD solve (qemb_frag_drop_amplitudes): `make_rdm2("CCSD")` and `ccsd_t` are refused
        until the fragment is solved again"""
        check(self.lib.qemb_frag_drop_amplitudes(self.h), "qemb_frag_drop_amplitudes", self.lib)

    def set_ccsd_t_mem_limit(self, nbytes):
        """device bytes `ccsd_t` of this fragment may take (qemb_frag_ccsd_t_mem_limit); negative: whatever is free"""
        check(self.lib.qemb_frag_ccsd_t_mem_limit(self.h, int(nbytes)), "qemb_frag_ccsd_t_mem_limit", self.lib)

    def set_rdm2_mem_limit(self, nbytes):
        """device bytes `make_rdm2` of this fragment may take, tensor and workspace (qemb_frag_rdm2_mem_limit); negative: whatever is free"""
        check(self.lib.qemb_frag_rdm2_mem_limit(self.h, int(nbytes)), "qemb_frag_rdm2_mem_limit", self.lib)

    def scf(self, nsocc, h, dm0=None, opts=None):
        """Fragment RHF only (Frags.scf(fs=True)); returns dict(mo_coeff, mo_energy, J, K, e_scf, converged, cycles)."""
        n = self.n
        h = np.ascontiguousarray(h, dtype=np.float64)
        dm0 = None if dm0 is None else np.ascontiguousarray(dm0, dtype=np.float64)
        opts = opts or default_opts(self.lib)
        mo = np.empty((n, n)); eps = np.empty(n); J = np.empty((n, n)); K = np.empty((n, n))
        e = C.c_double(); conv = C.c_int(); cyc = C.c_int()
        check(self.lib.qemb_frag_scf(self.h, int(nsocc), h.ctypes.data, _p(dm0), C.byref(opts), mo.ctypes.data, eps.ctypes.data,
                                     J.ctypes.data, K.ctypes.data, C.byref(e), C.byref(conv), C.byref(cyc)), "qemb_frag_scf", self.lib)
        return dict(mo_coeff=mo, mo_energy=eps, J=J, K=K, e_scf=e.value, converged=bool(conv.value), cycles=cyc.value)

    def cphf(self, nsocc, h, vpots, dm0=None, opts=None):
        """Density responses dP_p (npot, n, n) to the one-body perturbations vpots (npot, n, n)."""
        n = self.n
        h = np.ascontiguousarray(h, dtype=np.float64)
        v = np.ascontiguousarray(vpots, dtype=np.float64).reshape(-1, n, n)
        dm0 = None if dm0 is None else np.ascontiguousarray(dm0, dtype=np.float64)
        opts = opts or default_opts(self.lib)
        out = np.empty_like(v)
        check(self.lib.qemb_frag_cphf(self.h, int(nsocc), h.ctypes.data, _p(dm0), C.byref(opts), v.ctypes.data, v.shape[0],
                                      out.ctypes.data), "qemb_frag_cphf", self.lib)
        return out

    # ---- measurement hooks ---------------------------------------------------------------------------
    def prepare_ccsd(self, nsocc, h, dm0=None, opts=None):
        h = np.ascontiguousarray(h, dtype=np.float64)
        dm0 = None if dm0 is None else np.ascontiguousarray(dm0, dtype=np.float64)
        opts = opts or default_opts(self.lib)
        check(self.lib.qemb_frag_prepare_ccsd(self.h, int(nsocc), h.ctypes.data, _p(dm0), C.byref(opts)), "qemb_frag_prepare_ccsd", self.lib)

    def ccsd_iterate(self, niter=1):
        e, nt = C.c_double(), C.c_double()
        check(self.lib.qemb_frag_ccsd_iterate(self.h, int(niter), C.byref(e), C.byref(nt)), "qemb_frag_ccsd_iterate", self.lib)
        return e.value, nt.value

    def ccsd_export(self, name: str, shape):
        out = np.empty(shape)
        check(self.lib.qemb_frag_ccsd_export(self.h, name.encode(), out.ctypes.data, out.size), "qemb_frag_ccsd_export", self.lib)
        return out

    def ccsd_reset(self):
        check(self.lib.qemb_frag_ccsd_reset(self.h), "qemb_frag_ccsd_reset", self.lib)

    def free(self):
        if getattr(self, "h", None):
            self.lib.qemb_frag_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


RDM2_KINDS = {"CCSD": 0, "MP2": 1, "FCI-hip": 2, "SCI-hip": 3}      # QEMB_RDM2_CCSD, _MP2, _FCI, _SCI (include/qemb_hip.h)
SOLVERS = ("CCSD", "MP2", "FCI-hip", "SCI-hip")                      # the solver literals of be_func; everything else (the bare "FCI" and "SCI" included) is refused


def ccsd_t(t1, t2, ovvv, ovoo, ovov, eo, ev, tile=8, lib=None):
    """E_(T) of handed-in amplitudes and MO blocks (qemb_op_ccsd_t; the expression is in DeviceFragment.ccsd_t): t1 (o, v), t2 (o, o, v, v), ovvv (o, v, v, v) =
    (ia|bc), ovoo (o, v, o, o) = (ia|jk), ovov (o, v, o, v) = (ia|jb), eo (o,), ev (v,); tile: the tile of the virtual orbitals, forced (cut to v)."""
    from ._lib import DeviceBuffer
    lib = lib or _lib.init()
    t1 = np.ascontiguousarray(t1, dtype=np.float64)
    o, v = t1.shape
    shapes = dict(t2=(o, o, v, v), ovvv=(o, v, v, v), ovoo=(o, v, o, o), ovov=(o, v, o, v), eo=(o,), ev=(v,))
    arrs = dict(t2=t2, ovvv=ovvv, ovoo=ovoo, ovov=ovov, eo=eo, ev=ev)
    for k, a in arrs.items():
        if np.shape(a) != shapes[k]:
            raise ValueError(f"ccsd_t: {k} must have the shape {shapes[k]}, not {np.shape(a)}")
    if int(tile) < 1:
        raise ValueError("ccsd_t: tile must be at least 1")
    bufs = [DeviceBuffer.from_numpy(a, lib=lib) for a in (t1, t2, ovvv, ovoo, ovov, eo, ev)]
    try:
        e = C.c_double()
        check(lib.qemb_op_ccsd_t(o, v, *(b.ptr for b in bufs), int(tile), C.byref(e)), "qemb_op_ccsd_t", lib)
        return e.value
    finally:
        for b in bufs:
            b.free()


def rdm2_from_amplitudes(t1, t2, dm1=None, kind="CCSD", lib=None):
    """The fragment 2-RDM from amplitudes that are handed in (qemb_op_rdm2_assemble, the kernel behind DeviceFragment.make_rdm2): t1 (o, v) -- None for
    kind="MP2" --, t2 (o, o, v, v); dm1 (n, n): the 1-RDM whose products with the HF determinant are added (with_dm1=True of the reference; for CCSD
    make_rdm1_ccsd_t1(t1)), None for with_dm1=False.  Returns (n, n, n, n)."""
    from ._lib import DeviceBuffer
    if kind not in ("CCSD", "MP2"):      # (an FCI 2-RDM comes from a vector, not from amplitudes: fci_rdm12)
        raise ValueError("Solver not implemented")
    lib = lib or _lib.init()
    t2 = np.ascontiguousarray(t2, dtype=np.float64)
    o, v = t2.shape[0], t2.shape[2]
    n = o + v
    if t2.shape != (o, o, v, v) or (kind == "CCSD" and (t1 is None or np.shape(t1) != (o, v))):
        raise ValueError("rdm2_from_amplitudes: t1 must be (o, v) and t2 (o, o, v, v)")
    bufs = []
    def dev(a):
        bufs.append(DeviceBuffer.from_numpy(a, lib=lib))
        return bufs[-1].ptr
    p_t1 = dev(t1) if kind == "CCSD" and v > 0 else None
    p_t2 = dev(t2) if v > 0 else None
    p_d = None
    if dm1 is not None:
        d = np.array(dm1, dtype=np.float64)
        if d.shape != (n, n):
            raise ValueError(f"rdm2_from_amplitudes: dm1 must be ({n}, {n})")
        d[np.diag_indices(o)] -= 2.0
        p_d = dev(d)
    out = DeviceBuffer(n ** 4, lib=lib)
    bufs.append(out)
    try:
        check(lib.qemb_op_rdm2_assemble(RDM2_KINDS[kind], o, v, p_t1, p_t2, p_d, out.ptr), "qemb_op_rdm2_assemble", lib)
        return out.numpy((n, n, n, n))
    finally:
        for b in bufs:
            b.free()


def fci_sigma(h, V, c, nsocc, lib=None, slab_rows=0):
    """sigma = H c of the determinant-space Hamiltonian (qemb_op_fci_sigma): h (n, n), V (n, n, n, n) = (pq|rs), c (ns, ns); returns (ns, ns).
    slab_rows > 0: in slabs of that many alpha strings (qemb_op_fci_sigma_slab)"""
    from ._lib import DeviceBuffer
    lib = lib or _lib.init()
    h = np.ascontiguousarray(h, dtype=np.float64)
    n = h.shape[0]
    c = np.ascontiguousarray(c, dtype=np.float64)
    bufs = [DeviceBuffer.from_numpy(np.asarray(V).reshape(n * n, n * n), lib=lib), DeviceBuffer.from_numpy(c, lib=lib), DeviceBuffer(c.size, lib=lib)]
    try:
        if slab_rows:
            check(lib.qemb_op_fci_sigma_slab(n, int(nsocc), h.ctypes.data, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, int(slab_rows), None), "qemb_op_fci_sigma_slab", lib)
        else:
            check(lib.qemb_op_fci_sigma(n, int(nsocc), h.ctypes.data, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr), "qemb_op_fci_sigma", lib)
        return bufs[2].numpy(c.shape)
    finally:
        for b in bufs:
            b.free()


def fci_rdm12(c, n, nsocc, cumulant=False, lib=None, slab_rows=0):
    """(dm1, dm2) of the vector c (ns, ns) in PySCF's conventions (qemb_op_fci_rdm12); cumulant: dm2 minus the mean-field part of molbe/solver.py:513-527.
    slab_rows > 0: in slabs of that many alpha strings (qemb_op_fci_rdm12_slab)"""
    from ._lib import DeviceBuffer
    lib = lib or _lib.init()
    c = np.ascontiguousarray(c, dtype=np.float64)
    dm1 = np.empty((n, n))
    bufs = [DeviceBuffer.from_numpy(c, lib=lib), DeviceBuffer(n ** 4, lib=lib)]
    try:
        if slab_rows:
            check(lib.qemb_op_fci_rdm12_slab(int(n), int(nsocc), bufs[0].ptr, int(bool(cumulant)), int(slab_rows), dm1.ctypes.data, bufs[1].ptr), "qemb_op_fci_rdm12_slab", lib)
        else:
            check(lib.qemb_op_fci_rdm12(int(n), int(nsocc), bufs[0].ptr, int(bool(cumulant)), dm1.ctypes.data, bufs[1].ptr), "qemb_op_fci_rdm12", lib)
        return dm1, bufs[1].numpy((n, n, n, n))
    finally:
        for b in bufs:
            b.free()


def _sci_space(alpha, beta):
    a, b = np.ascontiguousarray(alpha, dtype=np.uint64), np.ascontiguousarray(beta, dtype=np.uint64)
    if a.ndim != 1 or a.shape != b.shape or a.size == 0:
        raise ValueError("a determinant space is two equally long 1-D arrays of occupation words")
    return a, b


def _sci_integrals(h, V, lib):
    from ._lib import DeviceBuffer
    h = np.ascontiguousarray(h, dtype=np.float64)
    n = h.shape[0]
    return h, n, DeviceBuffer.from_numpy(np.ascontiguousarray(V, dtype=np.float64).reshape(n * n, n * n), lib=lib)


def sci_screen(h, V, nsocc, alpha, beta, c, eps, slab=0, cap=0, lib=None):
    """the determinants outside the sorted space (alpha, beta) that pass |H_ai c_i| >= eps for some member, spin partners included (qemb_op_sci_screen): (alpha, beta),
    sorted.  slab / cap: determinants per pass and keys of the candidate buffer (0: the library's)"""
    lib = lib or _lib.init()
    a, b = _sci_space(alpha, beta)
    c = np.ascontiguousarray(c, dtype=np.float64)
    h, n, Vd = _sci_integrals(h, V, lib)
    try:
        nj = C.c_int64()
        args = (n, int(nsocc), h.ctypes.data, Vd.ptr, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, float(eps), int(slab), int(cap))
        check(lib.qemb_op_sci_screen(*args, 0, C.byref(nj), None, None), "qemb_op_sci_screen", lib)
        oa, ob = np.empty(nj.value, dtype=np.uint64), np.empty(nj.value, dtype=np.uint64)
        if nj.value:
            check(lib.qemb_op_sci_screen(*args, nj.value, C.byref(nj), oa.ctypes.data, ob.ctypes.data), "qemb_op_sci_screen", lib)
        return oa, ob
    finally:
        Vd.free()


def sci_pt2(h, V, nsocc, alpha, beta, c, e_var, eps_pt, max_ext=0, slab=0, cap=0, lib=None):
    """the screened Epstein-Nesbet second-order correction of the vector c with energy e_var over the sorted space (alpha, beta) (qemb_op_sci_pt2; the definition
    is in DeviceFragment.sci_pt2): dict(e_pt2, n_ext, batches).  max_ext: externals per range of the alpha word (0: no bound, one range); slab / cap as in
    `sci_screen`"""
    lib = lib or _lib.init()
    a, b = _sci_space(alpha, beta)
    c = np.ascontiguousarray(c, dtype=np.float64)
    h, n, Vd = _sci_integrals(h, V, lib)
    try:
        e, next_, nb = C.c_double(), C.c_int64(), C.c_int()
        check(lib.qemb_op_sci_pt2(n, int(nsocc), h.ctypes.data, Vd.ptr, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, float(e_var), float(eps_pt), int(max_ext), int(slab), int(cap),
                                  C.byref(e), C.byref(next_), C.byref(nb)), "qemb_op_sci_pt2", lib)
        return dict(e_pt2=e.value, n_ext=int(next_.value), batches=int(nb.value))
    finally:
        Vd.free()


def sci_merge(alpha, beta, c, jalpha, jbeta, lib=None):
    """the sorted space merged with sorted keys outside it, the vector padded with zeros (qemb_op_sci_merge): (alpha, beta, c)"""
    lib = lib or _lib.init()
    a, b = _sci_space(alpha, beta)
    ja, jb = _sci_space(jalpha, jbeta)
    c = np.ascontiguousarray(c, dtype=np.float64)
    N = a.size + ja.size
    oa, ob, oc = np.empty(N, dtype=np.uint64), np.empty(N, dtype=np.uint64), np.empty(N)
    check(lib.qemb_op_sci_merge(a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, ja.size, ja.ctypes.data, jb.ctypes.data, oa.ctypes.data, ob.ctypes.data, oc.ctypes.data),
          "qemb_op_sci_merge", lib)
    return oa, ob, oc


def sci_matrix(h, V, alpha, beta, lib=None):
    """the CSR matrix of H over the sorted space (qemb_op_sci_matrix): (rowptr int64 (N + 1), col int32 (nnz), val (nnz))"""
    lib = lib or _lib.init()
    a, b = _sci_space(alpha, beta)
    h, n, Vd = _sci_integrals(h, V, lib)
    try:
        nnz, rp = C.c_int64(), np.empty(a.size + 1, dtype=np.int64)
        args = (n, h.ctypes.data, Vd.ptr, a.size, a.ctypes.data, b.ctypes.data)
        check(lib.qemb_op_sci_matrix(*args, 0, C.byref(nnz), rp.ctypes.data, None, None), "qemb_op_sci_matrix", lib)
        col, val = np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value)
        check(lib.qemb_op_sci_matrix(*args, nnz.value, C.byref(nnz), rp.ctypes.data, col.ctypes.data, val.ctypes.data), "qemb_op_sci_matrix", lib)
        return rp, col, val
    finally:
        Vd.free()


def sci_spmv(h, V, alpha, beta, x, lib=None):
    """y = H x over the sorted space (qemb_op_sci_spmv)"""
    lib = lib or _lib.init()
    a, b = _sci_space(alpha, beta)
    x = np.ascontiguousarray(x, dtype=np.float64)
    h, n, Vd = _sci_integrals(h, V, lib)
    try:
        y = np.empty(a.size)
        check(lib.qemb_op_sci_spmv(n, h.ctypes.data, Vd.ptr, a.size, a.ctypes.data, b.ctypes.data, x.ctypes.data, y.ctypes.data), "qemb_op_sci_spmv", lib)
        return y
    finally:
        Vd.free()


def sci_rdm12(h, V, nsocc, alpha, beta, c, cumulant=False, lib=None):
    """(dm1, dm2) of the vector c over the sorted space in PySCF's conventions (qemb_op_sci_rdm12); cumulant: dm2 minus the mean-field part"""
    lib = lib or _lib.init()
    a, b = _sci_space(alpha, beta)
    c = np.ascontiguousarray(c, dtype=np.float64)
    h, n, Vd = _sci_integrals(h, V, lib)
    try:
        dm1, dm2 = np.empty((n, n)), np.empty((n, n, n, n))
        check(lib.qemb_op_sci_rdm12(n, int(nsocc), h.ctypes.data, Vd.ptr, a.size, a.ctypes.data, b.ctypes.data, c.ctypes.data, int(bool(cumulant)), dm1.ctypes.data,
                                    dm2.ctypes.data), "qemb_op_sci_rdm12", lib)
        return dm1, dm2
    finally:
        Vd.free()


def fci_links(n, nsocc, lib=None):
    """(strings, links) of one spin as the library built them (qemb_op_fci_links): strings (ns,) bit patterns, links (nlink, ns) words (J << 9) | (pq << 1) | neg"""
    lib = lib or _lib.init()
    ns, nl = C.c_int64(), C.c_int()
    check(lib.qemb_op_fci_links(int(n), int(nsocc), C.byref(ns), C.byref(nl), None, None), "qemb_op_fci_links", lib)
    strings = np.empty(ns.value, dtype=np.int32); links = np.empty((nl.value, ns.value), dtype=np.int32)
    check(lib.qemb_op_fci_links(int(n), int(nsocc), C.byref(ns), C.byref(nl), strings.ctypes.data, links.ctypes.data), "qemb_op_fci_links", lib)
    return strings, links


class _SolveCall:
    """What the solve entries of the library share on this side: h / dm0 / opts as they are handed over, the output dict of every fragment, the result scalars
    (__init__), the call itself (call) and the dicts filled from it (results).  batch: the entry takes arrays over the fragments (qemb_frag_solve_batch,
    _mp2_batch) where the single entries take one fragment's pointers; the result scalars are arrays of the call's length either way.  t1 / t2: whether the
    dicts carry those amplitudes."""

    def __init__(self, frags, nsoccs, hs, dm0s, opts, eeval, batch, t1=False, t2=False):
        F = len(frags)
        self.frags, self.batch, self.lib = frags, batch, frags[0].lib
        self.opts = opts or default_opts(self.lib)
        self.eeval = int(bool(eeval))
        self.ns = [int(o) for o in nsoccs]
        self.hs = [np.ascontiguousarray(h, dtype=np.float64) for h in hs]
        self.dm0s = [None if d is None else np.ascontiguousarray(d, dtype=np.float64) for d in (dm0s if dm0s is not None else [None] * F)]
        self.outs = []
        for fr, o in zip(frags, self.ns):
            n, v = fr.n, fr.n - o
            self.outs.append(dict(mo_coeff=np.empty((n, n)), mo_energy=np.empty(n), rdm1_emb=np.empty((n, n)), rdm1_mo=np.empty((n, n)),
                                  t1=np.empty((o, v)) if t1 else None, t2=np.empty((o, o, v, v)) if t2 else None))
        self.e_frag = np.zeros((F, 3))
        self.e, self.e_scf, self.ebe_hf = (C.c_double * F)(), (C.c_double * F)(), (C.c_double * F)()
        self.n_iter, self.scf_cycles = (C.c_int * F)(), (C.c_int * F)()

    def _ptr(self, xs):
        return (C.c_void_p * len(xs))(*[_p(x) for x in xs]) if self.batch else _p(xs[0])

    def call(self, name, amplitudes, n_iter=True, after_opts=(), last=()):
        """the entry `name`: the inputs up to opts (after_opts: what an entry takes next), eeval, the four arrays every solver returns, the entry's own
        `amplitudes` (keys of the dicts), the energies, n_iter where the entry has it, scf_cycles and what comes `last`"""
        F = len(self.frags)
        head = (F, (C.c_void_p * F)(*[fr.h for fr in self.frags]), (C.c_int * F)(*self.ns)) if self.batch else (self.frags[0].h, self.ns[0])
        arrays = [self._ptr([o_[k] for o_ in self.outs]) for k in ("mo_coeff", "mo_energy", "rdm1_emb", "rdm1_mo") + tuple(amplitudes)]
        check(getattr(self.lib, name)(*head, self._ptr(self.hs), self._ptr(self.dm0s), C.byref(self.opts), *after_opts, self.eeval, *arrays,
                                      self.e_frag.ctypes.data, self.e, self.e_scf, self.ebe_hf, *((self.n_iter,) if n_iter else ()), self.scf_cycles, *last), name, self.lib)

    def results(self, lambda_iters=False):
        """the dicts, filled after the call; lambda_iters: asked of the library (a CCSD solve), else 0"""
        for f, (fr, o_) in enumerate(zip(self.frags, self.outs)):
            nlam = C.c_int()
            if lambda_iters:
                check(self.lib.qemb_frag_lambda_iters(fr.h, C.byref(nlam)), "qemb_frag_lambda_iters", self.lib)
            o_.update(e_frag=self.e_frag[f].copy(), e_corr_mo=float(self.e[f]), e_scf=float(self.e_scf[f]), ebe_hf=float(self.ebe_hf[f]), n_iter=int(self.n_iter[f]),
                      scf_cycles=int(self.scf_cycles[f]), lambda_iters=nlam.value)
        return self.outs


def solve_batch(frags, nsoccs, hs, dm0s=None, opts: SolverOpts | None = None, eeval=True, want_t2=False, stats=None, solver="CCSD"):
    """qemb_frag_solve_batch: every fragment of `frags` (DeviceFragment objects of one library) in one call -- fragment RHF, MO transformation
    and the density / energy evaluation per fragment on its own stream, the CCSD iterations of all fragments in lock step (one grouped
    launch per operation).  Returns the list of dicts DeviceFragment.solve would return, bit for bit; `stats` (a dict) receives the
    launch counters of the lock-step iterations.
    solver="MP2": qemb_frag_solve_mp2_batch -- the fragments spread over the execution contexts that exist (there are no iterations to put in lock
    step); the dicts DeviceFragment.solve_mp2 would return, bit for bit."""
    if solver not in ("CCSD", "MP2"):
        raise ValueError("Solver not implemented")
    if len(frags) == 0:
        return []
    c = _SolveCall(frags, nsoccs, hs, dm0s, opts, eeval, batch=True, t1=solver == "CCSD", t2=want_t2)
    if solver == "MP2":
        c.call("qemb_frag_solve_mp2_batch", ("t2",), n_iter=False)
        return c.results()
    st = (C.c_int64 * 5)()
    c.call("qemb_frag_solve_batch", ("t1", "t2"), last=(st,))
    if stats is not None:
        for k, name in enumerate(("merged_runs", "launches", "grouped_launches", "operations", "max_group")):
            stats[name] = stats.get(name, 0) + int(st[k]) if name != "max_group" else max(stats.get(name, 0), int(st[k]))
    return c.results(lambda_iters=True)
