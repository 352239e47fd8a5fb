"""BE -- host mirror of the molecular bootstrap-embedding driver (molbe/mbe.py:149) over the device hot path.

`BE(mf, fobj)` accepts any mean-field object exposing the PySCF attributes the reference reads
(mbe.py:361-373): mo_energy, mo_coeff, e_tot, _eri, mol.nelectron, energy_nuc(), get_hcore(), get_ovlp(),
make_rdm1(), get_veff() -- a real `pyscf.scf.RHF` or `quemb_amd.integrals.RHF`.  What runs where:
  host (NumPy, once per system, out of scope per SURVEY 2): Loewdin localisation W = S^-1/2 (mbe.py:1395-1398);
  device (libqemb_hip): Schmidt decomposition, AO->fragment ERI transform, fragment Fock / SCF, CCSD, energies.
lo_method "lowdin", "boys", "PM" and "ER" and lo_bath_post_schmidt (lo.py: the rotations run on the device), restricted, are mirrored; frozen core as in mbe.py:397-419.
"""

from __future__ import annotations

import numpy as np

from . import eri_transform as et
from .be_parallel import be_func_parallel, fragment_cost, partition_fragments, world, all_reduce_sum
from .fragsolver import SOLVERS, default_opts
from .pfrag import Frags
from .solver import ErrorMap, be_func


def initialize_pot(n_frag, relAO_per_edge):
    """molbe/mbe.py:1614-1650: one zero per unique edge-AO pair (j <= k) of every fragment + the chemical potential."""
    n = 0
    if relAO_per_edge:
        for I in range(n_frag):
            for e in relAO_per_edge[I]:
                n += len(e) * (len(e) + 1) // 2
    return [0.0] * (n + 1)


class BE:
    def __init__(self, mf, fobj, *, lo_method="lowdin", thr_bath=1.0e-10, int_transform="in-core-hip", auxbasis=None,
                 df_ints=None, nproc=1, ompnum=1, initialize_fragment_idx=None, solver_opts=None, lib=None, distribute=True, nstreams=None, lockstep=None,
                 eri_file=None, scratch_dir=None, restart=False, schmidt_method="subspace", MO_coeff_epsilon=1e-5, AO_coeff_epsilon=1e-10, df_resident="factor",
                 integral_backend="host", int_direct_tile=None, int_direct_thresh=0.0, cd_tol=1e-8, cd_span=0.01, cd_panel=None, reuse_mf_df=False,
                 pop_method=None, init_guess="atomic", lo_bath_post_schmidt=None, fci_slab_rows=0):
        # lo_method "boys" / "PM": the Loewdin orbitals rotated by get_loc (lo.py: Jacobi sweeps on the device; mbe.py:1451-1481), pop_method / init_guess as there.
        # lo_bath_post_schmidt: the bath columns TA[:, n_f:] of every fragment localised after the Schmidt decomposition (mbe.py:1217-1223) -- a rotation inside
        # the embedding space, the fragment columns are not touched.  "ER" (either keyword) is defined on the factorised integrals and needs a dense 3-index context
        # before the fragments are transformed: int_transform "int-direct-DF-hip" from the geometry (`auxbasis`), "cholesky-hip", or reuse_mf_df=True (_loc_df);
        # the context is made once and serves the transform too.  "IAO" stays refused.
        if lo_method not in ("lowdin", "boys", "PM", "ER"):
            raise NotImplementedError("lo_method 'lowdin', 'boys', 'PM' and 'ER' are mirrored ('IAO' is not)")
        if lo_bath_post_schmidt not in (None, "cholesky", "ER", "PM", "boys"):
            raise ValueError("lo_bath_post_schmidt must be None, 'cholesky', 'ER', 'PM' or 'boys'")
        if (lo_method == "ER" or lo_bath_post_schmidt == "ER") and not (
                reuse_mf_df or int_transform == "cholesky-hip" or (int_transform == "int-direct-DF-hip" and df_ints is None and auxbasis)):
            raise ValueError("Edmiston-Ruedenberg localisation reads a dense 3-index context: int_transform='int-direct-DF-hip' with `auxbasis`, "
                             "int_transform='cholesky-hip', or reuse_mf_df=True")
        # fci_slab_rows: the slab height of solver="FCI-hip" on every fragment (DeviceFragment.set_fci_slab: 0 off, k > 0 rows, -1 automatic) -- what lets fragments
        # of 15 and 16 embedding orbitals fit; read wherever a sweep or a 2-RDM runs that solver, ignored by the other solvers
        if int(fci_slab_rows) < -1:
            raise ValueError("fci_slab_rows must be 0 (off), a positive slab height or -1 (automatic)")
        self.fci_slab_rows = int(fci_slab_rows)
        self._lo_cache = {}       # what get_loc needs of the molecule alone (dipole integrals, S^1/2): formed once for all fragments
        self._loc_ctx = None      # (context, owned): made by _loc_df for ER, used and released by _eri_transform
        if (lo_method != "lowdin" or lo_bath_post_schmidt is not None) and getattr(mf, "mol", None) is None:
            raise ValueError("orbital localisation evaluates its integrals from the geometry: the mean field needs `mol`")
        self.lo_method, self.pop_method, self.init_guess, self.lo_bath_post_schmidt = lo_method, pop_method, init_guess, lo_bath_post_schmidt
        self.lo_stats = {}      # what get_loc reports: "W" for lo_method, the fragment index for the bath of each fragment
        if restart:
            raise NotImplementedError("restart files are outside the hot path")
        self.mf, self.fobj, self.lib = mf, fobj, lib
        self.thr_bath = thr_bath
        self.schmidt_method = schmidt_method      # 'eigh' = reference formulation, 'subspace' = same bath, O(N_env n_f nocc)
        self.int_transform = int_transform
        # what a density-fitted fragment keeps resident: "factor" = the fitted 3-index factor bb alone (eri_onthefly.py:141; 8 naux npair bytes -- J / K, MO
        # integrals and energies come from it, the 4-fold block of dataset `f{I}` is formed on demand only), "block" = the block bb^T bb and the factor (round 4)
        if df_resident not in ("factor", "block"):
            raise ValueError("df_resident must be 'factor' or 'block'")
        self.df_resident = df_resident
        # where the from-geometry DF transforms take (mu nu|P) and (P|Q) from: "host" (libqemb_gto) or "hip" (the device kernels; nothing of size naux N^2 on the host).
        # With int_transform="in-core-hip" and no `mf._eri`, "hip" evaluates (mu nu|la si) on the device from mf.mol ("host" keeps the reference's error)
        if integral_backend not in ("host", "hip"):
            raise ValueError("integral_backend must be 'host' or 'hip'")
        if integral_backend == "hip" and df_ints is not None:
            raise ValueError("integral_backend='hip' evaluates the DF integrals from the geometry; with `df_ints` the integrals are the caller's")
        self.integral_backend = integral_backend
        # int_transform="int-direct-hip": the exact fragment integrals of "in-core-hip" from mf.mol with no N^4 array -- the AO integrals are evaluated tile by tile on
        # the device and consumed by every fragment (DeviceBasis.ao2mo).  int_direct_tile: AO pairs per tile (None: from the free device memory); int_direct_thresh:
        # Schwarz threshold of quartets and tiles (0: nothing skipped).  Needs integral_backend="hip" and a mean field with `mol`; `mf._eri` is ignored.
        if int_transform == "int-direct-hip":
            if integral_backend != "hip":
                raise ValueError("int_transform='int-direct-hip' evaluates the integrals on the device: it needs integral_backend='hip'")
            if getattr(mf, "mol", None) is None:
                raise ValueError("int_transform='int-direct-hip' evaluates the integrals from the geometry: the mean field needs `mol`")
        # int_transform="cholesky-hip": a 3-index factor from mf.mol with no auxiliary basis -- the AO integrals are Cholesky-decomposed on the device to cd_tol
        # (element-wise bound; DFContext.from_cholesky) and every fragment is transformed from the factor, as on the DF routes.  cd_span / cd_panel: the panel
        # selection of the decomposition.  Needs integral_backend="hip" and a mean field with `mol`; `mf._eri` is ignored.  `cd_stats`: rank, panels, columns.
        if int_transform == "cholesky-hip":
            if integral_backend != "hip":
                raise ValueError("int_transform='cholesky-hip' decomposes the integrals on the device: it needs integral_backend='hip'")
            if getattr(mf, "mol", None) is None:
                raise ValueError("int_transform='cholesky-hip' evaluates the integrals from the geometry: the mean field needs `mol`")
        # reuse_mf_df: on "int-direct-DF-hip" and "cholesky-hip" the fragments are transformed from the dense 3-index tensor the mean field already holds
        # (mf.with_df, RHF(density_fit=...)): no second tensor is filled, `auxbasis` is not needed and the context stays the mean field's
        self.reuse_mf_df = bool(reuse_mf_df)
        if self.reuse_mf_df:
            df, mol = getattr(mf, "with_df", None), getattr(mf, "mol", None)
            if mol is None or not isinstance(df, et.DFContext) or df.layout != "dense" or df.nao != mol.nao or getattr(df, "h", None) is None:
                raise ValueError("reuse_mf_df=True needs a mean field whose `with_df` is a dense DFContext of its molecule (RHF(..., density_fit=...) after kernel())")
            if int_transform not in ("int-direct-DF-hip", "cholesky-hip"):
                raise ValueError("reuse_mf_df=True goes with int_transform='int-direct-DF-hip' or 'cholesky-hip'")
            if (int_transform == "cholesky-hip") != bool(df.identity_metric):      # the tensor must be the one the branch would have filled
                raise ValueError("reuse_mf_df=True: int_transform='cholesky-hip' reads a Cholesky factor (density_fit='cholesky'), "
                                 "'int-direct-DF-hip' a fitted tensor (density_fit=<auxiliary basis>); the mean field holds the other kind")
            if int_transform == "cholesky-hip" and df.cd_tol is not None:
                cd_tol = df.cd_tol      # the factor exists already: its tolerance is the one that holds
        self.cd_tol, self.cd_span, self.cd_panel = float(cd_tol), float(cd_span), None if cd_panel is None else int(cd_panel)
        self.int_direct_tile = None if int_direct_tile is None else int(int_direct_tile)
        self.int_direct_thresh = float(int_direct_thresh)
        self.auxbasis = auxbasis
        self.MO_coeff_epsilon, self.AO_coeff_epsilon = float(MO_coeff_epsilon), float(AO_coeff_epsilon)      # mbe.py:191-192
        self.opts = solver_opts
        # fragments in flight at once on this GPU (solver.map_fragments) / all fragments of a sweep in one batched call (solver.solve_fragments, the
        # small-fragment regime).  None: chosen from the fragments' sizes at the first sweep (solver.sweep_mode)
        self.nstreams = None if nstreams is None else int(nstreams)
        self.lockstep = None if lockstep is None else bool(lockstep)
        self.unrestricted = False
        self.rdm2_mem_limit = None      # device bytes the full-basis 2-RDM may take (rdm12_fullbasis / compute_energy_full); None: whatever is free
        self.ebe_hf = 0.0
        self.ebe_tot = 0.0
        self.mo_energy = mf.mo_energy
        self.Nocc = mf.mol.nelectron // 2
        self.enuc = float(mf.energy_nuc())
        self.hcore = np.asarray(mf.get_hcore())
        self.S = np.asarray(mf.get_ovlp())
        self.C = np.array(mf.mo_coeff)
        self.hf_dm = np.asarray(mf.make_rdm1())
        self.hf_veff = np.asarray(mf.get_veff())
        self.hf_etot = float(mf.e_tot)
        self.E_core = 0.0
        self.ncore = 0
        self.C_core = self.P_core = self.core_veff = None
        self.frozen_core = bool(getattr(fobj, "frozen_core", False))
        if self.frozen_core:
            # mbe.py:397-419: the lowest `ncore` canonical MOs are frozen; their mean field moves from hf_veff into hcore
            if getattr(fobj, "ncore", None) is None and hasattr(fobj, "set_core"):
                fobj.set_core(mf.mol)
            if fobj.ncore is None or fobj.no_core_idx is None or fobj.core_list is None:
                raise ValueError("frozen-core fragmentation without ncore / no_core_idx / core_list")
            self.ncore, self.no_core_idx, self.core_list = fobj.ncore, fobj.no_core_idx, fobj.core_list
            self.Nocc -= self.ncore
            Cv = self.C[:, self.ncore: self.ncore + self.Nocc]
            self.hf_dm = 2.0 * Cv @ Cv.T
            self.C_core = self.C[:, : self.ncore]
            self.P_core = self.C_core @ self.C_core.T
            self.core_veff = np.asarray(mf.get_veff(dm=self.P_core * 2.0))
            self.E_core = float(np.einsum("ji,ji->", 2.0 * self.hcore + self.core_veff, self.P_core))
            self.hf_veff = self.hf_veff - self.core_veff
            self.hcore = self.hcore + self.core_veff
        self.pot = initialize_pot(fobj.n_frag, fobj.relAO_per_edge_per_frag)
        self.Fobjs: list[Frags] = []
        self.stats = {}
        # fragment ownership over ranks (all fragments on this rank when not distributed)
        self.rank, self.world = world() if distribute else (0, 1)
        self._df_ints = df_ints
        try:
            self.localize()
            self.initialize(getattr(mf, "_eri", None), initialize_fragment_idx)
        finally:
            self._release_loc_df()      # (a context made for Edmiston-Ruedenberg that a failure kept from reaching the transform)

    # ------------------------------------------------------------------ localisation (host; mbe.py:1395-1449)
    def localize(self):
        es_, vs_ = np.linalg.eigh(self.S)
        edx = es_ > 1.0e-15
        self.W = (vs_[:, edx] / np.sqrt(es_[edx])) @ vs_[:, edx].T
        if self.frozen_core:
            # mbe.py:1418-1431: project the core out of the Loewdin orbitals, keep the columns that stay populated (> 0.7; > 0.55 on the boys / PM branch,
            # mbe.py:1456-1468), re-orthonormalise symmetrically -- N - ncore valence LOs in the order of the valence AOs
            C_ = (np.eye(self.W.shape[0]) - self.P_core @ self.S) @ self.W
            Cpop = np.diag(C_.T @ self.S @ C_)
            C_ = C_[:, np.where(Cpop > (0.7 if self.lo_method == "lowdin" else 0.55))[0]]
            es_, vs_ = np.linalg.eigh(C_.T @ self.S @ C_)
            self.W = C_ @ ((vs_ / np.sqrt(es_)) @ vs_.T)
        if self.lo_method != "lowdin":
            from .lo import get_loc
            st = self.lo_stats["W"] = {}
            self.W = get_loc(self.mf.mol, self.W, self.lo_method, pop_method=self.pop_method, init_guess=self.init_guess, lib=self.lib, stats=st, cache=self._lo_cache,
                             df=self._loc_df() if self.lo_method == "ER" else None)      # mbe.py:1470-1476
        self.lmo_coeff = self.W.T @ self.S @ self.C[:, self.ncore:]

    def _dense_route(self):
        """whether the fragments are transformed from ONE dense 3-index context the driver makes or borrows: the mean field's (reuse_mf_df), the Cholesky factor of
        "cholesky-hip", the fitted tensor of "int-direct-DF-hip" from the geometry"""
        it = self.int_transform
        return (self.reuse_mf_df and it in ("int-direct-DF-hip", "cholesky-hip")) or it == "cholesky-hip" or (it == "int-direct-DF-hip" and self._df_ints is None)

    def _route_context(self):
        """-> (context, owned) of a dense route (_dense_route): the one place the driver makes it, for the transform and for Edmiston-Ruedenberg alike"""
        from . import _lib
        it = self.int_transform
        if self.reuse_mf_df:
            return self.mf.with_df, False      # the tensor of the mean field serves the fragments too: borrowed, not freed here
        if it == "cholesky-hip":
            # the Cholesky factor of the AO integrals, decomposed once on the device (csrc/int4c.cpp: int4c_cholesky), is the 3-index tensor of a DF context with an
            # identity metric.  `mf._eri` is ignored: the integrals come from mf.mol
            return et.DFContext.from_cholesky(self.mf.mol, tol=self.cd_tol, span=self.cd_span, panel_pairs=self.cd_panel, lib=self.lib or _lib.init()), True
        from . import eri_sparse_DF as sdf
        if not self.auxbasis:
            raise ValueError("`auxbasis` has to be defined.")                # mbe.py:1050
        return sdf.dense_df_context(self.mf.mol, self.auxbasis, lib=self.lib, integral_backend=self.integral_backend), True

    def _loc_df(self):
        """The dense 3-index context Edmiston-Ruedenberg reads, before the fragments are transformed: made once here (_route_context) and handed on to
        `_eri_transform`, which releases it."""
        if self._loc_ctx is None:
            self._loc_ctx = self._route_context()
        return self._loc_ctx[0]

    def _release_loc_df(self):
        if self._loc_ctx is not None and self._loc_ctx[1]:
            self._loc_ctx[0].free()
        self._loc_ctx = None

    # ------------------------------------------------------------------ initialisation (mbe.py:1183-1237)
    def initialize(self, eri_, initialize_fragment_idx=None):
        fo = self.fobj
        for I in range(fo.n_frag):
            f = Frags(fo.AO_per_frag[I], I, fo.AO_per_edge_per_frag[I], fo.ref_frag_idx_per_edge_per_frag[I],
                      fo.relAO_per_edge_per_frag[I], fo.relAO_in_ref_per_edge_per_frag[I],
                      fo.weight_and_relAO_per_center_per_frag[I], fo.relAO_per_origin_per_frag[I], lib=self.lib)
            f.fci_slab_rows = self.fci_slab_rows
            self.Fobjs.append(f)
        couti = 0
        for f in self.Fobjs:
            f.udim = couti
            couti = f.set_udim(couti)
        self.emap = ErrorMap(self.Fobjs) if fo.n_BE != 1 and any(fo.relAO_per_edge_per_frag) else None
        # Schmidt decomposition of every fragment this rank may own (cheap; sizes decide the partition)
        for f in self.Fobjs:
            f.sd(self.W, self.lmo_coeff, self.Nocc, thr_bath=self.thr_bath, method=self.schmidt_method)
        if self.lo_bath_post_schmidt is not None:
            # mbe.py:1217-1223: after the Schmidt decomposition of every fragment, before anything reads TA.  Beyond the reference, TA_lo_eo is rewritten too, so
            # that TA = W TA_lo_eo keeps holding
            from .lo import get_loc
            df = self._loc_df() if self.lo_bath_post_schmidt == "ER" else None
            for f in self.Fobjs:
                if f.TA.shape[1] > f.n_f:
                    st = self.lo_stats[f.ifrag] = {}
                    f.TA[:, f.n_f:] = get_loc(self.mf.mol, f.TA[:, f.n_f:], method=self.lo_bath_post_schmidt, lib=self.lib, stats=st, df=df, cache=self._lo_cache)
                    f.TA_lo_eo[:, f.n_f:] = self.W.T @ self.S @ f.TA[:, f.n_f:]
        for f in self.Fobjs:
            f.get_nsocc(self.S, self.C, self.Nocc, ncore=self.ncore)
        costs = [fragment_cost(f.nao, f.nsocc) for f in self.Fobjs]
        self.owner = partition_fragments(costs, self.world)
        if initialize_fragment_idx is None:
            initialize_fragment_idx = [i for i in range(fo.n_frag) if self.owner[i] == self.rank]
        self.my_frags = list(initialize_fragment_idx)
        self._eri_transform(eri_, self.my_frags)
        self._initialize_fragments(self.my_frags)

    def _eri_transform(self, eri_, idx):
        """BE._eri_transform (mbe.py:1004-1113) with the device literals of eri_transform.HIP_INT_TRANSFORMS."""
        it = self.int_transform
        if self._dense_route():
            # one dense context serves every fragment: the one Edmiston-Ruedenberg was localised on, if there was one, else made now; an owned one is released
            df, owned = self._loc_ctx if self._loc_ctx is not None else self._route_context()
            self._loc_ctx = (df, owned)
            try:
                if it == "cholesky-hip":
                    self.cd_stats = dict(getattr(df, "cd_stats", {}))
                for I in idx:
                    df.transform(self.Fobjs[I].TA, frag=self.Fobjs[I].dev, want_host=False, factor_only=self.df_resident == "factor")
            finally:
                self._release_loc_df()
            if self.reuse_mf_df or it == "cholesky-hip":
                self._eri_from_geometry = True
        elif it in ("in-core-hip", "in-core"):
            if eri_ is None and self.integral_backend != "hip":
                raise ValueError("ERIs have to be available in memory.")      # mbe.py:1036
            if eri_ is None:
                # from the geometry: (mu nu|la si) evaluated on the device and left there, 4-fold packed (csrc/int4c_ops.hip); no integral array on the host
                from . import _lib
                from .integrals import DeviceBasis
                basis = DeviceBasis(self.mf.mol, self.lib or _lib.init())
                try:
                    ao = et.AOEri.from_basis(basis)
                finally:
                    basis.free()
                self._eri_from_geometry = True
            else:
                ao = et.AOEri(eri_, self.S.shape[0], lib=self.lib)
            try:
                for I in idx:
                    ao.transform(self.Fobjs[I].TA, frag=self.Fobjs[I].dev, want_host=False)
            finally:
                ao.free()
        elif it == "int-direct-hip":
            # integral-direct: one pass over the AO integrals, tile by tile, serves every fragment of `idx` (csrc/int4c.cpp: int4c_ao2mo_direct); nothing of size
            # N^4 exists on the host or the device.  `eri_` (mf._eri) is ignored: the integrals come from mf.mol
            from . import _lib
            from .integrals import DeviceBasis
            basis = DeviceBasis(self.mf.mol, self.lib or _lib.init())
            try:
                if idx:
                    self.int_direct_bytes = basis.ao2mo_bytes([self.Fobjs[I].TA.shape[1] for I in idx], self.int_direct_tile)
                    basis.ao2mo([self.Fobjs[I].TA for I in idx], frags=[self.Fobjs[I].dev for I in idx], want_host=False, tile_pairs=self.int_direct_tile,
                                thresh=self.int_direct_thresh)
            finally:
                basis.free()
            self._eri_from_geometry = True
        elif it in ("sparse-DF-hip", "on-fly-sparse-DF-hip") and self._df_ints is None:
            # from the geometry alone, like the reference's "sparse-DF(-gpu)" / "on-fly-sparse-DF(-gpu)" branches (mbe.py:1049-1110; "int-direct-DF" is the dense
            # route above): auxiliary molecule, (P|Q), (mu nu|P) from the integral source, AO screening, device transform
            from . import eri_sparse_DF as sdf
            if not self.auxbasis:
                raise ValueError("`auxbasis` has to be defined.")                # mbe.py:1050
            frs = [self.Fobjs[I] for I in idx]
            self.df_stats = {}
            self.S_abs = sdf.transform_sparse_DF_integral_hip(self.mf, frs, self.auxbasis, AO_coeff_epsilon=self.AO_coeff_epsilon,
                                                              MO_coeff_epsilon=self.MO_coeff_epsilon, lib=self.lib,
                                                              precompute_P_mu_nu=(it == "sparse-DF-hip"), stats=self.df_stats,
                                                              factor_only=self.df_resident == "factor", integral_backend=self.integral_backend)
        elif it in ("int-direct-DF-hip", "sparse-DF-hip"):
            # df_ints: (ints, j2c, layout) or a dict(ints=, layout= | int_P_mu_nu=, j2c= | L_PQ=, S_abs=, MO_coeff_epsilon=).
            # "sparse-DF-hip" applies the MO-coefficient screening of the reference's semi-sparse transform
            # (eri_sparse_DF.py:535-656, MO_coeff_epsilon default 1e-5, mbe.py:189) when S_abs is given.
            if self._df_ints is None:
                raise ValueError("df_ints has to be given for a DF transform")
            d = self._df_ints
            if not isinstance(d, dict):
                d = dict(ints=d[0], j2c=d[1], layout=d[2])
            df = et.DFContext(j2c=d.get("j2c"), L_PQ=d.get("L_PQ"), lib=self.lib)
            if d.get("int_P_mu_nu") is not None:
                # the semi-sparse tensor itself (et.SemiSparseSym3DTensor or the reference's object, eri_sparse_DF.py:433-496)
                df.set_ints_semisparse(d["int_P_mu_nu"])
            else:
                df.set_ints(d["ints"], self.S.shape[0], d.get("layout", "pqL"))
            S_abs = d.get("S_abs") if it == "sparse-DF-hip" else None
            for I in idx:
                df.transform(self.Fobjs[I].TA, frag=self.Fobjs[I].dev, want_host=False, S_abs=S_abs,
                             MO_coeff_epsilon=d.get("MO_coeff_epsilon"), factor_only=self.df_resident == "factor")
            df.free()
        else:
            raise ValueError(f"int_transform {it!r} is not one of {et.HIP_INT_TRANSFORMS}")

    def _initialize_fragments(self, idx):
        """mbe.py:1116-1180: h1, Fock, fragment SCF, dm0, fragment HF energies, HF-in-HF check."""
        E_hf = 0.0
        err = None
        try:
            for I in idx:
                f = self.Fobjs[I]
                f.h1 = f.TA.T @ self.hcore @ f.TA
                f.cons_fock(self.hf_veff, self.S, self.hf_dm)
                f.heff = np.zeros_like(f.h1)
                f.scf(fs=True, opts=self.opts)
                f.dm0 = 2.0 * f._mo_coeffs[:, : f.nsocc] @ f._mo_coeffs[:, : f.nsocc].T
                f.update_ebe_hf()
                E_hf += f.ebe_hf
        except Exception as e:  # noqa: BLE001 -- a failure on one rank must not leave the others waiting in the all-reduce
            if self.world == 1:
                raise
            err = e
        buf = np.array([E_hf])
        if self.world > 1:
            all_reduce_sum(buf, error=err)
        self.ebe_hf = float(buf[0]) + self.enuc + self.E_core
        self.hf_err = self.hf_etot - self.ebe_hf
        if self.rank == 0:
            print(f"HF-in-HF error                 :  {self.hf_err:>.4e} Ha", flush=True)

    # ------------------------------------------------------------------ on-disk hand-off (mbe.py:1039, helper.py:182-189)
    def dump_fragment_eris(self, directory):
        """Spill the device-resident fragment ERIs: one `f{I}.npy` per owned fragment, the FP64 (npair(n), npair(n)) 4-fold packed
        array the reference keeps as dataset "f{I}" of scratch/eri_file.h5 (h5py is not available here; `.npy` is the stand-in)."""
        from pathlib import Path
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        for I in self.my_frags:
            np.save(d / f"{self.Fobjs[I].dname}.npy", self.Fobjs[I].dev.get_eri_s4())
        return d

    def load_fragment_eris(self, directory):
        """Inverse of dump_fragment_eris: put `f{I}.npy` back on the device (e.g. ERIs transformed elsewhere / by the reference)."""
        from pathlib import Path
        for I in self.my_frags:
            self.Fobjs[I].set_eri(np.load(Path(directory) / f"{self.Fobjs[I].dname}.npy"))

    # ------------------------------------------------------------------ full-basis 1-RDM (mbe.py:488-700)
    def rdm1_fullbasis(self, return_ao=True, only_rdm1=True, only_rdm2=False, return_lo=False, return_RDM2=False, print_energy=False):
        """The democratically partitioned one-particle density matrix of the whole system from the fragment solutions of the
        last sweep (mbe.py:560-577, :649-659): every fragment contributes P_c . rdm1_eo through the projector P_c on its
        centre AOs.  Only the 1-RDM is mirrored (`only_rdm1=True`): the reference's two-particle part transforms the dense
        n^4 fragment 2-RDMs, which the device path never forms (csrc/fragment.cpp contracts them in place)."""
        if not only_rdm1 or only_rdm2 or return_RDM2:
            raise NotImplementedError("rdm1_fullbasis: only the one-particle density matrix is mirrored (only_rdm1=True)")
        nao = self.C.shape[0]
        rdm1AO = np.zeros((nao, nao))
        for I in self.my_frags:
            f = self.Fobjs[I]
            if f.rdm1__ is None:
                raise RuntimeError("rdm1_fullbasis: run oneshot() or optimize() first")
            cind = [f.AO_in_frag[i] for i in f.weight_and_relAO_per_center[1]]
            SW = self.S @ self.W[:, cind]
            Pc_ = f.TA.T @ SW @ SW.T @ f.TA
            rdm1_eo = f.mo_coeffs @ f.rdm1__ @ f.mo_coeffs.T
            rdm1AO += f.TA @ (Pc_ @ rdm1_eo) @ f.TA.T
        if self.world > 1:
            all_reduce_sum(rdm1AO)
        rdm1AO = (rdm1AO + rdm1AO.T) / 2.0
        rdm1LO = self.W.T @ self.S @ rdm1AO @ self.S @ self.W if return_lo else None
        out = rdm1AO if return_ao else self.C.T @ self.S @ rdm1AO @ self.S @ self.C
        return (out, rdm1LO) if return_lo else out

    # ------------------------------------------------------------------ full-basis 2-RDM and energies (mbe.py:488-838)
    def _rdm2_full_device(self, rdm1AO, return_RDM2, transform=False, eri_words=0):
        """the symmetrised full-basis two-particle tensor as a device buffer ([N]^4): every owned fragment's centre-projected tensor accumulated on the
        device (rdm_full.accumulate), summed over the ranks, symmetrised, plus nc_AO of `rdm1AO` (the 1-RDM as accumulated, not yet symmetrised) when return_RDM2 (mbe.py:543-620)"""
        from . import rdm_full, _lib
        from ._lib import DeviceBuffer
        lib = self.lib or _lib.init()
        nao = self.C.shape[0]
        frags = [self.Fobjs[I] for I in self.my_frags]
        for f in frags:
            if f.rdm1__ is None:
                raise RuntimeError("rdm12_fullbasis: run oneshot() or optimize() first")
        rdm_full.guard(lib, nao, frags, transform, eri_words, getattr(self, "rdm2_mem_limit", None))
        acc = DeviceBuffer.from_numpy(np.zeros(nao ** 4), lib=lib)
        try:
            rdm_full.accumulate(lib, acc, nao, self.S, self.W, frags, return_RDM2)
            if self.world > 1:
                host = acc.numpy()
                all_reduce_sum(host)
                acc.upload(host)
            rdm_full.symmetrize(lib, acc, nao, rdm1AO if return_RDM2 else None)
        except BaseException:
            acc.free()
            raise
        return acc

    def _rdm1_full_accumulated(self):
        """the full-basis 1-RDM as the fragment loop leaves it (mbe.py:571-577), before its symmetrisation (:650): what nc_AO reads (:603-619)"""
        nao = self.C.shape[0]
        raw = np.zeros((nao, nao))
        for I in self.my_frags:
            f = self.Fobjs[I]
            cind = [f.AO_in_frag[i] for i in f.weight_and_relAO_per_center[1]]
            SW = self.S @ self.W[:, cind]
            raw += f.TA @ ((f.TA.T @ SW @ SW.T @ f.TA) @ (f.mo_coeffs @ f.rdm1__ @ f.mo_coeffs.T)) @ f.TA.T
        if self.world > 1:
            all_reduce_sum(raw)
        return raw

    def _eri_words(self):
        e = getattr(self.mf, "_eri", None)
        if e is None:
            if getattr(self, "_eri_from_geometry", False):      # evaluated on the device in the 8-fold packed form (_ao_integrals)
                npair = self.C.shape[0] * (self.C.shape[0] + 1) // 2
                return npair * (npair + 1) // 2
            raise ValueError("ERIs have to be available in memory.")
        return int(np.size(e))

    def _ao_integrals(self, lib, nao):
        """the AO integrals the full-basis energies contract, on the device: `mf._eri` in the form it has, or -- a driver that evaluated its integrals from the
        geometry (integral_backend="hip" without `mf._eri`) -- the 8-fold packed form from the device kernels.  On that route EVERY call evaluates the whole
        integral set again (on top of the 4-fold packed evaluation of `_eri_transform`): nothing of size N^4 is kept between calls, on the host or on the device, at
        the price of one more integral evaluation per compute_energy_full / rdm12_fullbasis(print_energy=True)"""
        from . import rdm_full
        if getattr(self.mf, "_eri", None) is None and getattr(self, "_eri_from_geometry", False):
            return rdm_full.AOIntegrals.from_mol(lib, self.mf.mol, nao)
        return rdm_full.AOIntegrals(lib, self.mf._eri, nao)

    def rdm12_fullbasis(self, return_ao=True, only_rdm2=False, return_lo=False, return_RDM2=True, print_energy=False):
        """The one- and two-particle density matrices of the whole system, the reference's `rdm1_fullbasis(only_rdm1=False)` (mbe.py:488-701) with its return
        conventions: (rdm1, rdm2) in the AO (return_ao) or MO basis, with (rdm1LO, rdm2LO) appended when return_lo, the two-particle tensor alone when only_rdm2.
        return_RDM2=True: the 2-RDM (the fragments' non-connected parts subtracted, nc_AO of the full 1-RDM added); False: the cumulant as the fragments hold it.
        The fragment tensors are those of the last sweep (unrelaxed; with_dm1=False, as solver.py:941 leaves rdm2__ with use_cumulant); they are assembled,
        rotated, projected and accumulated on the device (rdm_full.py, csrc/rdm2_ops.hip).  The 1-RDM is always formed: nc_AO needs it (the reference leaves it
        undefined under only_rdm2, mbe.py:538-539 / :603-607)."""
        from . import rdm_full, _lib
        lib = self.lib or _lib.init()
        nao = self.C.shape[0]
        if any(self.Fobjs[I].rdm1__ is None for I in self.my_frags):
            raise RuntimeError("rdm12_fullbasis: run oneshot() or optimize() first")
        raw = self._rdm1_full_accumulated()
        rdm1AO = (raw + raw.T) / 2.0
        want_energy = return_RDM2 and print_energy
        acc = self._rdm2_full_device(raw, return_RDM2, transform=return_lo or not return_ao, eri_words=self._eri_words() if want_energy else 0)
        try:
            rdm2AO = acc.numpy((nao,) * 4)
            CmoT_S, CloT_S = self.C.T @ self.S, self.W.T @ self.S
            rdm2MO = rdm_full.reexpress(lib, acc, nao, CmoT_S) if not return_ao else None
            rdm2LO = rdm_full.reexpress(lib, acc, nao, CloT_S) if return_lo else None
            if want_energy:
                ao = self._ao_integrals(lib, nao)
                try:
                    E2 = 0.5 * ao.dot(acc)
                finally:
                    ao.free()
        finally:
            acc.free()
        rdm1MO = CmoT_S @ rdm1AO @ CmoT_S.T if not return_ao else None
        rdm1LO = CloT_S @ rdm1AO @ CloT_S.T if return_lo else None
        if want_energy and self.rank == 0:
            Eh1 = float(np.einsum("ij,ij", self.hcore, rdm1AO))
            E_tot = Eh1 + E2 + self.E_core + self.enuc
            print(flush=True)
            print("-----------------------------------------------------", flush=True)
            print(" BE ENERGIES with cumulant-based expression", flush=True)
            print("-----------------------------------------------------", flush=True)
            print(f" 1-elec E        : {Eh1:>15.8f} Ha", flush=True)
            print(f" 2-elec E        : {E2:>15.8f} Ha", flush=True)
            print(f" E_BE            : {E_tot:>15.8f} Ha", flush=True)
            print(f" Ecorr BE        : {(E_tot) - self.ebe_hf:>15.8f} Ha", flush=True)
            print("-----------------------------------------------------", flush=True)
            print(flush=True)
        r1, r2 = (rdm1AO, rdm2AO) if return_ao else (rdm1MO, rdm2MO)
        if only_rdm2:
            return r2
        if return_lo:
            return (r1, r2, rdm1LO, rdm2LO)
        return r1, r2

    def compute_energy_full(self, approx_cumulant=False, use_full_rdm=False, return_rdm=True):
        """mbe.py:703-838: the BE energy from full-basis densities, E_HF + Tr(F del g) + Tr(V K_approx) / 2 and (approx_cumulant=False)
        Tr(h g) + Tr(V_eff[g] g) / 2 + Tr(V K_true) / 2; sets `ebe_tot`, prints the reference's table, returns (rdm1, RDM2_full) when return_rdm.  K_approx is
        rdm12_fullbasis(return_RDM2=False), K_true rdm12_fullbasis(only_rdm2=True).  The N^4 tensors stay on the device: the contractions with the AO
        integrals read `mf._eri` in its packed form (rdm2_ops.hip, a two-stage reduction in a fixed order).  The energies are kept in `self.e_full`."""
        from . import rdm_full, _lib
        from ._lib import DeviceBuffer, check
        lib = self.lib or _lib.init()
        nao = self.C.shape[0]
        if any(self.Fobjs[I].rdm1__ is None for I in self.my_frags):
            raise RuntimeError("compute_energy_full: run oneshot() or optimize() first")
        raw = self._rdm1_full_accumulated()
        rdm1f = (raw + raw.T) / 2.0
        words = self._eri_words() + (0 if approx_cumulant else nao ** 4)
        K = self._rdm2_full_device(rdm1f, False, eri_words=words)
        KT = ao = None
        RDM2_full = E2 = EKumul_T = None
        try:
            ao = self._ao_integrals(lib, nao)
            EKumul = ao.dot(K)
            if not approx_cumulant:
                KT = self._rdm2_full_device(raw, True, eri_words=words)
                EKumul_T = ao.dot(KT)
            if return_rdm:
                # RDM2_full = nc(rdm1f) + the cumulant (mbe.py:745-757), formed in place on the device
                full = K if approx_cumulant else KT
                g = DeviceBuffer.from_numpy(rdm1f, lib=lib)
                try:
                    check(lib.qemb_op_rdm2_add_nc(nao, g.ptr, 1.0, full.ptr), "qemb_op_rdm2_add_nc", lib)
                finally:
                    g.free()
                if use_full_rdm:
                    E2 = ao.dot(full)
                RDM2_full = full.numpy((nao,) * 4)
        finally:
            for b in (K, KT, ao):
                if b is not None:
                    b.free()
        del_gamma = rdm1f - self.hf_dm
        veff = np.asarray(self.mf.get_veff(dm=rdm1f))
        Eh1 = float(np.einsum("ij,ij", self.hcore, rdm1f))
        EVeff = float(np.einsum("ij,ij", veff, rdm1f))
        Eh1_dg = float(np.einsum("ij,ij", self.hcore, del_gamma))
        Eveff_dg = float(np.einsum("ij,ij", self.hf_veff, del_gamma))
        EKapprox = self.ebe_hf + Eh1_dg + Eveff_dg + EKumul / 2.0
        self.ebe_tot = EKapprox
        self.e_full = dict(EKapprox=EKapprox, EKumul=EKumul, Eh1_dg=Eh1_dg, Eveff_dg=Eveff_dg, Eh1=Eh1, EVeff=EVeff)
        if not approx_cumulant:
            EKtrue = Eh1 + EVeff / 2.0 + EKumul_T / 2.0 + self.enuc + self.E_core
            self.ebe_tot = EKtrue
            self.e_full.update(EKtrue=EKtrue, EKumul_T=EKumul_T)
        if E2 is not None:
            self.e_full["E2"] = E2
        if self.rank == 0:
            print("-----------------------------------------------------", flush=True)
            print(" BE ENERGIES with cumulant-based expression", flush=True)
            print("-----------------------------------------------------", flush=True)
            print(" E_BE = E_HF + Tr(F del g) + Tr(V K_approx)", flush=True)
            print(f" E_HF            : {self.ebe_hf:>14.8f} Ha", flush=True)
            print(f" Tr(F del g)     : {Eh1_dg + Eveff_dg:>14.8f} Ha", flush=True)
            print(f" Tr(V K_aprrox)  : {EKumul / 2.0:>14.8f} Ha", flush=True)
            print(f" E_BE            : {EKapprox:>14.8f} Ha", flush=True)
            print(f" Ecorr BE        : {EKapprox - self.ebe_hf:>14.8f} Ha", flush=True)
            if not approx_cumulant:
                print(flush=True)
                print(" E_BE = Tr(F[g] g) + Tr(V K_true)", flush=True)
                print(f" Tr(h1 g)        : {Eh1:>14.8f} Ha", flush=True)
                print(f" Tr(Veff[g] g)   : {EVeff / 2.0:>14.8f} Ha", flush=True)
                print(f" Tr(V K_true)    : {EKumul_T / 2.0:>14.8f} Ha", flush=True)
                print(f" E_BE            : {EKtrue:>14.8f} Ha", flush=True)
                if E2 is not None:
                    print(" E(g+G)          : {:>14.8f} Ha".format(Eh1 + 0.5 * E2 + self.E_core + self.enuc), flush=True)
                print(f" Ecorr BE        : {EKtrue - self.ebe_hf:>14.8f} Ha", flush=True)
                print(flush=True)
                print(f" True - approx   : {EKtrue - EKapprox:>14.4e} Ha")
            print("-----------------------------------------------------", flush=True)
            print(flush=True)
        if return_rdm:
            return (rdm1f, RDM2_full)

    def compute_numerical_jacobian(self, solver="CCSD", only_chem=False, nproc=1, step_size=1e-6, solver_args=None):
        from .numerical_jac import compute_numerical_jacobian
        return compute_numerical_jacobian(self, solver, only_chem, nproc, step_size=step_size, solver_args=solver_args)

    # ------------------------------------------------------------------ sweeps
    def _sweep(self, pot, solver="CCSD", **kw):
        if self.nstreams is None or self.lockstep is None:
            from .solver import sweep_mode
            mine = [f for i, f in enumerate(self.Fobjs) if self.world <= 1 or self.owner[i] == self.rank]
            self.nstreams, self.lockstep = sweep_mode(mine, self.nstreams, self.lockstep, solver=solver)
        if self.world > 1:
            return be_func_parallel(pot, self.Fobjs, self.Nocc, solver, self.enuc, owner=self.owner, opts=self.opts,
                                    stats=self.stats, emap=self.emap, nstreams=self.nstreams, lockstep=self.lockstep, **kw)
        return be_func(pot, self.Fobjs, self.Nocc, solver, self.enuc, opts=self.opts, stats=self.stats, nstreams=self.nstreams, lockstep=self.lockstep, **kw)

    def oneshot(self, solver="CCSD", use_cumulant=True, nproc=1, ompnum=1, solver_args=None):
        """mbe.py:1240-1310.  solver: "CCSD", "MP2" or "FCI-hip" (determinant-space FCI per fragment on the device, n <= 16 embedding orbitals) or "SCI-hip"
        (heat-bath selected CI per fragment on the device, n <= 64; `solver_args`: a solver.SHCI_ArgsUser with its cutoff, None for the defaults -- read by "SCI-hip" alone)."""
        if solver not in SOLVERS:
            raise ValueError("Solver not implemented")
        rets = self._sweep(None, solver=solver, eeval=True, use_cumulant=use_cumulant, return_vec=False, solver_args=solver_args)
        self.ebe_tot = rets[0] + self.ebe_hf
        self.e_corr = rets[0]
        self.e_components = rets[1]
        if self.rank == 0:
            print(f"One-shot BE  E_corr = {rets[0]:.12f}  Tr(F del g) = {rets[1][0] + rets[1][2]:.10f}  Tr(V K) = {rets[1][1]:.10f}"
                  f"  E_tot = {self.ebe_tot:.10f}", flush=True)
        return rets

    def sci_pt2(self, eps_pt, max_ext=0):
        """after `oneshot` / `optimize` with solver="SCI-hip": the screened Epstein-Nesbet second-order correction of every fragment's last solve (Frags.sci_pt2), one
        dict(e_var, e_pt2, n_ext, batches, ms) per fragment in fragment order (None for a fragment another rank owns).  e_var + e_pt2 against e_var tells whether
        `hci_cutoff` was small enough for that embedding problem.  It is a per-fragment diagnostic and is added to nothing: the BE energies are formed from the
        variational RDMs, as in the reference, whose hci_pt does not reach them either."""
        mine = [f for i, f in enumerate(self.Fobjs) if self.world <= 1 or self.owner[i] == self.rank]
        if not mine or any(f._solver != "SCI-hip" for f in mine):
            raise RuntimeError("BE.sci_pt2: run oneshot or optimize with solver='SCI-hip' first")
        return [f.sci_pt2(eps_pt, max_ext) if f in mine else None for f in self.Fobjs]

    def ccsd_t(self):
        """after `oneshot` / `optimize` with solver="CCSD": the perturbative triples correction E_(T) of every fragment's last solve (Frags.ccsd_t), one
        dict(e_t, tile, n_tile_triples, bytes, ms) per fragment in fragment order (None for a fragment another rank owns).  Raises ValueError before a sweep and
        after a sweep with another solver.  E_(T) is the triples energy of each fragment's embedding problem -- the standard measure of what CCSD leaves out
        there -- and a per-fragment diagnostic: it is added to no BE energy, and a centre-projected BE-level (T) energy is not formed."""
        mine = [f for i, f in enumerate(self.Fobjs) if self.world <= 1 or self.owner[i] == self.rank]
        if not mine or any(f._solver != "CCSD" for f in mine):
            raise ValueError("BE.ccsd_t: run oneshot or optimize with solver='CCSD' first")
        return [f.ccsd_t() if f in mine else None for f in self.Fobjs]

    def optimize(self, solver="CCSD", method="QN", only_chem=False, use_cumulant=True, conv_tol=1.0e-6, relax_density=False,
                 jac_solver="HF", nproc=1, ompnum=1, max_iter=500, trust_region=False, step_size=1e-6, solver_args=None,
                 warm_start=True):
        """mbe.py:841-977.  `warm_start` (addition): every sweep after the first starts each fragment's CCSD from the
        amplitudes of the previous sweep, which stay resident on the device (the reference restarts from MP2 at every
        objective evaluation, solver.py:894-907); the converged amplitudes, hence all results, are the same.  solver="MP2": MP2 has no
        iterations, `warm_start` changes nothing, and relax_density is not read (as in the reference's MP2 branch).  solver="FCI-hip": every sweep starts its Davidson
        iteration anew; relax_density is not read (as in the reference's FCI branch).  solver="SCI-hip": as "FCI-hip", every sweep
        selecting anew from the HF determinant with the cutoff of `solver_args` (SHCI_ArgsUser)."""
        from .opt import BEOPT
        from .jacobian import get_be_error_jacobian
        if solver not in SOLVERS:
            raise ValueError("Solver not implemented")
        if method != "QN":
            raise ValueError("This optimization method for BE is not supported")
        if not only_chem:
            pot = self.pot
            if self.fobj.n_BE == 1:
                raise ValueError("BE1 only works with chemical potential optimization. Set only_chem=True")
        else:
            pot = [0.0]
        be_ = BEOPT(pot, self.Fobjs, self.Nocc, self.enuc, solver=solver, only_chem=only_chem, use_cumulant=use_cumulant,
                    max_space=max_iter, conv_tol=conv_tol, relax_density=relax_density, ebe_hf=self.ebe_hf, solver_args=solver_args,
                    sweep=lambda p, **kw: self._sweep(p, solver=solver, **kw), verbose=self.rank == 0)
        if jac_solver == "Numerical":
            J0 = self.compute_numerical_jacobian(solver, only_chem, nproc, step_size=step_size, solver_args=solver_args)      # mbe.py:942-945
        else:
            J0 = get_be_error_jacobian(self.fobj.n_frag, self.Fobjs, jac_solver=jac_solver, owner=self.owner, rank=self.rank,
                                       world=self.world, opts=self.opts)
            if only_chem:
                J0 = J0[-1:, -1:]
        saved_opts = self.opts
        if warm_start:
            from ._lib import SolverOpts
            from .fragsolver import default_opts
            self.opts = SolverOpts.from_buffer_copy(saved_opts) if saved_opts is not None else default_opts(self.lib)
            self.opts.warm_start = 1
        try:
            be_.optimize(method, J0=J0, trust_region=trust_region)
        finally:
            self.opts = saved_opts
        self.pot = list(be_.pot)
        self.ebe_tot = be_.Ebe[0] + self.ebe_hf
        self.e_corr = be_.Ebe[0]
        self.e_components = be_.Ebe[1]
        self.beopt = be_
        if self.rank == 0:
            print(f"BE optimised  E_corr = {be_.Ebe[0]:.12f}  E_tot = {self.ebe_tot:.10f}  iterations = {be_.iter}", flush=True)
        return be_
