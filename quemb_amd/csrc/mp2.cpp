// mp2.cpp -- density-fitted fragment MP2 (see mp2.h).  Reference behaviour: molbe/solver.py:781-826 (`solve_mp2`: PySCF mp.MP2(mf).kernel()),
// mp2.make_rdm1 (unrelaxed) and the cumulant two-body term of get_frag_energy (molbe/helper.py:307-321), all as products with the fragment's factor.
#include "mp2.h"
#include "scf.h"

namespace qemb {

// Flops at n = 220, o = 20, naux = 660 (v = 200, o v = 4000): factor rotation 2 naux n^2 v + 2 naux n o v = 13.9e9, site rows 2 naux nf n^2,
// ovov 2 naux (o v)^2 = 21.1e9, Y the same: under 0.06 TFLOP, against 0.63 TFLOP of integral work before the first CCSD iteration.
int Mp2Solver::run_factor(int n, int o, int nf, int naux, const double* Bp, const double* C, const double* eps) {
  if (naux <= 0 || !Bp) { set_error("Mp2Solver: no factor"); return QEMB_ERR_ARG; }
  o_ = o; v_ = n - o; nf_ = nf; naux_ = naux; factor_ = true; ph_ready_ = false;
  const int64_t v = v_, n2 = (int64_t)n * n, nov = (int64_t)o * v;
  {
    DBuf Lu, Lhv;
    QTRY(Lu.alloc((int64_t)naux * n2)); QTRY(Lhv.alloc((int64_t)naux * n * v));
    QTRY(unpack_df_factor(n, naux, Bp, Lu));                                                           // B[L][p][q]
    QTRY(gemm((int64_t)naux * n, v, n, 1.0, Lu, n, true, C + o, n, false, 0.0, Lhv, v));              // Lhv[(L,p)][a] = sum_q B[L][p][q] C[q,o+a]: virtual columns only
    QTRY(Lov_.alloc((int64_t)naux * nov));
    QTRY(gemm(o, v, n, 1.0, C, n, false, Lhv, v, false, 0.0, Lov_, v, naux, 0, (int64_t)n * v, nov));   // Lov[L][i][a] = sum_p C[p,i] Lhv[L][p][a]
    Lhv.release();
    if (nf > 0) {      // site rows P < nf of B[L] C, as [P][L][i] and [P][L][a]: the right operands of Z2 and Z1
      DBuf tmp;
      QTRY(tmp.alloc((int64_t)naux * nf * std::max<int64_t>(o, v)));
      QTRY(LsoT_.alloc((int64_t)nf * naux * o)); QTRY(LsvT_.alloc((int64_t)nf * naux * v));
      QTRY(gemm(nf, o, n, 1.0, Lu, n, true, C, n, false, 0.0, tmp, o, naux, n2, 0, (int64_t)nf * o));
      QTRY(perm4(LsoT_, tmp, naux, nf, o, 1, 1, 0, 2, 3));
      QTRY(gemm(nf, v, n, 1.0, Lu, n, true, C + o, n, false, 0.0, tmp, v, naux, n2, 0, (int64_t)nf * v));
      QTRY(perm4(LsvT_, tmp, naux, nf, v, 1, 1, 0, 2, 3));
    }
  }
  QTRY(ovov_.alloc(nov * nov));
  QTRY(gemm(nov, nov, naux, 1.0, Lov_, nov, false, Lov_, nov, false, 0.0, ovov_, nov));              // (ia|jb) = sum_L Lov[L,(ia)] Lov[L,(jb)]
  return amplitudes(eps);
}

int Mp2Solver::run_blocks(MoIntegrals&& ints, const double* eps) {
  o_ = ints.o; v_ = ints.v; nf_ = ints.nf; naux_ = 0; factor_ = false; ph_ready_ = false;
  ovov_ = std::move(ints.ovov); A1_ = std::move(ints.A1); A2_ = std::move(ints.A2);
  ints = MoIntegrals();      // ovvv, the ladder operands, ...: nothing of it is read
  return amplitudes(eps);
}

int Mp2Solver::amplitudes(const double* eps) {
  const int64_t o = o_, v = v_, N2 = o * o * v * v;
  DBuf part, e;
  QTRY(t2_.alloc(N2)); QTRY(G_.alloc(N2)); QTRY(part.alloc(dev_mp2_partial_count(o, v))); QTRY(e.alloc(1));
  QTRY(dev_mp2_amplitudes(o, v, ovov_, eps, eps + o, t2_, G_, part, e));
  return dev_d2h(&e_corr_, e, sizeof(double));
}

int Mp2Solver::rdm1_blocks(std::vector<double>& doo, std::vector<double>& dvv) {
  const int64_t o = o_, v = v_;
  if (!ph_ready_) { QTRY(perm4(ovov_, t2_, o, o, v, v, 0, 2, 1, 3)); ph_ready_ = true; }      // t2 at [i][a][j][b], over the integrals (not read again)
  DBuf d1, d2;
  QTRY(d1.alloc(o * o)); QTRY(d2.alloc(v * v));
  QTRY(gemm_nt(o, o, v * o * v, -1.0, ovov_, G_, 0.0, d1));      // doo[i,j] = -sum_(akb) t2[i,a,k,b] G[j,a,k,b]      (K = o v^2; split by dev_gemm)
  QTRY(gemm_tn(v, v, o * v * o, 1.0, ovov_, G_, 0.0, d2));       // dvv[a,b] = sum_(jci) t2[j,c,i,a] G[j,c,i,b]       (K = o^2 v)
  doo.assign((size_t)(o * o), 0.0); dvv.assign((size_t)(v * v), 0.0);
  QTRY(dev_d2h(doo.data(), d1, sizeof(double) * o * o));
  return dev_d2h(dvv.data(), d2, sizeof(double) * v * v);
}

// The ovov block of PySCF's MP2 2-RDM is 2 (2 t2 - t2^T) = 2 G (bra and ket are both first order; <eri, cumulant> / 2 = 2 E_MP2), twice the block the
// unrelaxed CCSD 2-RDM has at t1 = 0: hence the factor 2 on both intermediates.
int Mp2Solver::energy_intermediates(std::vector<double>& Z1, std::vector<double>& Z2) {
  const int64_t o = o_, v = v_, nf = nf_, nov = o * v, naux = naux_;
  Z1.assign((size_t)(o * nf), 0.0); Z2.assign((size_t)(v * nf), 0.0);
  if (nf <= 0) return 0;
  DBuf z1, z2;
  QTRY(z1.alloc(o * nf)); QTRY(z2.alloc(v * nf));
  if (factor_) {
    DBuf Y, Yt;
    QTRY(Y.alloc(naux * nov)); QTRY(Yt.alloc(naux * nov));
    QTRY(gemm(naux, nov, nov, 1.0, Lov_, nov, true, G_, nov, false, 0.0, Y, nov));      // Y[L,(ia)] = sum_(jb) Lov[L,(jb)] G[(jb),(ia)]
    QTRY(perm4(Yt, Y, 1, naux, o, v, 0, 2, 1, 3));                                      // [i][L][a]
    QTRY(gemm_nt(o, nf, naux * v, 2.0, Yt, LsvT_, 0.0, z1));                            // Z1[i,P] = 2 sum_(L,a) Y[L,i,a] Ls[L,P,o+a]
    QTRY(perm4(Yt, Y, 1, naux, o, v, 3, 1, 2, 0));                                      // [a][L][i]
    QTRY(gemm_nt(v, nf, naux * o, 2.0, Yt, LsoT_, 0.0, z2));                            // Z2[a,P] = 2 sum_(L,i) Y[L,i,a] Ls[L,P,i]
  } else {      // as CcsdSolver::energy_intermediates, G already in place
    DBuf a2p;
    QTRY(a2p.alloc(o * o * v * nf));
    QTRY(gemm_nn(o, nf, v * o * v, 2.0, G_, A1_, 0.0, z1));
    QTRY(perm4(a2p, A2_, o, o, v, nf, 1, 2, 0, 3));
    QTRY(gemm_tn(v, nf, o * v * o, 2.0, G_, a2p, 0.0, z2));
  }
  QTRY(dev_d2h(Z1.data(), z1, sizeof(double) * o * nf));
  return dev_d2h(Z2.data(), z2, sizeof(double) * v * nf);
}

}  // namespace qemb
