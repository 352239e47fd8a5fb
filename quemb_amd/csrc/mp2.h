// mp2.h -- density-fitted MP2 of one embedded fragment on the device: solver == "MP2" of be_func (molbe/solver.py:313-317, solve_mp2 :781-826).
//
// After the fragment RHF (C, eps on the device) the factor route needs only products with the fragment's 3-index factor B[naux][npair(n)]:
//   Lov[L,(ia)] = C_o^T B[L] C_v              Ls[P][L][q'] = (B[L] C)[P,q'], P < nf (the site rows of the energies)
//   ovov = Lov^T Lov                          -> t2, G = 2 t2 - t2^T(ab), E_MP2 in one pass (dev_mp2_amplitudes)
//   doo = -t2 . G, dvv = t2 . G               (PySCF mp2.make_rdm1, unrelaxed; two long-K products)
//   Y = Lov G,  Z1[i,P] = 2 Ls[P,(L,a)] Y[i,(L,a)],  Z2[a,P] = 2 Ls[P,(L,i)] Y[a,(L,i)]  (the cumulant two-body energy without A1 / A2)
// No ovvv, vvvv, ladder operand or t2-sized work tensor beyond ovov, t2 and G exists.  A fragment that holds only its 4-fold packed block goes
// through mo_transform and uses its ovov, A1, A2 blocks (run_blocks).
#pragma once
#include <cstdint>
#include <vector>
#include "ccsd.h"

namespace qemb {

class Mp2Solver {
 public:
  // B_packed: [naux][npair(n)]; C: n x n MO coefficients (columns), eps: n orbital energies, all on the device; nf > 0: energies will be asked for
  int run_factor(int n, int o, int nf, int naux, const double* B_packed, const double* C, const double* eps);
  // the same from the blocks of mo_transform (ovov; A1, A2 when nf > 0); every other block of `ints` is released at once
  int run_blocks(MoIntegrals&& ints, const double* eps);
  double e_corr() const { return e_corr_; }
  const double* t2() const { return t2_.p; }         // [o][o][v][v]
  // doo[i,j] = -sum_kab t2[ikab] th[jkab], dvv[a,b] = sum_ijc t2[ijac] th[ijbc], th = 2 t2 - t2^T(ab)   (host, o*o and v*v; not yet symmetrised)
  int rdm1_blocks(std::vector<double>& doo, std::vector<double>& dvv);
  // Z1[i,P] = 2 sum_ajb G[iajb] (Pa|jb), Z2[a,P] = 2 sum_ijb G[iajb] (Pi|jb): the contraction of the ovov / vovo blocks of mp2.make_rdm2, which are 2 G --
  // twice what CcsdSolver::energy_intermediates yields at t1 = 0 (host, o*nf and v*nf)
  int energy_intermediates(std::vector<double>& Z1, std::vector<double>& Z2);

 private:
  int amplitudes(const double* eps);
  int o_ = 0, v_ = 0, nf_ = 0, naux_ = 0;
  bool factor_ = false;
  DBuf ovov_, t2_, G_;          // ovov_ holds t2 in the layout [i][a][j][b] once rdm1_blocks has run
  bool ph_ready_ = false;
  DBuf Lov_, LsoT_, LsvT_;      // factor route: Lov[L][(ia)], Ls[P][L][i], Ls[P][L][a]
  DBuf A1_, A2_;                // block route
  double e_corr_ = 0.0;
};

}  // namespace qemb
