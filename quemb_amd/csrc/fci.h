// fci.h -- determinant-space FCI of one embedding problem on the device: what `fci.FCI(mf, mo_coeff).kernel()`, make_rdm1 and make_rdm2 do for
// solver == "FCI" of be_func (molbe/solver.py:339-342, :507-528).  Occupation strings and link tables on the host (once per (n, nsocc), kept on the device),
// the Hamiltonian in Knowles-Handy form -- two gather passes around one FP64 product (fci_ops.hip, dev_gemm), over one slab of alpha rows at a time --, a
// Davidson-Liu iteration with the basis on the device and the small eigenproblem on the host (shared with sci.cpp), the 1- and 2-RDM from one more product of D
// with itself.  Plain C++ over dev_ops.h.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>
#include "tensor_utils.h"

namespace qemb {

struct FciOptions {
  double conv_tol = 1e-9;      // ||H c - E c||_2
  int max_cycle = 100;         // applications of H
  int max_space = 12;          // basis vectors before the collapse to the Ritz vector
  double lindep = 1e-14;       // a correction whose norm falls below this after orthogonalisation is dropped
};

// strings of one spin in lexical order and, for every string I, the nlink = nsocc (n - nsocc + 1) pairs (p,q) with <I|E_pq|J> = +-1 (the diagonal ones included);
// device copies in the layouts of dev_ops.h
struct FciTables {
  int n = 0, nsocc = 0, nlink = 0;
  int64_t ns = 0;
  std::vector<int32_t> strings, links;      // host: strings[I]; links[l * ns + I]
  int32_t* strings_dev = nullptr;
  int32_t* links_dev = nullptr;
  int64_t ndet() const { return ns * ns; }
};
// built on first use, uploaded once and kept for the life of the process (one table per (n, nsocc); any execution context may read it)
int fci_tables(int n, int nsocc, const FciTables** out);
int64_t fci_string_count(int n, int nsocc);
// Slabs: D and G hold the columns of `rows` alpha strings at a time (all beta strings: rows * ns determinants, contiguous in c), and one application of H, or
// one RDM build, walks the ceil(ns / rows) slabs in ascending order.  rows <= 0 is the whole space in one slab, and so is rows >= ns.
//   fci_bytes_slab: device bytes of a solve -- D and G (2 x 8 n^2 min(rows, ns) ns), the Davidson basis, its images and four work vectors
//                   ((2 max_space + 4) x 8 N_det), the tables and the n^4 pieces
//   fci_slab_count: ceil(ns / rows), 1 when rows <= 0
//   fci_rows_that_fit: the largest rows <= ns whose fci_bytes_slab is at most `room` bytes; 0 when not even one row fits
int64_t fci_bytes_slab(int n, int nsocc, int max_space, int64_t rows);
int64_t fci_slab_count(int64_t ns, int64_t rows);
int64_t fci_rows_that_fit(int n, int nsocc, int max_space, double room);

// k_pq = h_pq - 1/2 sum_r (pr|rq) on the host (h, V: [n][n] and [n^2][n^2] host arrays)
void fci_one_body(int n, const double* h, const double* V, double* k);

// one application of H: sigma = H c, slab by slab through dev_fci_gather_slab, dev_gemm and dev_fci_sigma_slab.  k_dev [n^2], V_dev [n^2][n^2]; D, G: work space of
// n^2 R ns doubles each, R = min(rows, ns) alpha rows per slab (rows <= 0: R = ns, one slab); for a given R two calls give the same bits
int fci_apply(const FciTables& T, const double* k_dev, const double* V_dev, const double* c, double* D, double* G, double* sigma, int64_t rows = 0);

struct FciResult { double e = 0.0, residual = 0.0; int n_iter = 0; bool converged = false; };
// lowest state of the M_s = 0 space of H(h, V) with nelec = (nsocc, nsocc); c (N_det doubles, device) receives the normalised vector, largest-magnitude component
// positive.  h_host: [n][n]; V_dev: [n^2][n^2] on the device.  rows: the slab height of every application of H (0: one slab, and the plain sum for |c|^2; > 0: the
// compensated one); the working set is fci_bytes_slab.  The start vector is the unit vector at the lowest diagonal element.
int fci_davidson(const FciTables& T, const double* h_host, const double* V_dev, const FciOptions& opt, double* c, FciResult* res, int64_t rows = 0);

// what the selected CI of sci.cpp shares with the solver above
namespace fci_detail {
// Davidson-Liu for the lowest eigenpair of a symmetric operator of dimension N given by y = apply(x) (device vectors) and its diagonal hdiag (device; the
// preconditioner dev_fci_precond): the basis and its images on the device (2 min(max_space, N) vectors, and two work vectors), the small eigenproblem on the host,
// every correction orthogonalised twice, collapse to the Ritz vector when the basis is full.  c: on entry the normalised start vector, on return the eigenvector
// with |c| = 1 (compensated: |c|^2 summed with Neumaier's compensation) and its largest-magnitude component positive.  res->n_iter counts the applications.
int davidson(int64_t N, const std::function<int(const double*, double*)>& apply, const double* hdiag, double conv_tol, int max_cycle, int max_space, double lindep,
             bool compensated, double* c, FciResult* res);
// the small symmetric eigenproblem (cyclic Jacobi; A [m][m] is overwritten, w ascending, eigenvectors in the columns of V), host[j] = <x, ys[j]> and
// out = sum_j coef[j] xs[j] (+ out) eight vectors per pass (scratch: >= 8 doubles on the device)
void small_eigh(int m, std::vector<double>& A, std::vector<double>& w, std::vector<double>& V);
int dots(int64_t N, const double* x, const std::vector<const double*>& ys, double* scratch, double* host);
int combine(int64_t N, const std::vector<double>& coef, const std::vector<const double*>& xs, bool accumulate, double* out);
// dm1 <- (dm1 + dm1^T) / 2 on the host
void symmetrise_dm1(int n, double* dm1);
}  // namespace fci_detail

// dm1[p,q] = sum_I c_I D[pq][I] (host, symmetrised) and, when dm2_dev != null, dm2[p,q,r,s] = <p+ r+ s q> (n^4 doubles, device); o_cum >= 0: minus the mean-field part.
// Slab by slab as fci_apply (dm1 += D_s c_s, A += D_s D_s^T), D at n^2 R ns doubles
int fci_rdm12(const FciTables& T, const double* c, int o_cum, double* dm1_host, double* dm2_dev, int64_t rows = 0);

}  // namespace qemb
