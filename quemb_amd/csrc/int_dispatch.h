// int_dispatch.h -- the one place where the runtime angular momenta of an integral class become compile-time ones.  Each dispatcher calls f with
// std::integral_constant arguments (a generic lambda: `[&](auto A, auto B) { ... kernel<A(), B()> ... }`) and returns what f returns (an error code); the set of
// calls it can make is the set of instantiations of the class family.  The device files (int3c_ops.hip, int4c_ops.hip) pass "launch this kernel", the scalar
// restatements of the mock device layer (*_hostcheck.cpp) pass "loop over the items": a class exists in both or in neither.
#pragma once
#include <string>
#include <type_traits>
#include "int4c_core.h"

namespace qemb {

template <int V>
using LConst = std::integral_constant<int, V>;

// the six orbital pair classes ss ps pp ds dp dd (int4c::pair_class): f(la, lb)
template <class F>
int dispatch_pair(int cls, F&& f) {
  switch (cls) {
    case 0: return f(LConst<0>{}, LConst<0>{});
    case 1: return f(LConst<1>{}, LConst<0>{});
    case 2: return f(LConst<1>{}, LConst<1>{});
    case 3: return f(LConst<2>{}, LConst<0>{});
    case 4: return f(LConst<2>{}, LConst<1>{});
    default: return f(LConst<2>{}, LConst<2>{});
  }
}

// the 21 canonical quartet classes, ket pair class <= bra pair class: f(la, lb, lc, ld); any other class is refused and instantiates nothing
template <class F>
int dispatch_quartet(int bra_cls, int ket_cls, const char* who, F&& f) {
  return dispatch_pair(bra_cls, [&](auto A, auto B) {
    constexpr int bra = int4c::pair_class(A(), B());
    return dispatch_pair(ket_cls, [&](auto C, auto D) {
      if constexpr (int4c::pair_class(C(), D()) <= bra) return f(A, B, C, D);
      else { set_error(std::string(who) + ": not a canonical class"); return (int)QEMB_ERR_UNSUPPORTED; }
    });
  });
}

// the classes (la, lb|lp) of the DF integrals, la >= lb: the six orbital pair classes and (3,0|.), (4,0|.) -- auxiliary shells of the metric only
// (int3c_check_class) -- each with lp = 0..4: f(la, lb, lp)
template <class F>
int dispatch_int3c(int la, int lb, int lp, F&& f) {
  auto aux = [&](auto A, auto B) {
    switch (lp) {
      case 0: return f(A, B, LConst<0>{});
      case 1: return f(A, B, LConst<1>{});
      case 2: return f(A, B, LConst<2>{});
      case 3: return f(A, B, LConst<3>{});
      default: return f(A, B, LConst<4>{});
    }
  };
  if (la == 3) return aux(LConst<3>{}, LConst<0>{});
  if (la == 4) return aux(LConst<4>{}, LConst<0>{});
  return dispatch_pair(int4c::pair_class(la, lb), aux);
}

}  // namespace qemb
