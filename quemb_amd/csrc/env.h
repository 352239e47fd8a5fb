// env.h -- the one way the library reads its environment (host code only; compiled by the product build and by the host-check build).
// Every QEMB_* switch goes through one of the four readers below with its name as a string literal, and is listed in the switch table of DESIGN.md section 5:
// tests/test_boundary_docs.py holds the two sets equal.  A call site keeps its value in a `static const`, so a switch is read once per process.
#pragma once
#include <cstdlib>
#include <cstring>

namespace qemb {

// the value of a switch; unset and empty are the same thing (nullptr)
inline const char* env_str(const char* name) { const char* e = std::getenv(name); return (e && e[0]) ? e : nullptr; }
// unset or empty: the default; a leading '0': off; anything else: on
inline bool env_flag(const char* name, bool dflt) { const char* e = env_str(name); return e ? e[0] != '0' : dflt; }
inline long long env_int(const char* name, long long dflt) { const char* e = env_str(name); return e ? std::atoll(e) : dflt; }
inline double env_real(const char* name, double dflt) { const char* e = env_str(name); return e ? std::atof(e) : dflt; }

// a run under rocprofv3 (its tool library is registered, or preloaded): such a run keeps eager launches instead of graph replay and plain streams instead of
// CU-masked ones (ccsd.cpp, dev_ops_hip.hip)
inline bool profiled_run() {
  static const bool on = [] {
    const char* pre = std::getenv("LD_PRELOAD");
    return std::getenv("ROCP_TOOL_LIBRARIES") != nullptr || (pre && std::strstr(pre, "rocprofiler"));
  }();
  return on;
}

}  // namespace qemb
