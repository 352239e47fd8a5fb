// region_workspace_hostcheck.cpp -- dev_region_workspace_reserve (dev_ops.h) for the mock device layer of tests/hostcheck.  Everything below is compiled only with
// -DQEMB_HOSTCHECK: in the product build this file is an empty object and dev_ops_hip.hip provides the operation.  The mock neither captures nor splits K: its
// products are plain loops without a workspace, so there is nothing to reserve.
#ifdef QEMB_HOSTCHECK
#include "dev_ops.h"

namespace qemb {

int dev_region_workspace_reserve(size_t) { return 0; }

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
