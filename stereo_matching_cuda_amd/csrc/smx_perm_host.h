// smx_perm_host.h -- the host arithmetic of the permeability filter (include/smx.h, above smx_perm_params): the parameter check
// and the weight table.  Plain C++ without HIP, so that tests/host_perm_check.cpp runs this very code under the sanitizers;
// smx_perm_table (smx_capi.hip), the launcher (smx_perm.hip) and the CPU twin (host/cpu_twins.cpp) call it.
#pragma once
#include <math.h>

#include "smx.h"

namespace smx {

inline bool perm_params_ok(const smx_perm_params* p) { return p && isfinite(p->sigma) && p->sigma > 0.0; }

// t[k] = (float)exp(-k / sigma) in double; t[0] == 1 whatever sigma is
inline void perm_table(const smx_perm_params* p, float* t) {
    for (int k = 0; k < 256; ++k) t[k] = (float)exp(-(double)k / p->sigma);
}

}  // namespace smx
