// smx_cscale_host.h -- the host arithmetic of cross-scale aggregation (include/smx.h, above smx_cscale_params): the parameter
// check, a level's geometry and the levels' weights.  Plain C++ without HIP, so that tests/host_cscale_check.cpp runs this very
// code under the sanitizers; smx_cscale_weights and smx_cscale_level (smx_capi.hip) and the launcher (smx_cscale.hip) call it.
#pragma once
#include <math.h>

#include "smx.h"

namespace smx {

inline bool cscale_params_ok(const smx_cscale_params* p) {
    return p && p->scales >= 1 && p->scales <= SMX_CSCALE_MAX_SCALES && isfinite(p->lambda) && p->lambda >= 0.0;
}

inline void cscale_level(int w, int h, int dmin, int size_d, int s, int* w_s, int* h_s, int* dmin_s, int* size_d_s) {
    for (int k = 0; k < s; ++k) { w = (w + 1) / 2; h = (h + 1) / 2; }
    const int lo = dmin >> s, hi = (dmin + size_d - 1) >> s;      // (arithmetic shifts: floor for negative labels)
    *w_s = w; *h_s = h; *dmin_s = lo; *size_d_s = hi - lo + 1;
}

// Row 0 of the inverse of the tridiagonal M (symmetric, so column 0: M x = e_0) by the Thomas elimination in double, each
// operation rounded on its own; tests/cscale_ref.py runs the same recurrence.  M is strictly diagonally dominant: no pivoting.
inline void cscale_weights(const smx_cscale_params* p, float* wt) {
    const int S = p->scales;
    const double off = -p->lambda;
    double c[SMX_CSCALE_MAX_SCALES], r[SMX_CSCALE_MAX_SCALES], x[SMX_CSCALE_MAX_SCALES];
    for (int i = 0; i < S; ++i) {
        const int nb = (i > 0 ? 1 : 0) + (i + 1 < S ? 1 : 0);
        const double d = 1.0 + p->lambda * (double)nb;
        const double m = i ? d - off * c[i - 1] : d;
        c[i] = off / m;
        r[i] = i ? (0.0 - off * r[i - 1]) / m : 1.0 / m;
    }
    x[S - 1] = r[S - 1];
    for (int i = S - 2; i >= 0; --i) x[i] = r[i] - c[i] * x[i + 1];
    for (int i = 0; i < S; ++i) wt[i] = (float)x[i];
}

}  // namespace smx
