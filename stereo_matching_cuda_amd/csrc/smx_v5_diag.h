// smx_v5_diag.h -- observe-only instruments of the comb walker k_v5_walk (smx_agg_v5.hip, its only includer).  They
// change neither what the kernel computes nor how it launches, and the product build compiles them to nothing:
//   -DSMX_V5_STAMPS=<workgroup> [-DSMX_V5_STAMP_G0=<first global slot>]: every wave of one workgroup records the shader
//       clock at the V5_STAMP(n) sites of 48 global slots; read back with smx_debug_read_stamps5 (tools/v5_stamps.py)
//   -DSMX_V5_MARK: comments in the ISA around the interior-path regions tools/isa_budget.py counts (V5_MARK sites)
#pragma once
#include "smx_common.h"

#ifdef SMX_V5_STAMPS
namespace smx {
namespace v5 {
constexpr int STAMP_W = 12;     // 0..5: slot phases; 6..10: after each of the five row pairs (comb waves) / quarters of the scan / cost batches
constexpr int STAMP_SLOTS = STAMP_W * 48;
// (the stamps are those of ONE workgroup -- SMX_V5_STAMPS mod 512 -- over 48 global slots from STAMP_G0: its items overlap)
#ifndef SMX_V5_STAMP_G0
#define SMX_V5_STAMP_G0 30
#endif
constexpr int STAMP_G0 = SMX_V5_STAMP_G0;
__device__ unsigned long long g_stamps[10 * STAMP_SLOTS];
}  // namespace v5

extern "C" __attribute__((visibility("default"))) int smx_debug_read_stamps5(unsigned long long* out, int n) {
    const int m = 10 * v5::STAMP_SLOTS;
    SMX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(v5::g_stamps), sizeof(unsigned long long) * (n < m ? n : m)));
    return m;
}
}  // namespace smx

// (at a site: `lane`, `wave` and the global slot `i` of the enclosing code)
#define V5_STAMP(n)                                                                          \
    do {                                                                                     \
        if ((int)blockIdx.x == SMX_V5_STAMPS % 512 && lane == 0 && i >= STAMP_G0 && (i - STAMP_G0) * STAMP_W + (n) < STAMP_SLOTS) \
            g_stamps[wave * STAMP_SLOTS + (i - STAMP_G0) * STAMP_W + (n)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
#else
#define V5_STAMP(n) ((void)0)
#endif

#ifdef SMX_V5_MARK
#define V5_MARK(name) asm volatile("; MARK " name)
#else
#define V5_MARK(name) ((void)0)
#endif
