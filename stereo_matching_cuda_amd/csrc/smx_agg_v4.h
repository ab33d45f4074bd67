// smx_agg_v4.h -- interface of the ring walker (smx_agg_v4.hip) towards the host orchestration of smx_agg.hip:
// strip / band / record geometry, argument block, eligibility, launchers.
#pragma once
#include "smx_agg_dev.h"

namespace smx {
namespace v4 {

using aggdev::PADX;
constexpr int OW = 64;                  // output columns per strip = one wave
constexpr int RMAX = 9;                 // largest supported box radius
constexpr int HWMAX = 2 * RMAX + 1;     // halo / overlap columns
// Band height 16: rings of 36 rows, 50 KB of LDS, three workgroups per CU, fewer idle rows at the bottom of a strip
// than with 32 (rings of 52 rows, 72 KB, two workgroups per CU)
constexpr int BH = 16;                  // band height
constexpr int WG_PER_CU = 3;

// Hand-off record of one iteration (per parity and slice-view), written and read in 16-byte units:
//   [0, BH)              stage-1 row carries of band i        (float2 per row)
//   [BH, 2 BH)           stage-2 row carries of band i-1
//   [2 BH, 2 BH + BH*HP) last 2R+1 columns of the stage-2 integral of band i-1, HP = 20 float2 per row
constexpr int HP = HWMAX + 1;
constexpr int REC_F2 = 2 * BH + BH * HP;          // float2 per record

inline int strips(int w, int R) { return (w + R + OW - 1) / OW; }
inline int bands(int h, int R) { return (h - 1 + 2 * R) / BH + 2; }     // the q rows of iteration i end at BH i - 2R
inline size_t sv_hand_floats(int h, int R) { return (size_t)2 * bands(h, R) * REC_F2 * 2; }   // parity x records x float2

struct View {
    const aggdev::fg_t* FG1;   // this view's image plane [h][w + 2 PADX], sentinel columns on either side
    const aggdev::fg_t* FG2;   // the other view's (costs built from the images)
    const float* cost;         // materialised costs: [slice][h][w]
    const aggdev::f2* guid;    // (mean_I, 1/(var_I + eps)) [h][w]
    float* q;                  // out: [slice][h][w]
    int d0;                    // disparity of local slice 0
};

struct Args {
    View v[2];
    int w, h, R, K, NI, nslices, nsv, nitems;
    aggdev::f2* hand;     // hand-off records [parity][sv][iteration] (see REC_F2)
    unsigned* flags;      // [sv][K]  published-record counters (zeroed before every launch)
    unsigned* ticket;     // work-item counter              (zeroed before every launch)
    unsigned* status;     // != 0: a flag wait timed out (results invalid)
    const unsigned* gate;      // != NULL: the launch does nothing unless this word is nonzero (the queued fall-back behind the comb walker)
    CostConst cc;
};

// What the guidance launches of one call read and write (device pointers; views beyond nviews stay NULL)
struct Guidance {
    const uint8_t* I[2];       // u8 images [h][w]: the views' guides; a single view's partner, if any, in I[1]
    aggdev::fg_t* FG[2];       // out: (value, x-derivative) planes [h][w + 2 PADX] of the images
    float* S0[2];              // per view: integral of I ...
    float* S1[2];              // ... and of I*I (scratch)
    aggdev::f2* G[2];          // out, per view: (mean_I, 1/(var_I + eps)) [h][w]
    uint8_t* mean_u8[2];       // out, per view, optional: mean_I as u8
    unsigned* zero[2];         // two word ranges the first launch clears (status words, control block of the first chunk):
    unsigned nzero[2];         // saves two fill launches per call
};

}  // namespace v4

bool v4_supported(const smx_params* p);          // radius 0 .. RMAX
// Image planes and guidance statistics of one call: k_v4_guid_rows, k_v4_guid_cols and -- `finish` -- k_v4_guid_finish
// (G, mean_u8 from the integrals).  finish == false: the caller's v5_perm_launch takes the third launch's place.  cols == false
// (with finish == false): k_v4_guid_rows alone -- S0 / S1 are left as ROW prefixes for the caller's v5_guid_block_launch.
int v4_guidance_launch(const v4::Guidance& g, int nviews, int w, int h, int R, double eps, bool finish, bool cols, hipStream_t st);
// the walker over a.nitems items: costs from a.v[].cost or built from the image planes; fast: the FAST mode (not bit-exact)
int v4_walk_launch(const v4::Args& a, bool use_cost, bool fast, hipStream_t st);

}  // namespace smx
