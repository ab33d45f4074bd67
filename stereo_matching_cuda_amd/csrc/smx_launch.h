// Launchers implemented in smx_kernels.hip (all asynchronous on `st`).
#pragma once
#include "smx_common.h"

namespace smx {
int launch_gray(const smx_params* p, const uint8_t* rgb, int64_t n, int ch, uint8_t* gray, hipStream_t st);
int launch_cost(const smx_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w, int h,
                int d0, int count, hipStream_t st);
int launch_integral(int mode, const float* in0, const float* in1, float* out0, float* out1, int w,
                    int h, int nplanes, hipStream_t st);
int launch_guid_prep(const uint8_t* I, float* im, float* sq, int64_t n, hipStream_t st);
int launch_guid_finish(const smx_params* p, const float* S_im, const float* S_sq, float* mean_im,
                       float* cinv, uint8_t* mean_u8, int w, int h, hipStream_t st);
int launch_ab(const smx_params* p, const float* Sp, const float* SIp, const float* mean_im,
              const float* cinv, float* A, float* B, int w, int h, int nplanes, hipStream_t st);
// (nbr != NULL: the pass also keeps the winners' neighbours in the view's state planes [3][h][w]; uq != NULL: their
// second-best cost, in planes of the same shape)
int launch_q_wta(const smx_params* p, const float* Sa, const float* Sb, const float* im,
                 int64_t* keys, float* nbr, float* uq, float* agg, int w, int h, int count, int slice0, hipStream_t st);
int launch_init_keys(int64_t* keys, int64_t n, hipStream_t st);
int launch_init_wta(float* best, float* dmap, int64_t n, hipStream_t st);
int launch_apply_keys(const int64_t* keys, int64_t n, int dmin, float* best, float* dmap, hipStream_t st);
int launch_detect_occlusion(const smx_params* p, float* dL, const float* dR, int dOcc, int w, int h,
                            hipStream_t st);
int launch_fill_occlusion(const float* src, float* disp, int w, int h, float vMin, hipStream_t st);
int launch_finish_keys(const int64_t* keys, int64_t n, int dminl, int dminr, float* best, float* dmap,
                       float* occlusion, hipStream_t st);
int launch_filter(const smx_params* p, const uint8_t* I, uint8_t* mean, float* var, int w, int h,
                  hipStream_t st);
bool finish_pair_row_supported(int w);
int launch_finish_pair_row(const smx_params* p, const int64_t* keys, int w, int h, int dminl, int dminr, int dOcc,
                           float vMin, float* best, float* dmap, float* occlusion, float* filled, hipStream_t st);
// smx_wmf.hip: weighted median (ws: spatial weights [0 .. 2 r^2], wc: range weights [0 .. 255])
int wmf_bucket_shift(int size_d);
int launch_weighted_median(int radius, const uint16_t* ws, const uint16_t* wc, const uint8_t* guide, const float* disp,
                           const float* select, float* out, int w, int h, int dmin, int size_d, hipStream_t st);
// smx_subpix.hip: sub-pixel maps of both views (smx_dev_subpixel_pair)
int launch_subpixel_pair(int mode, const int64_t* keys, const float* nbr, const float* dmap, const float* occlusion,
                         const float* filled, int w, int h, int dminl, float* sub, float* sub_filled, hipStream_t st);
// smx_census.hip: census codes of nimages planes; Hamming cost slices [s_begin, s_end) of one or both views (t = min(th, nbits))
int launch_census(int rx, int ry, const uint8_t* img, uint64_t* code, int w, int h, int nimages, hipStream_t st);
int launch_census_cost_pair(int t, const uint64_t* code, float* cost_l, float* cost_r, int w, int h, int dminl, int dminr,
                            int s_begin, int s_end, hipStream_t st);
// smx_adcensus.hip: AD-Census cost slices [s_begin, s_end) of one or both views (t = min(th, nbits); nch = 1 or 3 channels in
// the AD term; ch = bytes per pixel of img_l / img_r: 1, 3 or 4; table: SMX_ADCENSUS_TABLE_FLOATS floats on the device)
int launch_adcensus_cost_pair(int t, int nch, const float* table, const uint64_t* code, const uint8_t* img_l, const uint8_t* img_r,
                              int ch, float* cost_l, float* cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end,
                              hipStream_t st);
// smx_mi.hip: the mutual-information cost -- the joint histogram of a left map (the launch zeroes hist first), the table of a
// histogram on the host, the random start map, and the cost slices [s_begin, s_end) of one or both views from a device table
int launch_mi_histogram(const uint8_t* img_l, const uint8_t* img_r, const float* map, float mark, uint32_t* hist, int w, int h,
                        hipStream_t st);
void mi_table(const uint32_t* hist, uint8_t* table);
int launch_mi_random_map(float* map, int w, int h, int dmin, int size_d, uint32_t seed, hipStream_t st);
int launch_mi_cost_pair(const uint8_t* table, const uint8_t* img_l, const uint8_t* img_r, float* cost_l, float* cost_r, int w,
                        int h, int dminl, int dminr, int s_begin, int s_end, hipStream_t st);
// smx_zncc.hip: the ZNCC window cost -- the window moments {S, V} of nimages planes (8 bytes a pixel) and the cost slices
// [s_begin, s_end) of one or both views from them and the images; zncc_geometry: columns and rows of a cost workgroup
void zncc_geometry(int* cols, int* rows);
int launch_zncc_moments(int rx, int ry, const uint8_t* img, uint64_t* mom, int w, int h, int nimages, hipStream_t st);
int launch_zncc_cost_pair(int rx, int ry, const uint64_t* mom, const uint8_t* img_l, const uint8_t* img_r, float* cost_l,
                          float* cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end, hipStream_t st);
// smx_speckle.hip: the connected-component filter (smx_dev_speckle_filter); ws: speckle_workspace_bytes(w, h) bytes
size_t speckle_workspace_bytes(int w, int h);
int launch_speckle_filter(int max_size, float max_diff, const float* disp, float* out, int w, int h, float vmin,
                          float new_val, void* ws, hipStream_t st);
void speckle_tile(int* tw, int* th);
// smx_sgm.hip: semi-global matching of one or both whole cost volumes (smx_dev_sgm_wta_pair); ws: sgm_workspace_bytes bytes
int sgm_padded_d(int size_d);
size_t sgm_workspace_bytes(int w, int h, int size_d, int nviews);
int launch_sgm_wta_pair(int p1, int p2, int paths, const float* cost_l, const float* cost_r, int w, int h, int size_d,
                        int64_t* keys, float* agg, float* nbr, float* uq, void* ws, hipStream_t st);
// smx_bp.hip: hierarchical belief propagation of one or both whole cost volumes (smx_dev_bp_wta_pair); ws: bp_workspace_bytes bytes
size_t bp_workspace_bytes(int w, int h, int size_d, int levels, int nviews);
int launch_bp_wta_pair(const smx_bp_params* p, const float* cost_l, const float* cost_r, int w, int h, int size_d, int64_t* keys,
                       float* agg, float* nbr, float* uq, void* ws, hipStream_t st);
// smx_scanline.hip: the scan-line optimiser with colour-adaptive penalties (smx_dev_scanline_wta_pair); both guides always
size_t scanline_workspace_bytes(int w, int h, int size_d, int nviews);
int launch_scanline_wta_pair(const smx_scanline_params* p, const uint8_t* guide_l, const uint8_t* guide_r, int ch,
                             const float* cost_l, const float* cost_r, int w, int h, int size_d, int dminl, int dminr,
                             int64_t* keys, float* agg, float* nbr, float* uq, void* ws, hipStream_t st);
// smx_uniq.hip: the uniqueness test on a disparity map (smx_dev_uniqueness)
int launch_uniqueness(float ratio, const int64_t* keys, const float* uq, const float* disp, float* out, float* margin, int64_t n,
                      float vmin, float new_val, hipStream_t st);
// smx_cgf.hip: the colour-guided filter aggregation (smx_dev_cgf_wta_pair); ws: cgf_workspace_bytes bytes for the slices in
// flight, chunk: cgf_chunk of that workspace (>= 1)
size_t cgf_workspace_bytes(int w, int h, int nslices, int nviews);
int cgf_chunk(int w, int h, int nviews, size_t ws_bytes, int count, int max_chunk);
int launch_cgf_wta_pair(const smx_params* p, const uint8_t* rgb_l, const uint8_t* rgb_r, int ch, const float* cost_l,
                        const float* cost_r, int w, int h, int s_begin, int s_end, int64_t* keys, float* agg, float* nbr,
                        float* uq, void* ws, int chunk, hipStream_t st);
// smx_cross.hip: cross-based aggregation (smx_dev_cross_wta_pair); ws: cross_workspace_bytes bytes for the slices in flight,
// chunk: cross_chunk of that workspace (>= 1)
size_t cross_workspace_bytes(int w, int h, int nslices, int nviews);
int cross_chunk(int w, int h, int nviews, size_t ws_bytes, int count, int max_chunk);
int launch_cross_arms(const smx_cross_params* p, const uint8_t* guide_l, const uint8_t* guide_r, int ch, int w, int h,
                      uint32_t* arms, hipStream_t st);
int launch_cross_wta_pair(const smx_cross_params* p, const uint8_t* guide_l, const uint8_t* guide_r, int ch, const float* cost_l,
                          const float* cost_r, int w, int h, int s_begin, int s_end, int64_t* keys, float* agg, float* nbr,
                          float* uq, void* ws, int chunk, hipStream_t st);
// smx_vote.hip: region voting and interpolation on the cross arms (smx_dev_region_vote); ws: vote_workspace_bytes(w, h) bytes
size_t vote_workspace_bytes(int w, int h);
int launch_region_vote(const smx_vote_params* p, const uint32_t* arms, const uint8_t* guide, int ch, const float* disp,
                       const float* disp_r, float* out, int w, int h, int dmin, int size_d, int d_lr, void* ws, hipStream_t st);
void vote_tile(int* tw, int* th);
// smx_adjust.hip: depth-discontinuity adjustment from the aggregated costs (smx_dev_discontinuity_adjust); ws:
// adjust_workspace_bytes(w, h) bytes
size_t adjust_workspace_bytes(int w, int h);
int launch_discontinuity_adjust(const smx_adjust_params* p, const float* disp, const float* vol, float* out, int w, int h, int dmin,
                                int size_d, int mode, float* sub, void* ws, hipStream_t st);
void adjust_tile(int* tw, int* th);
// smx_cscale.hip: cross-scale aggregation -- one level of the u8 pyramid, and the combination with its winner-take-all pass
// (smx_dev_cscale_wta_pair; agg_l / agg_r: host arrays of p->scales device pointers, either may be NULL).  The host arithmetic
// (a level's geometry, the weights) is smx_cscale_host.h
int launch_pyr_down(const uint8_t* src, uint8_t* dst, int w, int h, int ch, hipStream_t st);
void pyr_down_tile(int* tw, int* th);
int launch_cscale_wta_pair(const smx_cscale_params* p, const float* const* agg_l, const float* const* agg_r, int w, int h, int dminl,
                           int dminr, int size_d, int64_t* keys, float* out, float* nbr, float* uq, hipStream_t st);
// smx_patchmatch.hip: PatchMatch stereo (smx_dev_patchmatch_pair, smx_dev_pm_plane_cost); ws: pm_workspace_bytes(w, h) bytes.
// planes [2][3][h][w], cost / disp / label [2][h][w], the left view first
size_t pm_workspace_bytes(int w, int h);
void pm_weights(const smx_pm_params* p, float* tab);
uint32_t pm_hash_host(uint32_t seed, uint32_t view, uint32_t pix, uint32_t draw);
int launch_patchmatch_pair(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h,
                           int size_d, int dminl, int dminr, float* planes, float* cost, float* disp, float* label, void* ws,
                           hipStream_t st);
int launch_pm_plane_cost(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h,
                         int size_d, int dminl, int dminr, const float* planes, float* cost, void* ws, hipStream_t st);
void pm_tile(int* tw, int* th);
// (a pair's sub-pixel filled map from PatchMatch: disp where `kept` passes fill_occlusion's validity test, `filled` elsewhere)
int launch_pm_sub_filled(const float* disp, const float* kept, const float* filled, size_t n, int dminl, float* out, hipStream_t st);
// smx_perm.hip: the permeability filter and the winner-take-all pass over it (smx_dev_permeability_wta_pair); table: the 256
// weights on the host (smx_perm_host.h); ws: perm_workspace_bytes bytes for the slices in flight, chunk: perm_chunk of that
// workspace (>= 1; own_out: the call keeps no volume, so the filtered slices live in the workspace too)
size_t perm_workspace_bytes(int w, int h, int nslices, int nviews);
int perm_chunk(int w, int h, int nviews, size_t ws_bytes, int count, bool own_out, int max_chunk);
int launch_perm_wta_pair(const float* table, const float* vol_l, const float* vol_r, const uint8_t* guide_l, const uint8_t* guide_r,
                         int ch, int w, int h, int size_d, int64_t* keys, float* out, float* nbr, float* uq, void* ws, int chunk,
                         hipStream_t st);
// smx_tree.hip: the non-local tree filter and the winner-take-all pass over it (smx_dev_tree_wta_pair); t, u: the two tables of
// 256 weights on the host (smx_tree_host.h); tree_l / tree_r: the views' tree blobs on the device; ws: tree_workspace_bytes
// bytes for the slices in flight, chunk: tree_chunk of that workspace (>= 1; own_out as in perm_chunk)
size_t tree_workspace_bytes(int w, int h, int nslices, int nviews);
int tree_chunk(int w, int h, int nviews, size_t ws_bytes, int count, bool own_out, int max_chunk);
int launch_tree_wta_pair(const float* t, const float* u, const float* vol_l, const float* vol_r, const uint8_t* tree_l,
                         const uint8_t* tree_r, int w, int h, int size_d, int64_t* keys, float* out, float* nbr, float* uq, void* ws,
                         int chunk, hipStream_t st);
}  // namespace smx
