/*
 * det6d_ext.h — C ABI of libdet6d_hip_ext.so, the extension library of entry points that have no twin in the CPU oracle
 * (oracle/libdet6d_oracle.so).  Each of them comes with an executable CPU model under tests/models/ instead
 * ("The extension library").  Conventions are those of det6d_ops.h: device pointers, caller-owned buffers,
 * asynchronous on `stream`, DET6D_OK or a negative DET6D_E* code, never exit().
 */
#ifndef DET6D_EXT_H
#define DET6D_EXT_H

#include "det6d_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

/* library identification: "det6d-hip-ext gfx950 <abi-version>" */
const char *det6d_ext_version(void);
/* last error seen by this library on the calling thread: a bad argument or a failed launch ("" if none) */
const char *det6d_ext_last_error(void);

/* ------------------------------------------------------------------ F-FPS --------------- */

/* F-FPS: farthest point sampling on the fused distance d(i, j) = cdist(xyz)(i, j) + cdist(features)(i, j) * gamma of the
 * reference's f-fps sampler (pointnet2_modules.py:382-387 -> pointnet2_utils.py:37-44 + sampling_gpu.cu:268-373), without
 * the B x n x n matrix.  Points are rows [x, y, z, f_0 .. f_{c-1}, pad] of `rows` (b, n_total, ld); scene s samples m points
 * of its slice [lo, hi) and writes pick + lo + idx_bias to idx[s * idx_stride + idx_offset + r] (r = 0 .. m-1).
 * Arithmetic (exact, tests/models/ffps.py): |v|^2 a sequential sum of rounded squares in channel order; G(i, j) one
 * ascending fmaf chain from 0 over (-2 v_i) . v_j, then + |v_i|^2, then + |v_j|^2 (i = the last pick, j = the candidate);
 * d = sqrtf(clamp(G_xyz)) + sqrtf(clamp(G_feat)) * gamma, clamp(g) = g <= 0 ? 0 : g (NaN stays NaN); the reference's
 * selection rule (first pick 0, min-distances from 1e10, d2 = fminf(d, temp), strict > per thread, halving tree).
 * Limits: 1 <= hi - lo <= 16384, 0 <= c <= 256, c + 3 <= ld, ld % 4 == 0, `rows` 16-byte aligned, m >= 0.
 * `workspace` holds at least det6d_ext_fps_features_workspace_bytes(b, hi - lo) bytes; its last b * 128 bytes are, after
 * the launch, uint32 counters [b][16 waves][2]: point-rounds whose feature row was read, and wave-rounds that read any. */
long long det6d_ext_fps_features_workspace_bytes(int b, int n);
int det6d_ext_fps_features(int b, int n_total, int lo, int hi, int m, const float *rows, int ld, int c, float gamma,
                           void *workspace, long long ws_bytes, int *idx, int idx_stride, int idx_offset, int idx_bias,
                           det6d_stream_t stream);

/* furthest_point_sampling_matrix_wrapper(b, n, m, matrix, temp, idx) (sampling.cpp -> sampling_gpu.cu:268-373): FPS on a
 * caller-supplied (b, n, n) distance matrix; temp (b, n) holds the initial min-distances (the reference fills 1e10) and the
 * final ones afterwards; idx (b, m).  The selection core of det6d_ext_fps_features.  1 <= n <= 16384, m >= 0. */
int det6d_ext_fps_matrix(int b, int n, int m, const float *matrix, float *temp, int *idx, det6d_stream_t stream);

/* ------------------------------------------------------------------ C-FPS --------------- */

/* C-FPS: the m points of a slice with the highest sigmoid(score) ** gamma, in descending order — the reference's
 * scores_slice.sigmoid() ** WEIGHT_GAMMA followed by .topk(npoint) (pointnet2_modules.py:425-430).  Scene s ranks the slice
 * [lo, hi) of `scores` (b, n_total) and writes k + lo + idx_bias to idx[s * idx_stride + idx_offset + r] (r = 0 .. m-1).
 * Weights: w[k] = d6_sigmoid_powf(scores[s, lo + k], gamma) (det6d_math.h), the bits S-FPS sees.
 * Order (exact, tests/models/score_topk.py): larger w first; NaN counts as larger than every number, as in torch.topk; among
 * equal w (-0 equals +0) and among NaNs the lower index first.  torch.topk leaves the order of equal values open; this rule is
 * one of the orders it may produce and the one this library guarantees.
 * Limits: 1 <= hi - lo <= 16384, 0 <= m <= hi - lo, idx_offset >= 0, idx_offset + m <= idx_stride. */
int det6d_ext_topk_scores(int b, int n_total, int lo, int hi, int m, const float *scores, float gamma, int *idx,
                          int idx_stride, int idx_offset, int idx_bias, det6d_stream_t stream);

/* ------------------------------------------------------------------ DF-FPS -------------- */

/* The weights of the reference's df-fps sampler (pointnet2_modules.py:389-414): 1 / (points of the same scene and slice in
 * the same 2 m x 2 m pillar).  xyz (b, n_total, 3); weights (b, hi - lo), dense.  With the constants of that branch (range
 * origin x = 0, y = -39.68, scale_y = 40), in fp32: cx = floor((x - 0.0f) / 2.0f), cy = floor((y - (-39.68f)) / 2.0f),
 * key = cx * 40 + cy; count[k] = points of the scene's slice whose key equals key[k] (a point outside the range counts with
 * whatever pillar its key collides with); weights[s, k] = 1.0f / (float)count[k], correctly rounded.
 * (tests/models/pillar_density.py.)  The picks are det6d_fps_weights(xyz slice, weights, m) of det6d_ops.h.
 * Counts are PER SCENE.  The reference adds batch_index * 1400 to the key and counts over the batch, so that a point with
 * cx >= 35 or a negative key shares a count with a pillar of a neighbouring scene of the batch; here a scene's weights
 * never depend on its neighbours.  The two agree for every scene whose keys lie in [0, 1400) and for batches of one scene.
 * Input domain: finite coordinates with |x|, |y| <= 1e6; beyond it the reference's float -> long conversion of the pillar
 * coordinate is itself undefined, and so is the result here.
 * Limits: 1 <= hi - lo <= 16384. */
int det6d_ext_pillar_weights(int b, int n_total, int lo, int hi, const float *xyz, float *weights, det6d_stream_t stream);

/* ------------------------------------------------------------------ target assignment -- */

/* Which full-pose box does each point lie in — the reference's box_utils.points_in_boxes3d (box_utils.py:336-350, a host-side
 * Delaunay hull test per box) and the two label assignments PointHeadBox6DVote builds on it (point_head_box6d_vote.py:171-326
 * with set_ignore_flag=False), as one kernel.
 * points (n_points, ld_points): coordinates in columns xyz_col .. xyz_col + 2; the scene of row r is (int)points[r][bs_col] when
 * bs_col >= 0 (rows of any scene in any order) and r / n_per_scene otherwise.  A row whose scene is not in [0, b) (NaN
 * included) is background.  boxes (b, m, ld_boxes): columns 0 .. 8 are [x, y, z, dx, dy, dz, rz, ry, rx]; extra_width (3 floats
 * or NULL = zeros) is added to dx, dy, dz (box_utils.enlarge_box3d).
 * box_idx[r] = the HIGHEST index of a box of the row's scene that contains the point, -1 if none (the reference assigns box
 * by box in ascending order, the last assignment stays).
 * Arithmetic (exact, tests/models/box_targets.py; every fp32 operation rounded once, nothing contracted):
 *   per box: (s*, c*) = d6_sincosf of rz, ry, rx (det6d_math.h); R = Rx(rx) Ry(ry) Rz(rz) (scipy's 'zyx' of
 *   box_utils.py:57-71), with t = sx*sy and u = cx*sy:
 *     R00 = cy*cz           R01 = -(cy*sz)        R02 = sy
 *     R10 = cx*sz + t*cz    R11 = cx*cz - t*sz    R12 = -(sx*cy)
 *     R20 = sx*sz - u*cz    R21 = sx*cz + u*sz    R22 = cx*cy
 *   w_k = d_k + extra_k; half_k = 0.5f * w_k; the box takes part only if w_x > 0 and w_y > 0 and w_z > 0 (NaN fails: the
 *   all-zero rows that pad gt_boxes contain nothing, as in the reference);
 *   per pair: d = p - c (fp32), l_k = fmaf(d_z, R2k, fmaf(d_y, R1k, d_x * R0k)); inside iff fabsf(l_k) <= half_k for
 *   k = x, y, z (a NaN anywhere: outside).  Of the boxes that contain the point the one with the highest index is taken.
 * Limits: 0 <= n_points <= 2^24, 0 <= b <= 4096, 0 <= m <= 1024, 3 <= ld_points <= 1024, 0 <= xyz_col <= ld_points - 3,
 * bs_col < ld_points, n_per_scene >= 1 when bs_col < 0, 9 <= ld_boxes <= 1024.  With n_points == 0, b == 0 or m == 0 nothing is
 * launched and nothing is written (no box: the caller's outputs keep their fill, -1 / 0). */
int det6d_ext_points_in_boxes9(int n_points, const float *points, int ld_points, int xyz_col, int bs_col, int n_per_scene,
                               int b, int m, const float *boxes, int ld_boxes, const float *extra_width, int *box_idx,
                               det6d_stream_t stream);

/* det6d_ext_points_in_boxes9 plus the labels of the head, in the same launch.  For a point inside a box, with d = p - c of the
 * winning box (the fp32 differences above): near = central_radius <= 0 (no ball constraint), or else, in double, each operation
 * rounded once, ((double)d_x*d_x + (double)d_y*d_y) + (double)d_z*d_z < (double)central_radius * (double)central_radius.
 *   cls_labels[r] = 0 outside every box; -1 inside but not near (ignored); otherwise 1 if num_class == 1 or class_col < 0,
 *                   else (long long)box[class_col];
 *   box_labels[r][0 .. n_cols) = columns 0 .. n_cols of the winning box if inside and near, zeros otherwise (columns from
 *                   n_cols to ld_box_labels are left alone).  n_cols = 3: the vote targets; n_cols = 9: point_box_labels.
 * Any of box_idx, cls_labels, box_labels may be NULL (not all three).
 * Further limits: class_col < ld_boxes, num_class >= 1, central_radius not NaN, 0 <= n_cols <= ld_boxes,
 * n_cols <= ld_box_labels <= 1024. */
int det6d_ext_assign_targets9(int n_points, const float *points, int ld_points, int xyz_col, int bs_col, int n_per_scene,
                              int b, int m, const float *boxes, int ld_boxes, const float *extra_width, int class_col,
                              int num_class, float central_radius, int *box_idx, long long *cls_labels, float *box_labels,
                              int ld_box_labels, int n_cols, det6d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DET6D_EXT_H */
