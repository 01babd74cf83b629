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

/* ------------------------------------------------------------------ training loss ------ */

/* The training loss of PointHeadBox6DVote (point_head_box6d_vote.py:426-776 with loss_utils.py:10-235) and its gradient with
 * respect to the predictions, for the PointBinResidual6DCoder code layout [6 offsets, angle_bin_num bin logits, angle_bin_num
 * bin residuals, then pitch_cls, pitch_res with DET6D_HEAD_LOSS_GROUND_AWARE, else pitch], LOSS_REG WeightedSmoothL1Loss
 * without code weights and LOSS_CLS WeightedBinaryCrossEntropyLoss[WithCenterness].  Executable model: tests/models/head_loss.py.
 * Row r of every tensor is one point; all tensors are dense: vote_preds (n, 3) = the vote coordinates, vote_reg_labels (n, 3),
 * vote_cls_labels (n) int64, cls_preds (n, num_class), cls_labels (n) int64 (-1 ignored, 0 background, c > 0 class c),
 * reg_preds and reg_labels (n, code_size), box_labels (n, ld_box_labels) = [x, y, z, dx, dy, dz, rz, ...].
 * With sl(d) = 0.5 d^2 / beta if |d| < beta else |d| - 0.5 beta (|d| itself when beta < 1e-5), pos = cls_label > 0,
 * valid = cls_label >= 0, bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)):
 *   vote_r = [vote_cls_label > 0] * sum_k sl(vote_preds - vote_reg_labels);
 *   cen_r  = pos ? cbrt(max(rl * rw * rh, 1e-6)) : 0, the ratios min / max of the distances to the two faces along each axis
 *            of the label box, in the frame turned about z by the LAST column of box_labels (rx for nine columns: the
 *            reference's behaviour); t_r = cmin + (cmax - cmin) * cen_r with DET6D_HEAD_LOSS_CENTERNESS, else 1;
 *   cls_r  = valid * w_cls * mean_c bce(cls_preds[c], pos and c == cls_label - 1 ? t_r : 0);
 *   box_r  = pos * (w_off * sum_{k<6} sl(pred_k - label_k) + w_acls * (logsumexp(bin logits) - logit[lb])
 *            + w_areg * sl(pred residual[lb] - label residual[lb]) + w_pcls * focal(pitch_cls))
 *            + w_preg * pw * S * sl(pitch_res difference) + pos * w_corner * corner_r,
 *            lb = the first maximum of the label's bin columns, focal(x) with t = the pitch_cls label:
 *            (0.25 t + 0.75 (1 - t)) * pt^2 * bce(x, t), pt = t (1 - sigmoid x) + (1 - t) sigmoid x;
 *            pw = pitch_cls label > 0 (ground aware) or pos (otherwise); S = max(#pos, 1) / max(#pw, 1);
 *   corner_r (DET6D_HEAD_LOSS_CORNER) = mean over the 8 yaw-only corners of min(sum_xyz sl1(P - G), sum_xyz sl1(P - G')),
 *            beta 1, P the corners of the decoded box (centre = offsets + vote point, sizes = exp, yaw = (db + residual[db])
 *            * 2 pi / angle_bin_num, db = the first maximum of the bin logits), G those of box_labels[0 .. 6], G' of the
 *            label turned by pi.  Rows that are not pos contribute exactly 0 (a select, never 0 * inf).
 *   sums[VOTE] = w_vote * sum vote_r / max(#vote+, 1); sums[CLS] = sum cls_r / max(#valid, 1);
 *   sums[BOX] = sum box_r / max(#pos, 1); sums[TOTAL] = their sum.
 * Reduction: 128 rows per workgroup, shuffles over the wave, LDS over the waves, one record per workgroup in `workspace`,
 * added in index order by a final launch: the same inputs give the same bits.  No floating-point atomics.
 * cfg: DET6D_HEAD_LOSS_NCFG floats in HOST memory, read during the call (no upload): the eight loss weights in the order
 * vote_reg, point_cls, point_offset_reg, point_angle_cls, point_angle_reg, point_pitch_cls, point_pitch_reg, point_corner,
 * then beta, centerness_min, centerness_max, and zeros.
 * loss_cls, loss_box (the per-point vectors cls_r and box_r) and centerness (cen_r), each (n), may be NULL.
 * Limits: 0 <= n <= 2^24, 1 <= num_class <= 16, 1 <= angle_bin_num <= 32, 7 <= ld_box_labels <= 1024, cfg finite, beta >= 0,
 * ws_bytes >= det6d_ext_head_loss_workspace_bytes(n).  n == 0: nothing is launched and nothing written. */
enum {
  DET6D_HEAD_LOSS_GROUND_AWARE = 1, DET6D_HEAD_LOSS_CENTERNESS = 2, DET6D_HEAD_LOSS_CORNER = 4      /* flags */
};
enum {
  DET6D_HEAD_LOSS_CFG_BETA = 8, DET6D_HEAD_LOSS_CFG_CMIN = 9, DET6D_HEAD_LOSS_CFG_CMAX = 10, DET6D_HEAD_LOSS_NCFG = 16
};
enum {                                                                                               /* sums[] */
  DET6D_HEAD_LOSS_TOTAL = 0, DET6D_HEAD_LOSS_VOTE = 1, DET6D_HEAD_LOSS_CLS = 2, DET6D_HEAD_LOSS_BOX = 3,
  DET6D_HEAD_LOSS_N_VOTE_POS = 4, DET6D_HEAD_LOSS_N_POS = 5, DET6D_HEAD_LOSS_N_PITCH_POS = 6, DET6D_HEAD_LOSS_N_VALID = 7,
  DET6D_HEAD_LOSS_INV_VOTE = 8, DET6D_HEAD_LOSS_INV_CLS = 9, DET6D_HEAD_LOSS_INV_BOX = 10, DET6D_HEAD_LOSS_PITCH_SCALE = 11,
  DET6D_HEAD_LOSS_NSUMS = 16
};
long long det6d_ext_head_loss_workspace_bytes(int n);
int det6d_ext_head_loss_forward(int n, int num_class, int angle_bin_num, int flags, const float *cfg, const float *vote_preds,
                                const float *vote_reg_labels, const long long *vote_cls_labels, const float *cls_preds,
                                const long long *cls_labels, const float *reg_preds, const float *reg_labels,
                                const float *box_labels, int ld_box_labels, void *workspace, long long ws_bytes, float *sums,
                                float *loss_cls, float *loss_box, float *centerness, det6d_stream_t stream);

/* upstream * d sums[TOTAL] / d (vote_preds, cls_preds, reg_preds), one launch.  `sums` is what the forward wrote for the same
 * inputs; grad_loss is ONE float in DEVICE memory (the upstream gradient autograd hands over).  Labels are constants.  The first
 * maximum (decoded bin) and the min (corner branch) pass the gradient through the branch taken; the counts are constants; the
 * corner term reaches the three centre offsets, the three log-sizes, the residual of the decoded bin, and vote_preds.
 * d_vote (n, 3), d_cls (n, num_class), d_reg (n, code_size): any may be NULL, not all three.  Every row is written. */
int det6d_ext_head_loss_backward(int n, int num_class, int angle_bin_num, int flags, const float *cfg, const float *vote_preds,
                                 const float *vote_reg_labels, const long long *vote_cls_labels, const float *cls_preds,
                                 const long long *cls_labels, const float *reg_preds, const float *reg_labels,
                                 const float *box_labels, int ld_box_labels, const float *sums, const float *grad_loss,
                                 float *d_vote, float *d_cls, float *d_reg, det6d_stream_t stream);

/* The two pieces of the loss the head also offers on caller-supplied rows, by the same arithmetic:
 * centerness[r] = pos_mask[r] ? cen_r : 0 for points (n, 3), box_labels (n, ld_box_labels) and a byte mask (generate_centerness_label);
 * loss[r] = corner_r for pred_boxes (n, ld_pred) and gt_boxes (n, ld_gt), columns 0 .. 6 = [x, y, z, dx, dy, dz, rz]
 * (get_corner_loss_lidar).  Limits: 0 <= n <= 2^24, 7 <= the row lengths <= 1024; n == 0 launches nothing. */
int det6d_ext_centerness_labels(int n, const float *points, const float *box_labels, int ld_box_labels,
                                const unsigned char *pos_mask, float *centerness, det6d_stream_t stream);
int det6d_ext_corner_loss(int n, const float *pred_boxes, int ld_pred, const float *gt_boxes, int ld_gt, float *loss,
                          det6d_stream_t stream);

/* ------------------------------------------------------------------ MLP backward ------- */

/* The backward pass of one pointwise layer z = x W + shift as det6d_linear computes it (BatchNorm folded: W (k, n) row-major,
 * the layer's input x (rows, k), its pre-activation output z (rows, n)), given dz = dL/dz:
 *   dx[r][c]  = sum_j dz[r][j] * w[wrow0 + c][j]          (rows, k)   the gradient of the layer's input
 *   dw[c][j]  = sum_r x[r][xcol0 + c] * dz[r][j]          (k, n)      the gradient of the folded weights
 *   dshift[j] = sum_r dz[r][j]                            (n)         the gradient of the folded shift
 * A tower is one call per layer, from the last layer to the first: the last layer has no activation, so its dz is the loss
 * gradient; with RELU_INPUT the dx of a call is already the dz of the layer before (x is that layer's ReLU output); the second
 * of two towers that read the same input adds its dx into the first one's with ACCUMULATE_DX.  No dz is materialised apart.
 * Executable model: tests/models/mlp_backward.py.
 * Arithmetic (a pure function of the inputs: no floating-point atomics, nothing depends on the grid, the number of CUs or the
 * order in which workgroups arrive):
 *   dx[r][c]: ONE fp32 accumulator from 0, the products in ascending j, each step an fma — the chain v_mfma_f32_32x32x2_f32
 *     gives (csrc/mfma_tile.h); then, with RELU_INPUT, dx = x[r][xcol0 + c] > 0 ? dx : 0 (a NaN in x compares false: 0); then,
 *     with ACCUMULATE_DX, dx = dx_before + dx, one add.
 *   dw[c][j]: the rows are cut into slabs of DET6D_EXT_LINEAR_BACKWARD_SLAB rows (the last one may be short); a slab's partial
 *     is the fma chain from 0 over its rows in ascending order; dw = (partial_0 + partial_1) + partial_2 ..., fp32 adds in
 *     ascending slab order.  dw is written, not accumulated.
 *   dshift[j]: the same slabs, a partial being the chain of fp32 adds from 0 over its rows; the same order over the slabs.
 * rows == 0: with neither dw nor dshift nothing is launched (dx has no rows; ACCUMULATE_DX leaves it alone); otherwise ONE fill
 * kernel (the slab-sum kernel over zero slabs, no memset: the padding of dw's rows is not touched) writes dw and dshift as zeros.
 * x and w follow the rules det6d_linear enforces for its a and w: ldx % 4 == 0, ldw % 4 == 0, both pointers 16-byte aligned,
 * xcol0 + k <= ldx, n <= ldw; dz, dx, dw, dshift take what det6d_linear's output takes: any 4-byte aligned pointer, n <= lddz,
 * dxcol0 + k <= lddx, n <= lddw.  x is read (and checked) only for dw and for RELU_INPUT, w only for dx.  Columns outside
 * [dxcol0, dxcol0 + k) of dx and [0, n) of dw are left alone.  dx must not overlap the inputs.
 * Limits: 0 <= rows <= 2^24, 1 <= k, n <= 4096, 0 <= xcol0, 0 <= dxcol0, 0 <= wrow0 <= 2^24, flags in [0, 3], at least one of
 * dx / dw / dshift, ACCUMULATE_DX only with dx, workspace_bytes >= det6d_ext_linear_backward_workspace_bytes(rows, k, n) when
 * dw or dshift is asked for (0 for a single slab: its partial is the result; else one (k, n) + (n) block per slab). */
enum { DET6D_EXT_LINEAR_BACKWARD_SLAB = 256 };
enum { DET6D_EXT_LINEAR_BACKWARD_RELU_INPUT = 1, DET6D_EXT_LINEAR_BACKWARD_ACCUMULATE_DX = 2 };      /* flags */
long long det6d_ext_linear_backward_workspace_bytes(int rows, int k, int n);
int det6d_ext_linear_backward(int rows, int k, int n,
        const float *x,  int ldx,  int xcol0,   /* the layer's input: columns [xcol0, xcol0 + k) of (rows, ldx)        */
        const float *w,  int ldw,  int wrow0,   /* folded weights as det6d_linear reads them: rows [wrow0, wrow0 + k),  */
                                                /* columns [0, n) of a row-major (.., ldw) matrix                       */
        const float *dz, int lddz,              /* (rows, n): gradient w.r.t. the layer's PRE-activation output         */
        int flags,                              /* 1 RELU_INPUT: dx[r][c] = x[r][c] > 0 ? dx[r][c] : 0  (x is itself a  */
                                                /*   ReLU output, so dx is the previous layer's dz)                      */
                                                /* 2 ACCUMULATE_DX: dx = dx_before + (masked) result, one add/element    */
        float *dx, int lddx, int dxcol0,        /* (rows, k) or NULL                                                    */
        float *dw, int lddw,                    /* (k, n), written not accumulated, or NULL                             */
        float *dshift,                          /* (n) column sums of dz, or NULL                                       */
        void *workspace, long long workspace_bytes, det6d_stream_t stream);

/* ------------------------------------------------------------------ grouped-MLP backward */

/* The parts of the backward pass of a grouped MLP (a radius group of a set-abstraction layer, pointnet2_modules.py:305-312 as the
 * vote head uses it, point_head_box6d_vote.py:815-821, :846) that are not a GEMM.  With idx (b, m, ns) and cnt (b, m) the ball
 * query's padded lists — constants: ball membership carries no gradient — the forward is
 *   X0[(c, s)] = [pts[idx[c][s]][0..3) - ctr[c] | pts[idx[c][s]][3..k)];  Y = the pointwise layers of X0 (det6d_linear);
 *   pooled[c][j] = (cnt[c] > 0) * max_s Y[(c, s)][j],
 * and its backward is det6d_ext_linear_backward per layer between the four entry points below (the points' own coordinates and
 * features are constants; the centres are not).  Executable model: tests/models/group_backward.py.
 * Each entry point is a pure function of its inputs: no floating-point atomics, no counters, nothing depends on the grid; all
 * stores are ordinary vector stores; asynchronous on `stream`; a bad argument returns DET6D_EINVAL with a message naming the
 * entry point before anything is launched; with zero rows nothing is launched.
 * Limits: groups * ns = b * m * ns <= 2^24, 1 <= ns <= 128, 1 <= c <= 4096, 3 <= k <= 4096.
 *
 * det6d_ext_group_gather: X0 as a matrix.  out[((bi * m + c) * ns + s)][a] = pts[bi][idx[bi][c][s]][a] - ctr[bi * m + c][a] for
 *   a < 3: ONE fp32 subtract, the one the forward's gather does; columns [3, k) are copied; columns [k, ldout) are zero-filled, so
 *   that `out` feeds det6d_linear and det6d_ext_linear_backward as it is.  pts (b, n, ldp), k <= ldp; ctr (b * m, ldctr),
 *   ldctr >= 3; out follows the rules of det6d_linear's a: ldout % 4 == 0, k <= ldout <= 8192, 16-byte aligned.  An idx outside
 *   [0, n) is the caller's error, as in det6d_linear mode 1.  16-byte accesses where ldp % 4 == 0 and pts is 16-byte aligned.
 *
 * det6d_ext_group_pool_backward: the mask, the max-pool and the last layer's ReLU.  For group r and channel j < c, with
 *   win = the LOWEST slot s whose y[r * ns + s][j] equals the maximum over all ns slots (the tie rule is part of the contract;
 *   the padding slots s >= cnt repeat earlier hits with identical bits, so a winner is always a real hit):
 *     dz[r * ns + s][j] = (s == win && cnt[r] > 0 && y[r * ns + win][j] > 0) ? g[r][gcol0 + j] : 0.
 *   Every element of dz[:, 0:c) is written, columns beyond c are left alone.  A channel whose maximum is 0 (or negative) passes
 *   nothing.  y is the last layer's ReLU output (groups * ns, ldy); a NaN in y is outside the contract.  16-byte accesses
 *   where c, ldy and lddz are multiples of 4 and y and dz are 16-byte aligned.
 *
 * det6d_ext_group_centre_grad: dctr[r][a] = -(((0 + dx[r * ns][a]) + dx[r * ns + 1][a]) + ...), a < 3, fp32 adds in ascending
 *   slot order; written, not accumulated.  dx (groups * ns, lddx) is the three-column dx of the first layer
 *   (det6d_ext_linear_backward with k = 3, wrow0 = 0); lddx >= 3, lddctr >= 3.
 *
 * det6d_ext_vote_backward: the clamp of vote = candidate + clamp(off, -R, R) (det6d_vote_points):
 *   doff[r][a] = (-R_a <= off[r][a] && off[r][a] <= R_a) ? dvote[r][a] : 0 for the UNCLAMPED off, a < 3, R = (rx, ry, rz) >= 0.
 *   A NaN in off gives 0.  At off == +-R exactly the whole gradient passes (torch's max / min backward passes half of it).
 *   0 <= rows <= 2^24; the three row lengths >= 3.
 * Every pointer is at least 4-byte aligned. */
int det6d_ext_group_gather(int b, int n, int m, int ns, const float *pts, int ldp, int k, const int *idx, const float *ctr,
                           int ldctr, float *out, int ldout, det6d_stream_t stream);
int det6d_ext_group_pool_backward(int groups, int ns, int c, const float *y, int ldy, const int *cnt, const float *g, int ldg,
                                  int gcol0, float *dz, int lddz, det6d_stream_t stream);
int det6d_ext_group_centre_grad(int groups, int ns, const float *dx, int lddx, float *dctr, int lddctr, det6d_stream_t stream);
int det6d_ext_vote_backward(int rows, const float *off, int ldoff, float rx, float ry, float rz, const float *dvote, int lddvote,
                            float *doff, int lddoff, det6d_stream_t stream);

/* ------------------------------------------------------------------ SASA loss ---------- */

/* The reference's yaw-only roiaware_pool3d_utils.points_in_boxes_gpu (roiaware_pool3d_kernel.cu:16-36, :313-336).
 * Point layouts are those of det6d_ext_points_in_boxes9.  boxes (b, m, ld_boxes >= 7): columns 0 .. 6 are
 * [x, y, z, dx, dy, dz, rz] and nothing else is read (the 9 + 1 column gt_boxes go in unsliced: ry and rx take no part);
 * extra_width (3 floats or NULL = zeros) is added to dx, dy, dz.
 * box_idx[r] = the LOWEST index of a box of the row's scene that contains the point, -1 if none — the reference's loop breaks at
 * its first hit.  det6d_ext_points_in_boxes9 takes the HIGHEST index.
 * Arithmetic, in fp32, every operation rounded once, nothing contracted:
 *   per box: (s, c) = d6_sincosf(-rz) (det6d_math.h); h_k = 0.5f * (d_k + extra_k); g_x = h_x + 1e-5f, g_y = h_y + 1e-5f;
 *   per pair: u = x - cx, v = y - cy; lx = u * c + v * (-s); ly = u * s + v * c;
 *   inside iff fabsf(z - cz) <= h_z and fabsf(lx) < g_x and fabsf(ly) < g_y.
 * A NaN coordinate, centre, angle or size is outside (every comparison is written so that a NaN fails it; the reference's
 * z test alone, `fabsf(z - cz) > dz / 2` means outside, would let a NaN z pass).  There is NO "degenerate boxes contain nothing"
 * rule: a zero-sized box still contains the points within the margin of its centre line, and an all-zero padding row enlarged
 * by extra_width is a small box at the origin, as in the reference.  (The reference forms h + margin in double; a point within
 * rounding distance of a face may fall on the other side.)
 * Limits: those of det6d_ext_points_in_boxes9 with 7 <= ld_boxes.  With n_points == 0, b == 0 or m == 0 nothing is launched and
 * nothing is written. */
int det6d_ext_points_in_boxes7(int n_points, const float *points, int ld_points, int xyz_col, int bs_col, int n_per_scene,
                               int b, int m, const float *boxes, int ld_boxes, const float *extra_width, int *box_idx,
                               det6d_stream_t stream);

/* PointSASALoss (loss_utils.py:418-547): the layer-wise foreground / background labels of the backbone's sampled points, the
 * loss of the confidence scores against them and its gradient, for all layers and scenes at once.
 * Executable model: tests/models/sasa.py.
 * A layer is a segment: coords (b, m, ld) dense, the coordinates in columns xyz_col .. xyz_col + 2 (the scene of row r is r / m);
 * scores (b * m) logits; weight = layer_weights[i].  A segment whose scores is NULL or whose weight is 0 is SKIPPED (the
 * reference's None entries): it has no rows, its labels are not computed, nothing of it is read or written, and its entries of
 * `sums` are zero.  `segments` is an array in HOST memory, read during the call.
 * boxes, extra_width: as det6d_ext_points_in_boxes7 reads them, shared by all segments; in(p, e) = p lies in some box of its
 * scene enlarged by e.
 *   label = in(p, extra) ? 1 : 0                                   without DET6D_EXT_SASA_IGNORE (extra_width NULL: zeros);
 *   label = in(p, 0) ? 1 : in(p, extra) ? -1 : 0                   with DET6D_EXT_SASA_IGNORE, the reference's set_ignore_flag
 *                                                                  (needs extra_width).
 * With z = [label > 0], bce = max(x, 0) - x z + log1p(exp(-|x|)), p = sigmoid(x):
 *   l = bce                                                                        func = DET6D_EXT_SASA_BCE
 *   l = (z alpha + (1 - z)(1 - alpha)) * pt^gamma * bce, pt = z (1 - p) + (1 - z) p          DET6D_EXT_SASA_FOCAL
 *   sums[4 i + 0] = weight_i * sum_{label >= 0} l / max(norm_i, 1), sums[4 i + 1] = norm_i = #(label >= 0),
 *   sums[4 i + 2] = #(label > 0), sums[4 i + 3] = #(label < 0); sums[4 n_segments] = the sum of the layers' losses (fp32 adds
 *   in layer order from 0).  sums holds 4 n_segments + 1 floats.
 * Reduction: slabs of DET6D_EXT_SASA_SLAB rows that never straddle a segment, shuffles over the wave, LDS over the waves, one
 * record per slab in `workspace`, added per segment in slab order (in double) by a final launch: the same inputs give the same
 * bits.  No floating-point atomics.  Two launches; with no rows (no segment, b == 0, every segment skipped or empty) nothing
 * is launched and nothing written.
 * forward: segment.labels (b * m) int64, or NULL, receives the labels; d_scores is not read.  With
 *   DET6D_EXT_SASA_LABELS_GIVEN segment.labels is READ instead (PointSASALoss.loss_forward on labels the caller holds): no
 *   coords, boxes or extra_width are read, and labels must not be NULL for a segment that is not skipped.
 * backward: one launch; d_scores[r] = grad_loss[i * grad_stride] * weight_i * (1.0f / max(norm_i, 1)) * dl/dx, exactly 0 where
 *   label < 0.  `sums` is what the forward wrote for the same inputs; grad_loss lives in DEVICE memory: ONE float, the upstream
 *   gradient of the total (grad_stride 0), or one per layer, grad_stride floats apart (4: the layout of `sums`; 0 .. 4).
 *   segment.labels, where not NULL, is READ instead of computing the labels again (coords and boxes are then not read for
 *   that segment), with or without DET6D_EXT_SASA_LABELS_GIVEN.
 * Limits: 0 <= n_segments <= 8, 0 <= b <= 4096, 0 <= m <= 1024 boxes, 7 <= ld_boxes <= 1024, per segment 0 <= m,
 * 3 <= ld <= 1024, 0 <= xyz_col <= ld - 3, a finite weight; at most 2^24 rows in all; alpha and gamma finite, gamma >= 0;
 * ws_bytes >= det6d_ext_sasa_workspace_bytes(n_segments, segments, b) (-1 for arguments out of range). */
enum { DET6D_EXT_SASA_SLAB = 256, DET6D_EXT_SASA_MAX_SEGMENTS = 8 };
enum { DET6D_EXT_SASA_BCE = 0, DET6D_EXT_SASA_FOCAL = 1 };                                           /* func */
enum { DET6D_EXT_SASA_IGNORE = 1, DET6D_EXT_SASA_LABELS_GIVEN = 2 };                                 /* flags */
typedef struct det6d_ext_sasa_segment {
  const float *coords;
  int m, ld, xyz_col;
  float weight;
  const float *scores;
  long long *labels;
  float *d_scores;
} det6d_ext_sasa_segment;
long long det6d_ext_sasa_workspace_bytes(int n_segments, const det6d_ext_sasa_segment *segments, int b);
int det6d_ext_sasa_forward(int n_segments, const det6d_ext_sasa_segment *segments, int b, int m, const float *boxes, int ld_boxes,
                           const float *extra_width, int flags, int func, float alpha, float gamma, void *workspace,
                           long long ws_bytes, float *sums, det6d_stream_t stream);
int det6d_ext_sasa_backward(int n_segments, const det6d_ext_sasa_segment *segments, int b, int m, const float *boxes, int ld_boxes,
                            const float *extra_width, int flags, int func, float alpha, float gamma, const float *sums,
                            const float *grad_loss, int grad_stride, det6d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DET6D_EXT_H */
