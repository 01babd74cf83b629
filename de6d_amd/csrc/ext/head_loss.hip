// head_loss.hip — the training loss of PointHeadBox6DVote and its gradient on gfx950, in libdet6d_hip_ext.so
// (include/det6d_ext.h states the arithmetic; tests/models/head_loss.py executes it in float64).
// The reference builds get_loss (point_head_box6d_vote.py:426-776, loss_utils.py:10-235) from about 150 elementwise torch
// launches with boolean indexing, a branch on a device sum and six .item() calls.  Here:
//  * forward, per point: one lane per row, 128 rows per workgroup.  The workgroup copies its rows of reg_preds into LDS with
//    consecutive lanes on consecutive addresses (row stride code_size | 1 words, so that the lanes of a wave, each walking its
//    own row, hit different banks); the label rows, of which a lane needs 10 + angle_bin_num words, are read in place.  Each
//    lane forms the vote, classification (with its centerness label) and box terms of its row; eight running sums are
//    reduced over the wave with shuffles, over the two waves through LDS, and stored as ONE record per workgroup;
//  * forward, final: one wave adds the records in index order (in double), one lane per column, and writes the 16 floats of `sums`
//    (the losses, the counts and the normalisers the gradient needs).  No floating-point atomic anywhere: the same inputs
//    give the same bits;
//  * the pitch-residual term is rescaled by clamp(#foreground, 1) / clamp(#pitch-positive, 1), two sums over all rows: the
//    records carry its unscaled sum and the final step scales it.  Only a caller that wants the per-point box-loss vector
//    pays a third, elementwise launch that adds the scaled term to that vector;
//  * backward: one per-point kernel.  It reads the normalisers from `sums` and the upstream gradient from device memory, builds
//    the gradient row of reg_preds in the LDS copy of the row and writes it out as it was read in.
// All stores are ordinary vector stores.
#include "../common.h"
#include "../../../include/det6d_ext.h"
#include "../../../include/det6d_math.h"
#include "ext_common.h"

namespace {

constexpr int kThreads = 128;
constexpr int kWaves = kThreads / 64;
constexpr int kRec = 8;                   // floats of a workgroup's record: the sums of vote, cls, box (without the pitch
                                          // residual), pitch residual (unscaled), and the counts vote+, label > 0, pitch+, label >= 0
constexpr int kMaxRows = 1 << 24;
constexpr int kMaxClass = 16;
constexpr int kMaxBins = 32;
constexpr int kMaxStride = (6 + 2 * kMaxBins + 2) | 1;
constexpr float kTwoPi = 6.283185307179586f;

struct LossArgs {
  int n, num_class, nb, code, flags, ld_box;
  float w_vote, w_cls, w_off, w_acls, w_areg, w_pcls, w_preg, w_corner, beta, cmin, cmax;
  const float *vote_preds, *vote_reg_labels;
  const long long *vote_cls_labels;
  const float *cls_preds;
  const long long *cls_labels;
  const float *reg_preds, *reg_labels, *box_labels;
};

__device__ __forceinline__ float sl1(float d, float beta) {
  const float n = fabsf(d);
  return beta < 1e-5f ? n : (n < beta ? 0.5f * n * n / beta : n - 0.5f * beta);
}
__device__ __forceinline__ float sl1_grad(float d, float beta) {
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return (beta >= 1e-5f && fabsf(d) < beta) ? d / beta : sg;
}
__device__ __forceinline__ float bce_logits(float x, float t) { return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_stable(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// the workgroup's rows [row0, row0 + rows) of a dense (n, code) tensor <-> LDS rows of `stride` words
__device__ __forceinline__ void rows_to_lds(const float *__restrict__ src, float *lds, long long row0, int rows, int code, int stride) {
  const float *s = src + row0 * code;
  for (int e = threadIdx.x; e < rows * code; e += kThreads) lds[(e / code) * stride + e % code] = s[e];
}
__device__ __forceinline__ void lds_to_rows(float *__restrict__ dst, const float *lds, long long row0, int rows, int code, int stride) {
  float *d = dst + row0 * code;
  for (int e = threadIdx.x; e < rows * code; e += kThreads) d[e] = lds[(e / code) * stride + e % code];
}

// sin and cos of a label angle in double: the argument less the nearest multiple of pi/2 (a two-part constant, exact for the
// angles a box can have), then the Taylor polynomials on [-pi/4, pi/4], whose first neglected terms are below 1e-16
__device__ __forceinline__ void sincos_f64(double x, double &s, double &c) {
  const double k = rint(x * 0.6366197723675814);
  const double r = (x - k * 1.5707963267341256) - k * 6.077100506506192e-11;
  const double z = r * r;
  double ps = -1.0 / 1307674368000.0, pc = 1.0 / 20922789888000.0;
  ps = ps * z + 1.0 / 6227020800.0, pc = pc * z - 1.0 / 87178291200.0;
  ps = ps * z - 1.0 / 39916800.0, pc = pc * z + 1.0 / 479001600.0;
  ps = ps * z + 1.0 / 362880.0, pc = pc * z - 1.0 / 3628800.0;
  ps = ps * z - 1.0 / 5040.0, pc = pc * z + 1.0 / 40320.0;
  ps = ps * z + 1.0 / 120.0, pc = pc * z - 1.0 / 720.0;
  ps = ps * z - 1.0 / 6.0, pc = pc * z + 1.0 / 24.0;
  pc = pc * z - 0.5;
  const double sr = r + r * (z * ps), cr = 1.0 + z * pc;
  const int q = (int)(long long)k & 3;
  s = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
  c = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

// centerness label of a foreground row: the cube root of the product of the min / max face-distance ratios in the frame turned
// about z by the LAST label column (rx for nine-column labels: the reference's behaviour).  The face distances are formed in
// double: near a face the smaller distance is a difference of nearly equal numbers, and an fp32 rotation (1e-7 of the offset)
// would show in the label magnified by (distance / offset)^(-2/3) — measured at 1.2e-6 of the largest label, above the bound.
// Once per foreground row; the cube root is taken of the rounded product in fp32.
__device__ __forceinline__ float centerness_of(float px, float py, float pz, const float *__restrict__ bl, int ld_box) {
  const double dx = (double)px - (double)bl[0], dy = (double)py - (double)bl[1], dz = (double)pz - (double)bl[2];
  double s, c;
  sincos_f64((double)bl[ld_box - 1], s, c);
  const double lx = dx * c + dy * s, ly = dy * c - dx * s;
  const double hx = 0.5 * (double)bl[3], hy = 0.5 * (double)bl[4], hz = 0.5 * (double)bl[5];
  const double rl = fmin(hx - lx, hx + lx) / fmax(hx - lx, hx + lx);
  const double rw = fmin(hy - ly, hy + ly) / fmax(hy - ly, hy + ly);
  const double rh = fmin(hz - dz, hz + dz) / fmax(hz - dz, hz + dz);
  return cbrtf((float)fmax(rl * rw * rh, 1e-6));
}

// corner term of one row: the eight yaw-only corners of the decoded box against those of the label and of the label turned by
// pi; smooth-L1 (beta 1) summed over xyz, the smaller of the two per corner, the mean over corners.  With Grad the derivative
// with respect to the centre (gc*), the log-sizes (gs*) and the yaw (gyaw) through the branch each corner took.
// (cx, cy, cz) is the decoded centre MINUS the label's centre, formed by the caller from small differences: corners taken in
// absolute coordinates of tens of metres and then subtracted would lose about five bits more.
template <bool Grad>
__device__ __forceinline__ float corner_term(float cx, float cy, float cz, float sx, float sy, float sz, float yaw,
                                             const float *__restrict__ g, float &gcx, float &gcy, float &gcz, float &gsx,
                                             float &gsy, float &gsz, float &gyaw) {
  float sn, cs, gsn, gcs;
  d6_sincosf(yaw, &sn, &cs);
  d6_sincosf(g[6], &gsn, &gcs);
  const float gdx = g[3], gdy = g[4], gdz = g[5];
  float total = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float tx = (j & 2) ? -0.5f : 0.5f, ty = ((j + 1) & 2) ? -0.5f : 0.5f, tz = (j & 4) ? 0.5f : -0.5f;
    const float lx = sx * tx, ly = sy * ty, lz = sz * tz;
    const float px = lx * cs - ly * sn + cx, py = lx * sn + ly * cs + cy, pz = lz + cz;
    const float glx = gdx * tx, gly = gdy * ty;
    const float rx = glx * gcs - gly * gsn, ry = glx * gsn + gly * gcs;
    const float ez = pz - gdz * tz;
    const float ax = px - rx, ay = py - ry;                        // against the label
    const float bx = px + rx, by = py + ry;                        // against the label turned by pi
    const float lz1 = sl1(ez, 1.f);
    const float l0 = sl1(ax, 1.f) + sl1(ay, 1.f) + lz1, l1 = sl1(bx, 1.f) + sl1(by, 1.f) + lz1;
    const bool first = l0 <= l1;
    total += first ? l0 : l1;
    if (Grad) {
      const float qx = sl1_grad(first ? ax : bx, 1.f), qy = sl1_grad(first ? ay : by, 1.f), qz = sl1_grad(ez, 1.f);
      gcx += qx, gcy += qy, gcz += qz;
      gsx += (qx * cs + qy * sn) * lx;
      gsy += (qy * cs - qx * sn) * ly;
      gsz += qz * lz;
      gyaw += qx * (-lx * sn - ly * cs) + qy * (lx * cs - ly * sn);
    }
  }
  if (Grad) gcx *= 0.125f, gcy *= 0.125f, gcz *= 0.125f, gsx *= 0.125f, gsy *= 0.125f, gsz *= 0.125f, gyaw *= 0.125f;
  return total * 0.125f;
}

// what both passes need of the bin columns of a row: the label's bin, the decoded bin (first maximum of the logits) and the
// log-sum-exp of the logits
__device__ __forceinline__ void scan_bins(const float *P, const float *__restrict__ L, int nb, int &lab_bin, int &dec_bin, float &lse) {
  float lmax = L[6], pmax = P[6];
  lab_bin = 0, dec_bin = 0;
  for (int b = 1; b < nb; ++b) {
    const float l = L[6 + b], p = P[6 + b];
    if (l > lmax) lmax = l, lab_bin = b;
    if (p > pmax) pmax = p, dec_bin = b;
  }
  float sum = 0.f;
  for (int b = 0; b < nb; ++b) sum += expf(P[6 + b] - pmax);
  lse = pmax + logf(sum);
}

__global__ __launch_bounds__(kThreads) void head_loss_forward_kernel(const LossArgs a, float *__restrict__ partial,
                                                                     float *__restrict__ pitch_rows, float *__restrict__ loss_cls,
                                                                     float *__restrict__ loss_box, float *__restrict__ centerness) {
  extern __shared__ float lds[];
  __shared__ float wave_rec[kWaves][kRec];
  const int tid = threadIdx.x, stride = a.code | 1;
  const long long row0 = (long long)blockIdx.x * kThreads;
  const int rows = a.n - row0 < kThreads ? (int)(a.n - row0) : kThreads;
  rows_to_lds(a.reg_preds, lds, row0, rows, a.code, stride);
  __syncthreads();

  float v_vote = 0.f, v_cls = 0.f, v_box = 0.f, v_pitch = 0.f, c_vote = 0.f, c_pos = 0.f, c_pitch = 0.f, c_valid = 0.f;
  if (tid < rows) {
    const long long r = row0 + tid;
    const float px = a.vote_preds[r * 3], py = a.vote_preds[r * 3 + 1], pz = a.vote_preds[r * 3 + 2];
    if (a.vote_cls_labels[r] > 0) {
      const float *vl = a.vote_reg_labels + r * 3;
      v_vote = sl1(px - vl[0], a.beta) + sl1(py - vl[1], a.beta) + sl1(pz - vl[2], a.beta);
      c_vote = 1.f;
    }
    const long long lab = a.cls_labels[r];
    const bool pos = lab > 0, valid = lab >= 0;
    c_pos = pos ? 1.f : 0.f, c_valid = valid ? 1.f : 0.f;
    const float *bl = a.box_labels + r * a.ld_box;
    const float cen = pos ? centerness_of(px, py, pz, bl, a.ld_box) : 0.f;
    if (centerness) centerness[r] = cen;

    // classification: BCE with logits against the one-hot (scaled by the centerness label), the mean over the class columns
    const float t_fg = (a.flags & DET6D_HEAD_LOSS_CENTERNESS) ? a.cmin + (a.cmax - a.cmin) * cen : 1.f;
    float s = 0.f;
    for (int c = 0; c < a.num_class; ++c) s += bce_logits(a.cls_preds[r * a.num_class + c], (pos && lab - 1 == c) ? t_fg : 0.f);
    v_cls = valid ? s / (float)a.num_class * a.w_cls : 0.f;
    if (loss_cls) loss_cls[r] = v_cls;

    // box
    const float *P = lds + tid * stride, *L = a.reg_labels + r * a.code;
    const int pc = 6 + 2 * a.nb;
    bool pitch_pos = pos;
    float d_pitch = P[pc] - L[pc];
    if (a.flags & DET6D_HEAD_LOSS_GROUND_AWARE) pitch_pos = L[pc] > 0.f, d_pitch = P[pc + 1] - L[pc + 1];
    c_pitch = pitch_pos ? 1.f : 0.f;
    v_pitch = pitch_pos ? sl1(d_pitch, a.beta) * a.w_preg : 0.f;
    if (pos) {
      float off = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) off += sl1(P[k] - L[k], a.beta);
      int lab_bin, dec_bin;
      float lse;
      scan_bins(P, L, a.nb, lab_bin, dec_bin, lse);
      v_box = off * a.w_off + (lse - P[6 + lab_bin]) * a.w_acls
              + sl1(P[6 + a.nb + lab_bin] - L[6 + a.nb + lab_bin], a.beta) * a.w_areg;
      if (a.flags & DET6D_HEAD_LOSS_GROUND_AWARE) {          // sigmoid focal loss (alpha 0.25, gamma 2) on the pitch class
        const float x = P[pc], t = L[pc], p = sigmoid_stable(x);
        const float pt = t * (1.f - p) + (1.f - t) * p;
        v_box += (t * 0.25f + (1.f - t) * 0.75f) * pt * pt * bce_logits(x, t) * a.w_pcls;
      }
      if (a.flags & DET6D_HEAD_LOSS_CORNER) {
        float u0, u1, u2, u3, u4, u5, u6;
        const float yaw = ((float)dec_bin + P[6 + a.nb + dec_bin]) * (kTwoPi / (float)a.nb);
        v_box += corner_term<false>(P[0] + (px - bl[0]), P[1] + (py - bl[1]), P[2] + (pz - bl[2]), expf(P[3]), expf(P[4]),
                                    expf(P[5]), yaw, bl, u0, u1, u2, u3, u4, u5, u6) * a.w_corner;
      }
    }
    if (loss_box) loss_box[r] = v_box, pitch_rows[r] = v_pitch;
  }

  // eight sums: over the wave, then over the waves, then one record
  float rec[kRec] = {v_vote, v_cls, v_box, v_pitch, c_vote, c_pos, c_pitch, c_valid};
#pragma unroll
  for (int k = 0; k < kRec; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) rec[k] += __shfl_down(rec[k], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kRec; ++k) wave_rec[tid >> 6][k] = rec[k];
  }
  __syncthreads();
  if (tid < kRec) {
    float t = wave_rec[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += wave_rec[w][tid];
    partial[(long long)blockIdx.x * kRec + tid] = t;
  }
}

// one wave: lane c < 8 adds column c of the records in index order, in double (the records are fp32 tree sums of 128 rows; a
// sequential fp32 sum over hundreds of them would lose more than all the arithmetic before it)
__global__ __launch_bounds__(64) void head_loss_final_kernel(const float *__restrict__ partial, int nrec, float w_vote,
                                                             float *__restrict__ sums) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  if (lane < kRec)
    for (int i = 0; i < nrec; ++i) acc += (double)partial[(long long)i * kRec + lane];
  const double s_vote = __shfl(acc, 0, 64), s_cls = __shfl(acc, 1, 64), s_box = __shfl(acc, 2, 64), s_pitch = __shfl(acc, 3, 64);
  const float n_vote = (float)__shfl(acc, 4, 64), n_pos = (float)__shfl(acc, 5, 64), n_pitch = (float)__shfl(acc, 6, 64);
  const float n_valid = (float)__shfl(acc, 7, 64);
  // the normalisers are fp32 values: the backward multiplies by exactly what the forward divided by
  const float inv_vote = 1.f / fmaxf(n_vote, 1.f), inv_cls = 1.f / fmaxf(n_valid, 1.f), inv_box = 1.f / fmaxf(n_pos, 1.f);
  const float scale = fmaxf(n_pos, 1.f) / fmaxf(n_pitch, 1.f);
  const float vote = (float)((double)w_vote * s_vote * (double)inv_vote), cls = (float)(s_cls * (double)inv_cls);
  const float box = (float)((s_box + (double)scale * s_pitch) * (double)inv_box);
  float out = 0.f;
  switch (lane) {
    case DET6D_HEAD_LOSS_TOTAL: out = vote + cls + box; break;
    case DET6D_HEAD_LOSS_VOTE: out = vote; break;
    case DET6D_HEAD_LOSS_CLS: out = cls; break;
    case DET6D_HEAD_LOSS_BOX: out = box; break;
    case DET6D_HEAD_LOSS_N_VOTE_POS: out = n_vote; break;
    case DET6D_HEAD_LOSS_N_POS: out = n_pos; break;
    case DET6D_HEAD_LOSS_N_PITCH_POS: out = n_pitch; break;
    case DET6D_HEAD_LOSS_N_VALID: out = n_valid; break;
    case DET6D_HEAD_LOSS_INV_VOTE: out = inv_vote; break;
    case DET6D_HEAD_LOSS_INV_CLS: out = inv_cls; break;
    case DET6D_HEAD_LOSS_INV_BOX: out = inv_box; break;
    case DET6D_HEAD_LOSS_PITCH_SCALE: out = scale; break;
    default: break;
  }
  if (lane < DET6D_HEAD_LOSS_NSUMS) sums[lane] = out;
}

// the per-point box-loss vector gets its pitch-residual term, rescaled
__global__ __launch_bounds__(256) void head_loss_pitch_rows_kernel(int n, const float *__restrict__ sums,
                                                                   const float *__restrict__ pitch_rows, float *__restrict__ loss_box) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < n) loss_box[r] += sums[DET6D_HEAD_LOSS_PITCH_SCALE] * pitch_rows[r];
}

__global__ __launch_bounds__(kThreads) void head_loss_backward_kernel(const LossArgs a, const float *__restrict__ sums,
                                                                      const float *__restrict__ grad_loss, float *__restrict__ d_vote,
                                                                      float *__restrict__ d_cls, float *__restrict__ d_reg) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, stride = a.code | 1;
  const long long row0 = (long long)blockIdx.x * kThreads;
  const int rows = a.n - row0 < kThreads ? (int)(a.n - row0) : kThreads;
  rows_to_lds(a.reg_preds, lds, row0, rows, a.code, stride);
  __syncthreads();

  const float g = grad_loss[0];
  const float g_vote = g * a.w_vote * sums[DET6D_HEAD_LOSS_INV_VOTE], g_cls = g * a.w_cls * sums[DET6D_HEAD_LOSS_INV_CLS];
  const float g_box = g * sums[DET6D_HEAD_LOSS_INV_BOX], scale = sums[DET6D_HEAD_LOSS_PITCH_SCALE];
  if (tid < rows) {
    const long long r = row0 + tid;
    const float px = a.vote_preds[r * 3], py = a.vote_preds[r * 3 + 1], pz = a.vote_preds[r * 3 + 2];
    float dvx = 0.f, dvy = 0.f, dvz = 0.f;
    if (a.vote_cls_labels[r] > 0) {
      const float *vl = a.vote_reg_labels + r * 3;
      dvx = g_vote * sl1_grad(px - vl[0], a.beta), dvy = g_vote * sl1_grad(py - vl[1], a.beta), dvz = g_vote * sl1_grad(pz - vl[2], a.beta);
    }
    const long long lab = a.cls_labels[r];
    const bool pos = lab > 0, valid = lab >= 0;
    const float *bl = a.box_labels + r * a.ld_box;
    if (d_cls) {
      float t_fg = 1.f;
      if ((a.flags & DET6D_HEAD_LOSS_CENTERNESS) && pos) t_fg = a.cmin + (a.cmax - a.cmin) * centerness_of(px, py, pz, bl, a.ld_box);
      for (int c = 0; c < a.num_class; ++c) {
        const float x = a.cls_preds[r * a.num_class + c];
        d_cls[r * a.num_class + c] = valid ? g_cls * (sigmoid_stable(x) - ((pos && lab - 1 == c) ? t_fg : 0.f)) / (float)a.num_class : 0.f;
      }
    }

    // the gradient row of reg_preds replaces the row in LDS: everything it depends on is read first
    float *P = lds + tid * stride;
    const float *L = a.reg_labels + r * a.code;
    const int pc = 6 + 2 * a.nb;
    const bool ground = a.flags & DET6D_HEAD_LOSS_GROUND_AWARE;
    bool pitch_pos = pos;
    float d_pitch = P[pc] - L[pc];
    if (ground) pitch_pos = L[pc] > 0.f, d_pitch = P[pc + 1] - L[pc + 1];
    const float gp_res = pitch_pos ? g_box * a.w_preg * scale * sl1_grad(d_pitch, a.beta) : 0.f;
    float gp_cls = 0.f;
    if (pos) {
      int lab_bin, dec_bin;
      float lse;
      scan_bins(P, L, a.nb, lab_bin, dec_bin, lse);
      float g_lab_res = g_box * a.w_areg * sl1_grad(P[6 + a.nb + lab_bin] - L[6 + a.nb + lab_bin], a.beta), g_dec_res = 0.f;
      float go0 = g_box * a.w_off * sl1_grad(P[0] - L[0], a.beta), go1 = g_box * a.w_off * sl1_grad(P[1] - L[1], a.beta);
      float go2 = g_box * a.w_off * sl1_grad(P[2] - L[2], a.beta), go3 = g_box * a.w_off * sl1_grad(P[3] - L[3], a.beta);
      float go4 = g_box * a.w_off * sl1_grad(P[4] - L[4], a.beta), go5 = g_box * a.w_off * sl1_grad(P[5] - L[5], a.beta);
      if (ground) {                                          // the focal weight depends on the logit too
        const float x = P[pc], t = L[pc], p = sigmoid_stable(x);
        const float pt = t * (1.f - p) + (1.f - t) * p;
        const float dfocal = (t * 0.25f + (1.f - t) * 0.75f)
                             * (2.f * pt * (1.f - 2.f * t) * p * (1.f - p) * bce_logits(x, t) + pt * pt * (p - t));
        gp_cls = g_box * a.w_pcls * dfocal;
      }
      if (a.flags & DET6D_HEAD_LOSS_CORNER) {
        float gcx = 0.f, gcy = 0.f, gcz = 0.f, gsx = 0.f, gsy = 0.f, gsz = 0.f, gyaw = 0.f;
        const float yaw = ((float)dec_bin + P[6 + a.nb + dec_bin]) * (kTwoPi / (float)a.nb);
        corner_term<true>(P[0] + (px - bl[0]), P[1] + (py - bl[1]), P[2] + (pz - bl[2]), expf(P[3]), expf(P[4]), expf(P[5]), yaw,
                          bl, gcx, gcy, gcz, gsx, gsy, gsz, gyaw);
        const float gc = g_box * a.w_corner;
        go0 += gc * gcx, go1 += gc * gcy, go2 += gc * gcz, go3 += gc * gsx, go4 += gc * gsy, go5 += gc * gsz;
        dvx += gc * gcx, dvy += gc * gcy, dvz += gc * gcz;
        g_dec_res = gc * gyaw * (kTwoPi / (float)a.nb);
      }
      P[0] = go0, P[1] = go1, P[2] = go2, P[3] = go3, P[4] = go4, P[5] = go5;
      const float g_acls = g_box * a.w_acls;
      for (int b = 0; b < a.nb; ++b) {
        P[6 + b] = g_acls * (expf(P[6 + b] - lse) - (b == lab_bin ? 1.f : 0.f));
        P[6 + a.nb + b] = (b == lab_bin ? g_lab_res : 0.f) + (b == dec_bin ? g_dec_res : 0.f);
      }
    } else {
      for (int k = 0; k < pc; ++k) P[k] = 0.f;
    }
    if (ground) P[pc] = gp_cls, P[pc + 1] = gp_res;
    else P[pc] = gp_res;
    if (d_vote) d_vote[r * 3] = dvx, d_vote[r * 3 + 1] = dvy, d_vote[r * 3 + 2] = dvz;
  }
  if (!d_reg) return;                                        // uniform
  __syncthreads();
  lds_to_rows(d_reg, lds, row0, rows, a.code, stride);
}

// generate_centerness_label and get_corner_loss_lidar on caller-supplied rows: the same device functions, one lane per row
__global__ __launch_bounds__(256) void head_centerness_kernel(int n, const float *__restrict__ points, const float *__restrict__ box_labels,
                                                              int ld_box, const unsigned char *__restrict__ pos_mask,
                                                              float *__restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < n) out[r] = pos_mask[r] ? centerness_of(points[r * 3], points[r * 3 + 1], points[r * 3 + 2], box_labels + r * ld_box, ld_box) : 0.f;
}

__global__ __launch_bounds__(256) void head_corner_loss_kernel(int n, const float *__restrict__ pred, int ld_pred,
                                                               const float *__restrict__ gt, int ld_gt, float *__restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float *p = pred + r * ld_pred, *g = gt + r * ld_gt;
  float u0, u1, u2, u3, u4, u5, u6;
  out[r] = corner_term<false>(p[0] - g[0], p[1] - g[1], p[2] - g[2], p[3], p[4], p[5], p[6], g, u0, u1, u2, u3, u4, u5, u6);
}

long long partial_bytes(int n) { return ((long long)det6d_divup(n > 0 ? n : 1, kThreads) * kRec * 4 + 15) / 16 * 16; }

int check_args(const char *who, int n, int num_class, int nb, int flags, const float *cfg, int ld_box, LossArgs &a) {
  if (n < 0 || n > kMaxRows) return det6d_ext_fail("%s: n = %d (0 .. %d)", who, n, kMaxRows);
  if (num_class < 1 || num_class > kMaxClass) return det6d_ext_fail("%s: num_class = %d (1 .. %d)", who, num_class, kMaxClass);
  if (nb < 1 || nb > kMaxBins) return det6d_ext_fail("%s: angle_bin_num = %d (1 .. %d)", who, nb, kMaxBins);
  if (flags < 0 || flags > (DET6D_HEAD_LOSS_GROUND_AWARE | DET6D_HEAD_LOSS_CENTERNESS | DET6D_HEAD_LOSS_CORNER))
    return det6d_ext_fail("%s: flags = %d holds unknown bits", who, flags);
  if (ld_box < 7 || ld_box > 1024) return det6d_ext_fail("%s: ld_box_labels = %d (7 .. 1024)", who, ld_box);
  if (!cfg) return det6d_ext_fail("%s: cfg is null", who);
  for (int i = 0; i < DET6D_HEAD_LOSS_NCFG; ++i)
    if (!(cfg[i] - cfg[i] == 0.f)) return det6d_ext_fail("%s: cfg[%d] is not finite", who, i);
  if (cfg[DET6D_HEAD_LOSS_CFG_BETA] < 0.f) return det6d_ext_fail("%s: beta = %g < 0", who, (double)cfg[DET6D_HEAD_LOSS_CFG_BETA]);
  a.n = n, a.num_class = num_class, a.nb = nb, a.flags = flags, a.ld_box = ld_box;
  a.code = 6 + 2 * nb + ((flags & DET6D_HEAD_LOSS_GROUND_AWARE) ? 2 : 1);
  a.w_vote = cfg[0], a.w_cls = cfg[1], a.w_off = cfg[2], a.w_acls = cfg[3], a.w_areg = cfg[4], a.w_pcls = cfg[5], a.w_preg = cfg[6];
  a.w_corner = cfg[7], a.beta = cfg[DET6D_HEAD_LOSS_CFG_BETA], a.cmin = cfg[DET6D_HEAD_LOSS_CFG_CMIN], a.cmax = cfg[DET6D_HEAD_LOSS_CFG_CMAX];
  return DET6D_OK;
}

bool any_null(const LossArgs &a) {
  return !a.vote_preds || !a.vote_reg_labels || !a.vote_cls_labels || !a.cls_preds || !a.cls_labels || !a.reg_preds ||
         !a.reg_labels || !a.box_labels;
}

static_assert(kThreads * kMaxStride * 4 <= 48 * 1024, "the staged rows fit the default dynamic LDS limit");

}  // namespace

DET6D_API long long det6d_ext_head_loss_workspace_bytes(int n) {
  if (n < 0 || n > kMaxRows) return -1;
  return partial_bytes(n) + ((long long)n * 4 + 15) / 16 * 16;
}

DET6D_API int det6d_ext_head_loss_forward(int n, int num_class, int angle_bin_num, int flags, const float *cfg,
                                          const float *vote_preds, const float *vote_reg_labels, const long long *vote_cls_labels,
                                          const float *cls_preds, const long long *cls_labels, const float *reg_preds,
                                          const float *reg_labels, const float *box_labels, int ld_box_labels, void *workspace,
                                          long long ws_bytes, float *sums, float *loss_cls, float *loss_box, float *centerness,
                                          det6d_stream_t stream) {
  const char *who = "det6d_ext_head_loss_forward";
  LossArgs a = {};
  if (check_args(who, n, num_class, angle_bin_num, flags, cfg, ld_box_labels, a) != DET6D_OK) return DET6D_EINVAL;
  if (ws_bytes < det6d_ext_head_loss_workspace_bytes(n))
    return det6d_ext_fail("%s: workspace of %lld bytes, %lld needed", who, ws_bytes, det6d_ext_head_loss_workspace_bytes(n));
  if (n == 0) return DET6D_OK;                               // nothing launched, nothing written: the caller's sums keep their zeros
  a.vote_preds = vote_preds, a.vote_reg_labels = vote_reg_labels, a.vote_cls_labels = vote_cls_labels, a.cls_preds = cls_preds;
  a.cls_labels = cls_labels, a.reg_preds = reg_preds, a.reg_labels = reg_labels, a.box_labels = box_labels;
  if (any_null(a) || !workspace || !sums) return det6d_ext_fail("%s: null pointer", who);
  float *partial = static_cast<float *>(workspace);
  float *pitch_rows = reinterpret_cast<float *>(static_cast<char *>(workspace) + partial_bytes(n));
  const int blocks = det6d_divup(n, kThreads);
  const unsigned lds_bytes = kThreads * (a.code | 1) * 4;
  hipLaunchKernelGGL(head_loss_forward_kernel, dim3(blocks), dim3(kThreads), lds_bytes, (hipStream_t)stream, a, partial, pitch_rows,
                     loss_cls, loss_box, centerness);
  hipLaunchKernelGGL(head_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, blocks, a.w_vote, sums);
  if (loss_box)
    hipLaunchKernelGGL(head_loss_pitch_rows_kernel, dim3(det6d_divup(n, 256)), dim3(256), 0, (hipStream_t)stream, n, sums, pitch_rows,
                       loss_box);
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_head_loss_backward(int n, int num_class, int angle_bin_num, int flags, const float *cfg,
                                           const float *vote_preds, const float *vote_reg_labels, const long long *vote_cls_labels,
                                           const float *cls_preds, const long long *cls_labels, const float *reg_preds,
                                           const float *reg_labels, const float *box_labels, int ld_box_labels, const float *sums,
                                           const float *grad_loss, float *d_vote, float *d_cls, float *d_reg,
                                           det6d_stream_t stream) {
  const char *who = "det6d_ext_head_loss_backward";
  LossArgs a = {};
  if (check_args(who, n, num_class, angle_bin_num, flags, cfg, ld_box_labels, a) != DET6D_OK) return DET6D_EINVAL;
  if (!d_vote && !d_cls && !d_reg) return det6d_ext_fail("%s: no output buffer", who);
  if (n == 0) return DET6D_OK;
  a.vote_preds = vote_preds, a.vote_reg_labels = vote_reg_labels, a.vote_cls_labels = vote_cls_labels, a.cls_preds = cls_preds;
  a.cls_labels = cls_labels, a.reg_preds = reg_preds, a.reg_labels = reg_labels, a.box_labels = box_labels;
  if (any_null(a) || !sums || !grad_loss) return det6d_ext_fail("%s: null pointer", who);
  const unsigned lds_bytes = kThreads * (a.code | 1) * 4;
  hipLaunchKernelGGL(head_loss_backward_kernel, dim3(det6d_divup(n, kThreads)), dim3(kThreads), lds_bytes, (hipStream_t)stream, a, sums,
                     grad_loss, d_vote, d_cls, d_reg);
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_centerness_labels(int n, const float *points, const float *box_labels, int ld_box_labels,
                                          const unsigned char *pos_mask, float *centerness, det6d_stream_t stream) {
  const char *who = "det6d_ext_centerness_labels";
  if (n < 0 || n > kMaxRows) return det6d_ext_fail("%s: n = %d (0 .. %d)", who, n, kMaxRows);
  if (ld_box_labels < 7 || ld_box_labels > 1024) return det6d_ext_fail("%s: ld_box_labels = %d (7 .. 1024)", who, ld_box_labels);
  if (n == 0) return DET6D_OK;
  if (!points || !box_labels || !pos_mask || !centerness) return det6d_ext_fail("%s: null pointer", who);
  hipLaunchKernelGGL(head_centerness_kernel, dim3(det6d_divup(n, 256)), dim3(256), 0, (hipStream_t)stream, n, points, box_labels,
                     ld_box_labels, pos_mask, centerness);
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_corner_loss(int n, const float *pred_boxes, int ld_pred, const float *gt_boxes, int ld_gt, float *loss,
                                    det6d_stream_t stream) {
  const char *who = "det6d_ext_corner_loss";
  if (n < 0 || n > kMaxRows) return det6d_ext_fail("%s: n = %d (0 .. %d)", who, n, kMaxRows);
  if (ld_pred < 7 || ld_pred > 1024 || ld_gt < 7 || ld_gt > 1024)
    return det6d_ext_fail("%s: box rows of %d and %d columns (7 .. 1024)", who, ld_pred, ld_gt);
  if (n == 0) return DET6D_OK;
  if (!pred_boxes || !gt_boxes || !loss) return det6d_ext_fail("%s: null pointer", who);
  hipLaunchKernelGGL(head_corner_loss_kernel, dim3(det6d_divup(n, 256)), dim3(256), 0, (hipStream_t)stream, n, pred_boxes, ld_pred,
                     gt_boxes, ld_gt, loss);
  return det6d_check_launch(who);
}
