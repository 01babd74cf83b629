// sasa_loss.hip — the SASA point-segmentation loss on gfx950, in libdet6d_hip_ext.so (include/det6d_ext.h states the
// arithmetic; tests/models/sasa.py executes it in float64): the yaw-only point-in-box test of the reference's roiaware_pool3d
// op, the layer-wise foreground / background labels PointSASALoss builds on it, its loss and the gradient of the loss.
// The reference labels one scene of one layer at a time (loss_utils.py:442-492: boolean indexing, a host read and two
// launches of points_in_boxes_kernel per scene), then spends about twenty elementwise launches per layer on the loss
// (:515-547).  Here:
//  * one lane per point, 256 points (a slab) per workgroup; a slab belongs to ONE layer segment, the segments' slabs are
//    numbered one after another and a workgroup finds its segment in the by-value argument block;
//  * the workgroup serves the scenes of its points one after another, lowest first, as box_targets.hip does; per scene the
//    boxes are staged in LDS in chunks of kChunk, from the LOWEST index up (the first box wins): centre, cos / sin of -rz
//    (the only trigonometry, once per box) and the half extents of the original and of the enlarged box with the margin
//    already added; the scan of a scene ends as soon as every one of its points is decided;
//  * forward: label and loss term per lane, four sums (loss, #valid, #foreground, #ignored) reduced over the wave with
//    shuffles, over the four waves through LDS, ONE record per slab; a final one-wave launch adds each segment's records in
//    slab order (in double) and writes `sums`.  No floating-point atomic anywhere: the same inputs give the same bits;
//  * backward: one launch over the same slabs; it reads the normalisers from `sums` and the upstream gradient from device
//    memory, and the labels from the caller or computes them again.
// All stores are ordinary vector stores.
#include "../common.h"
#include "../../../include/det6d_ext.h"
#include "../../../include/det6d_math.h"
#include "ext_common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;             // = DET6D_EXT_SASA_SLAB
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 128;               // boxes per LDS chunk: 128 records of 48 bytes
constexpr int kRec = 4;                   // floats of a slab's record: the sums of loss, label >= 0, label > 0, label < 0
constexpr int kMaxBoxes = 1024;
constexpr int kMaxScenes = 4096;
constexpr int kMaxPoints = 1 << 24;
constexpr int kMaxSegments = DET6D_EXT_SASA_MAX_SEGMENTS;
constexpr float kMargin = 1e-5f;
static_assert(kThreads == DET6D_EXT_SASA_SLAB, "the slab of the header is the workgroup");

struct BoxArgs {
  int b, m;
  const float *boxes;
  int ld_boxes;
  const float *extra;                     // 3 floats or null
};

// record of one box: [cx cy cz cos(-rz)] [sin(-rz) hx hy hz] [ex ey ez 0]: h = 0.5f * d of the first test, e of the second,
// the x and y entries with the margin added (hz, ez without: the z test has none)
__device__ __forceinline__ void box_record(const float *__restrict__ bx, float ax, float ay, float az, float ex, float ey, float ez,
                                           float4 *__restrict__ rec) {
  float sn, cs;
  d6_sincosf(-bx[6], &sn, &cs);
  rec[0] = make_float4(bx[0], bx[1], bx[2], cs);
  rec[1] = make_float4(sn, 0.5f * (bx[3] + ax) + kMargin, 0.5f * (bx[4] + ay) + kMargin, 0.5f * (bx[5] + az));
  rec[2] = make_float4(0.5f * (bx[3] + ex) + kMargin, 0.5f * (bx[4] + ey) + kMargin, 0.5f * (bx[5] + ez), 0.f);
}

// Every lane of the workgroup calls this with its point and scene (INT_MAX: no scene).  first = the lowest index of a box of
// the scene whose FIRST test (sizes + width_a) holds the point, -1 if none; with Two, second = some box's SECOND test (sizes +
// extra) holds it — looked for only while the lane has no `first` (the label is decided by then).
// The z test is written as !(|dz| <= hz) so that a NaN coordinate or size is outside, like a NaN in x or y.
template <bool Two>
__device__ __forceinline__ void scan_boxes(float4 *rec, int *next_scene, const BoxArgs &a, bool first_enlarged, int scene, float px,
                                           float py, float pz, int &first, bool &second) {
  const int tid = threadIdx.x;
  float ex = 0.f, ey = 0.f, ez = 0.f;
  if (a.extra) ex = a.extra[0], ey = a.extra[1], ez = a.extra[2];
  const float ax = first_enlarged ? ex : 0.f, ay = first_enlarged ? ey : 0.f, az = first_enlarged ? ez : 0.f;
  bool pending = scene != INT_MAX;
  first = -1, second = false;
  for (;;) {
    __syncthreads();                                         // the previous scene's last chunk (and next_scene) has been read
    if (tid == 0) *next_scene = INT_MAX;
    __syncthreads();
    if (pending) atomicMin(next_scene, scene);
    __syncthreads();
    const int s = *next_scene;
    if (s == INT_MAX) break;                                 // uniform: every lane is served
    const bool mine = pending && scene == s;
    const float *sb = a.boxes + (long long)s * a.m * a.ld_boxes;
    for (int lo = 0; lo < a.m; lo += kChunk) {
      const int cnt = a.m - lo < kChunk ? a.m - lo : kChunk;
      __syncthreads();                                       // the previous chunk has been read
      for (int j = tid; j < cnt; j += kThreads) box_record(sb + (long long)(lo + j) * a.ld_boxes, ax, ay, az, ex, ey, ez, rec + 3 * j);
      __syncthreads();
      if (mine && first < 0) {
        // without a break, so that the loads of several records are in flight at once; the guard keeps the lowest hit
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
          const float4 r0 = rec[3 * j], r1 = rec[3 * j + 1];
          const float sx = px - r0.x, sy = py - r0.y, dz = fabsf(pz - r0.z);
          // -ffp-contract=off: lidar_to_local_coords, every product and the sum rounded once
          const float lx = fabsf(sx * r0.w + sy * (-r1.x)), ly = fabsf(sx * r1.x + sy * r0.w);
          if (first < 0 && dz <= r1.w && lx < r1.y && ly < r1.z) first = lo + j;
          if (Two) {
            const float4 r2 = rec[3 * j + 2];
            if (dz <= r2.z && lx < r2.x && ly < r2.y) second = true;
          }
        }
      }
      if (!__syncthreads_or(mine && first < 0)) break;       // every point of the scene is decided
    }
    if (mine) pending = false;
  }
}

__global__ __launch_bounds__(kThreads) void points_in_boxes7_kernel(int n_points, const float *__restrict__ points, int ld_points,
                                                                    int xyz_col, int bs_col, int n_per_scene, const BoxArgs a,
                                                                    int *__restrict__ box_idx) {
  __shared__ float4 rec[kChunk * 3];
  __shared__ int next_scene;
  const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  int scene = INT_MAX;
  if (r < n_points) {
    const float *p = points + r * ld_points;
    px = p[xyz_col], py = p[xyz_col + 1], pz = p[xyz_col + 2];
    if (bs_col >= 0) {
      const float s = p[bs_col];
      if (s >= 0.f && s < (float)a.b) scene = (int)s;         // NaN and everything outside [0, b): no box
    } else {
      const long long s = r / n_per_scene;
      if (s < a.b) scene = (int)s;
    }
  }
  int first;
  bool second;
  scan_boxes<false>(rec, &next_scene, a, true, scene, px, py, pz, first, second);
  if (r < n_points) box_idx[r] = first;
}

struct Segment {
  const float *coords;                    // (b, m, ld), the coordinates in columns xyz_col ..
  const float *scores;                    // (b * m) logits; null: the segment has no slabs
  const long long *labels_in;             // labels to read instead of computing them
  long long *labels_out;                  // forward: labels to write
  float *d_scores;                        // backward
  float weight;
  int m, ld, xyz_col, rows, slab0, slabs;
};

struct SasaArgs {
  int n_segments, total_slabs, ignore, func;
  float alpha, gamma;
  BoxArgs box;
  Segment seg[kMaxSegments];
};

__device__ __forceinline__ float bce_logits(float x, float z) { return fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_stable(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// pt^(gamma - 1): pt itself for the gamma of PointSASALoss
__device__ __forceinline__ float focal_pow(float pt, float gamma) { return gamma == 2.f ? pt : powf(pt, gamma - 1.f); }

__device__ __forceinline__ float point_loss(const SasaArgs &a, float x, float z) {
  const float bce = bce_logits(x, z);
  if (a.func == DET6D_EXT_SASA_BCE) return bce;
  const float p = sigmoid_stable(x), pt = z * (1.f - p) + (1.f - z) * p;
  return (z * a.alpha + (1.f - z) * (1.f - a.alpha)) * (focal_pow(pt, a.gamma) * pt) * bce;
}

__device__ __forceinline__ float point_loss_grad(const SasaArgs &a, float x, float z) {
  const float p = sigmoid_stable(x);
  if (a.func == DET6D_EXT_SASA_BCE) return p - z;
  const float pt = z * (1.f - p) + (1.f - z) * p, pw = focal_pow(pt, a.gamma);
  return (z * a.alpha + (1.f - z) * (1.f - a.alpha))
         * (a.gamma * pw * (1.f - 2.f * z) * p * (1.f - p) * bce_logits(x, z) + pw * pt * (p - z));
}

// the segment of this workgroup's slab (uniform) and the label of this lane's row (0 for a lane past the segment's rows)
__device__ __forceinline__ int slab_labels(float4 *rec, int *next_scene, const SasaArgs &a, long long &row, bool &live,
                                           long long &label) {
  int si = 0;
  for (int i = 1; i < a.n_segments; ++i)                      // a skipped segment has no slabs and is never chosen
    if ((int)blockIdx.x >= a.seg[i].slab0 && (int)blockIdx.x < a.seg[i].slab0 + a.seg[i].slabs) si = i;
  const Segment &sg = a.seg[si];
  row = (long long)((int)blockIdx.x - sg.slab0) * kThreads + threadIdx.x;
  live = row < sg.rows;
  label = 0;
  if (sg.labels_in) {                                          // uniform
    if (live) label = sg.labels_in[row];
    return si;
  }
  float px = 0.f, py = 0.f, pz = 0.f;
  int scene = INT_MAX;
  if (live) {
    const float *p = sg.coords + row * sg.ld + sg.xyz_col;
    px = p[0], py = p[1], pz = p[2];
    scene = (int)(row / sg.m);
  }
  int first;
  bool second;
  if (a.ignore) {
    scan_boxes<true>(rec, next_scene, a.box, false, scene, px, py, pz, first, second);
    label = first >= 0 ? 1 : (second ? -1 : 0);
  } else {
    scan_boxes<false>(rec, next_scene, a.box, true, scene, px, py, pz, first, second);
    label = first >= 0 ? 1 : 0;
  }
  return si;
}

__global__ __launch_bounds__(kThreads) void sasa_forward_kernel(const SasaArgs a, float *__restrict__ partial) {
  __shared__ float4 rec[kChunk * 3];
  __shared__ int next_scene;
  __shared__ float wave_rec[kWaves][kRec];
  const int tid = threadIdx.x;
  long long row, label;
  bool live;
  const Segment &sg = a.seg[slab_labels(rec, &next_scene, a, row, live, label)];
  float sums[kRec] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    if (sg.labels_out) sg.labels_out[row] = label;
    if (label >= 0) sums[0] = point_loss(a, sg.scores[row], label > 0 ? 1.f : 0.f), sums[1] = 1.f;
    sums[2] = label > 0 ? 1.f : 0.f, sums[3] = label < 0 ? 1.f : 0.f;
  }
#pragma unroll
  for (int k = 0; k < kRec; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sums[k] += __shfl_down(sums[k], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kRec; ++k) wave_rec[tid >> 6][k] = sums[k];
  }
  __syncthreads();
  if (tid < kRec) {
    float t = wave_rec[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += wave_rec[w][tid];
    partial[(long long)blockIdx.x * kRec + tid] = t;
  }
}

// one wave: lane 4 i + c adds column c of the records of segment i in slab order, in double (as head_loss_final_kernel does);
// then sums[4 i ..] = [weight_i * sum_i / max(norm_i, 1), norm_i, n_pos_i, n_ignore_i] and sums[4 n_segments] = the total, the
// layers' fp32 losses added in layer order from 0
__global__ __launch_bounds__(64) void sasa_final_kernel(const SasaArgs a, const float *__restrict__ partial, float *__restrict__ sums) {
  const int lane = threadIdx.x, si = lane >> 2, col = lane & 3;
  double acc = 0.0;
  if (si < a.n_segments)
    for (int i = 0; i < a.seg[si].slabs; ++i) acc += (double)partial[(long long)(a.seg[si].slab0 + i) * kRec + col];
  const double s_loss = __shfl(acc, lane & ~3, 64);
  const float norm = (float)__shfl(acc, (lane & ~3) + 1, 64);
  const float weight = si < a.n_segments ? a.seg[si].weight : 0.f;
  const float layer = (float)((double)weight * s_loss * (double)(1.f / fmaxf(norm, 1.f)));
  float total = 0.f;
  for (int i = 0; i < a.n_segments; ++i) total += __shfl(layer, 4 * i, 64);
  if (si < a.n_segments) sums[lane] = col == 0 ? layer : (float)acc;
  if (lane == 0) sums[4 * a.n_segments] = total;
}

__global__ __launch_bounds__(kThreads) void sasa_backward_kernel(const SasaArgs a, const float *__restrict__ sums,
                                                                 const float *__restrict__ grad_loss, int grad_stride) {
  __shared__ float4 rec[kChunk * 3];
  __shared__ int next_scene;
  long long row, label;
  bool live;
  const int si = slab_labels(rec, &next_scene, a, row, live, label);
  const Segment &sg = a.seg[si];
  if (!live) return;
  // the forward divided the layer's sum by max(norm, 1): the same fp32 reciprocal
  const float scale = grad_loss[si * grad_stride] * sg.weight * (1.f / fmaxf(sums[4 * si + 1], 1.f));
  sg.d_scores[row] = label >= 0 ? scale * point_loss_grad(a, sg.scores[row], label > 0 ? 1.f : 0.f) : 0.f;
}

int check_boxes(const char *who, int b, int m, const float *boxes, int ld_boxes, BoxArgs &a) {
  if (b < 0 || b > kMaxScenes) return det6d_ext_fail("%s: b = %d (0 .. %d)", who, b, kMaxScenes);
  if (m < 0 || m > kMaxBoxes) return det6d_ext_fail("%s: m = %d boxes per scene (0 .. %d)", who, m, kMaxBoxes);
  if (ld_boxes < 7 || ld_boxes > 1024) return det6d_ext_fail("%s: ld_boxes = %d (7 .. 1024)", who, ld_boxes);
  a.b = b, a.m = m, a.boxes = boxes, a.ld_boxes = ld_boxes;
  return DET6D_OK;
}

// validates everything but the pointers a pass needs and numbers the slabs; total rows in `rows`
int check_sasa(const char *who, int n_segments, const det6d_ext_sasa_segment *segments, int b, int m, const float *boxes, int ld_boxes,
               const float *extra_width, int flags, int func, float alpha, float gamma, SasaArgs &a, long long &rows) {
  if (n_segments < 0 || n_segments > kMaxSegments) return det6d_ext_fail("%s: %d layer segments (0 .. %d)", who, n_segments, kMaxSegments);
  if (n_segments > 0 && !segments) return det6d_ext_fail("%s: segments is null", who);
  if (check_boxes(who, b, m, boxes, ld_boxes, a.box) != DET6D_OK) return DET6D_EINVAL;
  if (func != DET6D_EXT_SASA_BCE && func != DET6D_EXT_SASA_FOCAL) return det6d_ext_fail("%s: func = %d (0 BCE, 1 Focal)", who, func);
  if (flags < 0 || flags > (DET6D_EXT_SASA_IGNORE | DET6D_EXT_SASA_LABELS_GIVEN)) return det6d_ext_fail("%s: flags = %d holds unknown bits", who, flags);
  const bool given = flags & DET6D_EXT_SASA_LABELS_GIVEN;
  if ((flags & DET6D_EXT_SASA_IGNORE) && !extra_width && !given) return det6d_ext_fail("%s: the ignore flag needs extra_width", who);
  if (!(alpha - alpha == 0.f) || !(gamma - gamma == 0.f) || gamma < 0.f)
    return det6d_ext_fail("%s: alpha = %g, gamma = %g (finite, gamma >= 0)", who, (double)alpha, (double)gamma);
  a.n_segments = n_segments, a.ignore = flags & DET6D_EXT_SASA_IGNORE, a.func = func, a.alpha = alpha, a.gamma = gamma, a.box.extra = extra_width;
  rows = 0;
  int slab = 0;
  for (int i = 0; i < n_segments; ++i) {
    const det6d_ext_sasa_segment &s = segments[i];
    Segment &d = a.seg[i];
    if (s.m < 0 || s.m > kMaxPoints) return det6d_ext_fail("%s: segment %d: m = %d points per scene (0 .. %d)", who, i, s.m, kMaxPoints);
    if (s.xyz_col < 0 || s.ld < 3 || s.xyz_col > s.ld - 3 || s.ld > 1024)
      return det6d_ext_fail("%s: segment %d: xyz columns %d .. %d do not fit a row of %d (at most 1024)", who, i, s.xyz_col,
                            s.xyz_col + 2, s.ld);
    if (!(s.weight - s.weight == 0.f)) return det6d_ext_fail("%s: segment %d: the layer weight is not finite", who, i);
    const bool skipped = !s.scores || s.weight == 0.f;        // the reference's None entries
    const long long r = skipped ? 0 : (long long)b * s.m;
    rows += r;
    if (rows > kMaxPoints) return det6d_ext_fail("%s: more than %d points", who, kMaxPoints);
    d.coords = s.coords, d.scores = s.scores, d.weight = s.weight, d.m = s.m, d.ld = s.ld, d.xyz_col = s.xyz_col;
    if (given && !skipped && r > 0 && !s.labels) return det6d_ext_fail("%s: segment %d: labels is null", who, i);
    d.labels_in = given ? s.labels : nullptr, d.labels_out = given ? nullptr : s.labels, d.d_scores = nullptr;
    d.rows = (int)r, d.slab0 = slab, d.slabs = det6d_divup((int)r, kThreads);
    slab += d.slabs;
  }
  a.total_slabs = slab;
  return DET6D_OK;
}

long long partial_bytes(int slabs) { return ((long long)slabs * kRec * 4 + 15) / 16 * 16; }

}  // namespace

DET6D_API int det6d_ext_points_in_boxes7(int n_points, const float *points, int ld_points, int xyz_col, int bs_col,
                                         int n_per_scene, int b, int m, const float *boxes, int ld_boxes,
                                         const float *extra_width, int *box_idx, det6d_stream_t stream) {
  const char *who = "det6d_ext_points_in_boxes7";
  BoxArgs a = {};
  if (n_points < 0 || n_points > kMaxPoints) return det6d_ext_fail("%s: n_points = %d (0 .. %d)", who, n_points, kMaxPoints);
  if (check_boxes(who, b, m, boxes, ld_boxes, a) != DET6D_OK) return DET6D_EINVAL;
  if (xyz_col < 0 || ld_points < 3 || xyz_col > ld_points - 3 || ld_points > 1024)
    return det6d_ext_fail("%s: xyz columns %d .. %d do not fit a point row of %d (at most 1024)", who, xyz_col, xyz_col + 2, ld_points);
  if (bs_col >= ld_points) return det6d_ext_fail("%s: bs_col = %d in a point row of %d", who, bs_col, ld_points);
  if (bs_col < 0 && n_per_scene < 1) return det6d_ext_fail("%s: n_per_scene = %d without a scene column", who, n_per_scene);
  if (!box_idx) return det6d_ext_fail("%s: no output buffer", who);
  if (n_points == 0 || b == 0 || m == 0) return DET6D_OK;     // no point or no box: nothing launched, nothing written
  if (!points || !boxes) return det6d_ext_fail("%s: null pointer", who);
  a.extra = extra_width;
  hipLaunchKernelGGL(points_in_boxes7_kernel, dim3(det6d_divup(n_points, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, n_points,
                     points, ld_points, xyz_col, bs_col, n_per_scene, a, box_idx);
  return det6d_check_launch(who);
}

DET6D_API long long det6d_ext_sasa_workspace_bytes(int n_segments, const det6d_ext_sasa_segment *segments, int b) {
  if (n_segments < 0 || n_segments > kMaxSegments || (n_segments > 0 && !segments) || b < 0 || b > kMaxScenes) return -1;
  long long rows = 0, slabs = 0;
  for (int i = 0; i < n_segments; ++i) {
    if (segments[i].m < 0 || segments[i].m > kMaxPoints) return -1;
    const long long r = (!segments[i].scores || segments[i].weight == 0.f) ? 0 : (long long)b * segments[i].m;
    rows += r, slabs += (r + kThreads - 1) / kThreads;
    if (rows > kMaxPoints) return -1;
  }
  return partial_bytes((int)slabs);
}

DET6D_API int det6d_ext_sasa_forward(int n_segments, const det6d_ext_sasa_segment *segments, int b, int m, const float *boxes,
                                     int ld_boxes, const float *extra_width, int flags, int func, float alpha, float gamma,
                                     void *workspace, long long ws_bytes, float *sums, det6d_stream_t stream) {
  const char *who = "det6d_ext_sasa_forward";
  SasaArgs a = {};
  long long rows;
  if (check_sasa(who, n_segments, segments, b, m, boxes, ld_boxes, extra_width, flags, func, alpha, gamma, a, rows) != DET6D_OK)
    return DET6D_EINVAL;
  if (ws_bytes < partial_bytes(a.total_slabs))
    return det6d_ext_fail("%s: workspace of %lld bytes, %lld needed", who, ws_bytes, partial_bytes(a.total_slabs));
  if (rows == 0) return DET6D_OK;                             // nothing launched, nothing written: the caller's sums keep their zeros
  const bool given = flags & DET6D_EXT_SASA_LABELS_GIVEN;
  if (!workspace || !sums || (m > 0 && !boxes && !given)) return det6d_ext_fail("%s: null pointer", who);
  for (int i = 0; i < n_segments; ++i)
    if (a.seg[i].slabs > 0 && !a.seg[i].coords && !given) return det6d_ext_fail("%s: segment %d: coords is null", who, i);
  float *partial = static_cast<float *>(workspace);
  hipLaunchKernelGGL(sasa_forward_kernel, dim3(a.total_slabs), dim3(kThreads), 0, (hipStream_t)stream, a, partial);
  hipLaunchKernelGGL(sasa_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, partial, sums);
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_sasa_backward(int n_segments, const det6d_ext_sasa_segment *segments, int b, int m, const float *boxes,
                                      int ld_boxes, const float *extra_width, int flags, int func, float alpha, float gamma,
                                      const float *sums, const float *grad_loss, int grad_stride, det6d_stream_t stream) {
  const char *who = "det6d_ext_sasa_backward";
  SasaArgs a = {};
  long long rows;
  if (check_sasa(who, n_segments, segments, b, m, boxes, ld_boxes, extra_width, flags, func, alpha, gamma, a, rows) != DET6D_OK)
    return DET6D_EINVAL;
  if (rows == 0) return DET6D_OK;
  if (grad_stride < 0 || grad_stride > 4) return det6d_ext_fail("%s: grad_stride = %d (0 .. 4)", who, grad_stride);
  if (!sums || !grad_loss) return det6d_ext_fail("%s: null pointer", who);
  for (int i = 0; i < n_segments; ++i) {
    if (a.seg[i].slabs == 0) continue;
    if (!segments[i].d_scores) return det6d_ext_fail("%s: segment %d: d_scores is null", who, i);
    if (!segments[i].labels && (!a.seg[i].coords || (m > 0 && !boxes)))
      return det6d_ext_fail("%s: segment %d: neither labels nor coords and boxes", who, i);
    // labels the caller supplies are read, with or without DET6D_EXT_SASA_LABELS_GIVEN
    a.seg[i].labels_in = segments[i].labels, a.seg[i].labels_out = nullptr, a.seg[i].d_scores = segments[i].d_scores;
  }
  hipLaunchKernelGGL(sasa_backward_kernel, dim3(a.total_slabs), dim3(kThreads), 0, (hipStream_t)stream, a, sums, grad_loss, grad_stride);
  return det6d_check_launch(who);
}
