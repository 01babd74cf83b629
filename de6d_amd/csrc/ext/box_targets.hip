// box_targets.hip — point-in-box target assignment for full-pose (9-DoF) boxes on gfx950, in libdet6d_hip_ext.so
// (include/det6d_ext.h; the arithmetic is stated there and executed by tests/models/box_targets.py).
// The reference does this on the host (box_utils.py:336-350: corners, then a Delaunay hull test box by box); here
//  * one lane per point, 256 points per workgroup;
//  * the workgroup serves the scenes its points belong to one after another, lowest scene first (one scene when rows are
//    ordered by scene, the usual case; any mix of scenes is correct, only slower);
//  * per scene the boxes are taken in chunks of kChunk from the highest index down.  The workgroup computes the chunk's
//    records (centre, half extents, the nine entries of R = Rx Ry Rz and a bounding radius: 16 floats) into LDS once — the
//    only trigonometry — and every lane without a box yet scans the chunk and keeps its highest hit.  Per pair: one
//    wave-uniform 16-byte LDS load, 3 subtractions and the squared distance against the bounding radius; only when some lane
//    of the wave is that near, three more loads, 3 products, 6 FMAs and 3 compares.  The bounding test never decides
//    membership: it only skips pairs the exact test would refuse (radius^2 = 1.01 |half|^2 + 1e-30 against a rounding of
//    a few 1e-7 relative);
//  * the scan ends as soon as every point of the scene has its box.
// The label columns of the winners are written by the workgroup as one run of consecutive addresses (the winner of each row
// goes through LDS), gathered from `boxes`.  All stores are ordinary vector stores.
#include "../common.h"
#include "../../../include/det6d_ext.h"
#include "../../../include/det6d_math.h"
#include "ext_common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 128;              // boxes per LDS chunk: 128 records of 64 bytes
constexpr int kMaxBoxes = 1024;
constexpr int kMaxScenes = 4096;
constexpr int kMaxPoints = 1 << 24;

struct TargetArgs {
  int n_points;
  const float *points;
  int ld_points, xyz_col, bs_col, n_per_scene;
  int b, m;
  const float *boxes;
  int ld_boxes;
  const float *extra;                    // 3 floats or null
  int class_col, num_class;
  float radius;
  int *box_idx;
  long long *cls_labels;
  float *box_labels;
  int ld_box_labels, n_cols;
};

// record of one box: [cx cy cz rad2] [R00 R10 R20 hx] [R01 R11 R21 hy] [R02 R12 R22 hz].  rad2 bounds |p - c|^2 of every point
// the exact test can accept, with a margin far above its rounding; a box that takes no part has rad2 = hx = -1
__device__ __forceinline__ void box_record(const float *__restrict__ bx, float ex, float ey, float ez, float4 *__restrict__ rec) {
  float sz, cz, sy, cy, sx, cx;
  d6_sincosf(bx[6], &sz, &cz);
  d6_sincosf(bx[7], &sy, &cy);
  d6_sincosf(bx[8], &sx, &cx);
  const float wx = bx[3] + ex, wy = bx[4] + ey, wz = bx[5] + ez;
  const bool live = wx > 0.f && wy > 0.f && wz > 0.f;
  const float hx = 0.5f * wx, hy = 0.5f * wy, hz = 0.5f * wz;
  const float sxsy = sx * sy, cxsy = cx * sy;
  // -ffp-contract=off: every product and every sum below is rounded once, in the order written
  const float r00 = cy * cz, r01 = -(cy * sz), r02 = sy;
  const float r10 = cx * sz + sxsy * cz, r11 = cx * cz - sxsy * sz, r12 = -(sx * cy);
  const float r20 = sx * sz - cxsy * cz, r21 = sx * cz + cxsy * sz, r22 = cx * cy;
  rec[0] = make_float4(bx[0], bx[1], bx[2], live ? 1.01f * (hx * hx + hy * hy + hz * hz) + 1e-30f : -1.f);
  rec[1] = make_float4(r00, r10, r20, live ? hx : -1.f);
  rec[2] = make_float4(r01, r11, r21, hy);
  rec[3] = make_float4(r02, r12, r22, hz);
}

__global__ __launch_bounds__(kThreads) void box_targets9_kernel(const TargetArgs a) {
  __shared__ float4 rec[kChunk * 4];
  __shared__ int next_scene;
  const int tid = threadIdx.x;
  const long long r = (long long)blockIdx.x * kThreads + tid;
  const bool row = r < a.n_points;

  float px = 0.f, py = 0.f, pz = 0.f;
  int scene = INT_MAX;                                     // INT_MAX: background whatever the boxes are
  if (row) {
    const float *p = a.points + r * a.ld_points;
    px = p[a.xyz_col], py = p[a.xyz_col + 1], pz = p[a.xyz_col + 2];
    if (a.bs_col >= 0) {
      const float s = p[a.bs_col];
      if (s >= 0.f && s < (float)a.b) scene = (int)s;       // NaN and everything outside [0, b): background
    } else {
      const long long s = r / a.n_per_scene;
      if (s < a.b) scene = (int)s;
    }
  }
  float ex = 0.f, ey = 0.f, ez = 0.f;
  if (a.extra) ex = a.extra[0], ey = a.extra[1], ez = a.extra[2];

  bool pending = scene != INT_MAX;
  int hit = -1;
  for (;;) {
    if (tid == 0) next_scene = INT_MAX;
    __syncthreads();
    if (pending) atomicMin(&next_scene, scene);
    __syncthreads();
    const int s = next_scene;
    if (s == INT_MAX) break;                               // uniform: every lane is served
    const bool mine = pending && scene == s;
    const float *sb = a.boxes + (long long)s * a.m * a.ld_boxes;
    for (int hi = a.m; hi > 0; hi -= kChunk) {
      const int lo = hi > kChunk ? hi - kChunk : 0;
      __syncthreads();                                     // the previous chunk (and next_scene) has been read
      for (int j = tid; j < hi - lo; j += kThreads) box_record(sb + (long long)(lo + j) * a.ld_boxes, ex, ey, ez, rec + 4 * j);
      __syncthreads();
      if (mine && hit < 0) {
        // ascending and without a break, so that the loads of several records are in flight at once: the last hit of the
        // chunk is its highest, and no lower chunk is scanned for this lane once it has one
#pragma unroll 4
        for (int j = 0; j < hi - lo; ++j) {
          const float4 c = rec[4 * j];
          const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
          const float q = dx * dx + dy * dy + dz * dz;
          if (q > c.w && q <= 3.0e38f) continue;           // certainly outside (an infinite or NaN q goes to the exact test)
          const float4 r0 = rec[4 * j + 1], r1 = rec[4 * j + 2], r2 = rec[4 * j + 3];
          const float lx = D6_FMA(dz, r0.z, D6_FMA(dy, r0.y, dx * r0.x));
          const float ly = D6_FMA(dz, r1.z, D6_FMA(dy, r1.y, dx * r1.x));
          const float lz = D6_FMA(dz, r2.z, D6_FMA(dy, r2.y, dx * r2.x));
          if (fabsf(lx) <= r0.w && fabsf(ly) <= r1.w && fabsf(lz) <= r2.w) hit = lo + j;
        }
      }
      if (!__syncthreads_or(mine && hit < 0)) break;       // every point of the scene has its box
    }
    if (mine) pending = false;
  }
  // from here on `rec` is free: its first words take the winning box row of every point (-1: no label columns)
  int *win = reinterpret_cast<int *>(rec);
  bool fg = hit >= 0;
  if (row) {
    if (a.box_idx) a.box_idx[r] = hit;
    long long label = 0;
    const long long wrow = fg ? (long long)scene * a.m + hit : 0;
    if (fg && (a.cls_labels || a.box_labels)) {
      if (a.radius > 0.f) {                                // double, rounded once per operation: NumPy float64 gives the same bits
        const float *wc = a.boxes + wrow * a.ld_boxes;     // p - c again: the same fp32 differences the scan saw
        const float hdx = px - wc[0], hdy = py - wc[1], hdz = pz - wc[2];
        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn((double)hdx, (double)hdx), __dmul_rn((double)hdy, (double)hdy)),
                                    __dmul_rn((double)hdz, (double)hdz));
        fg = d2 < __dmul_rn((double)a.radius, (double)a.radius);
      }
      label = !fg ? -1 : (a.num_class == 1 || a.class_col < 0) ? 1 : (long long)a.boxes[wrow * a.ld_boxes + a.class_col];
    }
    if (a.cls_labels) a.cls_labels[r] = label;
    win[tid] = fg ? (int)wrow : -1;                        // b * m <= 2^22
  }
  if (!a.box_labels || a.n_cols == 0) return;              // uniform
  __syncthreads();
  // element e = tid + 256 i of the workgroup's rows x n_cols block: consecutive lanes write consecutive columns
  const long long row0 = (long long)blockIdx.x * kThreads;
  const int rows = a.n_points - row0 < kThreads ? (int)(a.n_points - row0) : kThreads;
  const int qstep = kThreads / a.n_cols, rstep = kThreads % a.n_cols;
  int lr = tid / a.n_cols, col = tid % a.n_cols;
  while (lr < rows) {
    const int w = win[lr];
    a.box_labels[(row0 + lr) * a.ld_box_labels + col] = w >= 0 ? a.boxes[(long long)w * a.ld_boxes + col] : 0.f;
    lr += qstep, col += rstep;
    if (col >= a.n_cols) col -= a.n_cols, ++lr;
  }
}

int launch_targets(const char *who, const TargetArgs &a, det6d_stream_t stream) {
  if (a.n_points < 0 || a.n_points > kMaxPoints) return det6d_ext_fail("%s: n_points = %d (0 .. %d)", who, a.n_points, kMaxPoints);
  if (a.b < 0 || a.b > kMaxScenes) return det6d_ext_fail("%s: b = %d (0 .. %d)", who, a.b, kMaxScenes);
  if (a.m < 0 || a.m > kMaxBoxes) return det6d_ext_fail("%s: m = %d boxes per scene (0 .. %d)", who, a.m, kMaxBoxes);
  if (a.xyz_col < 0 || a.ld_points < 3 || a.xyz_col > a.ld_points - 3 || a.ld_points > 1024)
    return det6d_ext_fail("%s: xyz columns %d .. %d do not fit a point row of %d (at most 1024)", who, a.xyz_col, a.xyz_col + 2,
                          a.ld_points);
  if (a.bs_col >= a.ld_points) return det6d_ext_fail("%s: bs_col = %d in a point row of %d", who, a.bs_col, a.ld_points);
  if (a.bs_col < 0 && a.n_per_scene < 1) return det6d_ext_fail("%s: n_per_scene = %d without a scene column", who, a.n_per_scene);
  if (a.ld_boxes < 9 || a.ld_boxes > 1024) return det6d_ext_fail("%s: ld_boxes = %d (9 .. 1024)", who, a.ld_boxes);
  if (a.class_col >= a.ld_boxes) return det6d_ext_fail("%s: class_col = %d in a box row of %d", who, a.class_col, a.ld_boxes);
  if (a.num_class < 1) return det6d_ext_fail("%s: num_class = %d < 1", who, a.num_class);
  if (a.radius != a.radius) return det6d_ext_fail("%s: central_radius is NaN", who);
  if (a.box_labels && (a.n_cols < 0 || a.n_cols > a.ld_boxes || a.ld_box_labels < a.n_cols || a.ld_box_labels > 1024))
    return det6d_ext_fail("%s: %d label columns of a box row of %d into a label row of %d (at most 1024)", who, a.n_cols, a.ld_boxes,
                          a.ld_box_labels);
  if (!a.box_idx && !a.cls_labels && !a.box_labels) return det6d_ext_fail("%s: no output buffer", who);
  if (a.n_points == 0 || a.b == 0 || a.m == 0) return DET6D_OK;          // no point or no box: nothing launched, nothing written
  if (!a.points || !a.boxes) return det6d_ext_fail("%s: null pointer", who);
  hipLaunchKernelGGL(box_targets9_kernel, dim3(det6d_divup(a.n_points, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a);
  return det6d_check_launch(who);
}

}  // namespace

DET6D_API int det6d_ext_points_in_boxes9(int n_points, const float *points, int ld_points, int xyz_col, int bs_col,
                                         int n_per_scene, int b, int m, const float *boxes, int ld_boxes,
                                         const float *extra_width, int *box_idx, det6d_stream_t stream) {
  TargetArgs a = {n_points, points, ld_points, xyz_col, bs_col, n_per_scene, b, m, boxes, ld_boxes, extra_width,
                  -1, 1, 0.f, box_idx, nullptr, nullptr, 0, 0};
  return launch_targets("det6d_ext_points_in_boxes9", a, stream);
}

DET6D_API int det6d_ext_assign_targets9(int n_points, const float *points, int ld_points, int xyz_col, int bs_col,
                                        int n_per_scene, int b, int m, const float *boxes, int ld_boxes,
                                        const float *extra_width, int class_col, int num_class, float central_radius,
                                        int *box_idx, long long *cls_labels, float *box_labels, int ld_box_labels, int n_cols,
                                        det6d_stream_t stream) {
  TargetArgs a = {n_points, points, ld_points, xyz_col, bs_col, n_per_scene, b, m, boxes, ld_boxes, extra_width,
                  class_col, num_class, central_radius, box_idx, cls_labels, box_labels, ld_box_labels, n_cols};
  return launch_targets("det6d_ext_assign_targets9", a, stream);
}
