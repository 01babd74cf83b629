// group_backward.hip — the parts of a grouped MLP's backward pass that are not a GEMM, in libdet6d_hip_ext.so
// (include/det6d_ext.h states the arithmetic; tests/models/group_backward.py executes it in float64).
// A grouped MLP (a radius group of a set-abstraction layer) is X0 = [xyz[idx] - centre | features[idx]] -> pointwise layers ->
// mask by cnt > 0 -> max over the ns slots of a centre.  Its GEMMs are det6d_linear forward and det6d_ext_linear_backward
// backward; what is left are four memory-bound passes:
//  * group_gather_kernel: X0 as a matrix (the dw of the first layer needs it as an operand).  One lane per 16 bytes of an output
//    row, consecutive lanes on consecutive addresses of the row; the three coordinates take the forward gather's one subtract.
//  * group_pool_backward_kernel: d(pooled) routed to the winning slot.  Lanes run along the channels (four per lane where the
//    strides allow), the ns slots of a group are walked twice: one pass over Y finds the lowest slot holding the maximum, one
//    pass over dz writes every element.  Nothing is kept between the passes but the winner: no LDS, no scratch.
//  * group_centre_grad_kernel: minus the sum over a centre's slots of the three coordinate columns of the first layer's dx, one
//    lane per (centre, axis), the slots added in ascending order.
//  * vote_backward_kernel: the mask of the vote offsets' clamp.
// Every launch is a pure function of its inputs: no atomics, no counters, nothing depends on the grid (the grid-stride loops
// only deal elements to lanes).  All stores are ordinary vector stores.
#include "../common.h"
#include "../../../include/det6d_ext.h"
#include "ext_common.h"

namespace {

constexpr int kMaxRows = 1 << 24;
constexpr int kMaxSlots = 128;
constexpr int kMaxWidth = 4096;
constexpr int kBlock = 256;
constexpr long long kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups: the rest is walked by the grid-stride loops

dim3 grid_for(long long total) {
  const long long blocks = (total + kBlock - 1) / kBlock;
  return dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks));
}

#define D6_GRID_STRIDE(i, total) \
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < (total); i += (long long)gridDim.x * kBlock)

// (i / d, i % d) with the 32-bit divider wherever the element count allows it (every shape of the head)
__device__ __forceinline__ void d6_divmod(long long i, int d, bool small, long long &q, int &r) {
  if (small) {
    const unsigned qq = (unsigned)i / (unsigned)d;
    q = qq;
    r = (int)((unsigned)i - qq * (unsigned)d);
  } else {
    q = i / d;
    r = (int)(i - q * d);
  }
}

// out[r][0..3) = pts[row][0..3) - ctr[centre][0..3), out[r][3..k) = pts[row][3..k), out[r][k..ldout) = 0
// VEC: one lane per float4 of an output row (ldp % 4 == 0, ldout % 4 == 0, both 16-byte aligned); else one lane per float.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void group_gather_kernel(long long total, int per_row, int n, int m, int ns, int k,
                                                              const float *__restrict__ pts, int ldp, const int *__restrict__ idx,
                                                              const float *__restrict__ ctr, int ldctr, float *__restrict__ out,
                                                              int ldout) {
  const bool small = total < (1ll << 32);
  D6_GRID_STRIDE(i, total) {
    long long r;
    int q;
    d6_divmod(i, per_row, small, r, q);
    const int centre = (int)(r / ns);              // rows <= 2^24
    const int bi = centre / m;
    if constexpr (VEC) {
      const int c0 = 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 < k) {
        const float *src = pts + ((size_t)bi * n + idx[r]) * ldp;
        v = *reinterpret_cast<const float4 *>(src + c0);
        if (c0 == 0) {
          const float *c = ctr + (size_t)centre * ldctr;
          v.x = v.x - c[0];
          v.y = v.y - c[1];
          v.z = v.z - c[2];
        }
        if (c0 + 1 >= k) v.y = 0.f;
        if (c0 + 2 >= k) v.z = 0.f;
        if (c0 + 3 >= k) v.w = 0.f;
      }
      *reinterpret_cast<float4 *>(out + (size_t)r * ldout + c0) = v;
    } else {
      float v = 0.f;
      if (q < k) {
        v = pts[((size_t)bi * n + idx[r]) * ldp + q];
        if (q < 3) v = v - ctr[(size_t)centre * ldctr + q];
      }
      out[(size_t)r * ldout + q] = v;
    }
  }
}

// For group gr and channel j: win = the LOWEST slot s with y[gr * ns + s][j] == max over the ns slots (a strict > from slot 0);
// dz[gr * ns + s][j] = (s == win && cnt[gr] > 0 && max > 0) ? g[gr][gcol0 + j] : 0.  A NaN in y is outside the contract
// (it never compares greater, so a NaN at slot 0 stays the "maximum" and passes nothing, a NaN elsewhere is ignored).
// V = channels per lane: 4 (16-byte accesses) or 1.
template <int V>
__global__ __launch_bounds__(kBlock) void group_pool_backward_kernel(long long total, int per_group, int ns,
                                                                     const float *__restrict__ y, int ldy,
                                                                     const int *__restrict__ cnt, const float *__restrict__ g,
                                                                     int ldg, int gcol0, float *__restrict__ dz, int lddz) {
  const bool small = total < (1ll << 32);
  D6_GRID_STRIDE(i, total) {
    long long gr;
    int q;
    d6_divmod(i, per_group, small, gr, q);
    const int j0 = V * q;
    const float *yp = y + (size_t)gr * ns * ldy + j0;
    float best[V], up[V];
    int win[V];
    if constexpr (V == 4) {
      const float4 v = *reinterpret_cast<const float4 *>(yp);
      best[0] = v.x, best[1] = v.y, best[2] = v.z, best[3] = v.w;
    } else {
      best[0] = yp[0];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) win[e] = 0;
    for (int s = 1; s < ns; ++s) {
      float cur[V];
      if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(yp + (size_t)s * ldy);
        cur[0] = v.x, cur[1] = v.y, cur[2] = v.z, cur[3] = v.w;
      } else {
        cur[0] = yp[(size_t)s * ldy];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const bool gt = cur[e] > best[e];
        best[e] = gt ? cur[e] : best[e];
        win[e] = gt ? s : win[e];
      }
    }
    const bool live = cnt[gr] > 0;
    const float *gp = g + (size_t)gr * ldg + gcol0 + j0;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      up[e] = gp[e];
      if (!(live && best[e] > 0.f)) win[e] = -1;    // an empty ball, or a channel whose maximum is not positive: no winner
    }
    float *zp = dz + (size_t)gr * ns * lddz + j0;
    for (int s = 0; s < ns; ++s) {
      if constexpr (V == 4) {
        float4 v;
        v.x = win[0] == s ? up[0] : 0.f;
        v.y = win[1] == s ? up[1] : 0.f;
        v.z = win[2] == s ? up[2] : 0.f;
        v.w = win[3] == s ? up[3] : 0.f;
        *reinterpret_cast<float4 *>(zp + (size_t)s * lddz) = v;
      } else {
        zp[(size_t)s * lddz] = win[0] == s ? up[0] : 0.f;
      }
    }
  }
}

// dctr[gr][a] = -(((0 + dx[gr * ns][a]) + dx[gr * ns + 1][a]) + ...), a < 3
__global__ __launch_bounds__(kBlock) void group_centre_grad_kernel(int total, int ns, const float *__restrict__ dx, int lddx,
                                                                   float *__restrict__ dctr, int lddctr) {
  D6_GRID_STRIDE(i, total) {
    const int gr = (int)i / 3, a = (int)i - 3 * gr;
    const float *p = dx + (size_t)gr * ns * lddx + a;
    float s = 0.f;
    for (int t = 0; t < ns; ++t) s += p[(size_t)t * lddx];
    dctr[(size_t)gr * lddctr + a] = -s;
  }
}

// doff[r][a] = (-R_a <= off[r][a] <= R_a) ? dvote[r][a] : 0 for the UNCLAMPED off (a NaN compares false: 0)
__global__ __launch_bounds__(kBlock) void vote_backward_kernel(int total, const float *__restrict__ off, int ldoff, float rx,
                                                               float ry, float rz, const float *__restrict__ dvote, int lddvote,
                                                               float *__restrict__ doff, int lddoff) {
  D6_GRID_STRIDE(i, total) {
    const int r = (int)i / 3, a = (int)i - 3 * r;
    const float R = a == 0 ? rx : (a == 1 ? ry : rz);
    const float o = off[(size_t)r * ldoff + a];
    doff[(size_t)r * lddoff + a] = (o >= -R && o <= R) ? dvote[(size_t)r * lddvote + a] : 0.f;
  }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

DET6D_API int det6d_ext_group_gather(int b, int n, int m, int ns, const float *pts, int ldp, int k, const int *idx,
                                     const float *ctr, int ldctr, float *out, int ldout, det6d_stream_t stream) {
  const char *who = "det6d_ext_group_gather";
  if (b < 0 || n < 1 || m < 0) return det6d_ext_fail("%s: b = %d, n = %d, m = %d", who, b, n, m);
  if (ns < 1 || ns > kMaxSlots) return det6d_ext_fail("%s: ns = %d (1 .. %d)", who, ns, kMaxSlots);
  const long long rows = (long long)b * m * ns;
  if (rows > kMaxRows) return det6d_ext_fail("%s: b * m * ns = %lld (0 .. %d)", who, rows, kMaxRows);
  if ((long long)b * n > (1ll << 31) - 1) return det6d_ext_fail("%s: b * n = %lld points", who, (long long)b * n);
  if (k < 3 || k > kMaxWidth) return det6d_ext_fail("%s: k = %d (3 .. %d)", who, k, kMaxWidth);
  if (k > ldp) return det6d_ext_fail("%s: ldp = %d < k = %d", who, ldp, k);
  if (ldctr < 3) return det6d_ext_fail("%s: ldctr = %d < 3", who, ldctr);
  // out feeds det6d_linear as its a: rows of a multiple of four floats, 16-byte aligned
  if (k > ldout || (ldout & 3) || ldout > 2 * kMaxWidth)
    return det6d_ext_fail("%s: ldout = %d (a multiple of 4, k = %d .. %d)", who, ldout, k, 2 * kMaxWidth);
  if (!aligned16(out)) return det6d_ext_fail("%s: out must be 16-byte aligned", who);
  if (!aligned4(pts) || !aligned4(idx) || !aligned4(ctr)) return det6d_ext_fail("%s: pts, idx and ctr must be 4-byte aligned", who);
  if (rows == 0) return DET6D_OK;
  if (!pts || !idx || !ctr || !out) return det6d_ext_fail("%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  if ((ldp & 3) == 0 && aligned16(pts)) {
    const int per_row = ldout / 4;
    const long long total = rows * per_row;
    hipLaunchKernelGGL(group_gather_kernel<true>, grid_for(total), dim3(kBlock), 0, s, total, per_row, n, m, ns, k, pts, ldp, idx,
                       ctr, ldctr, out, ldout);
  } else {
    const long long total = rows * ldout;
    hipLaunchKernelGGL(group_gather_kernel<false>, grid_for(total), dim3(kBlock), 0, s, total, ldout, n, m, ns, k, pts, ldp, idx,
                       ctr, ldctr, out, ldout);
  }
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_group_pool_backward(int groups, int ns, int c, const float *y, int ldy, const int *cnt, const float *g,
                                            int ldg, int gcol0, float *dz, int lddz, det6d_stream_t stream) {
  const char *who = "det6d_ext_group_pool_backward";
  if (groups < 0) return det6d_ext_fail("%s: groups = %d", who, groups);
  if (ns < 1 || ns > kMaxSlots) return det6d_ext_fail("%s: ns = %d (1 .. %d)", who, ns, kMaxSlots);
  if ((long long)groups * ns > kMaxRows) return det6d_ext_fail("%s: groups * ns = %lld (0 .. %d)", who, (long long)groups * ns, kMaxRows);
  if (c < 1 || c > kMaxWidth) return det6d_ext_fail("%s: c = %d (1 .. %d)", who, c, kMaxWidth);
  if (c > ldy) return det6d_ext_fail("%s: ldy = %d < c = %d", who, ldy, c);
  if (c > lddz) return det6d_ext_fail("%s: lddz = %d < c = %d", who, lddz, c);
  if (gcol0 < 0 || (long long)gcol0 + c > ldg) return det6d_ext_fail("%s: g columns [%d, %d + %d) of rows of %d floats", who, gcol0, gcol0, c, ldg);
  if (!aligned4(y) || !aligned4(cnt) || !aligned4(g) || !aligned4(dz))
    return det6d_ext_fail("%s: y, cnt, g and dz must be 4-byte aligned", who);
  if (groups == 0) return DET6D_OK;
  if (!y || !cnt || !g || !dz) return det6d_ext_fail("%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  if ((c & 3) == 0 && (ldy & 3) == 0 && (lddz & 3) == 0 && aligned16(y) && aligned16(dz)) {
    const int per_group = c / 4;
    const long long total = (long long)groups * per_group;
    hipLaunchKernelGGL(group_pool_backward_kernel<4>, grid_for(total), dim3(kBlock), 0, s, total, per_group, ns, y, ldy, cnt, g, ldg,
                       gcol0, dz, lddz);
  } else {
    const long long total = (long long)groups * c;
    hipLaunchKernelGGL(group_pool_backward_kernel<1>, grid_for(total), dim3(kBlock), 0, s, total, c, ns, y, ldy, cnt, g, ldg, gcol0, dz,
                       lddz);
  }
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_group_centre_grad(int groups, int ns, const float *dx, int lddx, float *dctr, int lddctr,
                                          det6d_stream_t stream) {
  const char *who = "det6d_ext_group_centre_grad";
  if (groups < 0) return det6d_ext_fail("%s: groups = %d", who, groups);
  if (ns < 1 || ns > kMaxSlots) return det6d_ext_fail("%s: ns = %d (1 .. %d)", who, ns, kMaxSlots);
  if ((long long)groups * ns > kMaxRows) return det6d_ext_fail("%s: groups * ns = %lld (0 .. %d)", who, (long long)groups * ns, kMaxRows);
  if (lddx < 3 || lddctr < 3) return det6d_ext_fail("%s: lddx = %d, lddctr = %d (3 at least)", who, lddx, lddctr);
  if (!aligned4(dx) || !aligned4(dctr)) return det6d_ext_fail("%s: dx and dctr must be 4-byte aligned", who);
  if (groups == 0) return DET6D_OK;
  if (!dx || !dctr) return det6d_ext_fail("%s: null pointer", who);
  const int total = groups * 3;
  hipLaunchKernelGGL(group_centre_grad_kernel, grid_for(total), dim3(kBlock), 0, (hipStream_t)stream, total, ns, dx, lddx, dctr, lddctr);
  return det6d_check_launch(who);
}

DET6D_API int det6d_ext_vote_backward(int rows, const float *off, int ldoff, float rx, float ry, float rz, const float *dvote,
                                      int lddvote, float *doff, int lddoff, det6d_stream_t stream) {
  const char *who = "det6d_ext_vote_backward";
  if (rows < 0 || rows > kMaxRows) return det6d_ext_fail("%s: rows = %d (0 .. %d)", who, rows, kMaxRows);
  if (!(rx >= 0.f) || !(ry >= 0.f) || !(rz >= 0.f)) return det6d_ext_fail("%s: the range (%g, %g, %g) must not be negative or NaN", who, rx, ry, rz);
  if (ldoff < 3 || lddvote < 3 || lddoff < 3) return det6d_ext_fail("%s: ldoff = %d, lddvote = %d, lddoff = %d (3 at least)", who, ldoff, lddvote, lddoff);
  if (!aligned4(off) || !aligned4(dvote) || !aligned4(doff)) return det6d_ext_fail("%s: off, dvote and doff must be 4-byte aligned", who);
  if (rows == 0) return DET6D_OK;
  if (!off || !dvote || !doff) return det6d_ext_fail("%s: null pointer", who);
  const int total = rows * 3;
  hipLaunchKernelGGL(vote_backward_kernel, grid_for(total), dim3(kBlock), 0, (hipStream_t)stream, total, off, ldoff, rx, ry, rz, dvote,
                     lddvote, doff, lddoff);
  return det6d_check_launch(who);
}
