// mlp_backward.hip — the backward pass of one pointwise (folded Conv1d / BatchNorm) layer on fp32 MFMA, in libdet6d_hip_ext.so
// (include/det6d_ext.h states the arithmetic; tests/models/mlp_backward.py executes it in float64).
// The forward is det6d_linear (csrc/linear.hip): z = x W + shift.  Its backward is three reductions, none of which the forward
// family has:
//  * dx = dz W^T reduces over the layer's OUTPUT columns and walks W along its row-major rows.  linear_backward_dx_kernel: a
//    64 x 64 tile of dx per 256-thread workgroup (2 x 2 waves of one 32 x 32 accumulator tile each, mfma_tile.h), the reduction
//    in slabs of 32 columns.  Both operands are fetched with consecutive lanes on consecutive addresses (along the reduction:
//    rows of dz, rows of W) and written TRANSPOSED into LDS, reduction index major, with the odd row stride 65: the 32 lanes
//    of a store group then hit 32 different banks (bank = (j + row) mod 32), and the fragment reads (consecutive lanes,
//    consecutive words) are conflict-free whatever the stride — the rule d6_acc_to_lds is used by.  The W slab is staged once
//    per workgroup and read by both wave rows.  17 KB of LDS: several workgroups per CU cover each other's barriers.  The
//    epilogue applies the ReLU mask from x and the optional add in the accumulator registers and stores the tile.
//  * dw = x^T dz reduces over the ROWS.  linear_backward_dw_kernel: a 64 x 64 tile of dw per workgroup and per slab of
//    DET6D_EXT_LINEAR_BACKWARD_SLAB rows; the slab is walked in pieces of 32 rows, staged row-major (both fragments read along a row:
//    no transpose, no padding needed).  The slab is a compile-time constant of the arithmetic contract, not a tuning knob of
//    a launch: the slabs are what fills the chip for the narrow layers (512 x 128: 16 tiles, 128 x 32: 2), and their
//    partials are added in slab order by linear_backward_sum_kernel, so the bits do not depend on the grid.  A single slab
//    writes dw directly.
//  * dshift = the column sums of dz: linear_backward_dshift_kernel, one lane per column and slab, the same two steps.
// The fp32 MFMA shares its issue port with the vector ALU: the main loops hold only LDS reads and MFMAs, the
// predicates of the loaders are formed before the loop's MFMA block.
// n = 1 and n = 3 take the same kernels: the reduction is padded with zeros to the MFMA's k-step of two (fma(0, 0, c) = c) and
// the columns are predicated.  No floating-point atomics, no counters: every launch is a pure function of its inputs.
// All stores are ordinary vector stores.
#include "../common.h"
#include "../mfma_tile.h"
#include "../../../include/det6d_ext.h"
#include "ext_common.h"

namespace {

constexpr int kSlab = DET6D_EXT_LINEAR_BACKWARD_SLAB;
constexpr int kMaxRows = 1 << 24;
constexpr int kMaxWidth = 4096;
constexpr int kTile = 64;                 // output tile of a workgroup, both ways
constexpr int kBK = 32;                   // reduction depth of one LDS stage
constexpr int kLdT = kTile + 1;           // odd row stride of the transposed stages
static_assert(kSlab % kBK == 0, "a slab is a whole number of stages");

struct BackwardArgs {
  int rows, k, n, flags;
  const float *x;
  int ldx, xcol0;
  const float *w;
  int ldw, wrow0;
  const float *dz;
  int lddz;
  float *dx;
  int lddx, dxcol0;
};

// dx[r][c] = sum_j dz[r][j] * w[wrow0 + c][j], j ascending in one accumulator; then the mask, then the add
template <bool FAST_STORE>
__global__ __launch_bounds__(256) void linear_backward_dx_kernel(const BackwardArgs a) {
  __shared__ float Zs[kBK * kLdT];        // Zs[j][row]
  __shared__ float Ws[kBK * kLdT];        // Ws[j][c]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, kh = lane >> 5, l31 = lane & 31;
  const int gn = (a.k + kTile - 1) / kTile;
  const int row0 = (int)(blockIdx.x / gn) * kTile, col0 = (int)(blockIdx.x % gn) * kTile;

  // loader: lane j = tid & 31 of the reduction, rows / columns tid >> 5 + 8 i of the tile
  const int lj = tid & 31, lr = tid >> 5;
  const float *zp[8], *wp[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = row0 + lr + 8 * i, c = col0 + lr + 8 * i;
    zp[i] = r < a.rows ? a.dz + (size_t)r * a.lddz : nullptr;
    wp[i] = c < a.k ? a.w + (size_t)(a.wrow0 + c) * a.ldw : nullptr;
  }
  float rz[8], rw[8];
  auto load = [&](int j0) {
    const int j = j0 + lj;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      rz[i] = (zp[i] && j < a.n) ? zp[i][j] : 0.f;
      rw[i] = (wp[i] && j < a.n) ? wp[i][j] : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      Zs[lj * kLdT + lr + 8 * i] = rz[i];
      Ws[lj * kLdT + lr + 8 * i] = rw[i];
    }
  };

  f32x16 acc;
  d6_acc_zero(acc);
  const float *zf = Zs + kh * kLdT + wm * 32 + l31, *wf = Ws + kh * kLdT + wn * 32 + l31;
  load(0);
  for (int j0 = 0; j0 < a.n; j0 += kBK) {
    stage();
    __syncthreads();
    if (j0 + kBK < a.n) load(j0 + kBK);
    if (j0 + kBK <= a.n) {
#pragma unroll
      for (int ks = 0; ks < kBK / 2; ++ks) d6_mfma(zf[2 * ks * kLdT], wf[2 * ks * kLdT], acc);
    } else {                              // the short last slab issues only the k-steps that hold data
      const int nks = (a.n - j0 + 1) >> 1;
#pragma unroll 1
      for (int ks = 0; ks < nks; ++ks) d6_mfma(zf[2 * ks * kLdT], wf[2 * ks * kLdT], acc);
    }
    __syncthreads();
  }

  // epilogue: register e of the lane is row rbase + d6_acc_row(e) + 4 kh, column cc
  const int rbase = row0 + wm * 32, cc = col0 + wn * 32 + l31;
  const bool cok = cc < a.k;
  if (a.flags & DET6D_EXT_LINEAR_BACKWARD_RELU_INPUT) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = rbase + d6_acc_row(e) + 4 * kh;
      if (cok && r < a.rows) acc[e] = a.x[(size_t)r * a.ldx + a.xcol0 + cc] > 0.f ? acc[e] : 0.f;     // NaN compares false
    }
  }
  if (a.flags & DET6D_EXT_LINEAR_BACKWARD_ACCUMULATE_DX) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = rbase + d6_acc_row(e) + 4 * kh;
      if (cok && r < a.rows) acc[e] = a.dx[(size_t)r * a.lddx + a.dxcol0 + cc] + acc[e];
    }
  }
  if (FAST_STORE && rbase + 32 <= a.rows && col0 + wn * 32 + 32 <= a.k) {      // interior tile, 32-bit offsets (checked by the host)
    d6_acc_store_rows(acc, d6_buffer(a.dx), (uint32_t)((rbase + 4 * kh) * a.lddx + a.dxcol0 + cc) * 4u, a.lddx * 4);
    return;
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int r = rbase + d6_acc_row(e) + 4 * kh;
    if (cok && r < a.rows) a.dx[(size_t)r * a.lddx + a.dxcol0 + cc] = acc[e];
  }
}

// the partial of slab blockIdx.x: out[c][j] = sum_r x[r][xcol0 + c] * dz[r][j] over the slab's rows, ascending, from 0.
// out = dw itself (ld = lddw) for a single slab, else the slab's (k, n) block of the workspace (ld = n).
__global__ __launch_bounds__(256) void linear_backward_dw_kernel(const BackwardArgs a, float *__restrict__ out, int ld_out,
                                                                 long long slab_stride) {
  __shared__ float Xs[kBK * kTile];       // Xs[row][c]
  __shared__ float Zs[kBK * kTile];       // Zs[row][j]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, kh = lane >> 5, l31 = lane & 31;
  const int gn = (a.n + kTile - 1) / kTile;
  const int c0 = (int)(blockIdx.y / gn) * kTile, j0 = (int)(blockIdx.y % gn) * kTile;
  const int slab = blockIdx.x;
  const int r_begin = slab * kSlab, r_end = min(a.rows, r_begin + kSlab);

  // loader: column tid & 63 of the tile, rows tid >> 6 + 4 i of the stage
  const int lc = tid & 63, lr = tid >> 6;
  const bool xok = c0 + lc < a.k, zok = j0 + lc < a.n;
  const float *xp = a.x + a.xcol0 + c0 + lc, *zp = a.dz + j0 + lc;
  float rx[8], rz[8];
  auto load = [&](int r0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + lr + 4 * i;
      rx[i] = (xok && r < r_end) ? xp[(size_t)r * a.ldx] : 0.f;
      rz[i] = (zok && r < r_end) ? zp[(size_t)r * a.lddz] : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      Xs[(lr + 4 * i) * kTile + lc] = rx[i];
      Zs[(lr + 4 * i) * kTile + lc] = rz[i];
    }
  };

  f32x16 acc;
  d6_acc_zero(acc);
  const float *xf = Xs + kh * kTile + wm * 32 + l31, *zf = Zs + kh * kTile + wn * 32 + l31;
  load(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += kBK) {
    stage();
    __syncthreads();
    if (r0 + kBK < r_end) load(r0 + kBK);
    if (r0 + kBK <= r_end) {
#pragma unroll
      for (int ks = 0; ks < kBK / 2; ++ks) d6_mfma(xf[2 * ks * kTile], zf[2 * ks * kTile], acc);
    } else {
      const int nks = (r_end - r0 + 1) >> 1;
#pragma unroll 1
      for (int ks = 0; ks < nks; ++ks) d6_mfma(xf[2 * ks * kTile], zf[2 * ks * kTile], acc);
    }
    __syncthreads();
  }

  float *dst = out + (size_t)slab * slab_stride;
  const int cbase = c0 + wm * 32, jj = j0 + wn * 32 + l31;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int c = cbase + d6_acc_row(e) + 4 * kh;
    if (c < a.k && jj < a.n) dst[(size_t)c * ld_out + jj] = acc[e];
  }
}

// the partial of slab blockIdx.x of the column sums: out[j] = ((0 + dz[r0][j]) + dz[r0 + 1][j]) + ...
__global__ __launch_bounds__(64) void linear_backward_dshift_kernel(int rows, int n, const float *__restrict__ dz, int lddz,
                                                                    float *__restrict__ out, int slab_stride) {
  const int j = blockIdx.y * 64 + threadIdx.x, slab = blockIdx.x;
  if (j >= n) return;
  const int r_end = min(rows, (slab + 1) * kSlab);
  float s = 0.f;
  for (int r = slab * kSlab; r < r_end; ++r) s += dz[(size_t)r * lddz + j];
  out[(size_t)slab * slab_stride + j] = s;
}

// element e of the (k, n) partials [and of the (n) partials behind them]: added in ascending slab order; no slab at all
// (rows == 0) leaves the zero.  One lane per element, consecutive lanes on consecutive addresses.
__global__ __launch_bounds__(256) void linear_backward_sum_kernel(int nslabs, int k, int n, const float *__restrict__ part_w,
                                                                  const float *__restrict__ part_s, float *__restrict__ dw, int lddw,
                                                                  float *__restrict__ dshift) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x, kn = (long long)k * n;
  if (e < kn) {
    if (!dw) return;
    float s = 0.f;
    if (nslabs > 0) s = part_w[e];
    for (int i = 1; i < nslabs; ++i) s += part_w[(size_t)i * kn + e];
    dw[(e / n) * lddw + e % n] = s;
  } else if (e < kn + n && dshift) {
    const int j = (int)(e - kn);
    float s = 0.f;
    if (nslabs > 0) s = part_s[j];
    for (int i = 1; i < nslabs; ++i) s += part_s[(size_t)i * n + j];
    dshift[j] = s;
  }
}

int slabs_of(int rows) { return det6d_divup(rows, kSlab); }
bool shape_ok(int rows, int k, int n) { return rows >= 0 && rows <= kMaxRows && k >= 1 && k <= kMaxWidth && n >= 1 && n <= kMaxWidth; }

}  // namespace

DET6D_API long long det6d_ext_linear_backward_workspace_bytes(int rows, int k, int n) {
  if (!shape_ok(rows, k, n)) return -1;
  const int nslabs = slabs_of(rows);
  if (nslabs <= 1) return 0;                                 // a single slab's partial is the result
  return ((long long)nslabs * ((long long)k * n + n) * 4 + 15) / 16 * 16;
}

DET6D_API int det6d_ext_linear_backward(int rows, int k, int n, const float *x, int ldx, int xcol0, const float *w, int ldw,
                                        int wrow0, const float *dz, int lddz, int flags, float *dx, int lddx, int dxcol0,
                                        float *dw, int lddw, float *dshift, void *workspace, long long workspace_bytes,
                                        det6d_stream_t stream) {
  const char *who = "det6d_ext_linear_backward";
  if (rows < 0 || rows > kMaxRows) return det6d_ext_fail("%s: rows = %d (0 .. %d)", who, rows, kMaxRows);
  if (k < 1 || k > kMaxWidth || n < 1 || n > kMaxWidth) return det6d_ext_fail("%s: k = %d, n = %d (1 .. %d)", who, k, n, kMaxWidth);
  if (flags < 0 || flags > (DET6D_EXT_LINEAR_BACKWARD_RELU_INPUT | DET6D_EXT_LINEAR_BACKWARD_ACCUMULATE_DX))
    return det6d_ext_fail("%s: flags = %d holds unknown bits", who, flags);
  if (!dx && !dw && !dshift) return det6d_ext_fail("%s: no output buffer", who);
  if ((flags & DET6D_EXT_LINEAR_BACKWARD_ACCUMULATE_DX) && !dx) return det6d_ext_fail("%s: ACCUMULATE_DX without dx", who);
  const bool need_x = dw || (dx && (flags & DET6D_EXT_LINEAR_BACKWARD_RELU_INPUT));
  // x and w as det6d_linear takes a and w: rows of a multiple of four floats, 16-byte aligned, wide enough
  if (need_x && (xcol0 < 0 || (ldx & 3) || (long long)xcol0 + k > ldx))
    return det6d_ext_fail("%s: x columns [%d, %d + %d) of rows of %d floats (a multiple of 4)", who, xcol0, xcol0, k, ldx);
  if (dx && (wrow0 < 0 || wrow0 > (1 << 24) || (ldw & 3) || n > ldw))
    return det6d_ext_fail("%s: w rows from %d, %d columns of rows of %d floats (a multiple of 4)", who, wrow0, n, ldw);
  if (n > lddz) return det6d_ext_fail("%s: lddz = %d < n = %d", who, lddz, n);
  if (dx && (dxcol0 < 0 || (long long)dxcol0 + k > lddx))
    return det6d_ext_fail("%s: dx columns [%d, %d + %d) of rows of %d floats", who, dxcol0, dxcol0, k, lddx);
  if (dw && n > lddw) return det6d_ext_fail("%s: lddw = %d < n = %d", who, lddw, n);
  if ((need_x && ((uintptr_t)x & 15)) || (dx && ((uintptr_t)w & 15))) return det6d_ext_fail("%s: x and w must be 16-byte aligned", who);
  if (((uintptr_t)dz | (uintptr_t)dx | (uintptr_t)dw | (uintptr_t)dshift | (uintptr_t)workspace) & 3)
    return det6d_ext_fail("%s: dz, dx, dw, dshift and the workspace must be 4-byte aligned", who);
  const int nslabs = slabs_of(rows);
  const bool reduce = (dw || dshift) && nslabs != 1;
  const long long ws_need = det6d_ext_linear_backward_workspace_bytes(rows, k, n);
  if ((dw || dshift) && workspace_bytes < ws_need)
    return det6d_ext_fail("%s: workspace of %lld bytes, %lld needed", who, workspace_bytes, ws_need);
  if (rows > 0 && (!dz || (need_x && !x) || (dx && !w) || (reduce && !workspace))) return det6d_ext_fail("%s: null pointer", who);
  if (rows == 0 && !dw && !dshift) return DET6D_OK;          // nothing to compute, nothing launched

  hipStream_t s = (hipStream_t)stream;
  BackwardArgs a = {rows, k, n, flags, x, ldx, xcol0, w, ldw, wrow0, dz, lddz, dx, lddx, dxcol0};
  if (dx && rows > 0) {
    const unsigned grid = (unsigned)det6d_divup(rows, kTile) * (unsigned)det6d_divup(k, kTile);
    if ((size_t)rows * lddx * 4 < 0xfff00000ull)
      hipLaunchKernelGGL(linear_backward_dx_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(linear_backward_dx_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  }
  float *part_w = static_cast<float *>(workspace);
  float *part_s = part_w ? part_w + (size_t)nslabs * k * n : nullptr;
  if (dw && rows > 0) {
    const dim3 grid((unsigned)nslabs, (unsigned)(det6d_divup(k, kTile) * det6d_divup(n, kTile)));      // up to 65536 slabs: x
    if (reduce) hipLaunchKernelGGL(linear_backward_dw_kernel, grid, dim3(256), 0, s, a, part_w, n, (long long)k * n);
    else hipLaunchKernelGGL(linear_backward_dw_kernel, grid, dim3(256), 0, s, a, dw, lddw, 0ll);
  }
  if (dshift && rows > 0)
    hipLaunchKernelGGL(linear_backward_dshift_kernel, dim3((unsigned)nslabs, (unsigned)det6d_divup(n, 64)), dim3(64), 0, s, rows, n, dz,
                       lddz, reduce ? part_s : dshift, reduce ? n : 0);
  if (reduce)                                                // with rows == 0 this is the fill kernel: it writes the zeros
    hipLaunchKernelGGL(linear_backward_sum_kernel, dim3((unsigned)(((long long)k * n + n + 255) / 256)), dim3(256), 0, s, nslabs, k, n,
                       part_w, part_s, dw, lddw, dshift);
  return det6d_check_launch(who);
}
