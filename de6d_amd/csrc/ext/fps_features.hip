// fps_features.hip — F-FPS (feature-space farthest point sampling) for gfx950, in libdet6d_hip_ext.so (include/det6d_ext.h).
//
// The reference samples f-fps on a (B, n, n) matrix cdist(xyz) + cdist(features) * gamma (pointnet2_utils.py:37-44) with
// furthest_point_sampling_matrix_kernel (sampling_gpu.cu:268-373).  Only row `old` of that matrix is read per round, so
// this kernel computes that row on the fly and never materialises the matrix (64 MB per 4096-point scene):
//  * one workgroup per scene, hardware thread h = the reference's thread tid; every thread holds its points' x, y, z,
//    |xyz|^2 and min-distance in registers (k = h + j * S, S = opt_n_threads(n), j = 0 .. PPT-1); |f|^2 is computed once
//    into the workspace and read beside the feature row of a point that needs it (in registers it spills at PPT = 16);
//  * the per-thread arg-max is the reference's strict > scan; the cross-thread / cross-wave rule is its halving tree,
//    restated as the order key of fps_common.h (fps_tie_key): max value, then smallest (bitrev(k mod S), k);
//  * every wave loads its candidate's row into LDS before the one barrier of the round (xyz as is, features x -2), so
//    the round after the decision starts without a dependent global load;
//  * exact skip: both parts of d are >= 0 and fl(a + b) >= a for b >= 0, so d >= d_xyz in floating point.  A point whose
//    min-distance is <= d_xyz(old, k) keeps it whatever its features are: its feature row is not read (tests/models/ffps.py
//    checks the inequality; the picks are the same bits by construction).
// The matrix form (ffps_matrix_kernel) runs the same selection core on a caller-supplied matrix: it pins that core against
// the reference's own matrices (tests/golden/ffps_ref.npz).
#include "../common.h"
#include "../fps_common.h"
#include "../../../include/det6d_ext.h"
#include "ext_common.h"
#include <math.h>

namespace {

constexpr int kFfMaxC = 256;
constexpr int kFfMaxWaves = 16;
constexpr int kFfMaxN = 16384;        // 1024 threads x 16 points

// the candidate of one wave in one round
struct FfSlot {
  float val;
  unsigned key;
  int k;
  int pad;
};

// ... and, for the feature sampler, its row: [x, y, z, -2 f_0 .. -2 f_{c-1}] (float4-aligned) and its two norms
struct FfPayload {
  float row[4 + kFfMaxC];
  float nxyz, nf, pad[2];
};

// reference's clamp_min(0) of a Gram entry: NaN stays NaN (the fminf of the round then ignores the point's distance)
__device__ __forceinline__ float ff_clamp0(float g) { return g <= 0.f ? 0.f : g; }

// One decision of the halving tree.  best / bk: this thread's strict-> maximum and its point (0 when nothing beat -1, like
// the reference's besti).  The wave's winner goes to sl[wave]; `payload(k)` (wave-wide) stores whatever the next round needs
// about it; after the round's barrier every wave reduces the slots the same way.  Returns the winning wave.
template <typename Payload>
__device__ __forceinline__ int ff_decide(float best, int bk, bool live, int log2s, int nwaves, FfSlot *sl, Payload payload) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float v = live ? best : -__builtin_inff();
  const float wm = d6_wave_max(v);
  const u64 tie = __ballot(v == wm);
  int wl = __builtin_ctzll(tie);
  if (__popcll(tie) != 1) wl = fps_min_key_lane(tie, fps_tie_key(bk, log2s));
  const int wk = d6_readlane_i(bk, wl);
  if (lane == 0) {
    sl[wave].val = wm;
    sl[wave].key = fps_tie_key(wk, log2s);
    sl[wave].k = wk;
  }
  payload(wk);
  __syncthreads();
  const bool in = lane < nwaves;
  const float v2 = in ? sl[lane].val : -__builtin_inff();
  const float bm = d6_wave_max(v2);
  const u64 tie2 = __ballot(in && v2 == bm);
  int ww = __builtin_ctzll(tie2);
  if (__popcll(tie2) != 1) ww = fps_min_key_lane(tie2, in ? sl[lane].key : 0xFFFFFFFFu);
  return ww;
}

// |v|^2 of a point's coordinates: a sequential sum of rounded squares (-ffp-contract=off)
__device__ __forceinline__ float ff_norm3(float x, float y, float z) {
  float s = x * x;
  s = s + y * y;
  return s + z * z;
}

// sum over the 64 lanes (statistics only)
__device__ __forceinline__ unsigned ff_wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
  return v;
}

// G_feat(old, k) without its two norms: one ascending fmaf chain from 0 over the c channels of (-2 f_old) . f_k
__device__ __forceinline__ float ff_feature_dot(const float *__restrict__ r, const float *w, int c) {
  float acc = 0.f;
  if (c <= 0) return acc;
  acc = D6_FMA(w[3], r[3], acc);
  const int rest = c - 1, nq = rest >> 2;
  const float4 *r4 = reinterpret_cast<const float4 *>(r + 4);
  const float4 *w4 = reinterpret_cast<const float4 *>(w + 4);
#pragma unroll 2
  for (int q = 0; q < nq; ++q) {
    const float4 a = r4[q], b = w4[q];
    acc = D6_FMA(b.x, a.x, acc);
    acc = D6_FMA(b.y, a.y, acc);
    acc = D6_FMA(b.z, a.z, acc);
    acc = D6_FMA(b.w, a.w, acc);
  }
  for (int e = 4 + 4 * nq; e < 3 + c; ++e) acc = D6_FMA(w[e], r[e], acc);
  return acc;
}

template <int PPT>
__global__ __launch_bounds__(1024) void ffps_features_kernel(int n, int m, int log2s, int c, float gamma, int skip_ok,
                                                             const float *__restrict__ rows, long long ld, long long scene_stride,
                                                             float2 *__restrict__ norms, unsigned *__restrict__ stats,
                                                             int *__restrict__ idx, long long idx_stride, int idx_add) {
  __shared__ FfSlot slots[2][kFfMaxWaves];
  __shared__ __attribute__((aligned(16))) FfPayload pay[2][kFfMaxWaves];
  const int S = 1 << log2s;
  const int h = threadIdx.x, lane = h & 63, wave = h >> 6;
  const int nwaves = (blockDim.x + 63) >> 6;
  const bool live = h < S;
  d6_sampler_priority();

  rows += (size_t)blockIdx.x * scene_stride;
  norms += (size_t)blockIdx.x * n;
  idx += (size_t)blockIdx.x * idx_stride;

  // |xyz|^2 of the points: in registers up to PPT = 8, recomputed every round at PPT = 16 (the same three rounded
  // squares in the same order: the same bits)
  constexpr bool kKeepNx = PPT <= 8;
  float px[PPT], py[PPT], pz[PPT], pnx[kKeepNx ? PPT : 1], pt[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int k = h + (j << log2s);
    px[j] = py[j] = pz[j] = 0.f;
    if (kKeepNx) pnx[kKeepNx ? j : 0] = 0.f;
    pt[j] = 1e10f;
    if (live && k < n) {
      const float *r = rows + (size_t)k * ld;
      px[j] = r[0]; py[j] = r[1]; pz[j] = r[2];
      const float s = ff_norm3(px[j], py[j], pz[j]);
      if (kKeepNx) pnx[kKeepNx ? j : 0] = s;
      float f = 0.f;
      for (int cc = 0; cc < c; ++cc) {
        const float v = r[3 + cc];
        f = f + v * v;
      }
      norms[k] = make_float2(s, f);
    }
  }
  // the candidate's row and norms -> this wave's payload slot of buffer `p`
  auto load_payload = [&](int p, int k) {
    const float *r = rows + (size_t)k * ld;
    FfPayload &P = pay[p][wave];
    for (int col = lane; col < 3 + c; col += 64) {
      const float v = r[col];
      P.row[col] = col < 3 ? v : -2.f * v;
    }
    if (lane == 0) {
      const float2 nn = norms[k];
      P.nxyz = nn.x;
      P.nf = nn.y;
    }
  };
  __syncthreads();                                        // norms[] written
  if (wave == 0) load_payload(0, 0);                      // the first pick is point 0
  if (m > 0 && h == 0) idx[0] = idx_add;
  __syncthreads();

  unsigned ev = 0, wev = 0;
  int p = 0, ww = 0;
  for (int r = 1; r < m; ++r) {
    const FfPayload &P = pay[p][ww];
    const float mx = -2.f * P.row[0], my = -2.f * P.row[1], mz = -2.f * P.row[2];
    const float onx = P.nxyz, onf = P.nf;
    float best = -1.f;
    int bj = 0;
    // (opaque per round: left alone, the compiler hoists the PPT point indices and 64-bit row addresses out of the round
    // loop — 3 x PPT registers live across the whole kernel, which spills at PPT = 8 / 16)
    int hh = h;
    const float *rb = rows;
    const float2 *nb = norms;
    asm volatile("" : "+v"(hh), "+s"(rb), "+s"(nb));
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int k = hh + (j << log2s);
      const bool ok = live && k < n;
      float g = D6_FMA(mx, px[j], 0.f);
      g = D6_FMA(my, py[j], g);
      g = D6_FMA(mz, pz[j], g);
      g = g + onx;
      g = g + (kKeepNx ? pnx[kKeepNx ? j : 0] : ff_norm3(px[j], py[j], pz[j]));
      const float dx = sqrtf(ff_clamp0(g));
      float t = pt[j];
      const bool need = ok && !(skip_ok && t <= dx);
      wev += __ballot(need) != 0ull;
      if (need) {
        float gf = ff_feature_dot(rb + (size_t)k * ld, P.row, c);
        gf = gf + onf;
        gf = gf + nb[k].y;
        const float d = dx + sqrtf(ff_clamp0(gf)) * gamma;
        t = fminf(d, t);
        pt[j] = t;
        ++ev;
      }
      const bool up = ok && t > best;
      bj = up ? j : bj;
      best = up ? t : best;
    }
    const int bk = best > -1.f ? h + (bj << log2s) : 0;
    const int pn = p ^ 1;
    ww = ff_decide(best, bk, live, log2s, nwaves, slots[pn], [&](int k) { load_payload(pn, k); });
    p = pn;
    if (h == 0) idx[r] = slots[p][ww].k + idx_add;
  }

  ev = ff_wave_sum(ev);
  if (lane == 0) {
    unsigned *st = stats + (size_t)blockIdx.x * kFfMaxWaves * 2;
    st[wave * 2 + 0] = ev;
    st[wave * 2 + 1] = wev;
    if (wave == 0)
      for (int w = nwaves; w < kFfMaxWaves; ++w) st[w * 2 + 0] = st[w * 2 + 1] = 0u;
  }
}

template <int PPT>
__global__ __launch_bounds__(1024) void ffps_matrix_kernel(int n, int m, int log2s, const float *__restrict__ matrix,
                                                           float *__restrict__ temp, int *__restrict__ idx) {
  __shared__ FfSlot slots[2][kFfMaxWaves];
  const int S = 1 << log2s;
  const int h = threadIdx.x;
  const int nwaves = (blockDim.x + 63) >> 6;
  const bool live = h < S;

  matrix += (size_t)blockIdx.x * n * n;
  temp += (size_t)blockIdx.x * n;
  idx += (size_t)blockIdx.x * m;

  float pt[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int k = h + (j << log2s);
    pt[j] = live && k < n ? temp[k] : 0.f;
  }
  if (h == 0) idx[0] = 0;
  int old = 0, p = 0;
  for (int r = 1; r < m; ++r) {
    const float *row = matrix + (size_t)old * n;
    float best = -1.f;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int k = h + (j << log2s);
      const bool ok = live && k < n;
      const float t = ok ? fminf(row[k], pt[j]) : 0.f;
      pt[j] = t;
      const bool up = ok && t > best;
      bj = up ? j : bj;
      best = up ? t : best;
    }
    const int bk = best > -1.f ? h + (bj << log2s) : 0;
    p ^= 1;
    const int ww = ff_decide(best, bk, live, log2s, nwaves, slots[p], [](int) {});
    old = slots[p][ww].k;
    if (h == 0) idx[r] = old;
  }
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int k = h + (j << log2s);
    if (live && k < n) temp[k] = pt[j];
  }
}

long long ff_stats_offset(int b, int n) { return ((long long)b * n * 8 + 15) / 16 * 16; }

}  // namespace

DET6D_API long long det6d_ext_fps_features_workspace_bytes(int b, int n) {
  if (b <= 0 || n <= 0) return 0;
  return ff_stats_offset(b, n) + (long long)b * kFfMaxWaves * 2 * 4;
}

DET6D_API int det6d_ext_fps_features(int b, int n_total, int lo, int hi, int m, const float *rows, int ld, int c, float gamma,
                                     void *workspace, long long ws_bytes, int *idx, int idx_stride, int idx_offset, int idx_bias,
                                     det6d_stream_t stream) {
  if (b < 0) return det6d_ext_fail("det6d_ext_fps_features: b = %d < 0", b);
  if (n_total <= 0 || lo < 0 || hi > n_total || hi <= lo)
    return det6d_ext_fail("det6d_ext_fps_features: bad slice [%d, %d) of %d points", lo, hi, n_total);
  const int n = hi - lo;
  if (n > kFfMaxN) return det6d_ext_fail("det6d_ext_fps_features: %d points per scene (at most %d)", n, kFfMaxN);
  if (c < 0 || c > kFfMaxC) return det6d_ext_fail("det6d_ext_fps_features: %d feature channels (0 .. %d)", c, kFfMaxC);
  if (ld < c + 3 || ld % 4 != 0) return det6d_ext_fail("det6d_ext_fps_features: row stride %d (needs >= c + 3 = %d, multiple of 4)", ld, c + 3);
  if (m < 0 || idx_offset < 0 || idx_stride < idx_offset + m)
    return det6d_ext_fail("det6d_ext_fps_features: m = %d at offset %d does not fit an index row of %d", m, idx_offset, idx_stride);
  if (b == 0 || m == 0) return DET6D_OK;
  if (!rows || !idx || !workspace) return det6d_ext_fail("det6d_ext_fps_features: null pointer");
  if (((uintptr_t)rows & 15u) != 0) return det6d_ext_fail("det6d_ext_fps_features: rows must be 16-byte aligned");
  if (((uintptr_t)workspace & 15u) != 0) return det6d_ext_fail("det6d_ext_fps_features: workspace must be 16-byte aligned");
  if (ws_bytes < det6d_ext_fps_features_workspace_bytes(b, n))
    return det6d_ext_fail("det6d_ext_fps_features: workspace of %lld bytes (needs %lld)", ws_bytes,
                    det6d_ext_fps_features_workspace_bytes(b, n));
  const int log2s = fps_opt_n_threads_log2(n);
  const int S = 1 << log2s;
  const int ppt = (n + S - 1) / S;
  const dim3 grid(b), block(S < 64 ? 64 : S);
  const float *x = rows + (size_t)lo * ld;
  float2 *norms = reinterpret_cast<float2 *>(workspace);
  unsigned *stats = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(workspace) + ff_stats_offset(b, n));
  const int skip_ok = !(gamma < 0.f);     // d >= d_xyz needs a non-negative feature term
  const long long scene = (long long)n_total * ld;
#define FFPS_CASE(P)                                                                                                    \
  hipLaunchKernelGGL((ffps_features_kernel<P>), grid, block, 0, (hipStream_t)stream, n, m, log2s, c, gamma, skip_ok, x, \
                     (long long)ld, scene, norms, stats, idx + idx_offset, (long long)idx_stride, lo + idx_bias)
  if (ppt <= 1) FFPS_CASE(1);
  else if (ppt <= 2) FFPS_CASE(2);
  else if (ppt <= 4) FFPS_CASE(4);
  else if (ppt <= 8) FFPS_CASE(8);
  else FFPS_CASE(16);
#undef FFPS_CASE
  return det6d_check_launch("det6d_ext_fps_features");
}

DET6D_API int det6d_ext_fps_matrix(int b, int n, int m, const float *matrix, float *temp, int *idx, det6d_stream_t stream) {
  if (b < 0 || m < 0) return det6d_ext_fail("det6d_ext_fps_matrix: b = %d, m = %d", b, m);
  if (n <= 0 || n > kFfMaxN) return det6d_ext_fail("det6d_ext_fps_matrix: %d points per scene (1 .. %d)", n, kFfMaxN);
  if (b == 0 || m == 0) return DET6D_OK;
  if (!matrix || !temp || !idx) return det6d_ext_fail("det6d_ext_fps_matrix: null pointer");
  const int log2s = fps_opt_n_threads_log2(n);
  const int S = 1 << log2s;
  const int ppt = (n + S - 1) / S;
  const dim3 grid(b), block(S < 64 ? 64 : S);
#define FFPM_CASE(P) \
  hipLaunchKernelGGL((ffps_matrix_kernel<P>), grid, block, 0, (hipStream_t)stream, n, m, log2s, matrix, temp, idx)
  if (ppt <= 1) FFPM_CASE(1);
  else if (ppt <= 2) FFPM_CASE(2);
  else if (ppt <= 4) FFPM_CASE(4);
  else if (ppt <= 8) FFPM_CASE(8);
  else FFPM_CASE(16);
#undef FFPM_CASE
  return det6d_check_launch("det6d_ext_fps_matrix");
}
