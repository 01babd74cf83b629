// sort_samplers.hip — the two sort-based samplers of the SA layer for gfx950, in libdet6d_hip_ext.so (include/det6d_ext.h):
//  * c-fps  (pointnet2_modules.py:425-430): the m highest sigmoid(score) ** gamma of a slice, in descending order;
//  * df-fps (pointnet2_modules.py:389-414): the weights 1 / (points in the same 2 m x 2 m pillar); the weighted FPS that
//    consumes them is det6d_fps_weights of the core library.
// Neither has a dependent chain of rounds.  One workgroup per scene holds the slice in LDS as 64-bit entries
// (order word << 32 | index word) and sorts them, descending, with a bitonic network (at most 16384 entries = 128 KiB of the
// CU's 160 KiB).  The entries of a scene are pairwise different, so the sorted order is unique and the result does not
// depend on the network: it is the order tests/models/score_topk.py and pillar_density.py state.
//  * top-k: order word = the weight's bits made monotone (NaN above +inf, -0 as +0), index word = ~k: equal weights come out
//    in ascending index.  The first m entries are the picks.
//  * pillars: order word = the pillar key (biased to unsigned), index word = k.  Equal keys are adjacent after the sort; each
//    entry finds both ends of its run by binary search (two times log2(N) LDS reads, no walk along a long run) and writes
//    1 / length to its point.  Counts are integers: the result does not depend on any order of arrival.
// Slots past n hold 0, which is below every live entry of either kind.
#include "../common.h"
#include "../../../include/det6d_ext.h"
#include "../../../include/det6d_math.h"
#include "ext_common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;

constexpr int kSortMaxLog = 14;
constexpr int kSortMinLog = 8;
constexpr int kSortMaxN = 1 << kSortMaxLog;        // 16384 entries of 8 bytes

// threads of the workgroup that sorts 1 << LOGN entries: one per compare-exchange pair, at most 1024
template <int LOGN>
struct SortShape {
  static constexpr int N = 1 << LOGN;
  static constexpr int T = N / 2 < 1024 ? N / 2 : 1024;
};

// descending bitonic sort of e[0 .. N) by the whole workgroup; ends with a barrier
template <int LOGN>
__device__ __forceinline__ void sort_desc(u64 *e) {
  constexpr int N = SortShape<LOGN>::N, T = SortShape<LOGN>::T;
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < N / 2 / T; ++q) {
        const int t = threadIdx.x + q * T;
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // bit j clear
        const int p = i | j;
        const u64 a = e[i], b = e[p];
        const bool desc = (i & k) == 0;
        if ((a < b) == desc) {
          e[i] = b;
          e[p] = a;
        }
      }
    }
  }
  __syncthreads();
}

// how many entries of the descending e[0 .. N) are >= bound
template <int LOGN>
__device__ __forceinline__ int count_ge(const u64 *e, u64 bound) {
  int pos = 0;
#pragma unroll
  for (int step = SortShape<LOGN>::N >> 1; step > 0; step >>= 1) pos += e[pos + step - 1] >= bound ? step : 0;
  return pos + (e[pos] >= bound ? 1 : 0);
}

// weight -> 32 bits whose unsigned order is: larger weight first, every NaN above +inf, -0 equal to +0
__device__ __forceinline__ unsigned order_word(float w) {
  if (w != w) return 0xffffffffu;
  if (w == 0.f) w = 0.f;
  const unsigned u = d6_f2bits(w);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

template <int LOGN>
__global__ __launch_bounds__(SortShape<LOGN>::T) void topk_scores_kernel(int n, int m, const float *__restrict__ scores,
                                                                        long long scene, float gamma, int *__restrict__ idx,
                                                                        long long idx_stride, int bias) {
  constexpr int N = SortShape<LOGN>::N, T = SortShape<LOGN>::T;
  __shared__ u64 e[N];
  scores += (long long)blockIdx.x * scene;
  idx += (long long)blockIdx.x * idx_stride;
#pragma unroll
  for (int q = 0; q < N / T; ++q) {
    const int k = threadIdx.x + q * T;
    u64 v = 0;
    if (k < n) v = ((u64)order_word(d6_sigmoid_powf(scores[k], gamma)) << 32) | (0xffffffffu - (unsigned)k);
    e[k] = v;
  }
  sort_desc<LOGN>(e);
  for (int r = threadIdx.x; r < m; r += T) idx[r] = (int)(0xffffffffu - (unsigned)e[r]) + bias;
}

// the constants of the reference's df-fps branch (pointnet2_modules.py:391-399): range [0, -39.68, ...], 2 m x 2 m pillars,
// scale_y = round((39.68 + 39.68) / 2) = 40
__device__ __forceinline__ int pillar_key(float x, float y) {
  const int cx = (int)floorf((x - 0.0f) / 2.0f);
  const int cy = (int)floorf((y - (-39.68f)) / 2.0f);
  return cx * 40 + cy;
}

template <int LOGN>
__global__ __launch_bounds__(SortShape<LOGN>::T) void pillar_weights_kernel(int n, const float *__restrict__ xyz, long long scene,
                                                                           float *__restrict__ weights) {
  constexpr int N = SortShape<LOGN>::N, T = SortShape<LOGN>::T;
  __shared__ u64 e[N];
  xyz += (long long)blockIdx.x * scene;
  weights += (long long)blockIdx.x * n;
#pragma unroll
  for (int q = 0; q < N / T; ++q) {
    const int k = threadIdx.x + q * T;
    u64 v = 0;
    if (k < n) v = ((u64)((unsigned)pillar_key(xyz[3 * k], xyz[3 * k + 1]) ^ 0x80000000u) << 32) | (unsigned)k;
    e[k] = v;
  }
  sort_desc<LOGN>(e);
  for (int p = threadIdx.x; p < N; p += T) {
    const u64 v = e[p];
    if (v == 0) continue;                       // a slot past n (a live entry's order word is never 0)
    const u64 key = v >> 32;                    // |key| < 2^31 - 1 inside the input domain: key + 1 does not wrap
    const int count = count_ge<LOGN>(e, key << 32) - count_ge<LOGN>(e, (key + 1) << 32);
    weights[(unsigned)v] = 1.0f / (float)count;
  }
}

int sort_log2(int n) {
  int l = kSortMinLog;
  while ((1 << l) < n) ++l;
  return l;
}

}  // namespace

#define SORT_DISPATCH(LOG, CASE)  \
  switch (LOG) {                  \
    case 8: CASE(8); break;       \
    case 9: CASE(9); break;       \
    case 10: CASE(10); break;     \
    case 11: CASE(11); break;     \
    case 12: CASE(12); break;     \
    case 13: CASE(13); break;     \
    default: CASE(14); break;     \
  }

DET6D_API int det6d_ext_topk_scores(int b, int n_total, int lo, int hi, int m, const float *scores, float gamma, int *idx,
                                    int idx_stride, int idx_offset, int idx_bias, det6d_stream_t stream) {
  if (b < 0) return det6d_ext_fail("det6d_ext_topk_scores: b = %d < 0", b);
  if (n_total <= 0 || lo < 0 || hi > n_total || hi <= lo)
    return det6d_ext_fail("det6d_ext_topk_scores: bad slice [%d, %d) of %d points", lo, hi, n_total);
  const int n = hi - lo;
  if (n > kSortMaxN) return det6d_ext_fail("det6d_ext_topk_scores: %d points per scene (at most %d)", n, kSortMaxN);
  if (m < 0 || m > n) return det6d_ext_fail("det6d_ext_topk_scores: m = %d of %d points", m, n);
  if (idx_offset < 0 || idx_stride < idx_offset + m)
    return det6d_ext_fail("det6d_ext_topk_scores: m = %d at offset %d does not fit an index row of %d", m, idx_offset, idx_stride);
  if (b == 0 || m == 0) return DET6D_OK;
  if (!scores || !idx) return det6d_ext_fail("det6d_ext_topk_scores: null pointer");
  const dim3 grid(b);
#define TOPK_CASE(L)                                                                                                       \
  hipLaunchKernelGGL((topk_scores_kernel<L>), grid, dim3(SortShape<L>::T), 0, (hipStream_t)stream, n, m, scores + lo,     \
                     (long long)n_total, gamma, idx + idx_offset, (long long)idx_stride, lo + idx_bias)
  SORT_DISPATCH(sort_log2(n), TOPK_CASE)
#undef TOPK_CASE
  return det6d_check_launch("det6d_ext_topk_scores");
}

DET6D_API int det6d_ext_pillar_weights(int b, int n_total, int lo, int hi, const float *xyz, float *weights,
                                       det6d_stream_t stream) {
  if (b < 0) return det6d_ext_fail("det6d_ext_pillar_weights: b = %d < 0", b);
  if (n_total <= 0 || lo < 0 || hi > n_total || hi <= lo)
    return det6d_ext_fail("det6d_ext_pillar_weights: bad slice [%d, %d) of %d points", lo, hi, n_total);
  const int n = hi - lo;
  if (n > kSortMaxN) return det6d_ext_fail("det6d_ext_pillar_weights: %d points per scene (at most %d)", n, kSortMaxN);
  if (b == 0) return DET6D_OK;
  if (!xyz || !weights) return det6d_ext_fail("det6d_ext_pillar_weights: null pointer");
  const dim3 grid(b);
#define PILLAR_CASE(L)                                                                                                     \
  hipLaunchKernelGGL((pillar_weights_kernel<L>), grid, dim3(SortShape<L>::T), 0, (hipStream_t)stream, n,                  \
                     xyz + (size_t)lo * 3, (long long)n_total * 3, weights)
  SORT_DISPATCH(sort_log2(n), PILLAR_CASE)
#undef PILLAR_CASE
  return det6d_check_launch("det6d_ext_pillar_weights");
}
