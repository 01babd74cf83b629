// fps_common.h — what the whole farthest-point-sampler family shares (fps.hip, fps_cells.hip, fps_seq.hip, fps_coop.hip,
// fps_multi.h, ext/fps_features.hip): ONE definition of the reference's tie rule and of the small device helpers every
// sampler needs, and the prototypes of the family's cross-file host functions.
//
// The tie rule.  The reference resolves equal maxima through the order of its strided scan + shared-memory halving tree
// (sampling_gpu.cu:94-99,159-216): among equal values the winner minimises (bitrev_{log2 S}(k mod S), k), S = the block
// size opt_n_threads(N).  Every sampler here must pick exactly that point; a new sampler takes the rule from this header.
#pragma once
#include "common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
typedef float fps_f32x2 __attribute__((ext_vector_type(2)));   // two points at a time: v_pk_add / mul / fma_f32

// the lowest `bits` bits of v, reversed
__device__ __forceinline__ unsigned fps_bitrev(unsigned v, int bits) {
  return bits == 0 ? 0u : (__builtin_bitreverse32(v) >> (32 - bits));
}
// order key of point k under the reference's tie rule (smaller wins): (bitrev_{log2 S}(k mod S), k)
__device__ __forceinline__ unsigned fps_tie_key(int k, int log2s) {
  return (fps_bitrev((unsigned)k & ((1u << log2s) - 1u), log2s) << (32 - log2s)) | ((unsigned)k >> log2s);
}
// the point a tie key belongs to
__device__ __forceinline__ int fps_tie_key_point(unsigned key, int log2s) {
  if (log2s == 0) return (int)key;
  return (int)(((key & ((1u << (32 - log2s)) - 1u)) << log2s) | fps_bitrev(key >> (32 - log2s), log2s));
}
// lane holding the smallest key among the lanes of `cand` (tie path only)
__device__ __forceinline__ int fps_min_key_lane(u64 cand, unsigned key) {
  const int lane = threadIdx.x & 63;
  const bool mine = (cand >> lane) & 1ull;
  const unsigned k = mine ? key : 0xFFFFFFFFu;
  unsigned m = k;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)m, off);
    m = o < m ? o : m;
  }
  return __builtin_ctzll(__ballot(mine && k == m));
}
// the same from the lanes' point indices k (every lane computes its key: callers are tie paths)
__device__ __forceinline__ int fps_min_key_lane(u64 cand, int k, int log2s) {
  return fps_min_key_lane(cand, fps_tie_key(k, log2s));
}

// exclusive prefix sum over the 1024 threads of a workgroup (the counting sorts of the pre-passes: cell_sort_kernel,
// coop_split_kernel): wave scan (six shuffles), the sixteen wave totals through LDS (`wtot`: 16 words; free again when the
// call returns)
__device__ __forceinline__ unsigned fps_block_exclusive_sum_1024(unsigned v, unsigned *__restrict__ wtot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned base = 0u;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  __syncthreads();
  return base + incl - v;
}

// coordinates of slot `ws` (wave-uniform) of lane `wl`: a scalar binary search down to the statically indexed slot, then
// three v_readlane
template <int LO, int HI, int N>
__device__ __forceinline__ void fps_pick_slot(int ws, int wl, const float (&px)[N], const float (&py)[N],
                                              const float (&pz)[N], float &sx, float &sy, float &sz) {
  if constexpr (HI - LO == 1) {
    sx = d6_readlane_f(px[LO], wl);
    sy = d6_readlane_f(py[LO], wl);
    sz = d6_readlane_f(pz[LO], wl);
  } else {
    constexpr int MID = (LO + HI) / 2;
    if (ws < MID) fps_pick_slot<LO, MID>(ws, wl, px, py, pz, sx, sy, sz);
    else fps_pick_slot<MID, HI>(ws, wl, px, py, pz, sx, sy, sz);
  }
}

}  // namespace

// log2 of the reference's block size S = opt_n_threads(work_size):
// core/pcdet/ops/pointnet2/pointnet2_batch/src/cuda_utils.h:10-14 (same double formula, same libm)
static inline int fps_opt_n_threads_log2(int work_size) {
  int pow_2 = (int)(log((double)work_size) / log(2.0));
  if (pow_2 > 10) pow_2 = 10;
  if (pow_2 < 0) pow_2 = 0;
  return pow_2;
}

// ---- host functions of the family that are called across files (libdet6d_hip.so only) -----------------------------------

// fps_cells.hip — D-FPS of 16384- / 4096-point scenes with fresh min-distances: k-d pre-pass + the multi-pick sampler.
// `perm` is (b, n) int32 scratch.
int det6d_fps_cells_launch(int b, int n, int m, int log2s, long long xyz_bstride, long long idx_bstride, int idx_add,
                           const float *xyz, int *perm, int *idx, hipStream_t stream);
// fps_cells.hip — the score-weighted form: the same pre-pass (the weights play no part in it) + fps_seq_w_kernel; word 0
// of a scene's `perm` becomes its "needs the exact-double sampler" flag.
int det6d_fps_cells_w_launch(int b, int n, int m, int log2s, long long xyz_bstride, long long idx_bstride, int idx_add,
                             const float *xyz, int *perm, int *idx, const float *weights, long long w_bstride, float gamma,
                             int w_is_score, hipStream_t stream);
// fps_cells.hip — k-d order (4 x 4 cells of equal counts, lanes ordered by the tie key) of every 16384-point part src[g] of
// `subscenes` scene parts; perm[g] = the part's points in that order.
int det6d_fps_cell_sort_parts(int subscenes, int parts, int log2s, long long xyz_bstride, const float *xyz, const int *src,
                              int *perm, hipStream_t stream);

// fps_seq.hip — the multi-pick sampler on a scene's k-d permutation `perm` (lane groups of n / 1024 positions ordered by
// tie key), n = 16384 / 4096.
int det6d_fps_seq_launch(int b, int n, int m, int log2s, long long xyz_bstride, long long idx_bstride, int idx_add,
                         const float *xyz, const int *perm, int *idx, hipStream_t stream);
// fps_seq.hip — its score-weighted form: `flags` = the scenes' scratch (b x n ints: the permutation the pre-pass wrote;
// word 0 of a scene becomes its flag), weights / raw scores (b x w_bstride).
int det6d_fps_seq_w_launch(int b, int n, int m, int log2s, long long xyz_bstride, long long idx_bstride, int idx_add,
                           const float *xyz, const int *perm, int *idx, const float *weights, long long w_bstride, float gamma,
                           int w_is_score, int *flags, hipStream_t stream);

// fps_coop.hip — does the cooperative sampler take n points per scene (32768 / 65536, fresh min-distances)?
bool det6d_fps_coop_handles(int n);
// fps_coop.hip — bytes of the workspace a cooperative launch of b scenes needs; 0 when it does not take (b, n).
long long det6d_fps_coop_workspace_bytes(int b, int n);
// fps_coop.hip — does the current device hold one cooperative launch (>= 8 x parts compute units)?
bool det6d_fps_coop_fits_device(int n);
// fps_coop.hip — D-FPS of b scenes of n = 32768 / 65536 points; `workspace` of det6d_fps_coop_workspace_bytes(b, n) bytes,
// 256-byte aligned.
int det6d_fps_coop_launch(int b, int n, int m, int log2s, long long xyz_bstride, long long idx_bstride, int idx_add,
                          const float *xyz, void *workspace, int *idx, hipStream_t stream);
// fps_coop.hip — error word of the cooperative launches on `workspace` since it was last read (synchronises `stream`):
// DET6D_OK = fine.  Reading a set word clears it.
int det6d_fps_coop_status(int b, int n, const void *workspace, hipStream_t stream);
// fps_coop.hip — byte offset of the (sticky) error word inside a cooperative workspace; -1 when it does not take (b, n).
long long det6d_fps_coop_status_offset(int b, int n);

#ifdef DET6D_EXPERIMENTS
// fps_seq.hip — DET6D_DBG_POISON_LDS=<pattern>: fills the LDS of every CU before a sampler kernel (tests only)
void det6d_dbg_poison_lds_hook(hipStream_t stream);
#endif
