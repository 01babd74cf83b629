// mlp_chain.hip — the three pointwise layers of a NARROW set-abstraction group (all widths <= 64:
// the first SA layer of Det6D, [4->16->16->32] and [4->32->32->64] on 0.5 M / 1 M rows per batch)
// fused into one launch: gather -> L1 -> L2 -> L3 -> mask -> max-pool, intermediates never leave
// the CU.
//
// Why a separate kernel: at these widths every layer of the generic GEMM (linear.hip) is bound by
// writing and re-reading (rows x 32) fp32 intermediates through HBM (~0.8 GB per batch) and by six
// launches; the arithmetic is only 7.6 GFLOP.
//
// Wave-autonomous design: one wave64 owns a 32-row tile (= nsample rows of one centre, or two centres
// at nsample 16) through all three layers, so there is NO workgroup barrier after the weights are
// staged.  A layer's 32x32 accumulator tiles (v_mfma_f32_32x32x2_f32: channel on the lane, rows in the
// registers) are written to a wave-private LDS tile laid out [channel][row] (row stride 33 floats:
// conflict-free both ways), which is exactly the k-major image the next layer's A fragment
// (A[i = lane&31][k = lane>>5]) reads with one ds_read_b32.  Weights (<= 13 KB for the three layers)
// sit in LDS for the whole kernel.
//
// Arithmetic is identical to three det6d_linear calls: every output is one ascending-k fmaf chain,
// + shift, ReLU; masked max over the nsample rows.
#include "common.h"
#include "compact_list.h"
#include "mfma_tile.h"
#include <stdlib.h>

namespace {

D6_GEMM_PRIO_DECL

constexpr int kChainWaves = 4;
constexpr int kPackTiles = 1;    // compact lists: tiles a wave must get before another workgroup is used (1: 9970, 2: 9910, 4: 9780 scenes/s)
constexpr int kTS = 33;       // row stride of the wave-private [channel][row] tiles
constexpr int kMaxK1 = 8;     // input row width (x,y,z,features + pad)
constexpr int kMaxC = 32;     // hidden widths
constexpr int kMaxC3 = 64;    // output width

struct ChainArgs {
  int rows;                   // b * m * ns
  int n, m, ns;
  const float *a; int lda;    // point rows (B, n, lda)
  const int *idx;             // (B, m, ns)
  const float *ctr; int ldctr;
  const int *cnt;             // (B*m)
  const float *w1, *w2, *w3;  // folded weights, row-major, leading dims ldw1.. (multiples of 4)
  int ldw1, ldw2, ldw3;
  const float *s1, *s2, *s3;  // shifts
  int k1, c1, c2, c3;         // true widths: k1 = lda, c1,c2 <= 32, c3 <= 64
  float *y; int ldy; int col0;
  // compact (ragged) rows (compact_list.h): live row count and class regions in hdr, one point row and one
  // centre tag per compact row; rows = capacity then
  const int *hdr; const int *crow_p; const int *crow_c;
};

// classes 1 and 2: every accumulator (pair) of a 32x32 tile is a group of its own: stored at once (no pending slot).
// tags[e] = centre tag of the row accumulator e of this lane holds (chain_row_tags).
__device__ __forceinline__ void chain_store_small(const ChainArgs &g, const f32x16 &o, int s, const int (&tags)[16], int col, float sh) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (s == 2 && (e & 1)) continue;
    const float raw = s == 2 ? d6_vmax(o[e], o[e + 1 < 16 ? e + 1 : e]) : o[e];
    const int tag = tags[e];
    if (tag >= 0) d6_compact_store(g.y + (size_t)d6_compact_centre(tag) * g.ldy + g.col0 + col, d6_compact_is_empty(tag) ? 0.f : d6_relu(raw + sh), tag);
  }
}
// Row tags of a tile from the lanes that loaded them (lane r and r + 32 hold the tag of row r): accumulator e of a lane in
// half kh is row (e & 3) + 8 (e >> 2) + 4 kh.  A cross-lane read (ds_bpermute, no memory) instead of a global load per
// accumulator: round 2 re-read crow_c inside the epilogue, 16 dependent L2 round trips per column tile, and — the class
// regions being contiguous — the workgroups that owned the tail of the list (classes 2 and 1) ran several times longer
// than the others (the kernels' matrix pipes were busy 33-42 %: profiles/r03_beam_*).
__device__ __forceinline__ void chain_row_tags(int my_tag, int kh, int (&tags)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) tags[e] = __shfl(my_tag, d6_acc_row(e) + 4 * kh);
}
// mlp_chain_kernel only: with d6_relu (common.h) in its place the compiler schedules that kernel differently (1118 -> 1241
// lines of code), so the LDS kernel keeps the C form; the register kernels use d6_relu
__device__ __forceinline__ float relu1(float v) { return v > 0.f ? v : 0.f; }

// column of a gathered row [x - cx, y - cy, z - cz, f_0 ..] at position j of the oracle's fma chain (chain_k in
// oracle/det6d_oracle.c): the feature columns first, the three relative coordinates last
__host__ __device__ __forceinline__ int chain_col(int j, int k1) { return j + 3 < k1 ? j + 3 : j + 3 - k1; }

__global__ __launch_bounds__(64 * kChainWaves) void mlp_chain_kernel(const ChainArgs g) {
  D6_GEMM_PRIO_APPLY();
  __shared__ float W1[kMaxK1 * kMaxC];
  __shared__ float W2[kMaxC * kMaxC];
  __shared__ float W3[kMaxC * kMaxC3];
  __shared__ float S1[kMaxC], S2[kMaxC], S3[kMaxC3];
  __shared__ float T[kChainWaves][2][kMaxC * kTS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, kh = lane >> 5;

  // ---- stage weights (zero padded to the tile widths) ----
  // layer 1 takes the gathered row in the oracle's chain order (chain_k): feature columns first, relative coordinates last
  for (int t = tid; t < kMaxK1 * kMaxC; t += blockDim.x) {
    const int k = t / kMaxC, c = t % kMaxC;
    W1[t] = (k < g.k1 && c < g.c1) ? g.w1[(size_t)chain_col(k, g.k1) * g.ldw1 + c] : 0.f;
  }
  for (int t = tid; t < kMaxC * kMaxC; t += blockDim.x) {
    const int k = t / kMaxC, c = t % kMaxC;
    W2[t] = (k < g.c1 && c < g.c2) ? g.w2[(size_t)k * g.ldw2 + c] : 0.f;
  }
  for (int t = tid; t < kMaxC * kMaxC3; t += blockDim.x) {
    const int k = t / kMaxC3, c = t % kMaxC3;
    W3[t] = (k < g.c2 && c < g.c3) ? g.w3[(size_t)k * g.ldw3 + c] : 0.f;
  }
  if (tid < kMaxC) { S1[tid] = tid < g.c1 ? g.s1[tid] : 0.f; S2[tid] = tid < g.c2 ? g.s2[tid] : 0.f; }
  if (tid < kMaxC3) S3[tid] = tid < g.c3 ? g.s3[tid] : 0.f;
  __syncthreads();

  float *T1 = T[wave][0], *T2 = T[wave][1];
  const int ntiles = g.rows / 32;
  const int k1e = (g.k1 + 1) & ~1, c1e = (g.c1 + 1) & ~1, c2e = (g.c2 + 1) & ~1;
  const int nt3 = (g.c3 + 31) / 32;

  for (int tile = blockIdx.x * kChainWaves + wave; tile < ntiles; tile += gridDim.x * kChainWaves) {
    const int r = tile * 32 + l31;                 // my row (both lane halves hold the same row)
    const int cj = r / g.ns;
    const int bi = cj / g.m;
    const int p = g.idx[r];
    const float *src = g.a + ((size_t)bi * g.n + p) * g.lda;
    const float *c = g.ctr + (size_t)cj * g.ldctr;
    // ---- layer 1: A' = [xyz - centre, features], K = k1 ----
    float av[kMaxK1];
#pragma unroll
    for (int k = 0; k < kMaxK1; ++k) av[k] = 0.f;
    {
      const float4 v0 = *reinterpret_cast<const float4 *>(src);
      av[0] = v0.x - c[0]; av[1] = v0.y - c[1]; av[2] = v0.z - c[2]; av[3] = v0.w;
      if (g.k1 > 4) {
        const float4 v1 = *reinterpret_cast<const float4 *>(src + 4);
        av[4] = v1.x; av[5] = v1.y; av[6] = v1.z; av[7] = v1.w;
      }
    }
    {
      float t8[kMaxK1];
#pragma unroll
      for (int k = 0; k < kMaxK1; ++k) t8[k] = av[k];
      if (g.k1 == 4) { av[0] = t8[3]; av[1] = t8[0]; av[2] = t8[1]; av[3] = t8[2]; }
      else { av[0] = t8[3]; av[1] = t8[4]; av[2] = t8[5]; av[3] = t8[6]; av[4] = t8[7]; av[5] = t8[0]; av[6] = t8[1]; av[7] = t8[2]; }
    }
    f32x16 acc;
    d6_acc_zero(acc);
#pragma unroll
    for (int s = 0; s < kMaxK1 / 2; ++s) {
      if (2 * s < k1e) {
        const float a = kh ? av[2 * s + 1] : av[2 * s];
        const float b = W1[(2 * s + kh) * kMaxC + l31];
        d6_mfma(a, b, acc);
      }
    }
    {
      const float sh = S1[l31];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = d6_acc_row(e) + 4 * kh;
        T1[l31 * kTS + row] = relu1(acc[e] + sh);
      }
    }
    d6_lds_wave_sync();
    // ---- layer 2: K = c1 ----
    d6_acc_zero(acc);
    for (int s = 0; s < c1e / 2; ++s) {
      const float a = T1[(2 * s + kh) * kTS + l31];
      const float b = W2[(2 * s + kh) * kMaxC + l31];
      d6_mfma(a, b, acc);
    }
    {
      const float sh = S2[l31];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = d6_acc_row(e) + 4 * kh;
        T2[l31 * kTS + row] = relu1(acc[e] + sh);
      }
    }
    d6_lds_wave_sync();
    // ---- layer 3: K = c2, N = c3 (1 or 2 column tiles), then mask + max over the nsample rows ----
    f32x16 acc3[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) d6_acc_zero(acc3[j]);
    for (int s = 0; s < c2e / 2; ++s) {
      const float a = T2[(2 * s + kh) * kTS + l31];
      const float b0 = W3[(2 * s + kh) * kMaxC3 + l31];
      d6_mfma(a, b0, acc3[0]);
      if (nt3 > 1) {
        const float b1 = W3[(2 * s + kh) * kMaxC3 + 32 + l31];
        d6_mfma(a, b1, acc3[1]);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j >= nt3) break;
      const int col = 32 * j + l31;
      const bool cok = col < g.c3;
      const float sh = S3[col];
      float q[4];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        float mx = relu1(acc3[j][4 * qq] + sh);
#pragma unroll
        for (int e = 1; e < 4; ++e) {
          const float v = relu1(acc3[j][4 * qq + e] + sh);
          mx = v > mx ? v : mx;
        }
        const float o = __shfl_xor(mx, 32);
        q[qq] = o > mx ? o : mx;
      }
      if (g.ns == 32) {
        float mx = q[0];
        mx = q[1] > mx ? q[1] : mx; mx = q[2] > mx ? q[2] : mx; mx = q[3] > mx ? q[3] : mx;
        if (cok && kh == 0) g.y[(size_t)tile * g.ldy + g.col0 + col] = (g.cnt[tile] > 0) ? mx : 0.f;
      } else {  // ns == 16: two centres per tile
        const float m0 = q[1] > q[0] ? q[1] : q[0];
        const float m1 = q[3] > q[2] ? q[3] : q[2];
        if (cok && kh == 0) {
          g.y[(size_t)(2 * tile) * g.ldy + g.col0 + col] = (g.cnt[2 * tile] > 0) ? m0 : 0.f;
          g.y[(size_t)(2 * tile + 1) * g.ldy + g.col0 + col] = (g.cnt[2 * tile + 1] > 0) ? m1 : 0.f;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();   // T1/T2 are rewritten by the next tile
  }
}

// ---- what the two register chain kernels share ----
// (Not the per-column-tile pooling block, the same text in both: as ONE function it changed the wide kernel's code.)

// tag of the row whose centre owns pooled value qq of this lane in a tile of class sc (-1: another lane writes it), from
// the lane that loaded it: lane r holds the tag cj of row r, so the list is not read a second time.  (References on purpose:
// with cj, sc and kh by value one kernel's registers are assigned differently.)
__device__ __forceinline__ int chain_pooled_tag(const int &cj, const int &sc, int qq, const int &kh) {
  const int r = d6_compact_out_row(sc, qq, kh);
  const int tg = __shfl(cj, r < 0 ? 0 : r);
  return r >= 0 ? tg : -1;
}

// ReLU of the first `nreg` of a transposed layer's 16 accumulator registers (per lane: 16 channels of ONE row) -> the
// activation fragments of the next layer's k-steps: frag[s] = {half0: channel 2s, half1: channel 2s + 1}
__device__ __forceinline__ void chain_to_fragments(const f32x16 &a, float *frag, int nreg) {
#pragma unroll
  for (int G = 0; G < 4; ++G) {
    if (4 * G >= nreg) break;
    float t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = d6_relu(a[4 * G + e]);
    // inline asm: this compiler drops the SECOND result of __builtin_amdgcn_permlane32_swap (seen in the ISA:
    // the source register is reused right after the swap).  a = [a.lo | b.lo], b = [a.hi | b.hi] afterwards.
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1\n\tv_permlane32_swap_b32 %2, %3\n\ts_nop 1"
                 : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
    frag[4 * G + 0] = t[0];   // channels 8G + 0, 1
    frag[4 * G + 1] = t[2];   // channels 8G + 2, 3
    frag[4 * G + 2] = t[1];   // channels 8G + 4, 5
    frag[4 * G + 3] = t[3];   // channels 8G + 6, 7
  }
}

// stores the pooled values of tile `pend_tile`, kept back for one iteration: pend[j] = column tile j; compact lists: one
// value per pooled row of the lane (pend_oc = its tag, -1: none), dense rows: one value per centre of the tile
template <int NS, bool COMPACT, int NT, int NP>
__device__ __forceinline__ void chain_flush(const ChainArgs &g, const float (&pend)[NT][NP], const int (&pend_oc)[4],
                                            int pend_tile, int l31) {
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = 32 * j + l31;
    if (COMPACT) {
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
        if (pend_oc[qq] >= 0) d6_compact_store(g.y + (size_t)d6_compact_centre(pend_oc[qq]) * g.ldy + g.col0 + col, pend[j][qq], pend_oc[qq]);
    } else if (NS == 32) {
      g.y[(size_t)pend_tile * g.ldy + g.col0 + col] = pend[j][0];
    } else {
      g.y[(size_t)(2 * pend_tile) * g.ldy + g.col0 + col] = pend[j][0];
      g.y[(size_t)(2 * pend_tile + 1) * g.ldy + g.col0 + col] = pend[j][1];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Register-resident variant for the widths Det6D's first SA layer uses ([4->16->16->32], [4->32->32->64]).
//
// Layers 1 and 2 are computed TRANSPOSED, D = W^T X^T: the weight fragment is the MFMA A operand (channel on
// lane&31), the activations the B operand (row on lane&31).  The accumulator then holds, per lane, 16
// CHANNELS of ONE row — and after ReLU that is, up to a lane-half exchange, exactly the B (or A) operand
// fragment of the next layer: `v_permlane32_swap` on register pairs turns {half0: ch 8G+0..3, half1: ch
// 8G+4..7} into per-step fragments {half0: ch 2s, half1: ch 2s+1}.  No LDS round trip, no barrier, no
// transposing stores; all weight fragments of the three layers stay in VGPRs (52 for the wide group).
// The folded-BN shift of layers 1-2 rides on one extra MFMA step (a = shift on the k0 half, b = 1):
// fma(shift, 1, acc) == acc + shift exactly, added last like the oracle does.  Layer 3 runs in the normal
// orientation (same fragments, operands swapped back) so that the max over the nsample rows is the cheap
// in-register / one-shuffle epilogue and the store is coalesced.
// Every output is still ONE ascending-k fma chain: bit-identical to det6d_linear x 3.
template <int C1, int C2, int C3, int NS, bool COMPACT = false>
__global__ __launch_bounds__(256) void mlp_chain_reg_kernel(const ChainArgs g) {
  D6_GEMM_PRIO_APPLY();
  constexpr int S1 = 2;            // k1 = 4: [dx, dy, dz, f]
  constexpr int S2 = C1 / 2, S3 = C2 / 2, NT3 = C3 / 32;
  const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
  int wave_global = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int n_waves = (gridDim.x * blockDim.x) >> 6;
  int pk_end = 0;
  if (COMPACT) {
    // Compact lists: the grid is sized for the capacity but the list holds a fraction of it.  Only the workgroups that get
    // at least kPackTiles tiles per wave stay (the others leave before they load or stage any weights), and the live tiles
    // go round the waves that stay: tile t -> wave t mod (active waves).  The class regions are contiguous (32-row parts
    // first, single rows last) and the small classes have the dearest epilogue, so every workgroup gets the same mix of
    // classes: contiguous chunks per workgroup (round 2) left the tail of the list to a few workgroups.
    // (The same lines open mlp_chain_wide_kernel: as a shared function they changed both kernels' code, LABNOTES.)
    const int wpw = blockDim.x >> 6, live = g.hdr[kCompactHdrLive] / 32;
    int nb = (live + wpw * kPackTiles - 1) / (wpw * kPackTiles);
    if (nb > (int)gridDim.x) nb = gridDim.x;
    if ((int)blockIdx.x >= nb) return;
    n_waves = nb * wpw;
    pk_end = live;
  }

  // weight fragments: lane (channel / column = l31, k = 2s + kh); one more step per transposed layer for the shift
  float wf1[S1 + 1], wf2[S2 + 1], wf3[NT3][S3];
#pragma unroll
  for (int s = 0; s < S1; ++s) wf1[s] = l31 < C1 ? g.w1[(size_t)chain_col(2 * s + kh, 4) * g.ldw1 + l31] : 0.f;   // rows 3,0 | 1,2
  wf1[S1] = (kh == 0 && l31 < C1) ? g.s1[l31] : 0.f;
#pragma unroll
  for (int s = 0; s < S2; ++s) wf2[s] = l31 < C2 ? g.w2[(size_t)(2 * s + kh) * g.ldw2 + l31] : 0.f;
  wf2[S2] = (kh == 0 && l31 < C2) ? g.s2[l31] : 0.f;
#pragma unroll
  for (int j = 0; j < NT3; ++j)
#pragma unroll
    for (int s = 0; s < S3; ++s) wf3[j][s] = g.w3[(size_t)(2 * s + kh) * g.ldw3 + 32 * j + l31];
  float sh3[NT3];
#pragma unroll
  for (int j = 0; j < NT3; ++j) sh3[j] = g.s3[32 * j + l31];
  const float one_k0 = kh == 0 ? 1.f : 0.f;

  int h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0;
  if (COMPACT) d6_compact_class_ends(g.hdr, h1, h2, h3, h4, h5);
  const int ntiles = COMPACT ? pk_end : g.rows / 32;   // end of this wave's tile range
  const int *nb_idx = COMPACT ? g.crow_p : g.idx;   // per-row neighbour: point index inside the scene / global point row
  // the tile index is wave-uniform: kept in SGPRs so that the batch index (a division by m) is scalar work
  int tile = __builtin_amdgcn_readfirstlane(wave_global);
  if (tile >= ntiles) return;
  // software pipeline: the neighbour index of the tile after next and the point row of the next tile are in
  // flight while this tile computes (index -> row is a dependent pair of loads)
  struct TileIn { float4 row; float cx, cy, cz; int cnt0, cnt1; int oc[4]; int tag; };
  // list entries of a tile: neighbour index, and on compact lists the centre tag of the row and the tags of the pooled
  // rows.  They are the FIRST of the gather's two dependent loads and travel a whole tile ahead of the rows / centres they
  // address (round 2 fetched the tags together with the rows: every iteration then waited for an L2 round trip between
  // the tag load and the centre load — the matrix pipe of this kernel was busy 39 % of the time on ray-cast scenes)
  struct TileIdx { int p, cj; };
  auto fetch_idx = [&](int t) {
    TileIdx ix;
    ix.p = nb_idx[t * 32 + l31];
    ix.cj = COMPACT ? g.crow_c[t * 32 + l31] : 0;
    return ix;
  };
  auto fetch = [&](int t, const TileIdx &ix) {   // t wave-uniform; for NS == 16 the two centres of a tile share the batch (m even)
    TileIn in;
    const int p = ix.p;
    if (COMPACT) {
      in.row = *reinterpret_cast<const float4 *>(g.a + (size_t)p * 4);
      const int cj = ix.cj;
      const float *c = g.ctr + (size_t)(cj < 0 ? 0 : cj & kCompactTagCentre) * g.ldctr;
      in.cx = c[0]; in.cy = c[1]; in.cz = c[2];
      in.cnt0 = in.cnt1 = 0;
      in.tag = cj;
      const int sc = d6_compact_class(t * 32, h1, h2, h3, h4, h5);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) in.oc[qq] = chain_pooled_tag(cj, sc, qq, kh);
      return in;
    }
    in.tag = 0;
    const int c0 = NS == 32 ? t : 2 * t;             // first centre of the tile (scalar)
    const int bi = c0 / g.m;                         // scalar division
    const int cj = NS == 32 ? c0 : c0 + (l31 >> 4);
    in.row = *reinterpret_cast<const float4 *>(g.a + ((size_t)bi * g.n + p) * 4);
    const float *c = g.ctr + (size_t)cj * g.ldctr;
    in.cx = c[0]; in.cy = c[1]; in.cz = c[2];
    in.cnt0 = g.cnt[c0];
    in.cnt1 = NS == 32 ? 0 : g.cnt[c0 + 1];
    return in;
  };
  TileIn nxt = fetch(tile, fetch_idx(tile));
  TileIdx ix_next = tile + n_waves < ntiles ? fetch_idx(tile + n_waves) : TileIdx{0, 0};
  // results are stored one iteration late, BEFORE the next prefetch is issued: the wait for the prefetched
  // inputs at the top of an iteration then never waits for this tile's stores (vmcnt counts in order)
  float pend[NT3][COMPACT ? 4 : 2];
  int pend_oc[4] = {-1, -1, -1, -1};
  int pend_tile = -1;
  auto flush = [&]() { chain_flush<NS, COMPACT>(g, pend, pend_oc, pend_tile, l31); };   // bound here: a direct call compiles differently
  for (; tile < ntiles; tile += n_waves) {
    const TileIn cur = nxt;
    if (pend_tile >= 0) flush();
    if (tile + n_waves < ntiles) {
      nxt = fetch(tile + n_waves, ix_next);
      if (tile + 2 * n_waves < ntiles) ix_next = fetch_idx(tile + 2 * n_waves);
    }
    const float4 v0 = cur.row;
    const float cx = cur.cx, cy = cur.cy, cz = cur.cz;
    const float x0 = v0.x - cx, x1 = v0.y - cy, x2 = v0.z - cz, x3 = v0.w;

    // ---- layer 1 (transposed): acc[e] = channel d6_acc_row(e) + 4 * kh of row l31 ----
    f32x16 acc;
    d6_acc_zero(acc);
    d6_mfma(wf1[0], kh ? x0 : x3, acc);   // chain order: f, dx, dy, dz
    d6_mfma(wf1[1], kh ? x2 : x1, acc);
    d6_mfma(wf1[2], one_k0, acc);
    float frag[16];   // frag[s] = activation fragment of k-step s: {half0: channel 2s, half1: channel 2s + 1}
    chain_to_fragments(acc, frag, S2);
    // ---- layer 2 (transposed) ----
    d6_acc_zero(acc);
#pragma unroll
    for (int s = 0; s < S2; ++s) d6_mfma(wf2[s], frag[s], acc);
    d6_mfma(wf2[S2], one_k0, acc);
    chain_to_fragments(acc, frag, S3);
    // ---- layer 3 (rows in the registers again), shift + ReLU + mask + max over the nsample rows ----
#pragma unroll
    for (int j = 0; j < NT3; ++j) {
      f32x16 o;
      d6_acc_zero(o);
#pragma unroll
      for (int s = 0; s < S3; ++s) d6_mfma(frag[s], wf3[j][s], o);
      const int col = 32 * j + l31;
      // max over the rows on the raw accumulators, shift + ReLU on the pooled value (monotone: same result)
      float q[4];
      if (COMPACT) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) q[qq] = d6_acc_max4(o, qq);
        const int sc = d6_compact_class(tile * 32, h1, h2, h3, h4, h5);
        if (sc < 4) {
          int tags[16];
          chain_row_tags(cur.tag, kh, tags);
          chain_store_small(g, o, sc, tags, col, sh3[j]);
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) pend[j][qq] = 0.f;
          continue;
        }
        d6_compact_pool(q, sc);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) pend[j][qq] = d6_compact_is_empty(cur.oc[qq]) ? 0.f : d6_relu(q[qq] + sh3[j]);
        continue;
      }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) q[qq] = d6_half_max(d6_acc_max4(o, qq));
      if (NS == 32) {
        const float mx = d6_relu(d6_vmax(d6_vmax(q[0], q[1]), d6_vmax(q[2], q[3])) + sh3[j]);
        pend[j][0] = (cur.cnt0 > 0) ? mx : 0.f;   // both lane halves hold the pooled value: all 64 lanes store it
      } else {
        const float m0 = d6_relu(d6_vmax(q[0], q[1]) + sh3[j]);
        const float m1 = d6_relu(d6_vmax(q[2], q[3]) + sh3[j]);
        pend[j][0] = (cur.cnt0 > 0) ? m0 : 0.f;
        pend[j][1] = (cur.cnt1 > 0) ? m1 : 0.f;
      }
    }
    pend_tile = tile;
    if (COMPACT) {
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) pend_oc[qq] = cur.oc[qq];
    }
  }
  flush();
}

// N k-steps of one 32 x 32 accumulator tile whose WEIGHT fragments come from LDS (w[u * stride], stride a compile-time
// multiple of the row length) and whose activation fragments x[0..N) sit in registers.  The fragments of block b + 1 (8
// k-steps) are requested BEFORE the MFMAs of block b and land in registers of their own: left to itself the compiler reads
// every fragment (pair) into the same register right before its use and waits for the LDS round trip with one MFMA in
// flight — the matrix pipe of mlp_chain_wide_kernel was busy 33-42 % of the time (rocprofv3 SQ_VALU_MFMA_BUSY_CYCLES,
// profiles/r03_beam_*).  W_IS_A: the weights are the A operand (transposed layers) or the B operand (layer 3).
template <int N, int STRIDE, bool W_IS_A>
__device__ __forceinline__ void mfma_steps_lds(const float *__restrict__ w, const float *x, f32x16 &acc) {
  constexpr int UB = 8, NB = (N + UB - 1) / UB;
  float wb[2][UB];
#pragma unroll
  for (int u = 0; u < UB; ++u)
    if (u < N) wb[0][u] = w[u * STRIDE];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b + 1 < NB) {
#pragma unroll
      for (int u = 0; u < UB; ++u)
        if ((b + 1) * UB + u < N) wb[(b + 1) & 1][u] = w[((b + 1) * UB + u) * STRIDE];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if (b * UB + u < N) {
        if (W_IS_A) d6_mfma(wb[b & 1][u], x[b * UB + u], acc);
        else d6_mfma(x[b * UB + u], wb[b & 1][u], acc);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---------------------------------------------------------------------------------------------------
// Wide register chain: the same transposed-accumulator scheme for the second SA layer's groups
// ([68->64->64->128], [68->64->96->128]): 264 / 361 MFMAs per 32-row tile.  The weights (66-92 KB with the
// shift appended as one more k-row pair) sit in LDS, row-major [k][C], which is conflict-free for the A
// fragment of the transposed layers (channel on lane&31) and for the B fragment of layer 3 alike; they
// are read one ds_read_b32 per MFMA (LDS instructions do not take vector-ALU slots).  The gathered input
// row never touches LDS either: lane (row, kh) loads x[row][2s + kh] directly, 34 dword loads with
// immediate offsets, issued for the NEXT tile as soon as layer 1 of the current one has consumed them.
// Per tile ~250 vector-ALU ops (ReLU, swaps, pooling) against 17-23 k cycles of matrix work.
template <int C2, int NS, bool COMPACT = false>
__global__ __launch_bounds__(512) void mlp_chain_wide_kernel(const ChainArgs g) {
  D6_GEMM_PRIO_APPLY();
  constexpr int K1 = 68, C1 = 64, C3 = 128;
  constexpr int S1 = K1 / 2, S2 = C1 / 2, S3 = C2 / 2;
  constexpr int T1 = C1 / 32, T2 = C2 / 32, T3 = C3 / 32;
  extern __shared__ float lds[];
  float *W1 = lds;                          // (K1 + 2) x C1 : rows K1, K1+1 = shift, 0
  float *W2 = W1 + (K1 + 2) * C1;           // (C1 + 2) x C2
  float *W3 = W2 + (C1 + 2) * C2;           // C2 x C3
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
  int pk_stride = 0, pk_first = 0, pk_end = 0;
  if (COMPACT) {   // the workgroups that stay and the deal of the live tiles: as in mlp_chain_reg_kernel, see there
    const int wpw = blockDim.x >> 6, live = g.hdr[kCompactHdrLive] / 32;
    int nb = (live + wpw * kPackTiles - 1) / (wpw * kPackTiles);
    if (nb > (int)gridDim.x) nb = gridDim.x;
    if ((int)blockIdx.x >= nb) return;
    pk_stride = nb * wpw;
    pk_first = blockIdx.x * wpw + (tid >> 6);
    pk_end = live;
  }
  // staging with 16-byte loads (all leading dimensions and widths are multiples of 4)
  auto stage = [&](float *dst, const float *w, int ldw, const float *shift, int k_rows, int cols, bool chain_order) {
    const int c4 = cols / 4;
    for (int t = tid; t < (k_rows + (shift ? 2 : 0)) * c4; t += blockDim.x) {
      const int k = t / c4, c = 4 * (t % c4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < k_rows) v = *reinterpret_cast<const float4 *>(w + (size_t)(chain_order ? chain_col(k, k_rows) : k) * ldw + c);
      else if (k == k_rows) v = *reinterpret_cast<const float4 *>(shift + c);
      *reinterpret_cast<float4 *>(dst + k * cols + c) = v;
    }
  };
  stage(W1, g.w1, g.ldw1, g.s1, K1, C1, true);    // layer 1 in the oracle's chain order: features, then dx, dy, dz
  stage(W2, g.w2, g.ldw2, g.s2, C1, C2, false);
  stage(W3, g.w3, g.ldw3, nullptr, C2, C3, false);
  float sh3[T3];
#pragma unroll
  for (int j = 0; j < T3; ++j) sh3[j] = g.s3[32 * j + l31];
  __syncthreads();

  const float one_k0 = kh == 0 ? 1.f : 0.f;
  const int wave_global = COMPACT ? pk_first : (int)((blockIdx.x * blockDim.x + tid) >> 6);
  const int n_waves = COMPACT ? pk_stride : (int)((gridDim.x * blockDim.x) >> 6);   // tile stride of this wave
  int h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0;
  if (COMPACT) d6_compact_class_ends(g.hdr, h1, h2, h3, h4, h5);
  const int ntiles = COMPACT ? pk_end : g.rows / 32;                                 // end of this wave's tile range
  int tile = __builtin_amdgcn_readfirstlane(wave_global);
  if (tile >= ntiles) return;

  float xin[S1 + 1];        // [S1] = the shift step's activation fragment (1 on the k0 half)
  float csub0, csub1;
  int cnt0, cnt1;
  int oc_n[4] = {-1, -1, -1, -1};
  // list entries of a tile (point row, centre tag, tags of the pooled rows): the FIRST of the gather's two dependent
  // loads, requested a whole tile ahead of the rows they address (fetch_entries(t + 2 strides) while tile t computes)
  int e_p = 0, e_c = 0, tag_n = 0;
  auto fetch_entries = [&](int t) {
    if (COMPACT) {
      e_p = g.crow_p[t * 32 + l31];
      e_c = g.crow_c[t * 32 + l31];
    } else {
      e_p = g.idx[t * 32 + l31];
    }
  };
  auto fetch = [&](int t) {   // t wave-uniform; consumes the entries fetch_entries(t) left in e_p / e_c
    if (COMPACT) {
      const int p = e_p;
      const float *row = g.a + (size_t)p * K1;
      const float *src = row + 3 + kh;          // chain position j = 2s + kh reads column j + 3 (features) ...
#pragma unroll
      for (int s = 0; s < S1 - 2; ++s) xin[s] = src[2 * s];
      xin[S1 - 2] = row[kh ? 0 : K1 - 1];       // ... then (pad, x) and (y, z): chain_col(64..67, 68) = 67, 0, 1, 2
      xin[S1 - 1] = row[kh ? 2 : 1];
      const int cj = e_c;
      const float *c = g.ctr + (size_t)(cj < 0 ? 0 : cj & kCompactTagCentre) * g.ldctr;
      csub0 = kh ? c[0] : 0.f;
      csub1 = kh ? c[2] : c[1];
      cnt0 = cnt1 = 0;
      tag_n = cj;
      const int sc = d6_compact_class(t * 32, h1, h2, h3, h4, h5);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) oc_n[qq] = chain_pooled_tag(cj, sc, qq, kh);
      return;
    }
    const int c0 = NS == 32 ? t : 2 * t;
    const int bi = c0 / g.m;
    const int cj = NS == 32 ? c0 : c0 + (l31 >> 4);
    const int p = e_p;
    const float *row = g.a + ((size_t)bi * g.n + p) * K1;
    const float *src = row + 3 + kh;
#pragma unroll
    for (int s = 0; s < S1 - 2; ++s) xin[s] = src[2 * s];
    xin[S1 - 2] = row[kh ? 0 : K1 - 1];
    xin[S1 - 1] = row[kh ? 2 : 1];
    const float *c = g.ctr + (size_t)cj * g.ldctr;
    csub0 = kh ? c[0] : 0.f;          // chain positions 64 | 65: pad | x
    csub1 = kh ? c[2] : c[1];         // chain positions 66 | 67: y | z
    cnt0 = g.cnt[c0];
    cnt1 = NS == 32 ? 0 : g.cnt[c0 + 1];
  };
  float pend[T3][COMPACT ? 4 : 2];
  int pend_oc[4] = {-1, -1, -1, -1};
  int pend_tile = -1;
  auto flush = [&]() { chain_flush<NS, COMPACT>(g, pend, pend_oc, pend_tile, l31); };   // bound here: a direct call compiles differently

  fetch_entries(tile);
  fetch(tile);
  if (tile + n_waves < ntiles) fetch_entries(tile + n_waves);
  for (; tile < ntiles; tile += n_waves) {
    if (pend_tile >= 0) flush();
    const int my_cnt0 = cnt0, my_cnt1 = cnt1, my_tag = tag_n;
    int my_oc[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) my_oc[qq] = oc_n[qq];
    xin[S1 - 2] = xin[S1 - 2] - csub0;     // pad | dx
    xin[S1 - 1] = xin[S1 - 1] - csub1;     // dy | dz
    xin[S1] = one_k0;
    // ---- layer 1 (transposed): K1 -> C1, the shift as one more k-step (rows K1, K1 + 1 of the staged matrix) ----
    float f1[S2 + 1];
#pragma unroll
    for (int t = 0; t < T1; ++t) {
      f32x16 acc;
      d6_acc_zero(acc);
      mfma_steps_lds<S1 + 1, 2 * C1, true>(W1 + kh * C1 + 32 * t + l31, xin, acc);
      chain_to_fragments(acc, f1 + 16 * t, 16);
    }
    f1[S2] = one_k0;
    // the input registers are free: start the next tile's gather now (its list entries arrived a tile ago), it lands
    // during layers 2 and 3; then request the list entries of the tile after next
    if (tile + n_waves < ntiles) {
      fetch(tile + n_waves);
      if (tile + 2 * n_waves < ntiles) fetch_entries(tile + 2 * n_waves);
    }
    // ---- layer 2 (transposed): C1 -> C2 ----
    float f2[S3];
#pragma unroll
    for (int t = 0; t < T2; ++t) {
      f32x16 acc;
      d6_acc_zero(acc);
      mfma_steps_lds<S2 + 1, 2 * C2, true>(W2 + kh * C2 + 32 * t + l31, f1, acc);
      chain_to_fragments(acc, f2 + 16 * t, 16);
    }
    // ---- layer 3 (rows in the registers): C2 -> C3, pool, shift, ReLU, mask ----
#pragma unroll
    for (int j = 0; j < T3; ++j) {
      f32x16 o;
      d6_acc_zero(o);
      mfma_steps_lds<S3, 2 * C3, false>(W3 + kh * C3 + 32 * j + l31, f2, o);
      float q[4];
      if (COMPACT) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) q[qq] = d6_acc_max4(o, qq);
        const int sc = d6_compact_class(tile * 32, h1, h2, h3, h4, h5);
        if (sc < 4) {
          int tags[16];
          chain_row_tags(my_tag, kh, tags);
          chain_store_small(g, o, sc, tags, 32 * j + l31, sh3[j]);
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) pend[j][qq] = 0.f;
          continue;
        }
        d6_compact_pool(q, sc);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) pend[j][qq] = d6_compact_is_empty(my_oc[qq]) ? 0.f : d6_relu(q[qq] + sh3[j]);
        continue;
      }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) q[qq] = d6_half_max(d6_acc_max4(o, qq));
      if (NS == 32) {
        const float mx = d6_relu(d6_vmax(d6_vmax(q[0], q[1]), d6_vmax(q[2], q[3])) + sh3[j]);
        pend[j][0] = my_cnt0 > 0 ? mx : 0.f;
      } else {
        pend[j][0] = my_cnt0 > 0 ? d6_relu(d6_vmax(q[0], q[1]) + sh3[j]) : 0.f;
        pend[j][1] = my_cnt1 > 0 ? d6_relu(d6_vmax(q[2], q[3]) + sh3[j]) : 0.f;
      }
    }
    pend_tile = tile;
    if (COMPACT) {
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) pend_oc[qq] = my_oc[qq];
    }
  }
  flush();
}

}  // namespace

// ---- host side ----

// dynamic LDS of mlp_chain_wide_kernel<C2, ..>
constexpr size_t chain_wide_lds_bytes(int c2) { return sizeof(float) * ((size_t)70 * 64 + (size_t)66 * c2 + (size_t)c2 * 128); }

// dense rows: idx / cnt and (n, m, ns), no list; compact rows: the list (hdr, crow_p, crow_c), rows = its capacity, the rest 0
static ChainArgs chain_args(int rows, int n, int m, int ns, const float *a, int lda, const int *idx, const float *ctr, int ldctr,
                            const int *cnt, const float *w1, int ldw1, const float *s1, int c1, const float *w2, int ldw2,
                            const float *s2, int c2, const float *w3, int ldw3, const float *s3, int c3, float *y, int ldy,
                            int col0, const int *hdr, const int *crow_p, const int *crow_c) {
  return ChainArgs{rows, n, m, ns, a, lda, idx, ctr, ldctr, cnt, w1, w2, w3, ldw1, ldw2, ldw3, s1, s2, s3, /* k1 = */ lda, c1, c2, c3,
                   y, ldy, col0, hdr, crow_p, crow_c};   // the struct's field order
}

// The plan of det6d_mlp_chain3 (dense rows: b scenes x m centres x ns rows) and det6d_mlp_chain3_compact (a row list of
// `capacity` rows; ns, b, m unused): refusal, or the route and its launch geometry.  b == 0 asks about the widths alone.
// a_aligned16: the point rows' address; w_aligned16: w1..w3, s1, s2 and ldw1..3 * 4 are multiples of 16 bytes.
static int chain_plan(int lda, int c1, int c2, int c3, int ns, int b, int m, bool compact, int capacity, bool a_aligned16,
                      bool w_aligned16, det6d_launch_plan &p) {
  if (compact ? (b && (capacity <= 0 || (capacity & 127))) : ((ns != 16 && ns != 32) || b < 0 || (b && m <= 0))) return DET6D_EINVAL;
  const long long rows = compact ? (b ? capacity : 0) : (long long)b * m * ns;
  if (rows % 32 || rows > 0x7fffffff) return DET6D_EINVAL;
  // a 32-row tile of ns = 16 rows holds two centres, which must be of ONE scene
  const bool pairs_ok = compact || !b || ns == 32 || !(m & 1);
  static const bool no_wide = det6d_env_set("DET6D_CHAIN_NO_WIDE"), use_lds_env = det6d_env_set("DET6D_CHAIN_LDS");
  const bool wide = lda == 68 && c1 == 64 && (c2 == 64 || c2 == 96) && c3 == 128 && pairs_ok && w_aligned16 && !no_wide;
  const bool reg = lda == 4 && ((c1 == 16 && c2 == 16 && c3 == 32) || (c1 == 32 && c2 == 32 && c3 == 64)) && (compact || (pairs_ok && !use_lds_env));
  const int ntiles = (int)(rows / 32);
  if (wide) {
    // one 512-thread workgroup per CU (the weights fill most of its LDS), two waves per SIMD
    p = det6d_launch_plan{DET6D_CHAIN_WIDE, det6d_min(det6d_divup(ntiles, 8), 256), 1, 512, (unsigned)chain_wide_lds_bytes(c2), 32};
    return DET6D_OK;
  }
  if (lda < 4 || lda > kMaxK1 || (lda & 3) || !a_aligned16 || (compact && !reg)) return DET6D_EINVAL;
  if (c1 <= 0 || c1 > kMaxC || c2 <= 0 || c2 > kMaxC || c3 <= 0 || c3 > kMaxC3) return DET6D_EINVAL;
  // four waves, a tile each.  LDS kernel: persistent-ish (256 * 6 workgroups amortise the weight staging over many tiles).
  // Register kernel, dense: a grid of exactly one residency round (256 CUs x 4 SIMDs x 4 waves) so that every wave walks the
  // same number of tiles (1536 blocks left half the chip idle in the second round); compact: up to 2048 workgroups, each wave
  // walks ceil(live tiles / waves) tiles (measured on 32-scene passes, SA1's wide group alone / with the chip full: 768
  // workgroups 137 / 65 us, 1024: 115 / 64, 2048: 97 / 65, 4096: 87 / 70; ray-cast scenes 578 / 205, 507 / 205, 366 / 201,
  // 299 / 206).  DET6D_CHAIN_BLOCKS: experiments build only.
  static const int reg_cap_dense = det6d_env_int("DET6D_CHAIN_BLOCKS", 1024), reg_cap_compact = det6d_env_int("DET6D_CHAIN_BLOCKS", 2048);
  const int cap = !reg ? 256 * 6 : compact ? reg_cap_compact : det6d_min(256 * 6, reg_cap_dense);
  p = det6d_launch_plan{reg ? DET6D_CHAIN_REG : DET6D_CHAIN_LDS, det6d_min(det6d_divup(ntiles, kChainWaves), cap), 1, 64 * kChainWaves, 0, 32};
  return DET6D_OK;
}

DET6D_API int det6d_mlp_chain3_plan(int lda, int c1, int c2, int c3, int ns, int b, int m, int compact, int capacity,
                                    det6d_launch_plan *plan) {
  return plan ? chain_plan(lda, c1, c2, c3, ns, b, m, compact != 0, capacity, true, true, *plan) : DET6D_EINVAL;
}

// Both entries from here: leading dimensions, the plan, the instance of (route, second width, ns, compact).  A case label
// carries its instance's template arguments (compact lists: NS = 32; the LDS kernel: run-time widths).
constexpr int chain_key(int route, int c2, int ns, bool compact) { return ((route * 128 + c2) * 64 + ns) * 2 + compact; }
static int chain_run(const ChainArgs &g, int b, bool compact, hipStream_t s, const char *what) {
  if (g.ldctr < 3 || g.ldw1 < g.c1 || g.ldw2 < g.c2 || g.ldw3 < g.c3) return DET6D_EINVAL;
  const bool w_aligned16 = !((g.ldw1 | g.ldw2 | g.ldw3) & 3) &&
                           !(((uintptr_t)g.w1 | (uintptr_t)g.w2 | (uintptr_t)g.w3 | (uintptr_t)g.s1 | (uintptr_t)g.s2) & 15);
  det6d_launch_plan p;
  if (chain_plan(g.lda, g.c1, g.c2, g.c3, g.ns, b, g.m, compact, g.rows, !((uintptr_t)g.a & 15), w_aligned16, p) != DET6D_OK) return DET6D_EINVAL;
  if (g.rows == 0) return DET6D_OK;
  const bool lds = p.route == DET6D_CHAIN_LDS;
  switch (chain_key(p.route, lds ? 0 : g.c2, lds ? 0 : compact ? 32 : g.ns, compact)) {
    case chain_key(DET6D_CHAIN_WIDE, 64, 16, false): return det6d_launch<mlp_chain_wide_kernel<64, 16, false>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_WIDE, 64, 32, false): return det6d_launch<mlp_chain_wide_kernel<64, 32, false>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_WIDE, 96, 16, false): return det6d_launch<mlp_chain_wide_kernel<96, 16, false>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_WIDE, 96, 32, false): return det6d_launch<mlp_chain_wide_kernel<96, 32, false>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_WIDE, 64, 32, true): return det6d_launch<mlp_chain_wide_kernel<64, 32, true>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_WIDE, 96, 32, true): return det6d_launch<mlp_chain_wide_kernel<96, 32, true>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_REG, 16, 16, false): return det6d_launch<mlp_chain_reg_kernel<16, 16, 32, 16>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_REG, 16, 32, false): return det6d_launch<mlp_chain_reg_kernel<16, 16, 32, 32>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_REG, 32, 16, false): return det6d_launch<mlp_chain_reg_kernel<32, 32, 64, 16>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_REG, 32, 32, false): return det6d_launch<mlp_chain_reg_kernel<32, 32, 64, 32>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_REG, 16, 32, true): return det6d_launch<mlp_chain_reg_kernel<16, 16, 32, 32, true>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_REG, 32, 32, true): return det6d_launch<mlp_chain_reg_kernel<32, 32, 64, 32, true>>(g, p, s, what);
    case chain_key(DET6D_CHAIN_LDS, 0, 0, false): return det6d_launch<mlp_chain_kernel>(g, p, s, what);
    default: return DET6D_EINVAL;      // unreachable: chain_plan names no other (route, widths, ns, compact)
  }
}

DET6D_API int det6d_mlp_chain3(int rows, int n, int m, int ns, const float *a, int lda, const int *idx,
                               const float *ctr, int ldctr, const int *cnt, const float *w1, int ldw1, const float *s1,
                               int c1, const float *w2, int ldw2, const float *s2, int c2, const float *w3, int ldw3,
                               const float *s3, int c3, float *y, int ldy, int col0, det6d_stream_t stream) {
  D6_GEMM_PRIO_HOST();
  if (rows < 0 || n <= 0 || m <= 0 || (ns != 16 && ns != 32) || !a || !idx || !ctr || !cnt || !w1 || !w2 || !w3 || !s1 || !s2 ||
      !s3 || !y || rows % (m * ns))
    return DET6D_EINVAL;
  return chain_run(chain_args(rows, n, m, ns, a, lda, idx, ctr, ldctr, cnt, w1, ldw1, s1, c1, w2, ldw2, s2, c2, w3, ldw3, s3, c3, y, ldy,
                              col0, nullptr, nullptr, nullptr), rows / (m * ns), false, (hipStream_t)stream, "det6d_mlp_chain3");
}

// The same chains over a compact (ragged) row list: rows, classes and output centres come from det6d_compact_groups
// (hdr / crow_p / crow_c on the device), `capacity` only sizes the persistent grid.
DET6D_API int det6d_mlp_chain3_compact(int capacity, const int *hdr, const int *crow_p, const int *crow_c, const float *a,
                                       int lda, const float *ctr, int ldctr, const float *w1, int ldw1, const float *s1,
                                       int c1, const float *w2, int ldw2, const float *s2, int c2, const float *w3, int ldw3,
                                       const float *s3, int c3, float *y, int ldy, int col0, det6d_stream_t stream) {
  D6_GEMM_PRIO_HOST();
  if (!hdr || !crow_p || !crow_c || !a || !ctr || !w1 || !w2 || !w3 || !s1 || !s2 || !s3 || !y) return DET6D_EINVAL;
  return chain_run(chain_args(capacity, 0, 0, 0, a, lda, nullptr, ctr, ldctr, nullptr, w1, ldw1, s1, c1, w2, ldw2, s2, c2, w3, ldw3, s3,
                              c3, y, ldy, col0, hdr, crow_p, crow_c), 1, true, (hipStream_t)stream, "det6d_mlp_chain3_compact");
}
