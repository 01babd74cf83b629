// mfma_tile.h — the 32 x 32 fp32 MFMA accumulator tile as code: ONE statement of what the GEMM family (linear.hip,
// mlp_chain.hip, mlp_group.hip, mlp_rows.hip) knows about v_mfma_f32_32x32x2_f32, and the idioms its kernels build from it.
//   D (32 x 32) += A (32 x 2) B (2 x 32) per wave64: every output is fma(a_k1, b_k1, fma(a_k0, b_k0, c)).
//   operands     lane (l31 = lane & 31, kh = lane >> 5) supplies A[row l31][k = kh] and B[k = kh][column l31];
//   accumulator  16 registers per lane, the lane's COLUMN is l31, register e holds ROW d6_acc_row(e) + 4 * kh: four consecutive
//                rows per four registers, those groups 8 rows apart, the lane halves interleaved by 4.  Registers 4q .. 4q + 3
//                of both halves together are the 8-row bundle [8q, 8q + 8).  With the operands swapped (A = weights: the
//                transposed layers of mlp_chain.hip) the same map reads: per lane, 16 CHANNELS of row l31.
// A kernel whose generated code changes under one of these helpers keeps its local form of that idiom and says so on the spot
// (register assignment and scheduling of these kernels follow the spelling of their unrolled loops).
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int d6_acc_row(int e) { return (e & 3) + 8 * (e >> 2); }      // lane half 0; half kh: + 4 * kh
// 32 (half, register) pairs, 32 rows: the xor of their row bits is all ones only if every row is held exactly once
constexpr unsigned d6_acc_row_bits(int i = 0) { return i == 32 ? 0u : (1u << (d6_acc_row(i & 15) + 4 * (i >> 4))) ^ d6_acc_row_bits(i + 1); }
static_assert(d6_acc_row_bits() == 0xffffffffu, "the 16 registers of the two lane halves are rows 0..31, each exactly once");
// one k-step of two: acc += A[:, 2s .. 2s + 1] B[2s .. 2s + 1, :]
__device__ __forceinline__ void d6_mfma(float a, float b, f32x16 &acc) { acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ void d6_acc_zero(f32x16 &acc) {
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
}

// raw buffer descriptor over the whole 32-bit offset range, or bounded (mlp_rows.hip's weights: reads past `bytes` return 0)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t d6_buffer(const void *p, unsigned bytes = 0xffffffff) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, bytes, 0x00020000);
}
// a wave's own LDS writes, visible to its own later reads: lgkmcnt(0) + the compiler-level wave barrier.  WAVE-PRIVATE LDS
// only: what another wave reads or writes needs __syncthreads().
__device__ __forceinline__ void d6_lds_wave_sync() { __builtin_amdgcn_s_waitcnt(0xC07F), __builtin_amdgcn_wave_barrier(); }
// The tile to memory through the buffer path (interior tiles: no bound predicate): voff = the lane's byte offset (its column,
// row 4 * kh), the row of every register as a scalar offset.  The local copy matters: __builtin_bit_cast straight on the vector
// ELEMENT stored element 0 sixteen times (seen in the ISA).
__device__ __forceinline__ void d6_acc_store_rows(const f32x16 &acc, __amdgpu_buffer_rsrc_t srd, uint32_t voff, int ld_bytes) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float v = acc[e];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), srd, voff, d6_acc_row(e) * ld_bytes, 0);
  }
}
// The tile as the row-major LDS image (odd row stride ld) the next layer's A fragments read; dst = the lane's column, row 4 * kh.
__device__ __forceinline__ void d6_acc_to_lds(const f32x16 &acc, float *dst, int ld) {
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[d6_acc_row(e) * ld] = acc[e];
}
// maximum over this lane's four rows of the 8-row bundle q (no NaN inputs: d6_vmax) ...
__device__ __forceinline__ float d6_acc_max4(const f32x16 &acc, int q) {
  return d6_vmax(d6_vmax(acc[4 * q], acc[4 * q + 1]), d6_vmax(acc[4 * q + 2], acc[4 * q + 3]));
}
// ... and the lane-half exchange that completes the bundle: max(v, v of lane ^ 32), the same value in both halves.  Two forms:
//  * d6_half_max: __shfl_xor = ds_bpermute, an LDS-queue instruction: no vector-ALU slot beside its address.  The chain and
//    group kernels and linear_kernel's general epilogue (and d6_compact_pool, compact_list.h) use it.
//  * d6_half_max_swap: one v_permlane32_swap (lo' = [lo.lanes 0-31 | hi.lanes 0-31], hi' = [lo.lanes 32-63 | hi.lanes 32-63])
//    + one v_max, nothing queued behind LDS traffic: linear_kernel's interior and compact pooled epilogues, which sit behind 45 %
//    of the GEMM time.  Inline asm: the compiler drops the SECOND result of __builtin_amdgcn_permlane32_swap, and asm gets no
//    hazard padding, hence the s_nop pair.
__device__ __forceinline__ float d6_half_max(float v) { return d6_vmax(v, __shfl_xor(v, 32)); }
__device__ __forceinline__ float d6_half_max_swap(float lo) {
  float hi = lo;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo), "+v"(hi));
  return d6_vmax(lo, hi);
}
