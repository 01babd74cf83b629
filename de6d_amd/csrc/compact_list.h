// compact_list.h — the compact (ragged) row list as code: ONE statement of the layout compact.hip builds and every
// grouped-MLP kernel consumes (linear.hip, expand.hip, mlp_chain.hip, mlp_group.hip), the helpers a consumer's pooling
// epilogue needs, and the rule that cuts a centre's rows into power-of-two parts, which compact.hip shares with the
// ball-query kernel that counts the parts of its own 256 centres while it still holds their hit counts
// (ball_query_grid.hip).  Why the list exists: compact.hip; the public description: include/det6d_ops.h.
//
// Row space: centres are binned by class s in {32, 16, 8, 4, 2, 1} (class index c <-> s = 32 >> c); each class owns one
// contiguous region of rows, the classes in descending s, every region padded to a multiple of 128 rows (a GEMM row tile,
// and so every 32-row tile, holds a single class), centres in ascending order inside a region.
//   hdr[kCompactHdr...]  the header words below; the per-block count table of the builder follows at kCompactHdrTable
//   crow_p[r]            global point row (scene * n + neighbour index) row r gathers
//   crow_c[r]            the row's tag: centre (scene * m + j) in bits 0..28 (kCompactTagCentre),
//                        bit 29 (kCompactTagSplit): the centre's rows are cut into several parts, whose pooled values are
//                          combined by an integer atomic max on the non-negative post-ReLU values (buffer zeroed first),
//                        bit 30 (kCompactTagEmpty): empty ball, pooled value 0 (pointnet2_modules.py:465-467),
//                        -1 on alignment rows (computed, never stored)
#pragma once
#include "common.h"

constexpr int kCompactClasses = 6;

// header words
constexpr int kCompactHdrLive = 0;        // live rows (multiple of 128): the consumers read their row count HERE, on the device
constexpr int kCompactHdrClassEnd = 1;    // [1 + c]: end of the region of class c, c = 0..5; the last one equals the live rows
constexpr int kCompactHdrCentres = 7;     // centres the list was built from
constexpr int kCompactHdrInfoRows = 8;    // sum of min(cnt, ns): rows that carry information
constexpr int kCompactHdrUnaligned = 9;   // rows before the 128-row alignment
constexpr int kCompactHdrTicket = 10;     // tile ticket of the persistent group kernels (mlp_group.hip: g_draw_ticket) ...
constexpr int kCompactHdrExit = 11;       // ... and their exit counter, the word after it; both zero between launches
constexpr int kCompactHdrTable = 16;      // per block of 256 centres: parts per class [0..5], information rows [6]

// tag bits of crow_c
constexpr int kCompactTagCentre = 0x1fffffff;
constexpr int kCompactTagSplit = 0x20000000;
constexpr int kCompactTagEmpty = 0x40000000;

__device__ __forceinline__ int d6_compact_centre(int tag) { return tag & kCompactTagCentre; }
__device__ __forceinline__ bool d6_compact_is_split(int tag) { return tag & kCompactTagSplit; }
__device__ __forceinline__ bool d6_compact_is_empty(int tag) { return tag & kCompactTagEmpty; }

// ---- consumers: a 32-row tile (32 x 32 MFMA accumulator: a lane in half kh holds rows 8*qq + 4*kh + (0..3), qq = 0..3) ----

// the ends of the regions of classes 32, 16, 8, 4, 2 (the region of class 1 ends with the live rows)
__device__ __forceinline__ void d6_compact_class_ends(const int *hdr, int &h1, int &h2, int &h3, int &h4, int &h5) {
  const int *e = hdr + kCompactHdrClassEnd;
  h1 = e[0]; h2 = e[1]; h3 = e[2]; h4 = e[3]; h5 = e[4];
}
// class (= pooling width) of the 32-row tile starting at row0, from those ends
__device__ __forceinline__ int d6_compact_class(int row0, int h1, int h2, int h3, int h4, int h5) {
  return row0 < h1 ? 32 : row0 < h2 ? 16 : row0 < h3 ? 8 : row0 < h4 ? 4 : row0 < h5 ? 2 : 1;
}
// row (inside a 32-row tile) whose centre owns pooled value qq of a lane in half kh, -1: another lane writes it.
// Class 4 groups end inside the lane, wider groups after the lane^32 exchange; classes 1 and 2 have no pooled slot (every
// accumulator, or pair, is a group of its own and is stored at once).
__device__ __forceinline__ int d6_compact_out_row(int s, int qq, int kh) {
  if (s < 4) return -1;
  if (s == 4) return 8 * qq + 4 * kh;
  if (kh) return -1;
  if (s == 8) return 8 * qq;
  if (s == 16) return (qq & 1) ? -1 : 8 * qq;
  return qq == 0 ? 0 : -1;
}
// the four 4-row maxima of a lane -> pooled values of class s >= 4 (in place; v[qq] valid where d6_compact_out_row >= 0)
__device__ __forceinline__ void d6_compact_pool(float (&v)[4], int s) {
  if (s == 4) return;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) v[qq] = d6_vmax(v[qq], __shfl_xor(v[qq], 32));
  if (s == 16) {
    v[0] = d6_vmax(v[0], v[1]);
    v[2] = d6_vmax(v[2], v[3]);
  } else if (s == 32) {
    v[0] = d6_vmax(d6_vmax(v[0], v[1]), d6_vmax(v[2], v[3]));
  }
}
// pooled value of one part of a centre: plain store, or (split centres) integer atomic max into the zeroed buffer
__device__ __forceinline__ void d6_compact_store(float *dst, float val, int tag) {
  if (d6_compact_is_split(tag)) __hip_atomic_fetch_max(reinterpret_cast<int *>(dst), __builtin_bit_cast(int, val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *dst = val;
}

// ---- producers: the parts of a centre ----

// classes (bit c <-> s = 32 >> c) the rows of a centre with `cnt` hits are placed in.
//   split = 0: one part, the next power of two >= max(cnt, smin);
//   split = g > 0: up to g hits the same single part; beyond, ceil(cnt / g) * g rows, cut along their binary digits
//              into parts of descending size (20 rows = 16 + 4: slots 0..15 form a class-16 group, slots 16..19 a
//              class-4 group); the pooled value of the centre is the maximum over its parts (kCompactTagSplit).
//              smin = 1, g = 4: singles and pairs are rows of their own, no atomics for them.
__device__ __forceinline__ int d6_compact_parts_of(int cnt, int ns, int smin, int split_tol, int *rows_out) {
  const int k = cnt < 1 ? 1 : (cnt > ns ? ns : cnt);
  const int split = split_tol & 0xff, tol = split_tol >> 8;   // tol t > 0: one power-of-two part when it wastes <= 1/t of its rows
  int p2 = smin;
  while (p2 < k) p2 <<= 1;
  int rows;
  if (split > 0 && k > split && !(tol > 0 && (p2 - k) * tol <= p2)) {
    rows = (k + split - 1) / split * split;
  } else {
    rows = p2;
  }
  *rows_out = rows;
  int mask = 0;
#pragma unroll
  for (int c = 0; c < kCompactClasses; ++c)
    if (rows & (32 >> c)) mask |= 1 << c;
  return mask;
}

// what the list builder needs from whoever counts: per block of 256 centres, parts per class [0..5] and information rows [6]
// -> table[block * 7 + c], table = hdr + kCompactHdrTable (compact.hip: compact_place_kernel reads it)
struct CompactCountArgs {
  int ns, smin, split;
  int *table;                // nullptr: no counting
};

// host side (compact.hip): validates one group's (ns, smin, split) and clamps split to ns; DET6D_OK or DET6D_EINVAL
int det6d_compact_check_group(int ns, int smin, int *split);
// split with the experiments build's DET6D_COMPACT_TOL folded in (bits 8..): what the kernels' parts_of() takes
int det6d_compact_split_tol(int split);
