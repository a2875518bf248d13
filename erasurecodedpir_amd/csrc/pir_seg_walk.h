// pir_seg_walk.h -- internal, device only: the core of the transposed four-Russians fold, once,
// for k_scan_t (pir_scan_t.hip) and the segment kernels k_shamir_seg (pir_shamir_q.hip) and
// k_woodruff_seg (pir_woodruff_q.hip).  pir_scan_t.hip's header says why the fold has this form.
//
//   FrTab<WD>         the layout of a wave's nibble tables, WD = 1 or 2 coefficient words per row
//   fr_build_tables   a 64-row chunk's 16 tables from the lanes' coefficient words (DPP)
//   fr_walk           the loop: 64-row chunks, 8 rows per software-pipelined step, into Zt
//   planes_out        Zt back to planes and the fold by the alpha powers: one dword per slot
//   seg_walk, seg_store, seg_takes, kSegThreads / kSegWaves: what the two segment kernels share
//
// A segment is a run of shard rows whose coefficient depends only on the row's position in the
// run, with one output record: sum_r c_g[r] * row(r) for every slot g.  A wave owns one
// (segment, 64-dword column group) item: lane l folds dword `voff / 4` of every row.
// No workgroup barrier anywhere: waves of a workgroup may leave early or walk different lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pir_bits.h"
#include "pir_kernels.h"

namespace pir {

// Per wave: the 16 nibble tables of a 64-row chunk, table t (rows 4t .. 4t + 3) at t * kBytes,
// its 16 entries of 4 or 8 bytes (ds_read_b32 / ds_read_b64).  A table aligned to its own size
// gives every entry its own bank(s): any set of indices reads without a bank conflict.  The
// wave's kWords dwords of LDS are 128-byte aligned
template <int WD>
struct FrTab {
  static_assert(WD == 1 || WD == 2, "coefficient words of 32 or 64 bits");
  using Ent = typename std::conditional<WD == 2, uint2, uint32_t>::type;
  static constexpr int ESH = WD == 2 ? 3 : 2;  // log2 of the entry size
  static constexpr int kBytes = 16 << ESH;     // a table: 64 or 128
  static constexpr int kWords = 16 * kBytes / 4;
};

// The chunk's 16 nibble tables, built lane-parallel: lane l holds row l's words cw, table l >> 2
// covers the lane's own quad of rows, and the lane writes its entries 4 (l & 3) .. + 3 (row bits
// 2-3 = l & 3 fixed, row bits 0-1 counting): 16 or 32 contiguous bytes.  Rows past the last have
// zero words, so a ragged chunk needs nothing of its own.  q2 / q3 = all ones in the lanes with
// bit 0 / bit 1 set: the caller makes them once, not per chunk
template <int WD>
__device__ __forceinline__ void fr_build_tables(const uint2& cw, uint32_t q2, uint32_t q3,
                                                uint32_t lane, uint32_t* tw) {
  uint32_t e[4][WD];
#pragma unroll
  for (int d = 0; d < WD; ++d) {
    const int s = (int)(d ? cw.y : cw.x);
    const uint32_t w0 = (uint32_t)__builtin_amdgcn_update_dpp(0, s, 0x00, 0xf, 0xf, false);
    const uint32_t w1 = (uint32_t)__builtin_amdgcn_update_dpp(0, s, 0x55, 0xf, 0xf, false);
    const uint32_t w2 = (uint32_t)__builtin_amdgcn_update_dpp(0, s, 0xaa, 0xf, 0xf, false);
    const uint32_t w3 = (uint32_t)__builtin_amdgcn_update_dpp(0, s, 0xff, 0xf, 0xf, false);
    e[0][d] = (w2 & q2) ^ (w3 & q3);
    e[1][d] = e[0][d] ^ w0;
    e[2][d] = e[0][d] ^ w1;
    e[3][d] = e[1][d] ^ w1;
  }
  __builtin_amdgcn_wave_barrier();  // the previous chunk's reads are issued (LDS keeps its order)
  uint4* const dst = reinterpret_cast<uint4*>(tw) + lane * WD;
  if constexpr (WD == 2) {
    dst[0] = make_uint4(e[0][0], e[0][1], e[1][0], e[1][1]);
    dst[1] = make_uint4(e[2][0], e[2][1], e[3][0], e[3][1]);
  } else {
    dst[0] = make_uint4(e[0][0], e[1][0], e[2][0], e[3][0]);
  }
  __builtin_amdgcn_wave_barrier();  // the wave's own tables: no workgroup barrier
}

// The fold of a wave's nrows rows: Zt = the sums as 32 x WD words of bit planes (planes_out).
// The caller gives
//   load(rel)   the lane's dword of row rel; the walker asks only for rel < nrows, and for row 0
//               in place of the rows past the last (they have zero coefficient words)
//   coefs(rb)   lane l: the coefficient words of row rb + l, byte g = slot g's coefficient, zero
//               for rb + l >= nrows
//   first, next(cur)   the wave's 64-row chunks in the order it folds them: `first`, then
//               next(cur) after cur, until one is >= the chunk count (cur + 1, or chunks claimed
//               from a workgroup's counter).  The rows and coefficient words loaded ahead come
//               from the next chunk past the current one's end
//   tw          the wave's own FrTab<WD>::kWords dwords of LDS
// IMG: the rows come from a fold image (pir_bits.h: fold_image4; k_fold_image builds it).  The
// wave's first row is a multiple of 4, load(blk) returns the four image words of the rows 4 blk ..
// 4 blk + 3 -- asked for only with 4 blk < nrows, and for block 0 in place of the blocks past the
// last -- and the two transposes per group, with the shift of the even nibbles, are not done
template <int WD, bool IMG = false, class Load, class Coefs, class Next>
__device__ __forceinline__ void fr_walk(uint32_t nrows, Load&& load, Coefs&& coefs, uint32_t first,
                                        Next&& next, uint32_t lane, uint32_t* tw,
                                        uint32_t (&Zt)[32][WD]) {
  using Ent = typename FrTab<WD>::Ent;
  constexpr int ESH = FrTab<WD>::ESH, kTabBytes = FrTab<WD>::kBytes;
#pragma unroll
  for (int j = 0; j < 32; ++j)
#pragma unroll
    for (int d = 0; d < WD; ++d) Zt[j][d] = 0;
  const uint32_t q2 = (lane & 1u) ? 0xffffffffu : 0u, q3 = (lane & 2u) ? 0xffffffffu : 0u;
  const uint32_t nch = (nrows + 63) / 64;
  uint32_t cur = first;
  uint32_t nxt = next(cur);
  auto load_rel = [&](uint32_t rel) __attribute__((always_inline)) {
    return load(rel < nrows ? rel : 0u);
  };
  uint32_t x[16];
  // rows rel .. rel + n - 1 into x[u0 ..] (IMG: rel a multiple of 4 or >= nrows, n of 4)
  auto fetch = [&](int u0, int n, uint32_t rel) __attribute__((always_inline)) {
    if constexpr (IMG) {
#pragma unroll
      for (int u = 0; u < n; u += 4) {
        const uint4 b = load(rel + (uint32_t)u < nrows ? (rel + (uint32_t)u) / 4 : 0u);
        x[u0 + u] = b.x, x[u0 + u + 1] = b.y, x[u0 + u + 2] = b.z, x[u0 + u + 3] = b.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < n; ++u) x[u0 + u] = load_rel(rel + (uint32_t)u);
    }
  };
  fetch(0, 16, cur * 64);
  uint2 cw = coefs(cur * 64);  // zero by itself when the wave has no chunk (cur >= nch)
  for (; cur < nch;) {
    const uint32_t rb = cur * 64;
    const uint2 cwn = nxt < nch ? coefs(nxt * 64) : make_uint2(0, 0);  // next chunk's, in flight
    const uint32_t nb = nrows - rb < 64 ? nrows - rb : 64;
    if constexpr (IMG) {
      // the 16-byte loads take aligned register quads: the two masks are made again per chunk
      // (from a copy of the lane number the compiler cannot see through) and not kept
      uint32_t l = lane;
      asm volatile("" : "+v"(l));
      fr_build_tables<WD>(cw, 0u - (l & 1u), 0u - ((l >> 1) & 1u), l, tw);
    } else {
      fr_build_tables<WD>(cw, q2, q3, lane, tw);
    }
    for (uint32_t j0 = 0; j0 < nb; j0 += 16) {
      const char* const tj = reinterpret_cast<const char*>(tw) + j0 / 4 * kTabBytes;  // rows j0 ..
      // the 16 rows loaded ahead: this chunk's next, or past its end the next chunk's first
      const uint32_t ahead = j0 < 48 ? rb + j0 + 16 : (nxt < nch ? nxt * 64 : nrows);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        // ---- bit jj of rows 0-3 and of rows 4-7 -> two nibble indices; two lookups per bit
        // position.  Nibble i of L[k] / H[k] is the index of bit 4 i + k into the low / high
        // rows' table
        uint32_t (&L)[4] = *reinterpret_cast<uint32_t(*)[4]>(&x[8 * g]);  // in place
        uint32_t (&H)[4] = *reinterpret_cast<uint32_t(*)[4]>(&x[8 * g + 4]);
        if constexpr (!IMG) {
          transpose4x32(L);
          transpose4x32(H);
        }
        // 8 steps of 4 bit positions (8 lookups), software-pipelined: step s + 1's reads are
        // issued before step s's XORs (16 reads in flight; left alone the scheduler waits on
        // each read).  Step s takes the even (s even) or odd nibbles of the words L[s / 2],
        // H[s / 2] -- bit positions 8 b + 4 (s & 1) + s / 2 -- as entry byte offsets, one per
        // byte of a pre-shifted, pre-masked copy: a lookup's address is then one byte select
        // added to the table's.  (The copies are opaque to the compiler, which would shift and
        // mask the word again for every lookup; made per word, they stay out of the registers.)
        const char* const tg = tj + g * (2 * kTabBytes);
        Ent ta[8], tb[8];
        auto issue = [&](Ent (&t)[8], int s) __attribute__((always_inline)) {
          uint32_t lo, hi;
          if constexpr (IMG) {  // image words: rotated left by kFoldImageRot already
            constexpr int R = kFoldImageRot - ESH;
            static_assert(R >= 0, "the image's rotation covers the entry size");
            lo = __builtin_rotateright32(L[s >> 1], (s & 1) ? R + 4 : R);
            hi = __builtin_rotateright32(H[s >> 1], (s & 1) ? R + 4 : R);
          } else {
            lo = (s & 1) ? L[s >> 1] >> (4 - ESH) : L[s >> 1] << ESH;
            hi = (s & 1) ? H[s >> 1] >> (4 - ESH) : H[s >> 1] << ESH;
          }
          lo &= 0x0f0f0f0fu << ESH;
          hi &= 0x0f0f0f0fu << ESH;
          asm volatile("" : "+v"(lo), "+v"(hi));
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            t[2 * b] = *reinterpret_cast<const Ent*>(tg + ((lo >> (8 * b)) & 0xffu));
            t[2 * b + 1] = *reinterpret_cast<const Ent*>(tg + kTabBytes + ((hi >> (8 * b)) & 0xffu));
          }
          __builtin_amdgcn_sched_barrier(0);
        };
        auto fold = [&](const Ent (&t)[8], int s) __attribute__((always_inline)) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            uint32_t (&z)[WD] = Zt[8 * b + 4 * (s & 1) + (s >> 1)];
            if constexpr (WD == 2) {
              z[0] = __builtin_amdgcn_bitop3_b32(z[0], t[2 * b].x, t[2 * b + 1].x, 0x96);
              z[1] = __builtin_amdgcn_bitop3_b32(z[1], t[2 * b].y, t[2 * b + 1].y, 0x96);
            } else {
              z[0] = __builtin_amdgcn_bitop3_b32(z[0], t[2 * b], t[2 * b + 1], 0x96);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        };
        issue(ta, 0);
        issue(tb, 1);
        fold(ta, 0);
        issue(ta, 2);
        fold(tb, 1);
        issue(tb, 3);
        fold(ta, 2);
        issue(ta, 4);
        fold(tb, 3);
        issue(tb, 5);
        fold(ta, 4);
        issue(ta, 6);
        fold(tb, 5);
        issue(tb, 7);
        fold(ta, 6);
        fold(tb, 7);
        fetch(8 * g, 8, ahead + 8 * g);
        __builtin_amdgcn_sched_barrier(0);  // one group at a time (register pressure)
      }
    }
    cw = cwn;
    cur = nxt;
    nxt = next(cur);
  }
}

// back to planes and the fold by the powers of alpha: put(g, dword) for every slot g < NS, the
// dword being slot g's four sum bytes of this lane's column.  Words and slots at or above NS
// cost nothing
template <int WD, int NS, class Put>
__device__ __forceinline__ void planes_out(const uint32_t (&Zt)[32][WD], Put&& put) {
  static_assert(NS >= 1 && NS <= 4 * WD, "slots");
#pragma unroll
  for (int d = 0; d < WD; ++d) {
    if (4 * d >= NS) continue;
    uint32_t Y[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) Y[j] = Zt[j][d];
    transpose32(Y);  // Y[q]: plane 32 d + q = (slot 4 d + q / 8, bit q % 8)
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
      if (4 * d + a4 >= NS) continue;
      uint32_t acc = Y[8 * a4 + 7];
#pragma unroll
      for (int b = 6; b >= 0; --b) acc = gf_xtime4(acc) ^ Y[8 * a4 + b];
      put(4 * d + a4, acc);
    }
  }
}

// ---- the segment kernels: one wave per (segment, column group), 8 slots ----------------------
constexpr int kSegThreads = 256;
constexpr int kSegWaves = kSegThreads / 64;

// the segmented passes take records of at least one wave row (64 dwords)
inline bool seg_takes(uint32_t pitch) {
  return pitch % 4 == 0 && pitch / 4 >= (uint32_t)kColGroupLanes;
}

// The segment's nrows rows in order: row rel starts at base + row(rel), row(rel) a wave-uniform
// 64-bit byte offset, and the lane adds voff; kw[rel] is the row's coefficient word
template <class Row>
__device__ __forceinline__ void seg_walk(const uint8_t* base, Row&& row, uint32_t nrows,
                                         const uint2* kw, uint32_t voff, uint32_t lane,
                                         uint32_t* tw, uint32_t (&Zt)[32][2]) {
  fr_walk<2>(
      nrows,
      [&](uint32_t rel) __attribute__((always_inline)) {
        // the row's offset stays in scalar registers: the load takes the scalar base beside the
        // lane's 32-bit offset
        const uint64_t o = row(rel);
        const uint64_t os = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o) |
                            (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o >> 32)) << 32;
        return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(base + os + voff));
      },
      [&](uint32_t rb) __attribute__((always_inline)) {
        const uint32_t rl = rb + lane;
        return rl < nrows ? kw[rl] : make_uint2(0, 0);
      },
      0u, [](uint32_t cur) __attribute__((always_inline)) { return cur + 1; }, lane, tw, Zt);
}

// Where a lane's dwords go: `rec` = the lane's bytes [off, off + 4) of the segment's record in
// slot 0's response, slot g's resp_len * g further; `in` = the lane has bytes of the record
struct SegOut {
  uint8_t* rec;
  uint64_t resp_len;
  uint32_t off, efs;
  int ng, al4;
  bool in;
};

// slot g's dword into its response record: stored, or (XOR) XORed into what is there
template <bool XOR>
__device__ __forceinline__ void seg_store(const SegOut& O, int g, uint32_t acc) {
  if (!O.in || g >= O.ng) return;
  uint8_t* const o = O.rec + (uint64_t)g * O.resp_len;
  if (O.al4) {
    uint32_t* const w = reinterpret_cast<uint32_t*>(o);
    *w = XOR ? *w ^ acc : acc;
  } else {  // records of efs % 4 != 0, or an unaligned response: bytewise
    for (uint32_t u = 0; u < 4u && O.off + u < O.efs; ++u) {
      const uint8_t v = (uint8_t)(acc >> (8 * u));
      o[u] = XOR ? (uint8_t)(o[u] ^ v) : v;
    }
  }
}

}  // namespace pir
