// pir_seg_walk.h -- internal, device only: the transposed four-Russians fold of one *segment* for
// up to 8 key slots (pir_scan_t.hip's inner loop, with the coefficient words given per row).
//
// A segment is a run of shard rows whose coefficient depends only on the row's position in the
// run, with one output record: sum_r c_g[r] * row(r) for every slot g.  A wave owns one
// (segment, 64-dword column group) item: lane l folds dword `voff / 4` of every row.  The caller
// gives
//   base, row(rel)   row rel < nrows starts at base + row(rel), row(rel) a wave-uniform 64-bit
//              byte offset; the lane adds voff
//   kw[rel]    the row's coefficient word: byte g = slot g's coefficient
//   tw         the wave's own kSegTabWords dwords of LDS, 128-byte aligned
// and gets the sums as 64 bit planes in Zt, which seg_planes_out turns into one dword per slot.
// No workgroup barrier anywhere: waves of a workgroup may leave early or walk different lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pir_bits.h"

namespace pir {

constexpr int kSegTabBytes = 128;  // 16 entries of 8 bytes: aligned to its size, conflict free
constexpr int kSegTabWords = 16 * kSegTabBytes / 4;  // a chunk's 16 nibble tables

__device__ __forceinline__ uint32_t seg_xtime4(uint32_t x) {  // 4 packed bytes times alpha
  return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du);
}

template <class Row>
__device__ __forceinline__ void seg_walk(const uint8_t* base, Row&& row, uint32_t nrows,
                                         const uint2* kw, uint32_t voff, uint32_t lane,
                                         uint32_t* tw, uint32_t (&Zt)[32][2]) {
#pragma unroll
  for (int j = 0; j < 32; ++j) Zt[j][0] = Zt[j][1] = 0;

  // rows past the segment's last re-read its first and have zero coefficient words
  auto load_rel = [&](uint32_t rel) __attribute__((always_inline)) {
    // the row's offset stays in scalar registers: the load takes the scalar base beside the
    // lane's 32-bit offset
    const uint64_t o = row(rel < nrows ? rel : 0u);
    const uint64_t os = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o >> 32)) << 32;
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(base + os + voff));
  };
  auto coefs64 = [&](uint32_t r0) __attribute__((always_inline)) {
    const uint32_t rl = r0 + lane;
    uint2 cw = make_uint2(0, 0);
    if (rl < nrows) cw = kw[rl];
    return cw;
  };
  // the chunk's 16 nibble tables, built lane-parallel as in k_scan_t
  const uint32_t q2 = (lane & 1u) ? 0xffffffffu : 0u, q3 = (lane & 2u) ? 0xffffffffu : 0u;
  auto build_tables = [&](const uint2& cw) __attribute__((always_inline)) {
    uint32_t e[4][2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
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
    uint4* const dst = reinterpret_cast<uint4*>(tw) + lane * 2;
    dst[0] = make_uint4(e[0][0], e[0][1], e[1][0], e[1][1]);
    dst[1] = make_uint4(e[2][0], e[2][1], e[3][0], e[3][1]);
    __builtin_amdgcn_wave_barrier();  // the wave's own tables: no workgroup barrier
  };

  const uint32_t nch = (nrows + 63) / 64;
  uint32_t x[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) x[u] = load_rel((uint32_t)u);
  uint2 cw = coefs64(0);
  for (uint32_t cur = 0; cur < nch; ++cur) {
    const uint32_t r0 = cur * 64;
    const uint2 cwn = cur + 1 < nch ? coefs64(r0 + 64) : make_uint2(0, 0);  // in flight
    const uint32_t nb = nrows - r0 < 64 ? nrows - r0 : 64;
    build_tables(cw);
    for (uint32_t j0 = 0; j0 < nb; j0 += 16) {
      const char* const tj = reinterpret_cast<const char*>(tw) + j0 / 4 * kSegTabBytes;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const uint32_t j = r0 + j0 + 8 * g;
        uint32_t (&L)[4] = *reinterpret_cast<uint32_t(*)[4]>(&x[8 * g]);  // in place
        uint32_t (&H)[4] = *reinterpret_cast<uint32_t(*)[4]>(&x[8 * g + 4]);
        transpose4x32(L);
        transpose4x32(H);
        // k_scan_t's 8 software-pipelined steps of 4 bit positions: step s takes the even or odd
        // nibbles of L[s / 2], H[s / 2] as entry byte offsets
        const char* const tg = tj + g * (2 * kSegTabBytes);
        uint2 ta[8], tb[8];
        auto issue = [&](uint2 (&t)[8], int s) __attribute__((always_inline)) {
          uint32_t lo = (s & 1) ? L[s >> 1] >> 1 : L[s >> 1] << 3;
          uint32_t hi = (s & 1) ? H[s >> 1] >> 1 : H[s >> 1] << 3;
          lo &= 0x0f0f0f0fu << 3;
          hi &= 0x0f0f0f0fu << 3;
          asm volatile("" : "+v"(lo), "+v"(hi));
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            t[2 * b] = *reinterpret_cast<const uint2*>(tg + ((lo >> (8 * b)) & 0xffu));
            t[2 * b + 1] =
                *reinterpret_cast<const uint2*>(tg + kSegTabBytes + ((hi >> (8 * b)) & 0xffu));
          }
          __builtin_amdgcn_sched_barrier(0);
        };
        auto fold = [&](const uint2 (&t)[8], int s) __attribute__((always_inline)) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            uint32_t (&z)[2] = Zt[8 * b + 4 * (s & 1) + (s >> 1)];
            z[0] = __builtin_amdgcn_bitop3_b32(z[0], t[2 * b].x, t[2 * b + 1].x, 0x96);
            z[1] = __builtin_amdgcn_bitop3_b32(z[1], t[2 * b].y, t[2 * b + 1].y, 0x96);
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
#pragma unroll
        for (int r = 0; r < 8; ++r) x[8 * g + r] = load_rel(j + 16 + r);
        __builtin_amdgcn_sched_barrier(0);  // one group at a time (register pressure)
      }
    }
    cw = cwn;
  }
}

// back to planes and the fold by the powers of alpha: put(g, dword) for every slot g < 8, the
// dword being slot g's four sum bytes of this lane's column
template <class Put>
__device__ __forceinline__ void seg_planes_out(const uint32_t (&Zt)[32][2], Put&& put) {
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    uint32_t Y[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) Y[j] = Zt[j][d];
    transpose32(Y);  // Y[q]: plane 32 d + q = (slot 4 d + q / 8, bit q % 8)
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
      uint32_t acc = Y[8 * a4 + 7];
#pragma unroll
      for (int b = 6; b >= 0; --b) acc = seg_xtime4(acc) ^ Y[8 * a4 + b];
      put(4 * d + a4, acc);
    }
  }
}

}  // namespace pir
