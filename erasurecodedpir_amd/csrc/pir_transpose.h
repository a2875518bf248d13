// pir_transpose.h -- internal: the byte transpose between share vectors and record-major share
// rows, in registers.  W vectors of 16 bytes (vector b = share byte b of 16 consecutive records)
// become the 16 W bytes the GF(2^8) scans read for those records (record k at bytes [k W,
// (k + 1) W)), as W 16-byte words.  v_perm_b32 only, every index a compile-time constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pir {

__device__ __forceinline__ uint32_t tr_word(uint4 v, int q) {
  return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
}
__device__ __forceinline__ uint32_t tr_byte(uint4 v, int k) {
  return (tr_word(v, k >> 2) >> (8 * (k & 3))) & 0xffu;
}

// t[k] = byte k of a0, a1, a2, a3 (a 4 x 4 byte transpose)
__device__ __forceinline__ void tr4x4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3,
                                      uint32_t (&t)[4]) {
  const uint32_t l01 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);
  const uint32_t h01 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
  const uint32_t l23 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
  const uint32_t h23 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
  t[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u);
  t[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
  t[2] = __builtin_amdgcn_perm(h23, h01, 0x05040100u);
  t[3] = __builtin_amdgcn_perm(h23, h01, 0x07060302u);
}

template <int W>
__device__ __forceinline__ void tr_records(const uint4 (&v)[W], uint4 (&o)[W]) {
  static_assert(W == 1 || W == 2 || W == 4 || W == 8, "share row of 1, 2, 4 or 8 bytes");
  if constexpr (W == 1) {
    o[0] = v[0];
  } else if constexpr (W == 2) {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t x = tr_word(v[0], q), y = tr_word(v[1], q);
      w[2 * q] = __builtin_amdgcn_perm(y, x, 0x05010400u);
      w[2 * q + 1] = __builtin_amdgcn_perm(y, x, 0x07030602u);
    }
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  } else if constexpr (W == 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t t[4];
      tr4x4(tr_word(v[0], q), tr_word(v[1], q), tr_word(v[2], q), tr_word(v[3], q), t);
      o[q] = make_uint4(t[0], t[1], t[2], t[3]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // records 4q .. 4q + 3: bytes 0-3 from v[0..3], 4-7 from v[4..7]
      uint32_t t0[4], t1[4];
      tr4x4(tr_word(v[0], q), tr_word(v[1], q), tr_word(v[2], q), tr_word(v[3], q), t0);
      tr4x4(tr_word(v[4], q), tr_word(v[5], q), tr_word(v[6], q), tr_word(v[7], q), t1);
      o[2 * q] = make_uint4(t0[0], t1[0], t0[1], t1[1]);
      o[2 * q + 1] = make_uint4(t0[2], t1[2], t0[3], t1[3]);
    }
  }
}

}  // namespace pir
