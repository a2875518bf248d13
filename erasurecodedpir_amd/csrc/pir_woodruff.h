// pir_woodruff.h -- internal: the Woodruff mode's pair-product scan (runWoodruffQueryThread,
// src/c/server.cpp:564-616, with WOODRUFF_D = 2).  Not part of the C ABI.
//
// The key is M bytes, M the smallest integer >= 3 with M (M - 1) / 2 >= N = 2^n
// (params.cpp:621-628).  Record i is the i-th pair (a, b), 0 <= a < b < M, in lexicographic order
// (makeCombi(M, 2) minus 1): row a of the triangle starts at start(a) = a (2M - a - 1) / 2 and
// b = a + 1 + i - start(a).  Pairs of rank >= N are unused.  The value answer over the records
// [lo, hi), all arithmetic in GF(2^8)/0x11d:
//     out = XOR_i key[a_i] * key[b_i] * row_i
// i.e. one coefficient byte per record in front of the one-round scan.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pir_bits.h"

namespace pir {

struct WdPair {
  uint32_t a, b;
};

// first record of triangle row a (a <= M - 1; start(M - 1) = the number of pairs)
__host__ __device__ inline uint64_t wd_start(uint32_t M, uint64_t a) {
  return a * (2ull * M - a - 1) / 2;
}

// The pair of record i < M (M - 1) / 2, exact for every i < 2^32 (M < 2^17): the closed form
// a = floor(((2M - 1) - sqrt((2M - 1)^2 - 8 i)) / 2) in double -- its argument, below 2^35, is
// exact, the root is not -- then a +-1 fix-up against start(a) in integers.
__host__ __device__ inline WdPair wd_pair(uint32_t M, uint64_t i) {
  const double t = 2.0 * M - 1.0;
  const double d = t * t - 8.0 * (double)i;
  int64_t a = (int64_t)((t - sqrt(d > 0.0 ? d : 0.0)) * 0.5);
  if (a < 0) a = 0;
  if (a > (int64_t)M - 2) a = (int64_t)M - 2;
  while (a > 0 && wd_start(M, (uint64_t)a) > i) --a;
  while (a < (int64_t)M - 2 && wd_start(M, (uint64_t)a + 1) <= i) ++a;
  WdPair p;
  p.a = (uint32_t)a;
  p.b = (uint32_t)(a + 1 + (int64_t)(i - wd_start(M, (uint64_t)a)));
  return p;
}

// the next record's pair
__host__ __device__ inline void wd_next(uint32_t M, WdPair& p) {
  ++p.b;
  if (p.b == M) {
    ++p.a;
    p.b = p.a + 1;
  }
}

// a * b in GF(2^8)/0x11d, branch-free shift-and-xor
__host__ __device__ inline uint32_t wd_gf_mul(uint32_t a, uint32_t b) {
  uint32_t m = 0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    m ^= a & (0u - ((b >> t) & 1u));
    a = ((a << 1) ^ ((0u - ((a >> 7) & 1u)) & 0x11du)) & 0xffu;
  }
  return m;
}

// four such products at once, one per byte lane of a and b (no carry crosses a lane)
__host__ __device__ inline uint32_t wd_gf_mul4(uint32_t a, uint32_t b) {
  uint32_t acc = 0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const uint32_t m = (b >> t) & 0x01010101u;
    acc ^= a & ((m << 8) - m);  // m * 0xff: the lanes whose bit t of b is set
    a = gf_xtime4(a);
  }
  return acc;
}

// calcWoodruffKeyLength / params.cpp:621-628 for N = 2^n records; 0 when n is outside [0, 31]
uint32_t wd_key_len(int n);

// d_c[(i - lo) * nrp] = key[a_i] * key[b_i] (bytes 1 .. nrp - 1 of a record zero) for the
// records [lo, hi): the record-major coefficients of the explicit-coefficient scan
hipError_t launch_woodruff_coefs(const uint8_t* d_key, uint32_t M, int nrp, uint64_t lo,
                                 uint64_t hi, uint8_t* d_c, hipStream_t s);

// The record-major shares of a group of ng <= W queued keys (d_keys: M bytes each, back to back,
// any alignment), W in {2, 4, 8} the scan's coefficient bytes per record: byte g of the W at
// d_c + (i - lo) * W is key_g[a_i] * key_g[b_i] for g < ng and 0 for g >= ng, for the records
// [lo, hi).  d_c is 16-byte aligned.  One walk of the pairs serves the group: the keys are
// interleaved into a table keyT[j] = key_0[j] .. key_{W-1}[j] and the W products of a record are
// one packed multiply (wd_gf_mul4).  The table lives in LDS where its W * M bytes fit
// (wd_key_table_in_lds), else in d_keyT: W * M bytes of scratch, 8-byte aligned, written by a
// transposing kernel in front ($PIR_WD_LDS=0 sends every shape that way: tests).
bool wd_key_table_in_lds(uint32_t M, int W);
hipError_t launch_woodruff_coefs_g(const uint8_t* d_keys, uint32_t M, int ng, int W, uint64_t lo,
                                   uint64_t hi, uint8_t* d_c, hipStream_t s,
                                   uint8_t* d_keyT = nullptr);

// The derivative answers (WOODRUFF_DERIVATIVE = 1, server.cpp:618-644) over the records
// [lo, hi) of `rows` (pitch bytes apart): M + 1 records of efs bytes at `out`, which the caller
// zeroed,
//     out[0]     = XOR_i key[a_i] * key[b_i] * row_i                 (the value answer)
//     out[1 + j] = XOR_{i : j in {a_i, b_i}} key[the other index] * row_i
// in two passes over the shard: k_woodruff_rows (out[1 + a] = XOR_b key[b] * row(a, b), the
// records of one a being contiguous), k_woodruff_totals (out[0] = XOR_a key[a] * out[1 + a]),
// then k_woodruff_cols (out[1 + b] ^= XOR_a key[a] * row(a, b)).
hipError_t launch_woodruff_deriv(const uint8_t* rows, uint32_t pitch, uint32_t efs,
                                 const uint8_t* d_key, uint32_t M, uint64_t lo, uint64_t hi,
                                 uint8_t* out, hipStream_t s);

// ---- queued derivative keys: up to kWdDerivSlots keys per pass (pir_woodruff_q.hip) ----------
constexpr int kWdDerivSlots = 8;
// the segmented pass takes records of at least one wave row (64 dwords)
bool woodruff_seg_takes(uint32_t pitch);
// d_keyT[j] (8-byte words, 8-byte aligned, M of them): byte g = key_g[j] for g < ng, zero above
// (d_keys: M bytes each, back to back, any alignment)
hipError_t launch_woodruff_key_table(const uint8_t* d_keys, uint32_t M, int ng, uint8_t* d_keyT,
                                     hipStream_t s);
// One derivative pass for the table's ng slots over the records [lo, hi): cols = false stores
// R[a] = XOR_b key[b] * row(a, b) into response record 1 + a of every triangle row the range
// touches, cols = true XORs C[b] = XOR_a key[a] * row(a, b) into record 1 + b; out = slot 0's
// response (slot g's is (M + 1) * efs * g further), which the caller zeroed before the rows pass.
// pair: a wave takes a long segment and then a short one (else: longest segments first).
hipError_t launch_woodruff_seg(const uint8_t* rows, uint32_t pitch, uint32_t efs,
                               const uint8_t* d_keyT, uint32_t M, int ng, uint64_t lo, uint64_t hi,
                               bool cols, bool pair, uint8_t* out, hipStream_t s);
// k_woodruff_totals alone: out[0] = XOR_a key[a] * out[1 + a] over the triangle rows the records
// [lo, hi) touch, from one key's finished rows pass
hipError_t launch_woodruff_totals(uint32_t efs, const uint8_t* d_key, uint32_t M, uint64_t lo,
                                  uint64_t hi, uint8_t* out, hipStream_t s);

}  // namespace pir
