// pir_bits.h -- bit-matrix transposes of the transposed four-Russians scan (pir_seg_walk.h) and
// the packed GF(2^8) "times alpha" every bit-plane fold ends with.  Plain integer code, host and
// device (tests/test_bits_nibble.py and tests/test_bits_xtime.py check it on the CPU).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PIR_HD __host__ __device__ __forceinline__
#else
#define PIR_HD inline
#endif

namespace pir {

// 4 packed bytes times alpha in GF(2^8), poly 0x11d (coding.cpp:9-21): no carry crosses a byte
PIR_HD uint32_t gf_xtime4(uint32_t x) {
  return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du);
}

// swap the off-diagonal S x S blocks of rows a (block row 0) and b (block row 1): positions p
// with (p & S) == 0 are selected by m
template <int S>
PIR_HD void bit_swap(uint32_t& a, uint32_t& b, uint32_t m) {
  const uint32_t t = ((a >> S) ^ b) & m;
  b ^= t;
  a ^= t << S;
}

// 4 rows x 32 bits -> 32 nibbles: afterwards nibble i of x[k] holds bit (4i + k) of the original
// rows, row r in bit r (eight independent 4 x 4 transposes, one per nibble column: the 2-bit and
// 1-bit stages of transpose8x32)
PIR_HD void transpose4x32(uint32_t (&x)[4]) {
  bit_swap<2>(x[0], x[2], 0x33333333u); bit_swap<2>(x[1], x[3], 0x33333333u);
  bit_swap<1>(x[0], x[1], 0x55555555u); bit_swap<1>(x[2], x[3], 0x55555555u);
}

// The fold image (pir_scan_t.hip, k_fold_image): the shard's bits in the nibble-index form the
// transposed scan looks tables up by, made once per shard.  The four dwords of rows 4B .. 4B + 3
// at one dword column become four image words: transpose4x32, each word then rotated left by
// kFoldImageRot bits.  The nibble of bit position j = 4 i + k (bit r = row r's bit j) so sits in
// image word k at bits (4 i + kFoldImageRot .. + 3) mod 32: the even nibbles of a word, masked in
// place, are byte offsets of 8-byte table entries (no shift), the odd ones after one shift by 4.
constexpr int kFoldImageRot = 3;
PIR_HD uint32_t fold_image_rotl(uint32_t w, int s) { return (w << s) | (w >> (32 - s)); }
// rows -> image words, in place
PIR_HD void fold_image4(uint32_t (&x)[4]) {
  transpose4x32(x);
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = fold_image_rotl(x[k], kFoldImageRot);
}
// image words -> rows, in place (the rotation undone, then the transpose, its own inverse)
PIR_HD void fold_image4_rows(uint32_t (&x)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = fold_image_rotl(x[k], 32 - kFoldImageRot);
  transpose4x32(x);
}
// the nibble of bit position j (0 .. 31) in the image words w
PIR_HD uint32_t fold_image_nibble(const uint32_t (&w)[4], int j) {
  return (fold_image_rotl(w[j & 3], 32 - kFoldImageRot) >> (4 * (j >> 2))) & 0xfu;
}

// 8 rows x 32 bits -> 32 bytes: afterwards byte i of x[k] holds bit (8i + k) of the original
// rows, row r in bit r (four independent 8 x 8 transposes, one per byte column)
PIR_HD void transpose8x32(uint32_t (&x)[8]) {
  bit_swap<4>(x[0], x[4], 0x0F0F0F0Fu); bit_swap<4>(x[1], x[5], 0x0F0F0F0Fu);
  bit_swap<4>(x[2], x[6], 0x0F0F0F0Fu); bit_swap<4>(x[3], x[7], 0x0F0F0F0Fu);
  bit_swap<2>(x[0], x[2], 0x33333333u); bit_swap<2>(x[1], x[3], 0x33333333u);
  bit_swap<2>(x[4], x[6], 0x33333333u); bit_swap<2>(x[5], x[7], 0x33333333u);
  bit_swap<1>(x[0], x[1], 0x55555555u); bit_swap<1>(x[2], x[3], 0x55555555u);
  bit_swap<1>(x[4], x[5], 0x55555555u); bit_swap<1>(x[6], x[7], 0x55555555u);
}

// 32 x 32 bits in place: afterwards bit j of a[p] = bit p of the original a[j]
PIR_HD void transpose32(uint32_t (&a)[32]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) bit_swap<16>(a[k], a[k + 16], 0x0000FFFFu);
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (!(k & 8)) bit_swap<8>(a[k], a[k + 8], 0x00FF00FFu);
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (!(k & 4)) bit_swap<4>(a[k], a[k + 4], 0x0F0F0F0Fu);
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (!(k & 2)) bit_swap<2>(a[k], a[k + 2], 0x33333333u);
#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (!(k & 1)) bit_swap<1>(a[k], a[k + 1], 0x55555555u);
}

}  // namespace pir
