// pir_update.hip -- live record updates: k_update_rows patches coded rows of the resident shard,
// and the fold image with them, in place.
//
// Every encoding of the shard is linear over GF(2^8) (k_encode_across, k_encode_within and its
// Hermite form), so a file that changes by delta = old ^ new changes a row by coef * delta: the
// host turns a batch of changed files into terms {row, delta, offset, coef} sorted by 4-row block
// (pir_update_plan.h).  One workgroup per touched block and column group of 256 dwords owns the
// block's four rows at its columns -- lane = one dword column, k_fold_image's mapping -- so that
// terms meeting in one row (across: files r, r + encdb, ...; one file twice) and rows meeting in
// one image block need no atomics: load the four dwords, XOR every term of the block into its
// row, store the changed rows, and store fold_image4 of the four new dwords over the image's 16
// bytes.  The image is a pure function of the block (pir_bits.h), so the patched image equals a
// rebuilt one.  The block's terms and their coefficients are wave-uniform: the multiply is
// gf_xtime4 over the coefficient's bits with uniform branches, as in k_encode_across.
#include <algorithm>

#include "pir_bits.h"
#include "pir_kernels.h"

namespace pir {

__device__ __forceinline__ uint32_t gf_mul_const1(uint32_t x, uint32_t c) {
  uint32_t acc = 0;
  for (int b = 0; b < 8; ++b) {
    if (c & (1u << b)) acc ^= x;
    x = gf_xtime4(x);
  }
  return acc;
}

// delta i at delta + i * dpitch; of a term's slice [off, off + efs) the bytes at or past `limit`
// (in the delta) count as zero and are not read, as the encoders' masks have it; the pad bytes
// of a row (at or past efs) are never changed.  Grid x = touched blocks (grid-stride), y =
// column groups of 256 dwords
__global__ __launch_bounds__(256) void k_update_rows(
    const UpdateBlock* __restrict__ blocks, uint32_t nblocks, const UpdateTerm* __restrict__ terms,
    const uint8_t* __restrict__ delta, uint64_t dpitch, uint32_t limit,
    uint8_t* __restrict__ shard, uint64_t nrows, uint32_t pitch, uint32_t efs,
    uint8_t* __restrict__ image) {
  const uint32_t col = blockIdx.y * 256 + threadIdx.x;
  if (col >= pitch / 4) return;
  const uint32_t b0 = 4 * col;  // the column's first byte of a row
  for (uint32_t bi = blockIdx.x; bi < nblocks; bi += gridDim.x) {
    const UpdateBlock B = blocks[bi];
    uint32_t x[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint64_t row = 4 * B.blk + r;
      x[r] = row < nrows ? *(reinterpret_cast<const uint32_t*>(shard + row * pitch) + col) : 0u;
    }
    uint32_t touched = 0;
    for (uint32_t t = B.t0; t < B.t1; ++t) {
      const UpdateTerm T = terms[t];
      // the slice's bytes that count: [0, end) of the row
      const uint32_t end = T.off < limit ? min(efs, limit - T.off) : 0u;
      const uint32_t nb = end > b0 ? min(4u, end - b0) : 0u;
      const uint8_t* p = delta + (uint64_t)T.delta * dpitch + T.off + b0;
      uint32_t v = 0;
      if (nb == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        v = *reinterpret_cast<const uint32_t*>(p);
      } else {
        for (uint32_t u = 0; u < nb; ++u) v |= (uint32_t)p[u] << (8 * u);
      }
      const uint32_t m = gf_mul_const1(v, T.coef & 0xffu);
      const uint32_t r = (uint32_t)T.row & 3u;
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] ^= r == (uint32_t)q ? m : 0u;
      touched |= 1u << r;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint64_t row = 4 * B.blk + r;
      if ((touched >> r & 1u) && row < nrows)
        *(reinterpret_cast<uint32_t*>(shard + row * pitch) + col) = x[r];
    }
    if (image) {
      fold_image4(x);
      *reinterpret_cast<uint4*>(image + B.blk * 4 * pitch + 16ull * col) =
          make_uint4(x[0], x[1], x[2], x[3]);
    }
  }
}

hipError_t launch_update_rows(const UpdateBlock* d_blocks, uint32_t nblocks,
                              const UpdateTerm* d_terms, const uint8_t* d_delta,
                              uint64_t delta_pitch, uint32_t limit, uint8_t* d_shard,
                              uint64_t nrows, uint32_t pitch, uint32_t efs, uint8_t* d_image,
                              hipStream_t s) {
  if (pitch % 16 != 0 || efs > pitch) return hipErrorInvalidValue;
  if (!nblocks) return hipSuccess;
  const dim3 grid(std::min<uint32_t>(nblocks, 1u << 16), (pitch / 4 + 255) / 256);
  hipLaunchKernelGGL(k_update_rows, grid, dim3(256), 0, s, d_blocks, nblocks, d_terms, d_delta,
                     delta_pitch, limit, d_shard, nrows, pitch, efs, d_image);
  return hipGetLastError();
}

// The delta of a CheckMAC record (payload || tag): out i = (old i ^ new i) over the payload
// bytes, then (tag of old i ^ tag of new i); tags: the num old tags, then the num new ones, 32
// bytes each.  One lane per byte
__global__ __launch_bounds__(256) void k_update_mac_delta(
    const uint8_t* __restrict__ d_old, const uint8_t* __restrict__ d_new, uint64_t pitch,
    const uint8_t* __restrict__ tags, uint64_t num, uint32_t payload, uint8_t* __restrict__ out) {
  const uint32_t efs = payload + 32u;
  for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < num * efs;
       idx += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = idx / efs;
    const uint32_t b = (uint32_t)(idx - i * efs);
    out[idx] = b < payload
                   ? (uint8_t)(d_old[i * pitch + b] ^ d_new[i * pitch + b])
                   : (uint8_t)(tags[i * 32 + (b - payload)] ^ tags[(num + i) * 32 + (b - payload)]);
  }
}

hipError_t launch_update_mac_delta(const uint8_t* d_old, const uint8_t* d_new, uint64_t pitch,
                                   const uint8_t* d_tags, uint64_t num, uint32_t payload,
                                   uint8_t* d_out, hipStream_t s) {
  if (!num) return hipSuccess;
  const uint64_t total = num * (payload + 32ull);
  const dim3 grid((unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 16));
  hipLaunchKernelGGL(k_update_mac_delta, grid, dim3(256), 0, s, d_old, d_new, pitch, d_tags, num,
                     payload, d_out);
  return hipGetLastError();
}

}  // namespace pir
