// pir_mac.hip -- k_hmac_sha256_files: the reference's CheckMAC record tags on the GPU.
//
// Every record of a CheckMAC database carries HMAC-SHA256(key[16], payload) behind its payload
// (client.cpp:29-31, utils.cpp:32-34).  One lane per file: the lane walks its own row in
// 64-byte SHA-256 blocks.  payload_bytes is the same for every file, so the block count, the
// padding and every branch below are wave-uniform; the 16-word message window is indexed by
// unrolled constants only (registers, no scratch) and the round constants are read through
// uniform addresses (scalar loads).  The states after the (key ^ ipad) and (key ^ opad) blocks
// do not depend on the file: the host computes them once and passes them by value.
#include <string.h>

#include "pir_mac.h"

namespace pir {
namespace {

#define PIR_SHA256_K                                                                              \
  0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, \
  0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, \
  0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, \
  0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, \
  0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, \
  0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, \
  0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, \
  0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2

__constant__ uint32_t kSha256KDev[64] = {PIR_SHA256_K};
const uint32_t kSha256KHost[64] = {PIR_SHA256_K};
const uint32_t kSha256Init[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

__host__ __device__ __forceinline__ uint32_t rotr(uint32_t x, int r) {
  return (x >> r) | (x << (32 - r));
}

// one SHA-256 round; i is an unrolled constant, so v[(j - i) & 7] names a register
#define PIR_SHA256_ROUND(i, kw)                                                                  \
  {                                                                                              \
    const uint32_t e_ = v[(4 - (i)) & 7], a_ = v[(0 - (i)) & 7];                                 \
    const uint32_t t1_ = v[(7 - (i)) & 7] + (rotr(e_, 6) ^ rotr(e_, 11) ^ rotr(e_, 25)) +        \
                         ((e_ & v[(5 - (i)) & 7]) ^ (~e_ & v[(6 - (i)) & 7])) + (kw);            \
    const uint32_t t2_ = (rotr(a_, 2) ^ rotr(a_, 13) ^ rotr(a_, 22)) +                           \
                         ((a_ & v[(1 - (i)) & 7]) ^ (a_ & v[(2 - (i)) & 7]) ^                    \
                          (v[(1 - (i)) & 7] & v[(2 - (i)) & 7]));                                \
    v[(3 - (i)) & 7] += t1_;                                                                     \
    v[(7 - (i)) & 7] = t1_ + t2_;                                                                \
  }

// h <- compress(h, w); w (the 16 big-endian message words) is used as the rolling window
__host__ __device__ __forceinline__ void sha256_compress(uint32_t h[8], uint32_t w[16],
                                                         const uint32_t* __restrict__ K) {
  uint32_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = h[j];
#pragma unroll
  for (int i = 0; i < 16; ++i) PIR_SHA256_ROUND(i, K[i] + w[i])
#pragma unroll 1
  for (int g = 16; g < 64; g += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
      w[i] += (rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] +
              (rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10));
      PIR_SHA256_ROUND(i, K[g + i] + w[i])
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] += v[j];
}

__device__ __forceinline__ uint32_t be_bytes(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// ld_align / st_align: 16, 4 or 1 -- what the base and pitch of the rows / of the tags allow
__global__ __launch_bounds__(256) void k_hmac_sha256_files(const uint8_t* files, uint64_t fpitch,
                                                           uint64_t nfiles, uint32_t payload,
                                                           HmacStates st, uint8_t* tags,
                                                           uint64_t tpitch, uint32_t ld_align,
                                                           uint32_t st_align) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nfiles) return;
  const uint8_t* row = files + f * fpitch;
  // the inner message is 64 (ipad block, already in st.inner) + payload bytes; 0x80, zeros and
  // the 8-byte bit length close its last block
  const uint32_t nb = (uint32_t)(((uint64_t)payload + 9 + 63) / 64);
  const uint64_t bits = (64ull + payload) * 8;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = st.inner[j];
#pragma unroll 1
  for (uint32_t b = 0; b <= nb; ++b) {
    const uint64_t off = (uint64_t)b * 64;
    uint32_t w[16];
    if (b == nb) {  // the outer hash: opad state, then the 32-byte inner digest as one block
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w[j] = h[j];
        h[j] = st.outer[j];
      }
      w[8] = 0x80000000u;
#pragma unroll
      for (int j = 9; j < 15; ++j) w[j] = 0;
      w[15] = (64 + 32) * 8;
    } else if (off + 64 <= payload) {  // a whole block of payload
      if (ld_align == 16) {
        const uint4* q = reinterpret_cast<const uint4*>(row + off);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint4 x = q[t];
          w[4 * t] = __builtin_bswap32(x.x);
          w[4 * t + 1] = __builtin_bswap32(x.y);
          w[4 * t + 2] = __builtin_bswap32(x.z);
          w[4 * t + 3] = __builtin_bswap32(x.w);
        }
      } else if (ld_align == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(row + off);
#pragma unroll
        for (int t = 0; t < 16; ++t) w[t] = __builtin_bswap32(q[t]);
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) w[t] = be_bytes(row + off + 4 * t);
      }
    } else {  // the payload's end, the padding, the length: nothing at or past `payload` is read
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const uint64_t p = off + 4 * t;
        uint32_t x = 0;
        if (p + 4 <= payload) {
          x = ld_align >= 4 ? __builtin_bswap32(*reinterpret_cast<const uint32_t*>(row + p))
                            : be_bytes(row + p);
        } else if (p <= payload) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint32_t c = p + u < payload ? row[p + u] : (p + u == payload ? 0x80u : 0u);
            x |= c << (24 - 8 * u);
          }
        }
        w[t] = x;
      }
      if (b == nb - 1) {
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
      }
    }
    sha256_compress(h, w, kSha256KDev);
  }
  uint8_t* tag = tags + f * tpitch;
  if (st_align == 16) {
    uint4* q = reinterpret_cast<uint4*>(tag);
    q[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]),
                      __builtin_bswap32(h[3]));
    q[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]),
                      __builtin_bswap32(h[7]));
  } else if (st_align == 4) {
#pragma unroll
    for (int j = 0; j < 8; ++j) reinterpret_cast<uint32_t*>(tag)[j] = __builtin_bswap32(h[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 32; ++j) tag[j] = (uint8_t)(h[j >> 2] >> (24 - 8 * (j & 3)));
  }
}

void load_block_host(const uint8_t* p, uint32_t w[16]) {
  for (int t = 0; t < 16; ++t)
    w[t] = (uint32_t)p[4 * t] << 24 | (uint32_t)p[4 * t + 1] << 16 | (uint32_t)p[4 * t + 2] << 8 |
           p[4 * t + 3];
}

uint32_t align_of(uint64_t base, uint64_t pitch) {
  const uint64_t m = base | pitch;
  return (m & 15) == 0 ? 16 : ((m & 3) == 0 ? 4 : 1);
}

}  // namespace

HmacStates hmac_states(const uint8_t key[16]) {
  HmacStates st;
  for (int pass = 0; pass < 2; ++pass) {
    uint8_t blk[64];
    memset(blk, pass ? 0x5c : 0x36, 64);
    for (int i = 0; i < 16; ++i) blk[i] ^= key[i];
    uint32_t w[16], *h = pass ? st.outer : st.inner;
    memcpy(h, kSha256Init, sizeof kSha256Init);
    load_block_host(blk, w);
    sha256_compress(h, w, kSha256KHost);
  }
  return st;
}

void hmac_sha256_host(const HmacStates& st, const uint8_t* msg, size_t len, uint8_t out[32]) {
  uint32_t h[8], w[16];
  memcpy(h, st.inner, sizeof h);
  size_t off = 0;
  for (; off + 64 <= len; off += 64) {
    load_block_host(msg + off, w);
    sha256_compress(h, w, kSha256KHost);
  }
  uint8_t tail[128] = {0};
  const size_t rem = len - off, tl = rem + 9 <= 64 ? 64 : 128;
  if (rem) memcpy(tail, msg + off, rem);
  tail[rem] = 0x80;
  const uint64_t bits = (64ull + len) * 8;
  for (int i = 0; i < 8; ++i) tail[tl - 1 - i] = (uint8_t)(bits >> (8 * i));
  for (size_t o = 0; o < tl; o += 64) {
    load_block_host(tail + o, w);
    sha256_compress(h, w, kSha256KHost);
  }
  for (int j = 0; j < 8; ++j) w[j] = h[j];
  w[8] = 0x80000000u;
  for (int j = 9; j < 15; ++j) w[j] = 0;
  w[15] = (64 + 32) * 8;
  memcpy(h, st.outer, sizeof h);
  sha256_compress(h, w, kSha256KHost);
  for (int j = 0; j < 32; ++j) out[j] = (uint8_t)(h[j >> 2] >> (24 - 8 * (j & 3)));
}

hipError_t launch_hmac_sha256_files(const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                                    uint32_t payload_bytes, const HmacStates& st, uint8_t* d_tags,
                                    uint64_t tag_pitch, hipStream_t s) {
  if (!num_files) return hipSuccess;
  const uint64_t blocks = (num_files + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_hmac_sha256_files, dim3((uint32_t)blocks), dim3(256), 0, s, d_files,
                     file_pitch, num_files, payload_bytes, st, d_tags, tag_pitch,
                     align_of((uint64_t)(uintptr_t)d_files, file_pitch),
                     align_of((uint64_t)(uintptr_t)d_tags, tag_pitch));
  return hipGetLastError();
}

}  // namespace pir
