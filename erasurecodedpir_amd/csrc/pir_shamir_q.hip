// pir_shamir_q.hip -- queued Shamir sqrt(N) keys that share shard passes (pir_shamir.h).
//
// Rx and Ry are one computation seen from two sides: a GF(2^8) matrix-vector product in which a
// record's coefficient depends only on its position inside a *segment* and every segment has one
// output record.  For Rx the segment is a matrix row delta (records `pitch` apart, coefficient
// kx[gamma]); for Ry it is a column gamma (records `pitch << y` apart, coefficient ky[delta]).
// Up to 8 virtual keys (the rounds of the queued keys) go through a pass together:
//   k_shamir_key_table  kT[j] = the 8 keys' byte j as one 64-bit word (slot g = byte g, absent
//                       slots zero): kyT = kT[0, X), kxT = kT[X, X + Y)
//   k_shamir_seg        one wave per (segment, 64-dword column group): the transposed
//                       four-Russians fold over the segment's rows (the index from the shard's
//                       bits, the nibble tables from the coefficient words; the cost per row does
//                       not depend on the number of planes), the per-segment sums stored straight
//                       into each virtual key's response record.  No slabs, no k_reduce.  The
//                       fold, the way back to planes and the store are pir_seg_walk.h's seg_walk,
//                       planes_out and seg_store; the kernel itself is the segment's geometry.
//   k_shamir_coefs_g    the Hermite scan's record-major share rows c[i] = kxT[gamma_i] *
//                       kyT[delta_i], byte-wise (two wd_gf_mul4)
#include "pir_kernels.h"
#include "pir_seg_walk.h"
#include "pir_shamir.h"
#include "pir_woodruff.h"

#include <algorithm>

namespace pir {

bool shamir_seg_takes(uint32_t pitch) { return seg_takes(pitch); }

namespace {

__global__ __launch_bounds__(256) void k_shamir_key_table(const uint8_t* __restrict__ keys,
                                                          uint64_t key_pitch, uint64_t key_stride,
                                                          int rounds, int v0, int ng, uint64_t klen,
                                                          uint2* __restrict__ kT) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= klen) return;
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int g = 0; g < kShamirSlots; ++g) {
    if (g < ng) {
      const int v = v0 + g;  // virtual key v = round v % rounds of key v / rounds
      const uint8_t* k = keys + (uint64_t)(v / rounds) * key_stride + (uint64_t)(v % rounds) * key_pitch;
      w[g >> 2] |= (uint32_t)k[j] << (8 * (g & 3));
    }
  }
  kT[j] = make_uint2(w[0], w[1]);
}

struct SegArgs {
  const uint8_t* vals;  // the value rows
  const uint2* kT;      // the coefficient words of a segment's rows: kT[r]
  uint8_t* out;         // slot g's response at out + g * resp_len
  uint64_t resp_len, lo, hi;
  uint64_t seg0, nseg;  // the segments launched: [seg0, seg0 + nseg)
  uint64_t rec_base;    // segment s writes response record rec_base + s
  uint32_t pitch, efs, ndw, ncg;  // dwords per row, column groups per row
  int y, ng, al4;
};

// STRIDED = false: segment = delta, rows r = gamma at (delta << y) + r, `pitch` apart.
// STRIDED = true:  segment = gamma, rows r = delta at (r << y) + gamma, `pitch << y` apart.
// Rows outside [lo, hi) are not walked (a zero word); a segment with none stores nothing (the
// response was zeroed).  Row addresses: a 64-bit wave-uniform base + a 32-bit lane offset.
template <bool STRIDED>
__global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(kScanTWavesPerEU)))
void k_shamir_seg(SegArgs A) {
  __shared__ alignas(128) uint32_t tab[kSegWaves][FrTab<2>::kWords];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t item = (uint64_t)blockIdx.x * kSegWaves + wv;
  if (item >= A.nseg * A.ncg) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint64_t seg = A.seg0 + item / A.ncg;
  const uint32_t cg = (uint32_t)(item % A.ncg);
  const uint32_t dw = cg * kColGroupLanes + lane;
  const bool active = dw < A.ndw;
  const uint64_t Ym = (1ull << A.y) - 1;
  uint64_t ra, rb, stride;
  const uint8_t* base;
  if constexpr (STRIDED) {
    ra = A.lo > seg ? (A.lo - seg + Ym) >> A.y : 0;
    rb = A.hi > seg ? (A.hi - seg + Ym) >> A.y : 0;
    stride = (uint64_t)A.pitch << A.y;
    base = A.vals + seg * A.pitch;
  } else {
    const uint64_t i0 = seg << A.y;
    ra = A.lo > i0 ? A.lo - i0 : 0;
    rb = A.hi > i0 ? (A.hi - i0 < Ym + 1 ? A.hi - i0 : Ym + 1) : 0;
    stride = A.pitch;
    base = A.vals + i0 * A.pitch;
  }
  if (ra >= rb) return;
  const uint32_t nrows = (uint32_t)(rb - ra);
  const uint8_t* const p0 = base + ra * stride;
  const uint32_t voff = (active ? dw : 0u) * 4u;  // inactive lanes: the row's first dword
  const uint2* const kw = A.kT + ra;
  uint32_t Zt[32][2];
  seg_walk(
      p0, [&](uint32_t rel) __attribute__((always_inline)) { return (uint64_t)rel * stride; },
      nrows, kw, voff, lane, &tab[wv][0], Zt);

  // back to planes, the fold by the powers of alpha, and each slot's dword into its response
  const uint32_t off = dw * 4u;
  const SegOut O{A.out + (A.rec_base + seg) * A.efs + off, A.resp_len, off, A.efs, A.ng, A.al4,
                 active && off < A.efs};
  planes_out<2, 8>(Zt, [&](int g, uint32_t acc) __attribute__((always_inline)) {
    seg_store<false>(O, g, acc);
  });
}

// two records per thread: one 16-byte store, the range's last odd record on its own
__global__ __launch_bounds__(256) void k_shamir_coefs_g(const uint2* __restrict__ kT, uint64_t X,
                                                        int y, uint64_t lo, uint64_t hi,
                                                        uint8_t* __restrict__ dst) {
  const uint64_t Ym = (1ull << y) - 1;
  const uint2* const kyT = kT;
  const uint2* const kxT = kT + X;
  const uint64_t npairs = (hi - lo + 1) / 2;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < npairs;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = lo + 2 * t;
    const uint2 a0 = kxT[i & Ym], b0 = kyT[i >> y];
    const uint32_t c0 = wd_gf_mul4(a0.x, b0.x), c1 = wd_gf_mul4(a0.y, b0.y);
    uint8_t* const d = dst + 16 * t;
    if (i + 1 < hi) {
      const uint2 a1 = kxT[(i + 1) & Ym], b1 = kyT[(i + 1) >> y];
      *reinterpret_cast<uint4*>(d) =
          make_uint4(c0, c1, wd_gf_mul4(a1.x, b1.x), wd_gf_mul4(a1.y, b1.y));
    } else {
      *reinterpret_cast<uint2*>(d) = make_uint2(c0, c1);
    }
  }
}

}  // namespace

hipError_t launch_shamir_key_table(const ShamirDims& d, const uint8_t* d_keys, uint64_t key_pitch,
                                   uint64_t key_stride, int rounds, int v0, int ng, uint8_t* d_kT,
                                   hipStream_t s) {
  if (rounds < 1 || v0 < 0 || ng < 1 || ng > kShamirSlots ||
      reinterpret_cast<uintptr_t>(d_kT) % 8 != 0)
    return hipErrorInvalidValue;
  const uint64_t klen = d.X + d.Y;
  hipLaunchKernelGGL(k_shamir_key_table, dim3((unsigned)((klen + 255) / 256)), dim3(256), 0, s,
                     d_keys, key_pitch, key_stride, rounds, v0, ng, klen,
                     reinterpret_cast<uint2*>(d_kT));
  return hipGetLastError();
}

hipError_t launch_shamir_seg(const ShamirDims& d, const uint8_t* vals, uint32_t pitch, uint32_t efs,
                             const uint8_t* d_kT, int ng, uint64_t lo, uint64_t hi, bool strided,
                             uint8_t* out, hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (!shamir_seg_takes(pitch) || efs < 1 || efs > pitch || hi > d.X * d.Y || ng < 1 ||
      ng > kShamirSlots || reinterpret_cast<uintptr_t>(d_kT) % 8 != 0)
    return hipErrorInvalidValue;
  SegArgs A;
  A.vals = vals;
  A.out = out;
  A.resp_len = d.resp_len;
  A.lo = lo;
  A.hi = hi;
  A.pitch = pitch;
  A.efs = efs;
  A.ndw = pitch / 4u;
  A.ncg = (A.ndw + kColGroupLanes - 1) / kColGroupLanes;
  A.y = d.y;
  A.ng = ng;
  A.al4 = efs % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
  const uint2* const kT = reinterpret_cast<const uint2*>(d_kT);
  if (strided) {  // Ry: every gamma (those the range leaves out store nothing), words ky[delta]
    A.kT = kT;
    A.seg0 = 0;
    A.nseg = d.Y;
    A.rec_base = d.X;
  } else {  // Rx: the deltas the range touches, words kx[gamma]
    A.kT = kT + d.X;
    A.seg0 = lo >> d.y;
    A.nseg = ((hi - 1) >> d.y) - A.seg0 + 1;
    A.rec_base = 0;
  }
  const uint64_t blocks = (A.nseg * A.ncg + kSegWaves - 1) / kSegWaves;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (strided)
    hipLaunchKernelGGL(k_shamir_seg<true>, dim3((unsigned)blocks), dim3(kSegThreads), 0, s, A);
  else
    hipLaunchKernelGGL(k_shamir_seg<false>, dim3((unsigned)blocks), dim3(kSegThreads), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_shamir_coefs_g(const ShamirDims& d, const uint8_t* d_kT, uint64_t lo, uint64_t hi,
                                 uint8_t* d_c, hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (hi > d.X * d.Y || reinterpret_cast<uintptr_t>(d_c) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(d_kT) % 8 != 0)
    return hipErrorInvalidValue;
  const uint64_t npairs = (hi - lo + 1) / 2;
  const dim3 grid((unsigned)std::min<uint64_t>((npairs + 255) / 256, 1u << 16));
  hipLaunchKernelGGL(k_shamir_coefs_g, grid, dim3(256), 0, s, reinterpret_cast<const uint2*>(d_kT),
                     d.X, d.y, lo, hi, d_c);
  return hipGetLastError();
}

}  // namespace pir
