// pir_shamir_q.hip -- queued Shamir sqrt(N) keys that share shard passes (pir_shamir.h).
//
// Rx and Ry are one computation seen from two sides: a GF(2^8) matrix-vector product in which a
// record's coefficient depends only on its position inside a *segment* and every segment has one
// output record.  For Rx the segment is a matrix row delta (records `pitch` apart, coefficient
// kx[gamma]); for Ry it is a column gamma (records `pitch << y` apart, coefficient ky[delta]).
// Up to 8 virtual keys (the rounds of the queued keys) go through a pass together:
//   k_shamir_key_table  kT[j] = the 8 keys' byte j as one 64-bit word (slot g = byte g, absent
//                       slots zero): kyT = kT[0, X), kxT = kT[X, X + Y)
//   k_shamir_seg        one wave per (segment, 64-dword column group): pir_scan_t.hip's transposed
//                       four-Russians fold over the segment's rows (the index from the shard's
//                       bits, the nibble tables from the coefficient words; the cost per row does
//                       not depend on the number of planes), the per-segment sums stored straight
//                       into each virtual key's response record.  No slabs, no k_reduce.
//   k_shamir_coefs_g    the Hermite scan's record-major share rows c[i] = kxT[gamma_i] *
//                       kyT[delta_i], byte-wise (two wd_gf_mul4)
#include "pir_bits.h"
#include "pir_kernels.h"
#include "pir_shamir.h"
#include "pir_woodruff.h"

#include <algorithm>

namespace pir {

bool shamir_seg_takes(uint32_t pitch) { return pitch % 4 == 0 && pitch / 4 >= (uint32_t)kColGroupLanes; }

namespace {

constexpr int kSegThreads = 256;
constexpr int kSegWaves = kSegThreads / 64;

__device__ __forceinline__ uint32_t xtime4_q(uint32_t x) {  // 4 packed bytes times alpha
  return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du);
}

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
  constexpr int kTabBytes = 128;  // 16 entries of 8 bytes: aligned to its size, conflict free
  __shared__ alignas(128) uint32_t tab[kSegWaves][16 * kTabBytes / 4];
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
  uint32_t* const tw = &tab[wv][0];

  uint32_t Zt[32][2];
#pragma unroll
  for (int j = 0; j < 32; ++j) Zt[j][0] = Zt[j][1] = 0;

  // rows past the segment's last re-read its first and have zero coefficient words
  auto load_rel = [&](uint32_t rel) __attribute__((always_inline)) {
    const uint64_t off = (uint64_t)(rel < nrows ? rel : 0u) * stride;
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p0 + off + voff));
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
      const char* const tj = reinterpret_cast<const char*>(tw) + j0 / 4 * kTabBytes;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const uint32_t j = r0 + j0 + 8 * g;
        uint32_t (&L)[4] = *reinterpret_cast<uint32_t(*)[4]>(&x[8 * g]);  // in place
        uint32_t (&H)[4] = *reinterpret_cast<uint32_t(*)[4]>(&x[8 * g + 4]);
        transpose4x32(L);
        transpose4x32(H);
        // k_scan_t's 8 software-pipelined steps of 4 bit positions: step s takes the even or odd
        // nibbles of L[s / 2], H[s / 2] as entry byte offsets
        const char* const tg = tj + g * (2 * kTabBytes);
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
            t[2 * b + 1] = *reinterpret_cast<const uint2*>(tg + kTabBytes + ((hi >> (8 * b)) & 0xffu));
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

  // back to planes, the fold by the powers of alpha, and each slot's dword into its response
  const uint32_t off = dw * 4u;
  const bool in = active && off < A.efs;
  uint8_t* const rec = A.out + (A.rec_base + seg) * A.efs + off;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    uint32_t Y[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) Y[j] = Zt[j][d];
    transpose32(Y);  // Y[q]: plane 32 d + q = (slot 4 d + q / 8, bit q % 8)
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
      const int a = 4 * d + a4;
      uint32_t acc = Y[8 * a4 + 7];
#pragma unroll
      for (int b = 6; b >= 0; --b) acc = xtime4_q(acc) ^ Y[8 * a4 + b];
      if (in && a < A.ng) {
        uint8_t* const o = rec + (uint64_t)a * A.resp_len;
        if (A.al4) {
          *reinterpret_cast<uint32_t*>(o) = acc;
        } else {  // records of efs % 4 != 0, or an unaligned response: bytewise
          for (uint32_t t = 0; t < 4u && off + t < A.efs; ++t) o[t] = (uint8_t)(acc >> (8 * t));
        }
      }
    }
  }
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
