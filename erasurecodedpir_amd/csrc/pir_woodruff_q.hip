// pir_woodruff_q.hip -- queued Woodruff derivative keys that share shard passes (pir_woodruff.h).
//
// Both derivative passes are a GF(2^8) matrix-vector product in which a record's coefficient
// depends only on its position inside a *segment* and every segment has one output record, as the
// Shamir queue's Rx / Ry passes are (pir_shamir_q.hip); only the geometry is the triangle's:
//   rows pass     segment = triangle row a: the records start(a) + j, j < M - 1 - a, `pitch`
//                 apart, coefficient key[a + 1 + j], output R[a]
//   columns pass  segment = column b: the records (a, b), a < b, at start(a) + b - a - 1 -- from
//                 a to a + 1 that is (M - a - 2) records further -- coefficient key[a], output C[b]
// and out[1 + j] = R[j] ^ C[j].  Up to 8 keys go through a pass together: keyT[j] (byte g = key
// g's byte j, k_woodruff_key_table<8>) is a row's coefficient word, and one wave per (segment,
// 64-dword column group) runs pir_seg_walk.h's transposed four-Russians fold and puts each key's
// dword straight into response record 1 + segment of that key: the rows pass stores, the columns
// pass XORs into what the rows pass stored (one owner per address, the passes stream-ordered).
// No slabs, no k_reduce, no workgroup barrier.
#include "pir_kernels.h"
#include "pir_seg_walk.h"
#include "pir_woodruff.h"

namespace pir {

bool woodruff_seg_takes(uint32_t pitch) { return seg_takes(pitch); }

namespace {

struct WdSegArgs {
  const uint8_t* rows;  // the shard: record i at rows + i * pitch
  const uint2* kT;      // keyT[j], j < M
  uint8_t* out;         // slot g's response (M + 1 records of efs bytes) at out + g * resp_len
  uint64_t resp_len, lo, hi;
  uint32_t M;
  uint32_t a0, b0, a1, b1;  // the pairs of the records lo and hi - 1
  uint32_t nseg;            // rows pass: the triangle rows a0 .. a1; columns pass: b = M - 1 .. 1
  uint32_t pitch, efs, ndw, ncg;  // dwords per row, column groups per row
  int ng, al4, pair;
};

// Segments are handed out longest first (rows: a ascending, columns: b descending); pair: a wave
// takes segment t and then segment nseg - 1 - t, whose lengths add up to about the same for every
// t.  Only the records inside [lo, hi) are walked; a segment with none stores nothing (the
// responses were zeroed).  Row addresses: a 64-bit wave-uniform base + a 32-bit lane offset.
template <bool COLS>
__global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(kScanTWavesPerEU)))
void k_woodruff_seg(WdSegArgs A) {
  __shared__ alignas(128) uint32_t tab[kSegWaves][FrTab<2>::kWords];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t item = (uint64_t)blockIdx.x * kSegWaves + wv;
  const uint32_t nt = A.pair ? (A.nseg + 1) / 2 : A.nseg;
  if (item >= (uint64_t)nt * A.ncg) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t t = (uint32_t)(item / A.ncg), cg = (uint32_t)(item % A.ncg);
  const uint32_t dw = cg * kColGroupLanes + lane;
  const bool active = dw < A.ndw;
  const uint32_t voff = (active ? dw : 0u) * 4u;  // inactive lanes: the row's first dword
  const uint32_t off = dw * 4u;
  const bool in = active && off < A.efs;
  uint32_t* const tw = &tab[wv][0];

#pragma nounroll
  for (int half = 0; half < 2; ++half) {
    const uint32_t s = half == 0 ? t : A.nseg - 1 - t;
    if (half == 1 && (!A.pair || s <= t)) break;  // the middle segment of an odd count: once
    uint32_t seg, nrows;
    const uint2* kw;
    uint32_t Zt[32][2];
    if constexpr (COLS) {
      // column b: a in [ra, rb) is the one contiguous run whose records lie in [lo, hi), for the
      // rank start(a) + b - a - 1 rises strictly with a
      const uint32_t b = A.M - 1 - s;
      const uint32_t ra = b >= A.b0 ? A.a0 : A.a0 + 1;
      uint32_t rb = b <= A.b1 ? A.a1 + 1 : A.a1;
      rb = rb < b ? rb : b;
      if (ra >= rb) continue;
      seg = b;
      nrows = rb - ra;
      kw = A.kT + ra;
      // start(a) + b - a - 1 = a (2M - a - 3) / 2 + b - 1: the closed form, in scalar registers
      const uint64_t ob = (uint64_t)(b - 1) * A.pitch;
      const uint32_t c = 2 * A.M - 3;
      seg_walk(
          A.rows,
          [&](uint32_t rel) __attribute__((always_inline)) {
            const uint32_t a = ra + rel;
            const uint32_t tri = (uint32_t)(((uint64_t)a * (c - a)) >> 1);  // < N <= 2^31
            return ob + (uint64_t)tri * A.pitch;
          },
          nrows, kw, voff, lane, tw, Zt);
    } else {
      const uint32_t a = A.a0 + s;
      const uint64_t i0 = wd_start(A.M, a), len = A.M - 1 - a;
      const uint64_t j0 = A.lo > i0 ? A.lo - i0 : 0;
      const uint64_t j1 = A.hi <= i0 ? 0 : (A.hi - i0 < len ? A.hi - i0 : len);  // cut at hi <= N
      if (j0 >= j1) continue;
      seg = a;
      nrows = (uint32_t)(j1 - j0);
      kw = A.kT + a + 1 + j0;
      const uint64_t o0 = (i0 + j0) * A.pitch;
      seg_walk(
          A.rows,
          [&](uint32_t rel) __attribute__((always_inline)) { return o0 + (uint64_t)rel * A.pitch; },
          nrows, kw, voff, lane, tw, Zt);
    }
    const SegOut O{A.out + (uint64_t)(1 + seg) * A.efs + off, A.resp_len, off, A.efs, A.ng, A.al4, in};
    planes_out<2, 8>(Zt, [&](int g, uint32_t acc) __attribute__((always_inline)) {
      seg_store<COLS>(O, g, acc);
    });
  }
}

}  // namespace

hipError_t launch_woodruff_seg(const uint8_t* rows, uint32_t pitch, uint32_t efs,
                               const uint8_t* d_keyT, uint32_t M, int ng, uint64_t lo, uint64_t hi,
                               bool cols, bool pair, uint8_t* out, hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (M < 3 || M >= (1u << 17) || hi > (uint64_t)M * (M - 1) / 2 || !woodruff_seg_takes(pitch) ||
      efs < 1 || efs > pitch || ng < 1 || ng > kWdDerivSlots ||
      reinterpret_cast<uintptr_t>(d_keyT) % 8 != 0)
    return hipErrorInvalidValue;
  const WdPair p0 = wd_pair(M, lo), p1 = wd_pair(M, hi - 1);
  WdSegArgs A;
  A.rows = rows;
  A.kT = reinterpret_cast<const uint2*>(d_keyT);
  A.out = out;
  A.resp_len = (uint64_t)(M + 1) * efs;
  A.lo = lo;
  A.hi = hi;
  A.M = M;
  A.a0 = p0.a;
  A.b0 = p0.b;
  A.a1 = p1.a;
  A.b1 = p1.b;
  A.nseg = cols ? M - 1 : p1.a - p0.a + 1;
  A.pitch = pitch;
  A.efs = efs;
  A.ndw = pitch / 4u;
  A.ncg = (A.ndw + kColGroupLanes - 1) / kColGroupLanes;
  A.ng = ng;
  A.al4 = efs % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
  A.pair = pair;
  const uint64_t nt = pair ? (A.nseg + 1) / 2 : A.nseg;
  const uint64_t blocks = (nt * A.ncg + kSegWaves - 1) / kSegWaves;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  if (cols)
    hipLaunchKernelGGL(k_woodruff_seg<true>, dim3((unsigned)blocks), dim3(kSegThreads), 0, s, A);
  else
    hipLaunchKernelGGL(k_woodruff_seg<false>, dim3((unsigned)blocks), dim3(kSegThreads), 0, s, A);
  return hipGetLastError();
}

}  // namespace pir
