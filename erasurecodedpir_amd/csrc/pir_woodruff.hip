// pir_woodruff.hip -- the Woodruff mode's two-kernel path (pir_woodruff.h): k_woodruff_coefs
// writes one coefficient byte per record of the range, then the explicit-coefficient scan
// (k_scan_uni + k_reduce) folds the rows.  It serves every range and record shape; the whole
// domain of a shape k_query tiles goes through k_query's Woodruff tile builder instead
// (wd_tile, pir_kernels.hip), which keeps the coefficients in LDS.
#include "pir_woodruff.h"

#include <stdlib.h>

#include <algorithm>

namespace pir {

uint32_t wd_key_len(int n) {
  if (n < 0 || n > 31) return 0;
  const uint64_t N = 1ull << n;
  uint64_t m = 3;
  while (m * (m - 1) / 2 < N) ++m;
  return (uint32_t)m;
}

namespace {

constexpr int kWdRun = 16;  // consecutive records per thread: one wd_pair, then the walk

__global__ __launch_bounds__(256) void k_woodruff_coefs(const uint8_t* __restrict__ key,
                                                        uint32_t M, int nrp, uint64_t lo,
                                                        uint64_t hi, uint8_t* __restrict__ dst) {
  const uint64_t nruns = (hi - lo + kWdRun - 1) / kWdRun;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nruns;
       r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i0 = lo + r * kWdRun;
    const uint64_t i1 = i0 + kWdRun < hi ? i0 + kWdRun : hi;
    WdPair p = wd_pair(M, i0);
    uint32_t pa = p.a, ka = key[p.a];
    for (uint64_t i = i0; i < i1; ++i) {
      if (p.a != pa) {
        pa = p.a;
        ka = key[pa];
      }
      uint8_t* d = dst + (i - lo) * (uint64_t)nrp;
      d[0] = (uint8_t)wd_gf_mul(ka, key[p.b]);
      for (int a = 1; a < nrp; ++a) d[a] = 0;
      wd_next(M, p);
    }
  }
}

// ---- queued keys: the shares of a group of keys in one walk (pir_woodruff.h) -----------------
constexpr uint32_t kWdLdsBytes = 48u << 10;  // the interleaved key table in LDS up to this size
constexpr unsigned kWdLdsBlocks = 1024;      // ... built once per workgroup, so few workgroups

// keyT[j]: byte g = key_g[j]
template <int W> struct WdEntry;
template <> struct WdEntry<2> { using T = uint16_t; };
template <> struct WdEntry<4> { using T = uint32_t; };
template <> struct WdEntry<8> { using T = uint2; };

template <int W>
__device__ __forceinline__ typename WdEntry<W>::T wd_key_entry(const uint8_t* __restrict__ keys,
                                                               uint32_t M, int ng, uint32_t j) {
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int g = 0; g < W; ++g)
    if (g < ng) w[g >> 2] |= (uint32_t)keys[(uint64_t)g * M + j] << (8 * (g & 3));
  if constexpr (W == 8) return make_uint2(w[0], w[1]);
  else return (typename WdEntry<W>::T)w[0];
}

template <int W>
__global__ __launch_bounds__(256) void k_woodruff_key_table(const uint8_t* __restrict__ keys,
                                                            uint32_t M, int ng,
                                                            typename WdEntry<W>::T* __restrict__ keyT) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < M) keyT[j] = wd_key_entry<W>(keys, M, ng, j);
}

// LDS: the workgroup interleaves the keys into LDS first; else keyT is k_woodruff_key_table's
template <int W, bool LDS>
__global__ __launch_bounds__(256) void k_woodruff_coefs_g(const uint8_t* __restrict__ keys,
                                                          const typename WdEntry<W>::T* __restrict__ keyT,
                                                          uint32_t M, int ng, uint64_t lo,
                                                          uint64_t hi, uint8_t* __restrict__ dst) {
  using T = typename WdEntry<W>::T;
  extern __shared__ uint4 wd_lds[];
  T* const lt = reinterpret_cast<T*>(wd_lds);
  if constexpr (LDS) {
#pragma unroll 4
    for (uint32_t j = threadIdx.x; j < M; j += 256u) lt[j] = wd_key_entry<W>(keys, M, ng, j);
    __syncthreads();
  }
  auto entry = [&](uint32_t j) __attribute__((always_inline)) -> T {
    if constexpr (LDS) return lt[j];
    else return keyT[j];
  };
  constexpr int RPS = 16 / W;  // records per 16-byte store
  const uint64_t nruns = (hi - lo + kWdRun - 1) / kWdRun;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nruns;
       r += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i0 = lo + r * kWdRun;
    const uint64_t i1 = i0 + kWdRun < hi ? i0 + kWdRun : hi;
    const bool full = i1 - i0 == (uint64_t)kWdRun;
    WdPair p = wd_pair(M, i0);  // i0 < hi <= the number of pairs: a < b < M, here and below
    uint32_t pa = p.a;
    T ka = entry(pa);
    uint8_t* const d = dst + (i0 - lo) * (uint64_t)W;
#pragma unroll
    for (int q = 0; q < kWdRun / RPS; ++q) {
      uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < RPS; ++u) {
        if (i0 + (uint64_t)(q * RPS + u) < i1) {
          if (p.a != pa) {
            pa = p.a;
            ka = entry(pa);
          }
          const T kb = entry(p.b);
          if constexpr (W == 8) {
            v[2 * u] = wd_gf_mul4(ka.x, kb.x);
            v[2 * u + 1] = wd_gf_mul4(ka.y, kb.y);
          } else if constexpr (W == 4) {
            v[u] = wd_gf_mul4(ka, kb);
          } else {
            v[u >> 1] |= wd_gf_mul4(ka, kb) << (16 * (u & 1));
          }
          wd_next(M, p);
        }
      }
      if (full) {
        *reinterpret_cast<uint4*>(d + q * 16) = make_uint4(v[0], v[1], v[2], v[3]);
      } else {  // the range's last run: record by record
#pragma unroll
        for (int u = 0; u < RPS; ++u) {
          if (i0 + (uint64_t)(q * RPS + u) >= i1) continue;
          uint8_t* const o = d + (q * RPS + u) * W;
          if constexpr (W == 8) *reinterpret_cast<uint2*>(o) = make_uint2(v[2 * u], v[2 * u + 1]);
          else if constexpr (W == 4) *reinterpret_cast<uint32_t*>(o) = v[u];
          else *reinterpret_cast<uint16_t*>(o) = (uint16_t)(v[u >> 1] >> (16 * (u & 1)));
        }
      }
    }
  }
}

template <int W>
hipError_t coefs_g(const uint8_t* d_keys, uint32_t M, int ng, uint64_t lo, uint64_t hi,
                   uint8_t* d_c, hipStream_t s, uint8_t* d_keyT, bool lds) {
  using T = typename WdEntry<W>::T;
  const uint64_t nruns = (hi - lo + kWdRun - 1) / kWdRun;
  const uint64_t blocks = (nruns + 255) / 256;
  if (lds) {
    const size_t bytes = ((size_t)M * W + 15) & ~(size_t)15;
    hipLaunchKernelGGL((k_woodruff_coefs_g<W, true>),
                       dim3((unsigned)std::min<uint64_t>(blocks, kWdLdsBlocks)), dim3(256), bytes, s,
                       d_keys, (const T*)nullptr, M, ng, lo, hi, d_c);
    return hipGetLastError();
  }
  if (!d_keyT || reinterpret_cast<uintptr_t>(d_keyT) % 8 != 0) return hipErrorInvalidValue;
  T* const keyT = reinterpret_cast<T*>(d_keyT);
  hipLaunchKernelGGL((k_woodruff_key_table<W>), dim3((M + 255u) / 256u), dim3(256), 0, s, d_keys,
                     M, ng, keyT);
  hipLaunchKernelGGL((k_woodruff_coefs_g<W, false>),
                     dim3((unsigned)std::min<uint64_t>(blocks, 1u << 16)), dim3(256), 0, s, d_keys,
                     (const T*)keyT, M, ng, lo, hi, d_c);
  return hipGetLastError();
}

// ---- derivative answers (server.cpp:618-644) -------------------------------------------------
__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}
__device__ __forceinline__ uint4 xtime16(uint4 x) {
  return make_uint4(gf_xtime4(x.x), gf_xtime4(x.y), gf_xtime4(x.z), gf_xtime4(x.w));
}
// Z[k] ^= x for the set bits k of this lane's coefficient c (the lanes of a wave hold different
// triangle rows / columns, so the masks are per lane)
__device__ __forceinline__ void planes_add(uint4 (&Z)[8], uint4 x, uint32_t c) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t m = 0u - ((c >> k) & 1u);
    Z[k] = make_uint4(Z[k].x ^ (x.x & m), Z[k].y ^ (x.y & m), Z[k].z ^ (x.z & m),
                      Z[k].w ^ (x.w & m));
  }
}
// ... and for a coefficient every active lane of the wave shares (U): scalar branches, the set
// bits only
template <bool U>
__device__ __forceinline__ void planes_add_u(uint4 (&Z)[8], uint4 x, uint32_t c) {
  if constexpr (U) {
    c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (c & (1u << k)) Z[k] = xor4(Z[k], x);
  } else {
    planes_add(Z, x, c);
  }
}
// sum_k alpha^k Z[k]
__device__ __forceinline__ uint4 planes_fold(const uint4 (&Z)[8]) {
  uint4 acc = Z[7];
#pragma unroll
  for (int k = 6; k >= 0; --k) acc = xor4(xtime16(acc), Z[k]);
  return acc;
}
__device__ __forceinline__ void planes_clear(uint4 (&Z)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) Z[k] = make_uint4(0, 0, 0, 0);
}
// x * c for a per-lane coefficient byte
__device__ __forceinline__ uint4 gf_mul16(uint4 x, uint32_t c) {
  uint4 Z[8];
  planes_clear(Z);
  planes_add(Z, x, c);
  return planes_fold(Z);
}

// bytes [16 ch, 16 ch + 16) of an answer record of efs bytes; al: efs % 16 == 0 and the answer
// 16-byte aligned
__device__ __forceinline__ void store_chunk(uint8_t* rec, uint32_t ch, uint32_t efs, uint4 v,
                                            bool al) {
  const uint32_t off = ch * 16u;
  if (off >= efs) return;
  if (al) {
    *reinterpret_cast<uint4*>(rec + off) = v;
    return;
  }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  for (uint32_t t = 0; t < 16u && off + t < efs; ++t)
    rec[off + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
}
__device__ __forceinline__ uint4 load_chunk(const uint8_t* rec, uint32_t ch, uint32_t efs,
                                            bool al) {
  const uint32_t off = ch * 16u;
  if (off >= efs) return make_uint4(0, 0, 0, 0);
  if (al) return *reinterpret_cast<const uint4*>(rec + off);
  uint32_t w[4] = {0, 0, 0, 0};
  for (uint32_t t = 0; t < 16u && off + t < efs; ++t)
    w[t >> 2] |= (uint32_t)rec[off + t] << (8 * (t & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

struct WdArgs {
  const uint8_t* rows;  // the shard: record i at rows + i * pitch
  const uint8_t* key;
  uint8_t* out;         // M + 1 records of efs bytes
  uint64_t lo, hi;      // the records answered
  uint32_t a0, a1;      // the triangle rows the range touches: [a0, a1]
  uint32_t M, pitch, efs;
  int al;
};

constexpr int kWdInFlight = 4;  // records in flight per lane (32 plane registers + 4 x 4 of rows)

// Rows pass: out[1 + a] = XOR_b key[b] * row(a, b) over the records of triangle row a inside
// [lo, hi), for a in [a0, a1] (the caller zeroed the answer).  The records of one a are
// contiguous, so a lane owns 16 bytes of one triangle row and walks it: a segmented scan.  Row a
// has M - 1 - a records, so a lane takes two rows, a0 + t and a1 - t, whose lengths add up to the
// same for every t.
// UNI: a record is a whole number of wave rows (pitch % 1024 == 0), so the lanes of a wave share
// the triangle row and with it every step's coefficient.
template <bool UNI>
__global__ __launch_bounds__(256) void k_woodruff_rows(WdArgs A) {
  const uint32_t cpr = A.pitch / 16u;
  const uint32_t na = A.a1 - A.a0 + 1, nt = (na + 1) / 2;
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= (uint64_t)nt * cpr) return;
  const uint32_t t = (uint32_t)(idx / cpr), ch = (uint32_t)(idx % cpr);
  for (int seg = 0; seg < 2; ++seg) {
    const uint32_t a = seg == 0 ? A.a0 + t : A.a1 - t;
    if (seg == 1 && a <= A.a0 + t) break;  // the middle row of an odd count: once
    const uint64_t i0 = wd_start(A.M, a);
    const uint64_t len = A.M - 1 - a;
    const uint64_t j0 = A.lo > i0 ? A.lo - i0 : 0;
    const uint64_t j1 = A.hi <= i0 ? 0 : (A.hi - i0 < len ? A.hi - i0 : len);
    const uint8_t* p = A.rows + i0 * A.pitch + ch * 16u;
    const uint8_t* kb = A.key + a + 1;
    uint4 Z[8];
    planes_clear(Z);
    uint64_t j = j0;
    for (; j + kWdInFlight <= j1; j += kWdInFlight) {
      uint4 v[kWdInFlight];
      uint32_t c[kWdInFlight];
#pragma unroll
      for (int u = 0; u < kWdInFlight; ++u) {
        v[u] = *reinterpret_cast<const uint4*>(p + (j + u) * A.pitch);
        c[u] = kb[j + u];
      }
#pragma unroll
      for (int u = 0; u < kWdInFlight; ++u) planes_add_u<UNI>(Z, v[u], c[u]);
    }
    for (; j < j1; ++j)
      planes_add_u<UNI>(Z, *reinterpret_cast<const uint4*>(p + j * A.pitch), kb[j]);
    store_chunk(A.out + (uint64_t)(1 + a) * A.efs, ch, A.efs, planes_fold(Z), A.al);
  }
}

// out[0] = XOR_a key[a] * out[1 + a] from the finished rows pass (before the columns pass adds
// to them): one workgroup per 16-byte chunk, its lanes split the a, then an LDS tree
__global__ __launch_bounds__(256) void k_woodruff_totals(WdArgs A) {
  __shared__ uint4 part[256];
  const uint32_t ch = blockIdx.x;
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (uint32_t a = A.a0 + threadIdx.x; a <= A.a1; a += 256u)
    acc = xor4(acc, gf_mul16(load_chunk(A.out + (uint64_t)(1 + a) * A.efs, ch, A.efs, A.al),
                             A.key[a]));
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] = xor4(part[threadIdx.x], part[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) store_chunk(A.out, ch, A.efs, part[0], A.al);
}

// Columns pass: out[1 + b] ^= XOR_a key[a] * row(a, b) over the records inside [lo, hi).  A lane
// owns 16 bytes of one column b and walks the triangle rows a in [a0, min(a1, b - 1)]; adjacent
// lanes (adjacent b) read adjacent records at every a, so a step of a workgroup reads its strip
// of columns x efs contiguous bytes.  Every lane still in the batched loop is at the same a, so
// there the coefficient key[a] is wave-uniform.  Column b has b records, so a lane takes two
// columns, 1 + t and M - 1 - t.  The truncated last triangle row and the range's ends are the
// bounds check on the record index.
__global__ __launch_bounds__(256) void k_woodruff_cols(WdArgs A) {
  const uint32_t cpr = A.pitch / 16u;
  const uint32_t nt = A.M / 2;  // columns 1 .. M - 1 in pairs (1 + t, M - 1 - t)
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= (uint64_t)nt * cpr) return;
  const uint32_t t = (uint32_t)(idx / cpr), ch = (uint32_t)(idx % cpr);
  for (int seg = 0; seg < 2; ++seg) {
    const uint32_t b = seg == 0 ? 1u + t : A.M - 1u - t;
    if (seg == 1 && b <= 1u + t) break;  // the middle column of an odd count: once
    const uint32_t e1 = A.a1 + 1 < b ? A.a1 + 1 : b;  // a in [a0, e1)
    if (A.a0 >= e1) continue;
    const uint8_t* p = A.rows + ch * 16u;
    auto row = [&](uint32_t a) __attribute__((always_inline)) {
      const uint64_t i = wd_start(A.M, a) + (b - a - 1);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (i >= A.lo && i < A.hi) v = *reinterpret_cast<const uint4*>(p + i * A.pitch);
      return v;
    };
    uint4 Z[8];
    planes_clear(Z);
    uint32_t a = A.a0;
    for (; a + kWdInFlight <= e1; a += kWdInFlight) {
      uint4 v[kWdInFlight];
      uint32_t c[kWdInFlight];
#pragma unroll
      for (int u = 0; u < kWdInFlight; ++u) {
        v[u] = row(a + u);
        c[u] = A.key[a + u];
      }
#pragma unroll
      for (int u = 0; u < kWdInFlight; ++u) planes_add_u<true>(Z, v[u], c[u]);
    }
    // (the lanes reach the tail at different a: per-lane masks)
    for (; a < e1; ++a) planes_add(Z, row(a), A.key[a]);
    uint8_t* o = A.out + (uint64_t)(1 + b) * A.efs;
    store_chunk(o, ch, A.efs, xor4(load_chunk(o, ch, A.efs, A.al), planes_fold(Z)), A.al);
  }
}

}  // namespace

hipError_t launch_woodruff_deriv(const uint8_t* rows, uint32_t pitch, uint32_t efs,
                                 const uint8_t* d_key, uint32_t M, uint64_t lo, uint64_t hi,
                                 uint8_t* out, hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (M < 3 || hi > (uint64_t)M * (M - 1) / 2 || pitch % 16 != 0 || efs > pitch || efs < 1)
    return hipErrorInvalidValue;
  WdArgs A;
  A.rows = rows;
  A.key = d_key;
  A.out = out;
  A.lo = lo;
  A.hi = hi;
  A.a0 = wd_pair(M, lo).a;
  A.a1 = wd_pair(M, hi - 1).a;
  A.M = M;
  A.pitch = pitch;
  A.efs = efs;
  A.al = efs % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const uint32_t cpr = pitch / 16u;
  const uint64_t rt = (uint64_t)((A.a1 - A.a0 + 2) / 2) * cpr, ct = (uint64_t)(M / 2) * cpr;
  if ((rt + 255) / 256 > 0x7fffffffull || (ct + 255) / 256 > 0x7fffffffull)
    return hipErrorInvalidValue;
  if (cpr % 64u == 0)
    hipLaunchKernelGGL(k_woodruff_rows<true>, dim3((unsigned)((rt + 255) / 256)), dim3(256), 0, s, A);
  else
    hipLaunchKernelGGL(k_woodruff_rows<false>, dim3((unsigned)((rt + 255) / 256)), dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_woodruff_totals, dim3((efs + 15u) / 16u), dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_woodruff_cols, dim3((unsigned)((ct + 255) / 256)), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_woodruff_totals(uint32_t efs, const uint8_t* d_key, uint32_t M, uint64_t lo,
                                  uint64_t hi, uint8_t* out, hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (M < 3 || hi > (uint64_t)M * (M - 1) / 2 || efs < 1) return hipErrorInvalidValue;
  WdArgs A{};
  A.key = d_key;
  A.out = out;
  A.lo = lo;
  A.hi = hi;
  A.a0 = wd_pair(M, lo).a;
  A.a1 = wd_pair(M, hi - 1).a;
  A.M = M;
  A.efs = efs;
  A.al = efs % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  hipLaunchKernelGGL(k_woodruff_totals, dim3((efs + 15u) / 16u), dim3(256), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_woodruff_key_table(const uint8_t* d_keys, uint32_t M, int ng, uint8_t* d_keyT,
                                     hipStream_t s) {
  if (M < 3 || ng < 1 || ng > 8 || !d_keyT || reinterpret_cast<uintptr_t>(d_keyT) % 8 != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_woodruff_key_table<8>), dim3((M + 255u) / 256u), dim3(256), 0, s, d_keys, M,
                     ng, reinterpret_cast<uint2*>(d_keyT));
  return hipGetLastError();
}

hipError_t launch_woodruff_coefs(const uint8_t* d_key, uint32_t M, int nrp, uint64_t lo,
                                 uint64_t hi, uint8_t* d_c, hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (M < 3 || nrp < 1 || hi > (uint64_t)M * (M - 1) / 2) return hipErrorInvalidValue;
  const uint64_t nruns = (hi - lo + kWdRun - 1) / kWdRun;
  const dim3 grid((unsigned)std::min<uint64_t>((nruns + 255) / 256, 1u << 16));
  hipLaunchKernelGGL(k_woodruff_coefs, grid, dim3(256), 0, s, d_key, M, nrp, lo, hi, d_c);
  return hipGetLastError();
}

bool wd_key_table_in_lds(uint32_t M, int W) {
  const char* v = getenv("PIR_WD_LDS");
  return (uint64_t)M * W <= kWdLdsBytes && !(v && atoi(v) == 0);
}

hipError_t launch_woodruff_coefs_g(const uint8_t* d_keys, uint32_t M, int ng, int W, uint64_t lo,
                                   uint64_t hi, uint8_t* d_c, hipStream_t s, uint8_t* d_keyT) {
  if (lo >= hi) return hipSuccess;
  if (M < 3 || M >= (1u << 17) || hi > (uint64_t)M * (M - 1) / 2 || ng < 1 || ng > W ||
      reinterpret_cast<uintptr_t>(d_c) % 16 != 0)
    return hipErrorInvalidValue;
  const bool lds = wd_key_table_in_lds(M, W);
  switch (W) {
    case 2: return coefs_g<2>(d_keys, M, ng, lo, hi, d_c, s, d_keyT, lds);
    case 4: return coefs_g<4>(d_keys, M, ng, lo, hi, d_c, s, d_keyT, lds);
    case 8: return coefs_g<8>(d_keys, M, ng, lo, hi, d_c, s, d_keyT, lds);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pir
