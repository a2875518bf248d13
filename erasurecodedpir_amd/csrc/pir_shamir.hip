// pir_shamir.hip -- the Shamir sqrt(N) mode's answer kernels (pir_shamir.h).
//
// The answer is built from three shard-sized passes and two small kernels:
//   k_shamir_rows    value rows -> Rx: a lane owns 16 bytes of one matrix row delta and walks
//                    its 2^y records; kx[gamma] is the same for every lane at every step.
//   k_shamir_strips  value rows -> Ry: a lane owns 16 bytes of one column gamma and walks the
//                    deltas; ky[delta] is the same for every lane at every step, and a step of
//                    the whole grid reads one matrix row front to back.
//   k_shamir_coefs + the explicit-coefficient scan (k_scan_uni + k_reduce) over the Hermite
//                    rows -> tot1.
//   k_shamir_totals  tot2 = XOR_delta ky[delta] * Rx[delta], from the finished row sums.
// Both passes accumulate in bit planes (Z_k ^= x for the set bits k of the coefficient, the
// fold sum_k alpha^k Z_k once at the end, poly 0x11d) for up to kShamirRounds rounds at a time.
// Every shape goes through these kernels: records of any efs >= 1 (rows are pitch = 16-byte
// multiples apart, pad bytes zero), n >= 0, ranges that cut matrix rows.
#include "pir_bits.h"
#include "pir_shamir.h"

#include <algorithm>

namespace pir {

ShamirDims shamir_dims(int n, uint32_t efs) {
  ShamirDims d;
  d.x = (n + 1) / 2;
  d.y = n - d.x;
  d.X = 1ull << d.x;
  d.Y = 1ull << d.y;
  d.resp_len = (d.X + d.Y + 2) * (uint64_t)efs;
  return d;
}

namespace {

__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}
__device__ __forceinline__ uint4 xtime16(uint4 x) {
  return make_uint4(gf_xtime4(x.x), gf_xtime4(x.y), gf_xtime4(x.z), gf_xtime4(x.w));
}
// x * c for a per-lane coefficient byte
__device__ __forceinline__ uint4 gf_mul16(uint4 x, uint32_t c) {
  uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const uint32_t m = 0u - ((c >> b) & 1u);
    acc = make_uint4(acc.x ^ (x.x & m), acc.y ^ (x.y & m), acc.z ^ (x.z & m), acc.w ^ (x.w & m));
    x = xtime16(x);
  }
  return acc;
}
__device__ __forceinline__ uint32_t gf_mul8(uint32_t a, uint32_t b) {
  uint32_t m = 0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    m ^= a & (0u - ((b >> t) & 1u));
    a = ((a << 1) ^ ((a & 0x80u) ? 0x11du : 0u)) & 0xffu;
  }
  return m;
}

// Z[k] ^= x for the set bits k of the (wave-uniform) coefficient c
__device__ __forceinline__ void planes_add(uint4 (&Z)[8], uint4 x, uint32_t c) {
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (c & (1u << k)) Z[k] = xor4(Z[k], x);
}
// sum_k alpha^k Z[k]
__device__ __forceinline__ uint4 planes_fold(const uint4 (&Z)[8]) {
  uint4 acc = Z[7];
#pragma unroll
  for (int k = 6; k >= 0; --k) acc = xor4(xtime16(acc), Z[k]);
  return acc;
}

// bytes [16 ch, 16 ch + 16) of a response record of efs bytes; al: efs % 16 == 0 and the
// response 16-byte aligned
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
  for (uint32_t t = 0; t < 16u && off + t < efs; ++t) w[t >> 2] |= (uint32_t)rec[off + t] << (8 * (t & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The coefficient bytes k[0 .. U) of one round as U / 4 words.  The address is the same for
// every lane; when it is 4-byte aligned (al4) the words are dword loads, which a uniform address
// turns into scalar loads -- byte loads from a uniform address stay vector loads, one per
// record and round, in the same queue as the rows.
template <int U>
__device__ __forceinline__ void coef_words(const uint8_t* k, bool al4, uint32_t (&w)[U / 4]) {
  if (al4) {
#pragma unroll
    for (int i = 0; i < U / 4; ++i) w[i] = reinterpret_cast<const uint32_t*>(k)[i];
  } else {
#pragma unroll
    for (int i = 0; i < U / 4; ++i)
      w[i] = k[4 * i] | (k[4 * i + 1] << 8) | (k[4 * i + 2] << 16) | ((uint32_t)k[4 * i + 3] << 24);
  }
}

struct ShamirArgs {
  const uint8_t* vals;
  const uint8_t* keys;
  uint8_t* out;
  uint64_t key_pitch, X, resp_len, lo, hi;
  uint64_t d0, nd;  // the deltas the range touches: [d0, d0 + nd)
  uint32_t pitch, efs;
  int y, nr, al;
  int kal;  // keys, keys + X and key_pitch are multiples of 4 (coef_words)
};

// records in flight per lane in the two passes (registers: 32 R of planes + 4 U of rows)
template <int R>
constexpr int kInFlight = R == 1 ? 8 : 4;

// lane = (delta, chunk); walks gamma.  Rx[delta] of rounds [0, nr).
template <int R>
__global__ __launch_bounds__(256) void k_shamir_rows(ShamirArgs A) {
  const uint32_t cpr = A.pitch / 16u;
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= A.nd * cpr) return;
  const uint64_t delta = A.d0 + idx / cpr;
  const uint32_t ch = (uint32_t)(idx % cpr);
  const uint64_t Y = 1ull << A.y, i0 = delta << A.y;
  const uint64_t g_lo = A.lo > i0 ? A.lo - i0 : 0;
  const uint64_t g_hi = A.hi - i0 < Y ? A.hi - i0 : Y;  // hi > i0: delta is in [d0, d0 + nd)
  uint4 Z[R][8];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int k = 0; k < 8; ++k) Z[a][k] = make_uint4(0, 0, 0, 0);
  const uint8_t* p = A.vals + i0 * A.pitch + ch * 16u;
  const uint8_t* kx = A.keys + A.X;
  auto row = [&](uint64_t g) __attribute__((always_inline)) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g >= g_lo && g < g_hi) v = *reinterpret_cast<const uint4*>(p + g * A.pitch);
    return v;
  };
  auto fold = [&](uint4 v, uint64_t g) __attribute__((always_inline)) {
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const uint32_t c = a < A.nr ? kx[(uint64_t)a * A.key_pitch + g] : 0u;
      planes_add(Z[a], v, c);
    }
  };
  // U records in flight per lane: the loads of a batch are issued before its folds
  constexpr int U = kInFlight<R>;
  uint64_t g = 0;
  for (; g + U <= Y; g += U) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = row(g + u);
    uint32_t cw[R][U / 4];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      if (a < A.nr) {
        coef_words<U>(kx + (uint64_t)a * A.key_pitch + g, A.kal, cw[a]);
      } else {
#pragma unroll
        for (int i = 0; i < U / 4; ++i) cw[a][i] = 0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int a = 0; a < R; ++a) planes_add(Z[a], v[u], (cw[a][u / 4] >> (8 * (u % 4))) & 0xffu);
  }
  for (; g < Y; ++g) fold(row(g), g);
#pragma unroll
  for (int a = 0; a < R; ++a)
    if (a < A.nr)
      store_chunk(A.out + (uint64_t)a * A.resp_len + delta * A.efs, ch, A.efs, planes_fold(Z[a]),
                  A.al);
}

// lane = (gamma, chunk); walks delta.  Ry[gamma] of rounds [0, nr).
template <int R>
__global__ __launch_bounds__(256) void k_shamir_strips(ShamirArgs A) {
  const uint32_t cpr = A.pitch / 16u;
  const uint64_t Y = 1ull << A.y;
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (idx >= Y * cpr) return;
  const uint64_t gamma = idx / cpr;
  const uint32_t ch = (uint32_t)(idx % cpr);
  uint4 Z[R][8];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int k = 0; k < 8; ++k) Z[a][k] = make_uint4(0, 0, 0, 0);
  const uint8_t* p = A.vals + gamma * A.pitch + ch * 16u;
  auto row = [&](uint64_t d) __attribute__((always_inline)) {
    const uint64_t i = (d << A.y) + gamma;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i >= A.lo && i < A.hi) v = *reinterpret_cast<const uint4*>(p + (d << A.y) * A.pitch);
    return v;
  };
  auto fold = [&](uint4 v, uint64_t d) __attribute__((always_inline)) {
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const uint32_t c = a < A.nr ? A.keys[(uint64_t)a * A.key_pitch + d] : 0u;
      planes_add(Z[a], v, c);
    }
  };
  constexpr int U = kInFlight<R>;
  const uint64_t d1 = A.d0 + A.nd;
  uint64_t d = A.d0;
  for (; d < d1 && d % U != 0; ++d) fold(row(d), d);  // up to a batch boundary (aligned words)
  for (; d + U <= d1; d += U) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = row(d + u);
    uint32_t cw[R][U / 4];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      if (a < A.nr) {
        coef_words<U>(A.keys + (uint64_t)a * A.key_pitch + d, A.kal, cw[a]);
      } else {
#pragma unroll
        for (int i = 0; i < U / 4; ++i) cw[a][i] = 0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int a = 0; a < R; ++a) planes_add(Z[a], v[u], (cw[a][u / 4] >> (8 * (u % 4))) & 0xffu);
  }
  for (; d < d1; ++d) fold(row(d), d);
#pragma unroll
  for (int a = 0; a < R; ++a)
    if (a < A.nr)
      store_chunk(A.out + (uint64_t)a * A.resp_len + (A.X + gamma) * A.efs, ch, A.efs,
                  planes_fold(Z[a]), A.al);
}

__global__ __launch_bounds__(256) void k_shamir_coefs(const uint8_t* __restrict__ keys,
                                                      uint64_t key_pitch, uint64_t X, int y,
                                                      int nq, int nrp, uint64_t lo, uint64_t hi,
                                                      uint8_t* __restrict__ dst) {
  const uint64_t Ym = (1ull << y) - 1;
  for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t delta = i >> y, gamma = i & Ym;
    for (int a = 0; a < nrp; ++a) {
      uint32_t c = 0;
      if (a < nq) {
        const uint8_t* k = keys + (uint64_t)a * key_pitch;
        c = gf_mul8(k[X + gamma], k[delta]);
      }
      dst[(i - lo) * (uint64_t)nrp + a] = (uint8_t)c;
    }
  }
}

// one workgroup per (chunk, round): its lanes split the deltas, then an LDS tree
__global__ __launch_bounds__(256) void k_shamir_totals(const uint8_t* __restrict__ keys,
                                                       uint64_t key_pitch, uint64_t X, uint64_t Y,
                                                       uint64_t resp_len, uint32_t efs,
                                                       const uint8_t* __restrict__ tot1,
                                                       uint8_t* out, int al) {
  __shared__ uint4 part[256];
  const uint32_t ch = blockIdx.x;
  const int a = blockIdx.y;
  const uint8_t* ky = keys + (uint64_t)a * key_pitch;
  uint8_t* resp = out + (uint64_t)a * resp_len;
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (uint64_t d = threadIdx.x; d < X; d += 256u)
    acc = xor4(acc, gf_mul16(load_chunk(resp + d * efs, ch, efs, al), ky[d]));
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] = xor4(part[threadIdx.x], part[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    store_chunk(resp + (X + Y + 1) * efs, ch, efs, part[0], al);
    store_chunk(resp + (X + Y) * efs, ch, efs, load_chunk(tot1 + (uint64_t)a * efs, ch, efs, al),
                al);
  }
}

bool fill_args(const ShamirDims& d, const uint8_t* vals, uint32_t pitch, uint32_t efs,
               const uint8_t* d_keys, uint64_t key_pitch, int nr, uint64_t lo, uint64_t hi,
               uint8_t* out, ShamirArgs* A) {
  if (nr < 1 || nr > kShamirRounds || pitch % 16 != 0 || efs > pitch || efs < 1 || lo >= hi ||
      hi > d.X * d.Y)
    return false;
  A->vals = vals;
  A->keys = d_keys;
  A->out = out;
  A->key_pitch = key_pitch;
  A->X = d.X;
  A->resp_len = d.resp_len;
  A->lo = lo;
  A->hi = hi;
  A->d0 = lo >> d.y;
  A->nd = ((hi - 1) >> d.y) - A->d0 + 1;
  A->pitch = pitch;
  A->efs = efs;
  A->y = d.y;
  A->nr = nr;
  A->al = efs % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  A->kal = reinterpret_cast<uintptr_t>(d_keys) % 4 == 0 && d.X % 4 == 0 && key_pitch % 4 == 0;
  return true;
}

}  // namespace

#define PIR_SHAMIR_LAUNCH(KERNEL, total)                                                  \
  do {                                                                                    \
    const uint64_t blocks = ((total) + 255) / 256;                                        \
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;                              \
    const dim3 grid((unsigned)blocks);                                                    \
    if (nr == 1) hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, s, A);                 \
    else if (nr == 2) hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, s, A);            \
    else hipLaunchKernelGGL(KERNEL<kShamirRounds>, grid, dim3(256), 0, s, A);             \
    return hipGetLastError();                                                             \
  } while (0)

hipError_t launch_shamir_rows(const ShamirDims& d, const uint8_t* vals, uint32_t pitch,
                              uint32_t efs, const uint8_t* d_keys, uint64_t key_pitch, int nr,
                              uint64_t lo, uint64_t hi, uint8_t* out, hipStream_t s) {
  ShamirArgs A;
  if (!fill_args(d, vals, pitch, efs, d_keys, key_pitch, nr, lo, hi, out, &A))
    return hipErrorInvalidValue;
  PIR_SHAMIR_LAUNCH(k_shamir_rows, A.nd * (pitch / 16u));
}

hipError_t launch_shamir_strips(const ShamirDims& d, const uint8_t* vals, uint32_t pitch,
                                uint32_t efs, const uint8_t* d_keys, uint64_t key_pitch, int nr,
                                uint64_t lo, uint64_t hi, uint8_t* out, hipStream_t s) {
  ShamirArgs A;
  if (!fill_args(d, vals, pitch, efs, d_keys, key_pitch, nr, lo, hi, out, &A))
    return hipErrorInvalidValue;
  PIR_SHAMIR_LAUNCH(k_shamir_strips, d.Y * (pitch / 16u));
}
#undef PIR_SHAMIR_LAUNCH

hipError_t launch_shamir_coefs(const ShamirDims& d, const uint8_t* d_keys, uint64_t key_pitch,
                               int nq, int nrp, uint64_t lo, uint64_t hi, uint8_t* d_c,
                               hipStream_t s) {
  if (lo >= hi) return hipSuccess;
  if (hi > d.X * d.Y || nq < 1 || nq > nrp) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<uint64_t>((hi - lo + 255) / 256, 1u << 16));
  hipLaunchKernelGGL(k_shamir_coefs, grid, dim3(256), 0, s, d_keys, key_pitch, d.X, d.y, nq, nrp,
                     lo, hi, d_c);
  return hipGetLastError();
}

hipError_t launch_shamir_totals(const ShamirDims& d, uint32_t efs, const uint8_t* d_keys,
                                uint64_t key_pitch, int nq, const uint8_t* tot1, uint8_t* out,
                                hipStream_t s) {
  if (nq < 1 || efs < 1) return hipErrorInvalidValue;
  const int al = efs % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(tot1) % 16 == 0;
  const dim3 grid((efs + 15u) / 16u, (unsigned)nq);
  hipLaunchKernelGGL(k_shamir_totals, grid, dim3(256), 0, s, d_keys, key_pitch, d.X, d.Y,
                     d.resp_len, efs, tot1, out, al);
  return hipGetLastError();
}

}  // namespace pir
