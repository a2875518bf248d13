// pir_coefs.hip -- the coefficient layout step of explicit-coefficient answers (pir_coefs.h).
// Round-major vectors (what the client sends: key[k][i], server.cpp:337) become record-major
// share bytes (what k_scan reads per record).  Reads are coalesced along i for each round; each
// lane writes its record's nrp bytes (one 1/2/4/8/16-byte store).  HBM-bound: nq + nrp bytes
// per record, against the record_bytes of shard the scan then reads.
// Also here: the Hollanti-mode shard encode (k_encode_within) and the client's Hollanti
// coefficient vectors themselves (k_hollanti_keys), which share its packed constant multiply.
#include "pir_coefs.h"
#include "pir_aes.h"
#include "pir_bits.h"
#include "pir_transpose.h"

#include <algorithm>

namespace pir {

template <int NRP>
__global__ __launch_bounds__(256) void k_interleave_coefs(const uint8_t* __restrict__ src,
                                                          uint64_t pitch, uint64_t nrows, int nq,
                                                          uint8_t* __restrict__ dst) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows;
       i += (uint64_t)gridDim.x * blockDim.x) {
    uint8_t b[NRP];
#pragma unroll
    for (int a = 0; a < NRP; ++a) b[a] = a < nq ? src[(uint64_t)a * pitch + i] : 0;
    if constexpr (NRP == 1) {
      dst[i] = b[0];
    } else if constexpr (NRP == 2) {
      reinterpret_cast<uint16_t*>(dst)[i] = (uint16_t)(b[0] | (b[1] << 8));
    } else {
      uint32_t w[NRP / 4];
#pragma unroll
      for (int k = 0; k < NRP / 4; ++k)
        w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
      if constexpr (NRP == 4) reinterpret_cast<uint32_t*>(dst)[i] = w[0];
      else if constexpr (NRP == 8) reinterpret_cast<uint2*>(dst)[i] = make_uint2(w[0], w[1]);
      else reinterpret_cast<uint4*>(dst)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

hipError_t launch_interleave_coefs(const uint8_t* src, uint64_t src_pitch, uint64_t nrows, int nq,
                                   int nrp, uint8_t* d_c, hipStream_t s) {
  if (nrows == 0) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((nrows + 255) / 256, 1u << 16));
#define PIR_IL(N) hipLaunchKernelGGL(k_interleave_coefs<N>, grid, dim3(256), 0, s, src, src_pitch, nrows, nq, d_c)
  switch (nrp) {
    case 1: PIR_IL(1); break;
    case 2: PIR_IL(2); break;
    case 4: PIR_IL(4); break;
    case 8: PIR_IL(8); break;
    case 16: PIR_IL(16); break;
    default: return hipErrorInvalidValue;
  }
#undef PIR_IL
  return hipGetLastError();
}

// ---- k_interleave_coefs_g: the vectors of a group of queued keys -> one W-byte share row ----
// Byte b of a record's share row is round a = b % nrp of key slot g = b / nrp (zero for g >= ng
// and a >= nq).  One thread = 16 consecutive records: a 16-byte load per vector whose address
// is aligned (byte loads at the range's tail and for vectors that are not), the byte transpose
// of pir_transpose.h in registers, W 16-byte stores.  HBM-bound: (ng nq + W) bytes per record.
template <int W>
__global__ __launch_bounds__(256) void k_interleave_coefs_g(
    const uint8_t* __restrict__ src, uint64_t coef_pitch, uint64_t key_stride, int ng, int nq,
    int lg_nrp, uint64_t nrows, uint8_t* __restrict__ dst) {
  const uint64_t nitems = (nrows + 15) / 16;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nitems;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i0 = 16 * t;
    const int cnt = (int)(nrows - i0 < 16 ? nrows - i0 : 16);
    uint4 v[W];
#pragma unroll
    for (int b = 0; b < W; ++b) {
      const int g = b >> lg_nrp, a = b & ((1 << lg_nrp) - 1);
      v[b] = make_uint4(0, 0, 0, 0);
      if (g < ng && a < nq) {
        const uint8_t* p = src + (uint64_t)g * key_stride + (uint64_t)a * coef_pitch + i0;
        if (cnt == 16 && ((uintptr_t)p & 15) == 0) {
          v[b] = *reinterpret_cast<const uint4*>(p);
        } else {
          uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const uint32_t x = k < cnt ? (uint32_t)p[k] << (8 * (k & 3)) : 0u;
            if (k < 4) w0 |= x; else if (k < 8) w1 |= x; else if (k < 12) w2 |= x; else w3 |= x;
          }
          v[b] = make_uint4(w0, w1, w2, w3);
        }
      }
    }
    if (cnt == 16) {
      uint4 o[W];
      tr_records<W>(v, o);
      uint4* out = reinterpret_cast<uint4*>(dst + i0 * W);
#pragma unroll
      for (int m = 0; m < W; ++m) out[m] = o[m];
    } else {  // the range's tail: byte stores
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < cnt) {
#pragma unroll
          for (int b = 0; b < W; ++b) dst[(i0 + k) * W + b] = (uint8_t)tr_byte(v[b], k);
        }
    }
  }
}

hipError_t launch_interleave_coefs_g(const uint8_t* src, uint64_t coef_pitch, uint64_t key_stride,
                                     int ng, int nq, int nrp, int W, uint64_t nrows, uint8_t* d_c,
                                     hipStream_t s) {
  if (nrows == 0) return hipSuccess;
  int lg = 0;
  while ((1 << lg) < nrp) ++lg;
  if ((1 << lg) != nrp || nq < 1 || nq > nrp || ng < 1 || ng * nrp > W ||
      ((uintptr_t)d_c & 15) != 0)
    return hipErrorInvalidValue;
  const uint64_t nitems = (nrows + 15) / 16;
  const dim3 grid((unsigned)std::min<uint64_t>((nitems + 255) / 256, 1u << 16));
#define PIR_ILG(N) hipLaunchKernelGGL(k_interleave_coefs_g<N>, grid, dim3(256), 0, s, src, coef_pitch, key_stride, ng, nq, lg, nrows, d_c)
  switch (W) {
    case 2: PIR_ILG(2); break;
    case 4: PIR_ILG(4); break;
    case 8: PIR_ILG(8); break;
    default: return hipErrorInvalidValue;
  }
#undef PIR_ILG
  return hipGetLastError();
}

// ---- k_encode_within: the Hollanti-mode shard on the GPU ------------------------------------
// One lane per 16-byte chunk of an encoded row; the k coefficients gf_pow(party, j) are
// wave-uniform (scalar branches over their bits, x * alpha^b by xtime, poly 0x11d).
struct WithinCoefs {
  uint8_t c[16];
};

__device__ __forceinline__ uint4 gf_mul_const4_w(uint4 x, uint32_t c) {
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (int b = 0; b < 8; ++b) {
    if (c & (1u << b)) acc = make_uint4(acc.x ^ x.x, acc.y ^ x.y, acc.z ^ x.z, acc.w ^ x.w);
    x = make_uint4(gf_xtime4(x.x), gf_xtime4(x.y), gf_xtime4(x.z), gf_xtime4(x.w));
  }
  return acc;
}

// bytes [off, off + 4) of file v, zero at or past fbytes (synthetic database, client.cpp:16-33)
__device__ __forceinline__ uint32_t synth_word_w(uint64_t v, uint32_t off, uint32_t fbytes) {
  uint32_t w = 0;
  for (uint32_t t = 0; t < 4; ++t)
    if (off + t < fbytes) w |= (v == 1 ? ((off + t) & 0xffu) : (uint32_t)(v & 0xffu)) << (8 * t);
  return w;
}

__global__ __launch_bounds__(256) void k_encode_within(
    const uint8_t* __restrict__ files, uint64_t fpitch, uint64_t nfiles, uint32_t fbytes, int k,
    WithinCoefs co, uint8_t* __restrict__ shard, uint64_t rows, uint64_t row0, uint32_t pitch,
    uint32_t efs) {
  const uint32_t cpr = pitch / 16;
  for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < rows * cpr;
       idx += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = idx / cpr;
    const uint32_t ch = (uint32_t)(idx - r * cpr);
    const uint64_t gr = row0 + r;  // file gr
    uint4 acc = make_uint4(0, 0, 0, 0);
    if (gr < nfiles && ch * 16u < efs) {
      for (int j = 0; j < k; ++j) {
        const uint32_t off = (uint32_t)j * efs + ch * 16u;  // byte offset in the file
        if (off >= fbytes) break;
        uint32_t w[4];
        for (int t = 0; t < 4; ++t) {
          const uint32_t o = off + 4u * t;
          if (files) {
            uint32_t v = 0;
            const uint8_t* f = files + gr * fpitch;
            for (uint32_t u = 0; u < 4; ++u)
              if (o + u < fbytes && ch * 16u + 4u * t + u < efs) v |= (uint32_t)f[o + u] << (8 * u);
            w[t] = v;
          } else {
            w[t] = synth_word_w(gr, o, fbytes);
          }
        }
        const uint4 m = gf_mul_const4_w(make_uint4(w[0], w[1], w[2], w[3]), co.c[j]);
        acc = make_uint4(acc.x ^ m.x, acc.y ^ m.y, acc.z ^ m.z, acc.w ^ m.w);
      }
    }
    uint32_t o[4] = {acc.x, acc.y, acc.z, acc.w};
    for (int t = 0; t < 16; ++t)  // bytes of a part past efs (the row's pad): zero
      if (ch * 16u + t >= efs) o[t >> 2] &= ~(0xffu << (8 * (t & 3)));
    *reinterpret_cast<uint4*>(shard + r * pitch + ch * 16u) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// gf_pow(party, j) (coding.cpp:46-60; pow(0, e) == 1)
static uint8_t gf_pow_h(int party, int j) {
  uint32_t r = 1;
  for (int t = 0; t < j && party; ++t) {
    uint32_t a = r, b = (uint32_t)party, m = 0;
    while (b) {
      if (b & 1) m ^= a;
      a = ((a << 1) ^ ((a & 0x80) ? 0x11d : 0)) & 0xff;
      b >>= 1;
    }
    r = m;
  }
  return (uint8_t)r;
}

static hipError_t launch_encode_parts(const WithinCoefs& co, const uint8_t* d_files,
                                      uint64_t file_pitch, uint64_t num_files,
                                      uint32_t file_bytes, int k, uint8_t* d_shard, uint64_t rows,
                                      uint64_t row0, uint32_t pitch, uint32_t efs, hipStream_t s) {
  if (k < 1 || k > 16 || pitch % 16 != 0 || efs > pitch) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  const uint64_t total = rows * (pitch / 16);
  const dim3 grid((unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 16));
  hipLaunchKernelGGL(k_encode_within, grid, dim3(256), 0, s, d_files, file_pitch, num_files,
                     file_bytes, k, co, d_shard, rows, row0, pitch, efs);
  return hipGetLastError();
}

hipError_t launch_encode_within(const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                                uint32_t file_bytes, int k, int party, uint8_t* d_shard,
                                uint64_t rows, uint64_t row0, uint32_t pitch, uint32_t efs,
                                hipStream_t s) {
  WithinCoefs co{};
  for (int j = 0; j < k && j < 16; ++j) co.c[j] = gf_pow_h(party, j);
  return launch_encode_parts(co, d_files, file_pitch, num_files, file_bytes, k, d_shard, rows,
                             row0, pitch, efs, s);
}

// The formal derivative of the within-file polynomial sum_j part_j x^j at x = party: over
// GF(2^8) only the odd j survive, with coefficient gf_pow(party, j - 1).  The same kernel as
// the value rows with that coefficient vector (a zero coefficient adds nothing).
hipError_t launch_encode_hermite(const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                                 uint32_t file_bytes, int k, int party, uint8_t* d_shard,
                                 uint64_t rows, uint64_t row0, uint32_t pitch, uint32_t efs,
                                 hipStream_t s) {
  WithinCoefs co{};
  for (int j = 1; j < k && j < 16; j += 2) co.c[j] = gf_pow_h(party, j - 1);
  return launch_encode_parts(co, d_files, file_pitch, num_files, file_bytes, k, d_shard, rows,
                             row0, pitch, efs, s);
}

// ---- k_hollanti_keys: the client's coefficient vectors of Hollanti queries -------------------
// genHollantiDPF (shamir_dpf.cpp:190-237) with its random bytes from AES-128-CTR (pir_client.h:
// the key stream).  One lane owns 16 consecutive records = AES block `item` of every stream:
// per round it runs the t blocks of its item (top coefficient first), Horner's rule at the
// points q + 1 on the packed bytes (the points are compile-time constants of the unrolled party
// loop), and writes p x 16 bytes.  Grid y is the key of the launch; a block derives the t
// stream keys of a round from the key's seed into LDS before its lanes walk the items.
// 16-byte stores where the destination is aligned, the bytes below N alone at a vector's tail.
__device__ __forceinline__ void xor_byte(uint4& v, uint32_t pos, uint32_t b) {
  const uint32_t m = b << (8 * (pos & 3)), w = pos >> 2;
  v.x ^= w == 0 ? m : 0u;
  v.y ^= w == 1 ? m : 0u;
  v.z ^= w == 2 ? m : 0u;
  v.w ^= w == 3 ? m : 0u;
}

__global__ __launch_bounds__(256) void k_hollanti_keys(HollantiBatch hb, uint64_t nrec, int t,
                                                       int p, int nq, uint8_t* __restrict__ keys,
                                                       uint64_t coef_pitch, uint64_t key_stride,
                                                       uint64_t party_stride) {
  __shared__ uint32_t tab[2 * 256 * 32];
  __shared__ uint4 sk[256];  // the stream keys of one round (t <= 254)
  load_tables_n<256>(tab);
  const Tab T(tab);
  const int k = blockIdx.y, tid = threadIdx.x;
  const uint4 seed = make_uint4(hb.seed[k][0], hb.seed[k][1], hb.seed[k][2], hb.seed[k][3]);
  const uint64_t index = hb.index[k], own = index >> 4;
  const uint32_t pos = (uint32_t)(index & 15);
  const uint64_t nitems = (nrec + 15) / 16;
  uint8_t* const kbase = keys + (uint64_t)k * key_stride;
  for (int a = 0; a < nq; ++a) {
    __syncthreads();  // the tables are filled; the last round's stream keys are read
    if (tid < t) sk[tid] = aes_ctr_block_be32(T, seed, (uint32_t)(a * t + tid));
    __syncthreads();
    for (uint64_t item = (uint64_t)blockIdx.x * 256 + tid; item < nitems;
         item += (uint64_t)gridDim.x * 256) {
      uint4 acc[kHollantiMaxParties];
      const uint4 top = aes_ctr_block_be32(T, sk[t - 1], (uint32_t)item);
#pragma unroll
      for (int q = 0; q < kHollantiMaxParties; ++q) acc[q] = top;
      for (int m = t - 2; m >= 0; --m) {
        const uint4 r = aes_ctr_block_be32(T, sk[m], (uint32_t)item);
#pragma unroll
        for (int q = 0; q < kHollantiMaxParties; ++q)
          if (q < p) acc[q] = xor4(gf_mul_const4_w(acc[q], (uint32_t)(q + 1)), r);
      }
      if (item == own) {  // the secret term: one record of one lane
#pragma unroll
        for (int q = 0; q < kHollantiMaxParties; ++q)
          if (q < p) xor_byte(acc[q], pos, hb.secpow[a][q]);
      }
      const uint64_t x0 = 16 * item;
      const int cnt = (int)(nrec - x0 < 16 ? nrec - x0 : 16);
#pragma unroll
      for (int q = 0; q < kHollantiMaxParties; ++q) {
        uint8_t* dst = kbase + (uint64_t)q * party_stride + (uint64_t)a * coef_pitch + x0;
        if (q >= p) {
        } else if (cnt == 16 && ((uintptr_t)dst & 15) == 0) {
          *reinterpret_cast<uint4*>(dst) = acc[q];
        } else {
#pragma unroll
          for (int b = 0; b < 16; ++b)
            if (b < cnt) dst[b] = (uint8_t)tr_byte(acc[q], b);
        }
      }
    }
  }
}

hipError_t launch_hollanti_keys(const HollantiBatch& hb, int num_keys, uint64_t num_records, int t,
                                int p, int nq, uint8_t* d_keys, uint64_t coef_pitch,
                                uint64_t key_stride, uint64_t party_stride, hipStream_t s) {
  if (num_keys < 1 || num_keys > kHollantiBatch || t < 1 || t > 254 || p < 1 ||
      p > kHollantiMaxParties || nq < 1 || nq > kHollantiMaxRounds || num_records == 0 ||
      num_records > (1ull << 36) || coef_pitch < num_records)
    return hipErrorInvalidValue;
  const uint64_t nitems = (num_records + 15) / 16;
  // every block fills the 64 KiB AES tables once, and two blocks fit a CU's LDS: one resident
  // set of blocks over all the keys of the launch, the items strided
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return hipErrorInvalidDevice;
  const uint64_t per_key = std::max<uint64_t>(1, (2 * (uint64_t)cus + num_keys - 1) / num_keys);
  const dim3 grid((unsigned)std::min<uint64_t>((nitems + 255) / 256, per_key), (unsigned)num_keys);
  hipLaunchKernelGGL(k_hollanti_keys, grid, dim3(256), 0, s, hb, num_records, t, p, nq, d_keys,
                     coef_pitch, key_stride, party_stride);
  return hipGetLastError();
}

}  // namespace pir
