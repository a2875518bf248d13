// pir_client.hip -- client side: DPF key generation on the GPU (include/pir_client.h).
//
// genOptimizedDPF (dpf_tree.cpp:142-274) walks the p parties' seeds down the path of `index`:
// at each level every party's node is expanded (3 AES-CTR blocks = 3 lanes), the correction
// words are formed from the LOSE children, and each party keeps its KEEP child corrected by
// the CWs its control bits select.  One 64-lane workgroup: 3p <= 51 lanes expand, lane 0
// forms the CWs, every lane writes key bytes.
//
// The Hollanti coefficient vectors (pir_gen_hollanti_keys[_dev]) are here too: the argument
// checks, and k_hollanti_keys (pir_coefs.hip) launched once per 16 keys with their seeds and
// indices in the kernel arguments.
//
// The CheckMAC record tags (pir_mac_files_dev / _rows / pir_mac_check) are here too: the
// argument checks and the staging of host rows around k_hmac_sha256_files (pir_mac.hip).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

#include "../../include/pir_client.h"
#include "../../include/pir_engine.h"
#include "pir_aes.h"
#include "pir_coefs.h"
#include "pir_mac.h"

namespace pir {
namespace {

struct KeygenSmem {
  uint32_t tab[2 * 256 * 32];
  uint4 s[PIR_MAX_PARTIES];
  uint32_t t[PIR_MAX_PARTIES];
  uint4 out[PIR_MAX_PARTIES][3];
  uint4 scw[PIR_MAX_PARTIES];
  uint32_t tcw[PIR_MAX_PARTIES];
};

__device__ inline uint4 load_seed(const uint8_t* b) {
  uint32_t w[4];
  for (int i = 0; i < 4; ++i)
    w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ inline uint8_t byte_of(const uint4& v, int i) {
  const uint32_t w = i < 4 ? v.x : (i < 8 ? v.y : (i < 12 ? v.z : v.w));
  return (uint8_t)(w >> (8 * (i & 3)));
}

__global__ __launch_bounds__(64) void k_keygen(int n, uint64_t index, const uint8_t* __restrict__ fcw,
                                               int p, int nq, const uint8_t* __restrict__ seeds,
                                               uint8_t* __restrict__ keys, int kl) {
  __shared__ KeygenSmem sm;
  load_tables(sm.tab);
  const Tab T(sm.tab);
  const int tid = threadIdx.x, pm1 = p - 1, CWk = 16 + 2 * p - 2, CW = pm1 * CWk;
  const uint32_t tbits = 2 * pm1;
  const uint32_t tb_mask = tbits >= 32 ? 0xffffffffu : ((1u << tbits) - 1u);
  const uint32_t tmask = (1u << pm1) - 1u;
  if (tid < p) {
    sm.s[tid] = load_seed(seeds + 16 * tid);
    sm.t[tid] = tid >= 1 ? (1u << (tid - 1)) : 0u;  // dpf_tree.cpp:154-163
  }
  for (int i = tid; i < p * 16; i += blockDim.x) keys[(size_t)(i >> 4) * kl + (i & 15)] = seeds[i];
  __syncthreads();
  for (int L = 1; L <= n; ++L) {
    if (tid < 3 * p) {  // G(s[j]) for every party (dpf_tree.cpp:172-179)
      const int j = tid / 3, r = tid - 3 * j;
      sm.out[j][r] = aes_ctr_block(T, sm.s[j], (uint32_t)r);
    }
    __syncthreads();
    if (tid == 0) {
      const uint32_t bit = (uint32_t)((index >> (n - L)) & 1u);  // getbit(index, n, L)
      const int KEEP = (int)bit, LOSE = 1 - (int)bit;
      const uint32_t t0 = sm.out[0][2].x & tb_mask;
      for (int j = 0; j < pm1; ++j) {  // dpf_tree.cpp:189-204
        sm.scw[j] = xor4(sm.out[0][LOSE], sm.out[j + 1][LOSE]);
        const uint32_t tj = sm.out[j + 1][2].x & tb_mask;
        uint32_t m = (t0 ^ tj) & tb_mask;
        m ^= ((bit ^ 1u) << j) | (bit << (pm1 + j));
        sm.tcw[j] = m;
      }
      for (int b = 0; b < p; ++b) {  // dpf_tree.cpp:215-235
        uint4 ns = sm.out[b][KEEP];
        uint32_t nt = ((sm.out[b][2].x & tb_mask) >> (KEEP * pm1)) & tmask;
        for (int k = 0; k < pm1; ++k)
          if ((sm.t[b] >> k) & 1u) {
            ns = xor4(ns, sm.scw[k]);
            nt ^= (sm.tcw[k] >> (KEEP * pm1)) & tmask;
          }
        sm.s[b] = ns;
        sm.t[b] = nt;
      }
    }
    __syncthreads();
    // key bytes of this level for every party (dpf_tree.cpp:204-212, :254-262)
    for (int i = tid; i < p * CW; i += blockDim.x) {
      const int q = i / CW, o = i - q * CW, j = o / CWk, b = o - j * CWk;
      const uint8_t v = b < 16 ? byte_of(sm.scw[j], b) : (uint8_t)((sm.tcw[j] >> (b - 16)) & 1u);
      keys[(size_t)q * kl + 16 + (size_t)(L - 1) * CW + o] = v;
    }
    __syncthreads();
  }
  if (tid < p) sm.out[tid][0] = aes_ctr_block(T, sm.s[tid], 0u);  // convert (dpf_tree.cpp:238-244)
  __syncthreads();
  for (int i = tid; i < p * nq * pm1; i += blockDim.x) {  // lastCW (dpf_tree.cpp:246-251)
    const int q = i / (nq * pm1), o = i - q * (nq * pm1), a = o / pm1, j = o - a * pm1 + 1;
    const uint8_t v = fcw[a * pm1 + j - 1] ^ byte_of(sm.out[0][0], a) ^ byte_of(sm.out[j][0], a);
    keys[(size_t)q * kl + 16 + (size_t)n * CW + o] = v;
  }
}

uint8_t gf_mul_h(uint8_t a, uint8_t b) {
  uint8_t r = 0;
  while (b) {
    if (b & 1) r ^= a;
    a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1d : 0));
    b >>= 1;
  }
  return r;
}

static_assert(kHollantiMaxParties == PIR_MAX_PARTIES && kHollantiMaxRounds == PIR_MAX_ROUNDS,
              "k_hollanti_keys is unrolled for the engine's limits");

// every refusal of pir_gen_hollanti_keys[_dev] that needs no device (the strides apart)
bool hollanti_args_ok(uint64_t num_records, const uint64_t* indices, int num_keys, int t, int p,
                      int nq, int rho, const uint8_t* seeds, const uint8_t* out) {
  if (num_keys < 0 || t < 1 || t > 255 || nq < 1 || nq > PIR_MAX_ROUNDS || rho < 1 || rho > 255 ||
      p < 1 || p > PIR_MAX_PARTIES || t + rho * nq > 255 || num_records == 0 ||
      num_records > (1ull << 36))
    return false;
  if (num_keys > 0 && (!indices || !seeds || !out)) return false;
  for (int k = 0; k < num_keys; ++k)
    if (indices[k] >= num_records) return false;
  return true;
}

// the launches of a checked call: 16 keys each, asynchronous on s
int launch_hollanti(uint64_t num_records, const uint64_t* indices, int num_keys, int t, int p,
                    int nq, int rho, const uint8_t* seeds, uint8_t* d_keys, uint64_t coef_pitch,
                    uint64_t key_stride, uint64_t party_stride, hipStream_t s) {
  HollantiBatch hb{};
  for (int a = 0; a < nq; ++a)
    for (int q = 0; q < p; ++q) {
      uint8_t r = 1;  // (q + 1)^(t + (a + 1) rho - 1)
      for (int e = 0; e < t + (a + 1) * rho - 1; ++e) r = gf_mul_h(r, (uint8_t)(q + 1));
      hb.secpow[a][q] = r;
    }
  for (int k0 = 0; k0 < num_keys; k0 += kHollantiBatch) {
    const int nk = std::min(kHollantiBatch, num_keys - k0);
    for (int k = 0; k < nk; ++k) {
      memcpy(hb.seed[k], seeds + 16 * (size_t)(k0 + k), 16);  // little-endian words (load_seed)
      hb.index[k] = indices[k0 + k];
    }
    if (launch_hollanti_keys(hb, nk, num_records, t, p, nq, d_keys + (uint64_t)k0 * key_stride,
                             coef_pitch, key_stride, party_stride, s) != hipSuccess)
      return PIR_EHIP;
  }
  return PIR_OK;
}

// host threads that gather payloads and scatter tags ($PIR_GATHER_THREADS, as the engine's
// staged copies)
int host_threads() {
  if (const char* v = getenv("PIR_GATHER_THREADS")) return std::max(1, atoi(v));
  int n = (int)std::thread::hardware_concurrency();
  if (const char* v = getenv("OMP_NUM_THREADS")) n = std::min(n, std::max(1, atoi(v)));
  return std::max(1, std::min(8, n));
}

}  // namespace
}  // namespace pir

extern "C" {

void pir_final_cw(int p, int nq, int rho, uint8_t* out) {
  for (int a = 1; a <= nq; ++a)
    for (int j = 2; j <= p; ++j) {
      uint8_t r = 1;  // gf_pow(j, rho*a) with the exponent taken mod 256 as uint8_t (coding.cpp:46)
      const int e = (rho * a) & 0xff;
      for (int k = 0; k < e; ++k) r = pir::gf_mul_h(r, (uint8_t)j);
      out[(a - 1) * (p - 1) + (j - 2)] = (uint8_t)(r ^ 1);
    }
}

int pir_gen_keys(int device, int n, uint64_t index, const uint8_t* fcw, int p, int nq,
                 const uint8_t* root_seeds, uint8_t* keys_out) {
  if (!fcw || !root_seeds || !keys_out || p < 2 || p > PIR_MAX_PARTIES || nq < 1 ||
      nq > PIR_MAX_ROUNDS || n < 0 || n > PIR_MAX_LOG_RECORDS || (n < 64 && (index >> n) != 0))
    return PIR_EINVAL;
  const int kl = pir_engine_key_len(p, n, nq);
  if (hipSetDevice(device) != hipSuccess) return PIR_EHIP;
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return PIR_EHIP;
  uint8_t *d_fcw = nullptr, *d_seeds = nullptr, *d_keys = nullptr;
  int rc = PIR_OK;
  if (hipMalloc(&d_fcw, (size_t)nq * (p - 1)) != hipSuccess ||
      hipMalloc(&d_seeds, (size_t)p * 16) != hipSuccess ||
      hipMalloc(&d_keys, (size_t)p * kl) != hipSuccess) {
    rc = PIR_ENOMEM;
  } else if (hipMemcpyAsync(d_fcw, fcw, (size_t)nq * (p - 1), hipMemcpyHostToDevice, s) != hipSuccess ||
             hipMemcpyAsync(d_seeds, root_seeds, (size_t)p * 16, hipMemcpyHostToDevice, s) != hipSuccess) {
    rc = PIR_EHIP;
  } else {
    hipLaunchKernelGGL(pir::k_keygen, dim3(1), dim3(64), 0, s, n, index, d_fcw, p, nq, d_seeds,
                       d_keys, kl);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(keys_out, d_keys, (size_t)p * kl, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = PIR_EHIP;
  }
  if (d_fcw) (void)hipFree(d_fcw);
  if (d_seeds) (void)hipFree(d_seeds);
  if (d_keys) (void)hipFree(d_keys);
  (void)hipStreamDestroy(s);
  return rc;
}

int pir_gen_hollanti_keys_dev(int device, uint64_t num_records, const uint64_t* indices,
                              int num_keys, int t, int p, int nq, int rho, const uint8_t* seeds,
                              uint8_t* d_keys, uint64_t coef_pitch, uint64_t key_stride,
                              uint64_t party_stride, void* stream) {
  if (!pir::hollanti_args_ok(num_records, indices, num_keys, t, p, nq, rho, seeds, d_keys) ||
      coef_pitch < num_records || key_stride / (uint64_t)nq < coef_pitch ||
      (num_keys > 0 && party_stride / (uint64_t)num_keys < key_stride))
    return PIR_EINVAL;
  if (!num_keys) return PIR_OK;
  if (hipSetDevice(device) != hipSuccess) return PIR_EHIP;
  return pir::launch_hollanti(num_records, indices, num_keys, t, p, nq, rho, seeds, d_keys,
                              coef_pitch, key_stride, party_stride,
                              static_cast<hipStream_t>(stream));
}

int pir_gen_hollanti_keys(int device, uint64_t num_records, const uint64_t* indices, int num_keys,
                          int t, int p, int nq, int rho, const uint8_t* seeds, uint8_t* keys_out) {
  if (!pir::hollanti_args_ok(num_records, indices, num_keys, t, p, nq, rho, seeds, keys_out))
    return PIR_EINVAL;
  if (!num_keys) return PIR_OK;
  // device vectors at a pitch of whole 16-byte stores, copied back packed
  const uint64_t pitch = (num_records + 15) & ~15ull, rows = (uint64_t)p * num_keys * nq;
  if (hipSetDevice(device) != hipSuccess) return PIR_EHIP;
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return PIR_EHIP;
  uint8_t* d_keys = nullptr;
  int rc = PIR_OK;
  if (hipMalloc(&d_keys, (size_t)(rows * pitch)) != hipSuccess) {
    rc = PIR_ENOMEM;
  } else {
    rc = pir::launch_hollanti(num_records, indices, num_keys, t, p, nq, rho, seeds, d_keys, pitch,
                              nq * pitch, (uint64_t)num_keys * nq * pitch, s);
    if (rc == PIR_OK) {
      const hipError_t e =
          pitch == num_records
              ? hipMemcpyAsync(keys_out, d_keys, (size_t)(rows * pitch), hipMemcpyDeviceToHost, s)
              : hipMemcpy2DAsync(keys_out, num_records, d_keys, pitch, num_records, rows,
                                 hipMemcpyDeviceToHost, s);
      if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = PIR_EHIP;
    }
  }
  if (d_keys) (void)hipFree(d_keys);
  (void)hipStreamDestroy(s);
  return rc;
}

int pir_mac_files_dev(int device, const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                      uint32_t payload_bytes, const uint8_t key[16], uint8_t* d_tags,
                      uint64_t tag_pitch, void* stream) {
  if (!d_files || !d_tags || !key || payload_bytes == 0 || file_pitch < payload_bytes ||
      tag_pitch < PIR_MAC_BYTES)
    return PIR_EINVAL;
  if (!num_files) return PIR_OK;
  if (hipSetDevice(device) != hipSuccess) return PIR_EHIP;
  return pir::launch_hmac_sha256_files(d_files, file_pitch, num_files, payload_bytes,
                                       pir::hmac_states(key), d_tags, tag_pitch,
                                       static_cast<hipStream_t>(stream)) == hipSuccess
             ? PIR_OK
             : PIR_EHIP;
}

int pir_mac_files_rows(int device, uint8_t* const* files, uint64_t num_files,
                       uint32_t payload_bytes, const uint8_t key[16]) {
  if (!files || !key || payload_bytes == 0) return PIR_EINVAL;
  if (!num_files) return PIR_OK;
  uint64_t m = std::max<uint64_t>(1, (64ull << 20) / payload_bytes);
  if (const char* v = getenv("PIR_MAC_CHUNK_FILES")) m = std::max<uint64_t>(1, strtoull(v, nullptr, 10));
  m = std::min(m, num_files);
  const uint64_t nchunks = (num_files + m - 1) / m;
  const pir::HmacStates st = pir::hmac_states(key);
  if (hipSetDevice(device) != hipSuccess) return PIR_EHIP;
  // chunk c: host threads gather the payloads into pinned h_pay[c & 1]; copy, kernel and the copy
  // of the tags into pinned h_tag[c & 1] are enqueued; the tags of chunk c - 2 are scattered to
  // their files once that chunk's event has fired, before its buffers are reused
  hipStream_t s = nullptr;
  uint8_t *h_pay[2] = {}, *h_tag[2] = {}, *d_pay[2] = {}, *d_tag[2] = {};
  hipEvent_t done[2] = {};
  int rc = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? PIR_OK : PIR_EHIP;
  for (int i = 0; i < 2 && !rc; ++i)
    if (hipHostMalloc(&h_pay[i], (size_t)m * payload_bytes) != hipSuccess ||
        hipHostMalloc(&h_tag[i], (size_t)m * PIR_MAC_BYTES) != hipSuccess ||
        hipMalloc(&d_pay[i], (size_t)m * payload_bytes) != hipSuccess ||
        hipMalloc(&d_tag[i], (size_t)m * PIR_MAC_BYTES) != hipSuccess ||
        hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess)
      rc = PIR_ENOMEM;
  const int T = pir::host_threads();
  auto chunk_len = [&](uint64_t c) { return std::min(m, num_files - c * m); };
  auto on_rows = [&](uint64_t n, const std::function<void(uint64_t)>& fn) {
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t)
      th.emplace_back([&, t] {
        for (uint64_t i = n * t / T; i < n * (t + 1) / T; ++i) fn(i);
      });
    for (uint64_t i = 0; i < n / T; ++i) fn(i);
    for (auto& x : th) x.join();
  };
  auto scatter = [&](uint64_t c) {  // tags of chunk c -> files
    const int b = (int)(c & 1);
    if (hipEventSynchronize(done[b]) != hipSuccess) return PIR_EHIP;
    on_rows(chunk_len(c), [&](uint64_t i) {
      memcpy(files[c * m + i] + payload_bytes, h_tag[b] + i * PIR_MAC_BYTES, PIR_MAC_BYTES);
    });
    return PIR_OK;
  };
  for (uint64_t c = 0; c < nchunks && !rc; ++c) {
    const int b = (int)(c & 1);
    const uint64_t n = chunk_len(c);
    if (c >= 2 && (rc = scatter(c - 2))) break;
    on_rows(n, [&](uint64_t i) {
      memcpy(h_pay[b] + i * payload_bytes, files[c * m + i], payload_bytes);
    });
    if (hipMemcpyAsync(d_pay[b], h_pay[b], (size_t)n * payload_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
        pir::launch_hmac_sha256_files(d_pay[b], payload_bytes, n, payload_bytes, st, d_tag[b],
                                      PIR_MAC_BYTES, s) != hipSuccess ||
        hipMemcpyAsync(h_tag[b], d_tag[b], (size_t)n * PIR_MAC_BYTES, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipEventRecord(done[b], s) != hipSuccess)
      rc = PIR_EHIP;
  }
  for (uint64_t c = nchunks >= 2 ? nchunks - 2 : 0; c < nchunks && !rc; ++c) rc = scatter(c);
  if (s) (void)hipStreamSynchronize(s);
  for (int i = 0; i < 2; ++i) {
    if (h_pay[i]) (void)hipHostFree(h_pay[i]);
    if (h_tag[i]) (void)hipHostFree(h_tag[i]);
    if (d_pay[i]) (void)hipFree(d_pay[i]);
    if (d_tag[i]) (void)hipFree(d_tag[i]);
    if (done[i]) (void)hipEventDestroy(done[i]);
  }
  if (s) (void)hipStreamDestroy(s);
  return rc;
}

int pir_mac_check(const uint8_t* record, uint32_t payload_bytes, const uint8_t key[16]) {
  if (!record || !key || payload_bytes == 0) return PIR_EINVAL;
  uint8_t tag[PIR_MAC_BYTES];
  pir::hmac_sha256_host(pir::hmac_states(key), record, payload_bytes, tag);
  uint32_t diff = 0;
  for (int i = 0; i < PIR_MAC_BYTES; ++i) diff |= (uint32_t)(tag[i] ^ record[payload_bytes + i]);
  return diff ? 1 : 0;
}

}  // extern "C"
