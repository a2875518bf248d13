// pir_scan_t.hip -- the many-round GF(2^8) scan as a transposed four-Russians fold (k_scan_t).
//
// The answer of round a is ans_a = sum_i c_a[i] * x_i over GF(2^8) (server.cpp:121-127).  Over
// bit planes (coding.cpp:9-21, poly 0x11d): ans_a = sum_b alpha^b Z_{a,b}, Z_{a,b} = XOR of the
// rows whose round-a coefficient has bit b set.  With one record per wave row the coefficient
// word w_i (the record's NRP <= 8 coefficient bytes, round a = byte a, as 64 bits: plane
// p = 8a + b) is wave-uniform, and the scans of pir_kernels.hip select each plane's row
// combination by GPR index (pir_m4r.h): one index switch per plane per 4 rows, whose cost grows
// with the number of planes (2.2 TB/s at 64 planes, 3.4 at 40: profiles/r02_micro/).
//
// Here the roles are swapped: the index comes from the shard's bits, the table from the
// coefficients.  For every 4 consecutive rows of a wave's 64-row chunk the wave keeps in LDS the
// 16 XOR combinations of the rows' coefficient words, T_t[v] = XOR_{r: bit r of v} w_{4t+r}: 16
// tables per chunk, each aligned to its own size (128 B of 8-byte entries), so that every entry
// has banks of its own and any set of indices reads without a bank conflict.  Per lane and 8
// rows, bit j of rows 0-3 and of rows 4-7 forms two 4-bit indices (4 x 32 bit transposes of the
// rows, pir_bits.h), and for every bit position j: Zt[j] ^= T_lo[n_j] ^ T_hi[n'_j] -- two
// ds_read_b64 and two v_bitop3 (XOR3) -- where Zt[j] (64 bits) is bit j of the lane's dword in
// every plane at once.  The cost per row does not depend on the number of planes (up to 64), and
// no scalar index setting is left in the loop.  At the end Zt is transposed back to planes (32 x
// 32 bit transposes) and folded by the alpha powers as in k_scan_uni; slabs and k_reduce are
// unchanged.  (One 256-entry table per 8 rows, the first form, spent 63 % of its LDS cycles on
// bank conflicts and rebuilt the table every 8 rows: DESIGN.md, Transposed four-Russians scan.)
//
// One record per wave row at one dword per lane (pitch >= 256 B; column groups of 64 dwords
// along grid y), NRP = 4 or 8 coefficient bytes per record (NQ <= NRP rounds), rows of a wave
// through one buffer resource with the row offset in soffset (< 2^31 B of rows per wave: host).
//
// The fold itself -- the table build, the pipelined 8-row step, the way back to planes -- is
// pir_seg_walk.h's fr_walk and planes_out, shared with the segment kernels of pir_shamir_q.hip
// and pir_woodruff_q.hip.  Here are what is k_scan_t's own: the row loads, the coefficient gather
// (record- or key-major), the chunk claims, red[] and the slabs, and the launch.
#include <stdlib.h>

#include <algorithm>
#include "pir_kernels.h"
#include "pir_seg_walk.h"

namespace pir {

constexpr int kScanTWaves = kScanTThreads / 64;

// The fold image of rows [0, nrows) of `shard` (pir_bits.h: fold_image4): lane = one dword column
// of one block of 4 rows, 4 dword loads and one 16-byte store at block * 4 * pitch + 16 * column;
// the rows past nrows of the last block count as zero.  Grid x = blocks, y = column groups of 256
__global__ __launch_bounds__(256) void k_fold_image(const uint8_t* __restrict__ shard,
                                                    uint64_t nrows, uint32_t pitch,
                                                    uint8_t* __restrict__ image) {
  const uint32_t col = blockIdx.y * 256 + threadIdx.x;
  if (col >= pitch / 4) return;
  const uint64_t blocks = (nrows + 3) / 4;
  for (uint64_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    uint32_t x[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint64_t row = 4 * blk + r;
      x[r] = row < nrows ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(
                               shard + row * pitch) + col)
                         : 0u;
    }
    fold_image4(x);
    *reinterpret_cast<uint4*>(image + blk * 4 * pitch + 16ull * col) =
        make_uint4(x[0], x[1], x[2], x[3]);
  }
}

// IMG: `shard` is the fold image of the rows (k_fold_image), the first of them a multiple of 4 in
// the image's row numbering: block loads of 16 bytes per lane, no transposes in the loop.  The
// waves' (workgroups') row ranges start on multiples of 4
template <int NQ, int NRP, bool IMG>
__global__ __launch_bounds__(kScanTThreads) __attribute__((amdgpu_waves_per_eu(kScanTWavesPerEU)))
void k_scan_t(const uint8_t* __restrict__ shard, uint64_t nrec, uint32_t pitch, uint32_t cpr,
              const uint8_t* __restrict__ c, uint8_t* __restrict__ slabs, int accumulate,
              uint32_t ckey, uint64_t ckoff) {
  static_assert(NRP == 4 || NRP == 8, "coefficient words of 32 or 64 bits");
  static_assert(NQ >= 1 && NQ <= NRP, "rounds");
  constexpr int WD = NRP / 4;  // coefficient words per record (rounds 0-3, 4-7)
  constexpr int GW = kColGroupLanes;
  __shared__ alignas(128) uint32_t tab[kScanTWaves][FrTab<WD>::kWords];  // each wave's tables
  __shared__ uint32_t red[NQ * GW];
  __shared__ uint32_t next_chunk;
  for (int i = threadIdx.x; i < NQ * GW; i += blockDim.x) red[i] = 0;
  // accumulate bit 1 (launch_scan_t, $PIR_SCAN_DYN): the waves claim 64-row chunks of the
  // workgroup's rows (as k_scan_uni: equal-priority waves issue oldest first, so fixed ranges
  // leave the youngest waves folding the tail alone)
  const bool dyn = (accumulate >> 1) & 1;
  accumulate &= 1;

  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t wave = (uint64_t)blockIdx.x * kScanTWaves + wv;
  const uint64_t nwaves = (uint64_t)gridDim.x * kScanTWaves;
  const uint32_t chunk = blockIdx.y * kColGroupLanes + lane;
  const bool active = chunk < cpr;
  // the wave's rows, or (dyn) the workgroup's
  // (IMG: every boundary but the last rounded down to a block of 4 rows)
  auto bound = [&](uint64_t i) __attribute__((always_inline)) {
    const uint64_t r = i * nrec / nwaves;
    return IMG && i < nwaves ? r & ~(uint64_t)3 : r;
  };
  const uint64_t r0 = bound(dyn ? (uint64_t)blockIdx.x * kScanTWaves : wave);
  const uint64_t r1 = bound(dyn ? ((uint64_t)blockIdx.x + 1) * kScanTWaves : wave + 1);
  if (dyn) {
    if (threadIdx.x == 0) next_chunk = 0;
    __syncthreads();
  }

  uint32_t Zt[32][WD] = {};  // a wave without rows adds nothing
  if (r1 > r0) {
    const uint32_t nrows = (uint32_t)(r1 - r0);
    // (IMG: whole blocks of 4 rows, block b of the wave's at b * 4 * pitch, the lane's 16 bytes
    // at 16 * chunk)
    const uint32_t nspan = IMG ? (nrows + 3u) & ~3u : nrows;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(shard + r0 * pitch), (short)0, (int)(nspan * pitch), kBufRsrcWord3);
    const uint32_t voff = (active ? chunk : 0u) * (IMG ? 16u : 4u);  // inactive lanes: column 0
    auto load = [&](uint32_t rel) __attribute__((always_inline)) {
      if constexpr (IMG) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, rel * 4u * pitch, 2);
        return make_uint4(v.x, v.y, v.z, v.w);
      } else {
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, voff, rel * pitch, 2);
      }
    };
    // lane l: the coefficient words of row rb + l (zero past the wave's rows); key-major
    // coefficients (ckey bytes per key) are gathered key by key: one ckey-byte load per key,
    // coalesced across the wave's 64 rows
    auto coefs64 = [&](uint32_t rb) __attribute__((always_inline)) {
      const uint32_t rl = rb + lane;
      uint2 cw = make_uint2(0, 0);
      if (rl < nrows) {
        const uint64_t row = r0 + rl;
        if (ckey == 0) {
          const uint8_t* p = c + row * NRP;
          if constexpr (NRP == 8) cw = *reinterpret_cast<const uint2*>(p);
          else cw.x = *reinterpret_cast<const uint32_t*>(p);
        } else {
          uint64_t w = 0;
          for (uint32_t g = 0; g * ckey < (uint32_t)NRP; ++g) {
            const uint8_t* p = c + g * ckoff + row * ckey;
            const uint64_t v = ckey == 1 ? *p : (ckey == 2 ? *reinterpret_cast<const uint16_t*>(p)
                                                           : *reinterpret_cast<const uint32_t*>(p));
            w |= v << (8 * g * ckey);
          }
          cw = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
        }
      }
      return cw;
    };
    // chunk claims (dyn): the wave folds the chunks it claims from the workgroup's counter
    const uint32_t nch = (nrows + 63) / 64;
    auto claim = [&]() __attribute__((always_inline)) -> uint32_t {
      uint32_t v = 0;
      if (lane == 0)
        v = __hip_atomic_fetch_add(&next_chunk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return (uint32_t)__builtin_amdgcn_readfirstlane(v);
    };
    fr_walk<WD, IMG>(
        nrows, load, coefs64, dyn ? claim() : 0u,
        [&](uint32_t cur) __attribute__((always_inline)) {
          return dyn ? (cur < nch ? claim() : nch) : cur + 1;
        },
        lane, &tab[wv][0], Zt);
  }
  __syncthreads();  // red[] zeroed
  if (active)
    planes_out<WD, NQ>(Zt, [&](int a, uint32_t acc) __attribute__((always_inline)) {
      if (acc) atomicXor(&red[a * GW + lane], acc);
    });
  __syncthreads();
  uint32_t* slab = reinterpret_cast<uint32_t*>(slabs) +
                   ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * (NQ * GW);
  if (accumulate)
    for (int i = threadIdx.x; i < NQ * GW; i += blockDim.x) slab[i] ^= red[i];
  else
    for (int i = threadIdx.x; i < NQ * GW; i += blockDim.x) slab[i] = red[i];
}

// $PIR_SCAN_T: 0 = never, 2 = every 4-8 round shape it can take (diagnostics), else the default
static int scan_t_mode() {  // read per plan (tests switch it within one process)
  const char* v = getenv("PIR_SCAN_T");
  return v ? atoi(v) : 1;
}
bool scan_t_enabled() { return scan_t_mode() != 0; }

// 6-8 rounds (64 and 48 planes: 3.9 TB/s against 2.2 for the GPR-index fold at configs[2]'s
// 8); 4-5 rounds only for records narrower than a VEC = 2 wave row (the 768-thread GPR-index
// k_scan_uni at two dwords per lane is faster there: Hollanti 5 rounds at 1 KiB 4.53 against
// 4.91 ms, profiles/r03_bench_ch5_*.json)
bool scan_t_shape(int nq, int nrp, uint32_t pitch, bool prefer) {
  if (!scan_t_enabled() || nq < 4 || nq > 8 || nq > nrp || (nrp != 4 && nrp != 8)) return false;
  if (pitch % 4 != 0 || pitch / 4 < (uint32_t)kColGroupLanes) return false;
  return nq >= 6 || pitch / 8 < (uint32_t)kColGroupLanes || prefer || scan_t_mode() == 2;
}

template <int NQ, int NRP>
static hipError_t scan_t_launch(const ScanShape& sh, const uint8_t* d_shard, uint64_t nrec,
                                const uint8_t* d_c, uint8_t* d_slabs, int acc, hipStream_t s,
                                const uint8_t* d_image) {
  if (sh.ckey != 0 && (sh.ckey > 4 || NRP % sh.ckey != 0)) return hipErrorInvalidValue;
  if (d_image)
    hipLaunchKernelGGL((k_scan_t<NQ, NRP, true>), sh.grid, dim3(kScanTThreads), 0, s, d_image,
                       nrec, sh.pitch, sh.cpr, d_c, d_slabs, acc, sh.ckey, sh.ckoff);
  else
    hipLaunchKernelGGL((k_scan_t<NQ, NRP, false>), sh.grid, dim3(kScanTThreads), 0, s, d_shard,
                       nrec, sh.pitch, sh.cpr, d_c, d_slabs, acc, sh.ckey, sh.ckoff);
  return hipGetLastError();
}

hipError_t launch_scan_t(const ScanShape& sh, const uint8_t* d_shard, uint64_t nrec,
                         const uint8_t* d_c, uint8_t* d_slabs, int acc, hipStream_t s,
                         const uint8_t* d_image) {
  if (sh.threads != kScanTThreads || sh.vec != 1 || !sh.uniform) return hipErrorInvalidValue;
  if (d_image && (sh.pitch % 16 != 0 || ((uintptr_t)d_image & 15) != 0)) return hipErrorInvalidValue;
#define PIR_ST(NQ, NRP) \
  if (sh.nq == NQ && sh.nrp == NRP) return scan_t_launch<NQ, NRP>(sh, d_shard, nrec, d_c, d_slabs, acc, s, d_image)
  PIR_ST(4, 4); PIR_ST(4, 8); PIR_ST(5, 8); PIR_ST(6, 8); PIR_ST(7, 8); PIR_ST(8, 8);
#undef PIR_ST
  return hipErrorInvalidValue;
}

hipError_t launch_fold_image(const uint8_t* d_shard, uint64_t nrows, uint32_t pitch,
                             uint8_t* d_image, hipStream_t s) {
  if (pitch % 16 != 0 || nrows == 0) return hipErrorInvalidValue;
  const uint64_t blocks = (nrows + 3) / 4;
  const dim3 grid((unsigned)std::min<uint64_t>(blocks, 1u << 20), (pitch / 4 + 255) / 256);
  hipLaunchKernelGGL(k_fold_image, grid, dim3(256), 0, s, d_shard, nrows, pitch, d_image);
  return hipGetLastError();
}

}  // namespace pir
