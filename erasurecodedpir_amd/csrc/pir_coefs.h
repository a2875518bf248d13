// pir_coefs.h -- internal: explicit-coefficient answers (the Hollanti/Goldberg polynomial-PIR
// server scan, src/c/server.cpp:321-382).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pir {

// d_c[i * nrp + a] = a < nq ? src[a * src_pitch + i] : 0 for i < nrows: the client's per-round
// coefficient vectors (one row of N bytes per round) interleaved into the record-major share
// layout the GF(2^8) scan kernels read (coefficient bytes of record i at d_c + i * nrp)
hipError_t launch_interleave_coefs(const uint8_t* src, uint64_t src_pitch, uint64_t nrows, int nq,
                                   int nrp, uint8_t* d_c, hipStream_t s);

// The vectors of a group of ng queued keys as one W-byte share row per record (W = 2, 4 or 8; W
// >= ng * nrp): d_c[i * W + g * nrp + a] = src[g * key_stride + a * coef_pitch + i] for g < ng and
// a < nq, zero for every other byte, i < nrows.  d_c 16-byte aligned; the vectors may have any
// alignment (an aligned one is read with 16-byte loads).
hipError_t launch_interleave_coefs_g(const uint8_t* src, uint64_t coef_pitch, uint64_t key_stride,
                                     int ng, int nq, int nrp, int W, uint64_t nrows, uint8_t* d_c,
                                     hipStream_t s);

// The Hollanti-mode shard, encoded within files on the GPU (client.cpp:43-56, 99-103; the
// shim's encode_within_files_server): row r (file r, r < num_files; rows past are zero) =
// XOR_{j<k} gf_pow(party, j) * part j of file r, part j = bytes [j*efs, (j+1)*efs) of the
// file zero-padded past file_bytes.  d_files: num_files rows file_pitch apart, or nullptr for
// the reference's synthetic database (client.cpp:16-33: file v = the byte v & 0xff, file 1 =
// 0, 1, 2, ...).  Rows [row0, row0 + rows) of the global encoded database.
hipError_t launch_encode_within(const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                                uint32_t file_bytes, int k, int party, uint8_t* d_shard,
                                uint64_t rows, uint64_t row0, uint32_t pitch, uint32_t efs,
                                hipStream_t s);

// The Shamir mode's derivative ("Hermite") rows (client.cpp:57-68, 103-107): row r = XOR over odd
// j, 1 <= j < k, of gf_pow(party, j - 1) * part j of file r; otherwise as launch_encode_within.
hipError_t launch_encode_hermite(const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                                 uint32_t file_bytes, int k, int party, uint8_t* d_shard,
                                 uint64_t rows, uint64_t row0, uint32_t pitch, uint32_t efs,
                                 hipStream_t s);

// The client's Hollanti coefficient vectors (pir_gen_hollanti_keys_dev, include/pir_client.h: the
// key stream) for up to kHollantiBatch keys in one launch, the keys' seeds and indices and the
// secret term's factors by value in the kernel arguments (nothing to stage or free).
constexpr int kHollantiBatch = 16;
constexpr int kHollantiMaxParties = 17;  // PIR_MAX_PARTIES
constexpr int kHollantiMaxRounds = 16;   // PIR_MAX_ROUNDS
struct HollantiBatch {
  uint32_t seed[kHollantiBatch][4];  // little-endian words of the 16 seed bytes
  uint64_t index[kHollantiBatch];
  uint8_t secpow[kHollantiMaxRounds][kHollantiMaxParties + 3];  // (q+1)^(t + (a+1) rho - 1)
};
// party q, key k, round a, record x -> d_keys[q*party_stride + k*key_stride + a*coef_pitch + x],
// x < num_records; no byte at or past num_records of a vector is written
hipError_t launch_hollanti_keys(const HollantiBatch& hb, int num_keys, uint64_t num_records, int t,
                                int p, int nq, uint8_t* d_keys, uint64_t coef_pitch,
                                uint64_t key_stride, uint64_t party_stride, hipStream_t s);

}  // namespace pir
