// pir_shamir.h -- internal: the Shamir sqrt(N) mode's row/column scan (runOptShamirDPFQuery /
// runOptShamirDPFQueryThread, src/c/server.cpp:203-319).  Not part of the C ABI.
//
// The N = 2^n value rows are a 2^x x 2^y matrix (x = ceil(n/2), y = n - x; record i sits at
// delta = i >> y, gamma = i & (2^y - 1)).  Round a's key is ky[delta] = key[a][delta],
// kx[gamma] = key[a][2^x + gamma]; its response is 2^x + 2^y + 2 records of efs bytes:
//   Rx[delta]  = XOR_gamma kx[gamma] * A[delta][gamma]      record delta
//   Ry[gamma]  = XOR_delta ky[delta] * A[delta][gamma]      record 2^x + gamma
//   tot1       = XOR kx[gamma] ky[delta] * H[delta][gamma]  record 2^x + 2^y
//   tot2       = XOR kx[gamma] ky[delta] * A[delta][gamma]  record 2^x + 2^y + 1
// restricted to the records [rec0, rec0 + nrec) of a Thread call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pir {

struct ShamirDims {
  int x, y;
  uint64_t X, Y;       // matrix rows (deltas), columns (gammas)
  uint64_t resp_len;   // (X + Y + 2) * efs: bytes of one round's response
};
ShamirDims shamir_dims(int n, uint32_t efs);

constexpr int kShamirRounds = 4;  // rounds per pass over the value rows (k_shamir_rows/_strips)

// Rounds [0, nr) of the keys at d_keys (round a at + a * key_pitch), nr <= kShamirRounds, over
// the records [lo, hi) of `vals` (N rows, pitch bytes apart); out: round a's response at
// + a * resp_len.  Rows pass: Rx of the deltas the range touches (the caller zeroes the others).
hipError_t launch_shamir_rows(const ShamirDims& d, const uint8_t* vals, uint32_t pitch,
                              uint32_t efs, const uint8_t* d_keys, uint64_t key_pitch, int nr,
                              uint64_t lo, uint64_t hi, uint8_t* out, hipStream_t s);
// Strips pass: Ry of every gamma.
hipError_t launch_shamir_strips(const ShamirDims& d, const uint8_t* vals, uint32_t pitch,
                                uint32_t efs, const uint8_t* d_keys, uint64_t key_pitch, int nr,
                                uint64_t lo, uint64_t hi, uint8_t* out, hipStream_t s);
// d_c[(i - lo) * nrp + a] = kx_a[gamma(i)] * ky_a[delta(i)] (a < nq; 0 for nq <= a < nrp): the
// record-major coefficients of the explicit-coefficient scan that gives tot1 from the Hermite rows
hipError_t launch_shamir_coefs(const ShamirDims& d, const uint8_t* d_keys, uint64_t key_pitch,
                               int nq, int nrp, uint64_t lo, uint64_t hi, uint8_t* d_c,
                               hipStream_t s);
// tot2[a] = XOR_delta ky_a[delta] * Rx_a[delta] from the finished row sums in `out`, and tot1[a]
// copied from tot1 (nq x efs bytes, the Hermite scan's answer)
hipError_t launch_shamir_totals(const ShamirDims& d, uint32_t efs, const uint8_t* d_keys,
                                uint64_t key_pitch, int nq, const uint8_t* tot1, uint8_t* out,
                                hipStream_t s);

// ---- queued keys: up to kShamirSlots virtual keys per pass (pir_shamir_q.hip) ----------------
// The rounds of the queued keys are independent virtual keys: virtual key v is round v % rounds
// of key v / rounds, at d_keys + (v / rounds) * key_stride + (v % rounds) * key_pitch (any
// alignment), and its response sits at out + v * resp_len.
constexpr int kShamirSlots = 8;
// the segmented pass takes records of at least one wave row (64 dwords)
bool shamir_seg_takes(uint32_t pitch);
// d_kT[j] (8-byte words, 8-byte aligned, X + Y of them): byte g = byte j of virtual key v0 + g
// for g < ng, zero above: kyT = d_kT[0, X), kxT = d_kT[X, X + Y)
hipError_t launch_shamir_key_table(const ShamirDims& d, const uint8_t* d_keys, uint64_t key_pitch,
                                   uint64_t key_stride, int rounds, int v0, int ng, uint8_t* d_kT,
                                   hipStream_t s);
// One value pass for the table's ng slots over the records [lo, hi): strided = false gives
// Rx[delta] (response record delta) of the deltas the range touches, strided = true Ry[gamma]
// (record X + gamma) of the gammas it touches; out = slot 0's response, which the caller zeroed.
hipError_t launch_shamir_seg(const ShamirDims& d, const uint8_t* vals, uint32_t pitch, uint32_t efs,
                             const uint8_t* d_kT, int ng, uint64_t lo, uint64_t hi, bool strided,
                             uint8_t* out, hipStream_t s);
// d_c + 8 (i - lo): byte g = kx_g[gamma_i] * ky_g[delta_i], the share rows of an 8-round
// explicit-coefficient scan of the Hermite rows; d_c 16-byte aligned
hipError_t launch_shamir_coefs_g(const ShamirDims& d, const uint8_t* d_kT, uint64_t lo, uint64_t hi,
                                 uint8_t* d_c, hipStream_t s);

}  // namespace pir
