// pir_mac.h -- HMAC-SHA256 record tags (the reference's CheckMAC: client.cpp:29-31,
// utils.cpp:32-34): k_hmac_sha256_files on the device, the same hash on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pir {

// the SHA-256 state after the 64-byte (key ^ ipad) block and after the (key ^ opad) block:
// computed once per call on the host, passed to the kernel by value
struct HmacStates {
  uint32_t inner[8];
  uint32_t outer[8];
};
HmacStates hmac_states(const uint8_t key[16]);

// HMAC-SHA256(key[16], msg[0, len)) on the host
void hmac_sha256_host(const HmacStates& st, const uint8_t* msg, size_t len, uint8_t out[32]);

// tag i = HMAC(d_files + i * file_pitch, payload_bytes) -> d_tags + i * tag_pitch, 32 bytes
hipError_t launch_hmac_sha256_files(const uint8_t* d_files, uint64_t file_pitch, uint64_t num_files,
                                    uint32_t payload_bytes, const HmacStates& st, uint8_t* d_tags,
                                    uint64_t tag_pitch, hipStream_t s);

}  // namespace pir
