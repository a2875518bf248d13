// pir_server_shamir.cpp -- the Shamir sqrt(N) mode (mode 2) of the pir_server.h shim:
// runOptShamirDPFQuery / runOptShamirDPFQueryThread (src/c/server.cpp:203-302) answered by the
// engine's row/column scan (pir_engine_answer_shamir) from the device-resident value and Hermite
// rows.  A unit of its own because pir_server.cpp must link without the engine entry points
// this mode added (pir_server_internal.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <random>
#include <vector>

#include "pir_server_internal.h"

namespace {

// encode_within_files_server's Hermite rows on the GPU
struct RegisterHooks {
  RegisterHooks() { pir_shim::g_encode_hermite = pir_engine_encode_hermite_rows; }
} g_register;

void need_mode(const char* fn) {
  if (MODE != 2 || !IS_HERMITE) {
    fprintf(stderr, "pir shim: %s needs a Shamir setup (setSystemParams mode 2 after "
                    "pirEnableShamirMode(1)); the mode is %d\n", fn, MODE);
    abort();
  }
}

// records [rec0, rec0 + nrec) of the domain -> result[a], a < NUM_ROUNDS, response_len bytes
void answer(server* s, uint8_t** keys, uint64_t rec0, uint64_t nrec, uint8_t** result,
            const char* fn) {
  const size_t len = (size_t)calcShamirResponseLength(LOG_NUM_ENCODED_FILES, ENCODED_FILE_SIZE_BYTES);
  std::vector<uint8_t> out((size_t)NUM_ROUNDS * len);
  pir_shim::with_engine(s, NUM_ROUNDS, [&](pir_engine_t* e) {
    if (pir_engine_answer_shamir(e, keys, rec0, nrec, out.data()) != PIR_OK)
      pir_shim::engine_failure(fn);
  });
  for (int a = 0; a < NUM_ROUNDS; ++a) memcpy(result[a], out.data() + a * len, len);
}

}  // namespace

extern "C" {

// server.cpp:203-239: random answers for a Byzantine server, else every record
void runOptShamirDPFQuery(server* s, uint8_t** keys, uint8_t** result) {
  need_mode("runOptShamirDPFQuery");
  if (s->isByzantine) {  // gen_rand_bytes (server.cpp:215-218)
    const size_t len =
        (size_t)calcShamirResponseLength(LOG_NUM_ENCODED_FILES, ENCODED_FILE_SIZE_BYTES);
    static std::mutex rmu;
    static std::mt19937_64 rng{std::random_device{}()};
    std::lock_guard<std::mutex> lk(rmu);
    for (int a = 0; a < NUM_ROUNDS; ++a)
      for (size_t j = 0; j < len; ++j) result[a][j] = (uint8_t)rng();
    return;
  }
  answer(s, keys, 0, (uint64_t)NUM_ENCODED_FILES, result, "runOptShamirDPFQuery");
}

// server.cpp:241-302: records [startIndex, endIndex) (both of the reference's branches compute
// the honest answer).  Every call is one pass over its own range: the T ranges of a query are
// one pass over the shard in total, so no slice group is kept.
void runOptShamirDPFQueryThread(server* s, uint8_t** keys, int threadNum, int startIndex,
                                int endIndex, uint8_t** result) {
  (void)threadNum;
  need_mode("runOptShamirDPFQueryThread");
  if (startIndex < 0 || endIndex < startIndex || endIndex > NUM_ENCODED_FILES) {
    fprintf(stderr, "pir shim: records [%d,%d) outside [0,%d)\n", startIndex, endIndex,
            NUM_ENCODED_FILES);
    abort();
  }
  answer(s, keys, (uint64_t)startIndex, (uint64_t)(endIndex - startIndex), result,
         "runOptShamirDPFQueryThread");
}

}  // extern "C"
