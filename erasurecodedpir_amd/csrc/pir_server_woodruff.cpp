// pir_server_woodruff.cpp -- the Woodruff mode (mode 5) of the pir_server.h shim:
// runWoodruffQueryThread (src/c/server.cpp:564-645) on the engine's pair-product scan
// (pir_engine_answer_woodruff, or with WOODRUFF_DERIVATIVE pir_engine_answer_woodruff_deriv)
// from the device-resident shard.  A unit of its own because pir_server.cpp must link without
// the engine entry points this mode added (pir_server_internal.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pir_server_internal.h"

namespace {

// records [startIndex, endIndex) -> result[0], ENCODED_FILE_SIZE_BYTES bytes, and with
// WOODRUFF_DERIVATIVE result[1 .. WOODRUFF_M] too (all overwritten: DESIGN.md, reference
// defects).  The whole domain is one call of the engine (its single-launch path where the
// policy picks it), a Thread slice one coefficient kernel + scan over its own range: the T
// ranges of a query are one pass over the shard in total.  isByzantine changes nothing in the
// reference, and nothing here.
void run_thread(server* s, uint8_t* key, int threadNum, int startIndex, int endIndex,
                uint8_t** result) {
  (void)threadNum;
  if (MODE != 5) {
    fprintf(stderr, "pir shim: runWoodruffQueryThread needs a Woodruff setup (setSystemParams "
                    "mode 5); the mode is %d\n", MODE);
    abort();
  }
  if (startIndex < 0 || endIndex < startIndex || endIndex > NUM_ENCODED_FILES) {
    fprintf(stderr, "pir shim: records [%d,%d) outside [0,%d)\n", startIndex, endIndex,
            NUM_ENCODED_FILES);
    abort();
  }
  if (WOODRUFF_DERIVATIVE) {
    const size_t efs = (size_t)ENCODED_FILE_SIZE_BYTES;
    std::vector<uint8_t> out((size_t)(WOODRUFF_M + 1) * efs);
    pir_shim::with_engine(s, 1, [&](pir_engine_t* e) {
      if (pir_engine_answer_woodruff_deriv(e, key, (uint64_t)WOODRUFF_M, (uint64_t)startIndex,
                                           (uint64_t)(endIndex - startIndex), out.data()) != PIR_OK)
        pir_shim::engine_failure("runWoodruffQueryThread");
    });
    for (int j = 0; j <= WOODRUFF_M; ++j) memcpy(result[j], out.data() + (size_t)j * efs, efs);
    return;
  }
  pir_shim::with_engine(s, 1, [&](pir_engine_t* e) {
    if (pir_engine_answer_woodruff(e, key, (uint64_t)WOODRUFF_M, (uint64_t)startIndex,
                                   (uint64_t)(endIndex - startIndex), result[0]) != PIR_OK)
      pir_shim::engine_failure("runWoodruffQueryThread");
  });
}

const pir_shim::WoodruffHooks kHooks = {run_thread, pir_engine_woodruff_pair};

struct RegisterHooks {
  RegisterHooks() { pir_shim::g_woodruff = &kHooks; }
} g_register;

}  // namespace
