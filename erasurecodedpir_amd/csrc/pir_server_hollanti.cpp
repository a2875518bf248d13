// pir_server_hollanti.cpp -- pirClientHollantiKeygenOnGpu of the pir_server.h shim:
// generateHollantiQuery's coefficient vectors (genHollantiDPF, shamir_dpf.cpp:190-237) made on
// the GPU by pir_gen_hollanti_keys under one fresh seed per query.  A unit of its own because
// pir_server.cpp must link without the entry points newer than its own modes
// (pir_server_internal.h): the hook it sets is the only seam.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/pir_client.h"
#include "pir_server_internal.h"

namespace {

void gen_on_gpu(int index, uint8_t*** keys) {
  const int p = NUM_PARTIES, nq = NUM_ROUNDS;
  const uint64_t N = (uint64_t)NUM_ENCODED_FILES;
  if (index < 0 || (uint64_t)index >= N) {
    fprintf(stderr, "pir shim: generateHollantiQuery: index %d outside [0,%d)\n", index,
            NUM_ENCODED_FILES);
    abort();
  }
  uint8_t seed[16];
  pir_shim::random_bytes(seed, sizeof seed);  // a seed is a secret of one query
  const uint64_t idx = (uint64_t)index;
  std::vector<uint8_t> out((size_t)p * nq * N);
  const int rc = pir_gen_hollanti_keys(pir_shim::device(), N, &idx, 1, T, p, nq, RHO, seed,
                                       out.data());
  if (rc != PIR_OK) {
    fprintf(stderr, "pir shim: generateHollantiQuery: pir_gen_hollanti_keys failed (%d)\n", rc);
    abort();
  }
  for (int q = 0; q < p; ++q)
    for (int a = 0; a < nq; ++a) memcpy(keys[q][a], out.data() + ((size_t)q * nq + a) * N, N);
}

}  // namespace

extern "C" void pirClientHollantiKeygenOnGpu(int on) {
  pir_shim::g_hollanti_keygen = on ? gen_on_gpu : nullptr;
}
