// pir_server_internal.h -- the seam between pir_server.cpp and the translation units that add
// modes to the shim (pir_server_shamir.cpp, _woodruff, _mac, _hollanti).  Not part of the C ABI.
//
// pir_server.cpp names no engine entry point newer than its own modes need, so that it links
// against a stub of the engine (tests/tsan); a mode's unit reaches the server's engine through
// with_engine and hands pir_server.cpp what its setup needs through the hooks below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>

#include "../../include/pir_engine.h"
#include "../../include/pir_server.h"

namespace pir_shim {

// fn(engine) under the server's lock, the engine made for nq rounds and holding the server's
// current rows (what every query entry point of pir_server.cpp does first)
void with_engine(server* s, int nq, const std::function<void(pir_engine_t*)>& fn);
// "pir engine failure in <what>: <last error>" and abort (the reference's handleErrors())
[[noreturn]] void engine_failure(const char* what);
// the device the shim's engines and client helpers use (pirSetDevice, $PIR_DEVICE or 0)
int device();

// The Hermite half of encode_within_files_server's GPU setup: pir_engine_encode_hermite_rows,
// registered by pir_server_shamir.cpp when it is linked (nullptr otherwise: the setup refuses).
using HermiteEncodeFn = int (*)(pir_engine_t*, const uint8_t* const* files, uint64_t num_files,
                                uint32_t file_bytes, int k, int party);
extern HermiteEncodeFn g_encode_hermite;

// The Woodruff mode (mode 5): runWoodruffQueryThread's answers on the engine (value, or with
// WOODRUFF_DERIVATIVE the M + 1 derivative answers) and the record -> pair map genWoodruffQuery
// needs (pir_engine_woodruff_pair), registered by
// pir_server_woodruff.cpp when it is linked (nullptr otherwise: the Woodruff entry points abort).
struct WoodruffHooks {
  void (*run_thread)(server* s, uint8_t* key, int threadNum, int startIndex, int endIndex,
                     uint8_t** result);
  int (*pair)(uint32_t m, uint64_t i, uint32_t* a, uint32_t* b);
};
extern const WoodruffHooks* g_woodruff;

// generateHollantiQuery on the GPU (pir_gen_hollanti_keys), set by pirClientHollantiKeygenOnGpu
// of pir_server_hollanti.cpp (nullptr, the default: the host loop of pir_server.cpp).
using HollantiKeygenFn = void (*)(int index, uint8_t*** keys);
extern HollantiKeygenFn g_hollanti_keygen;
// the OS CSPRNG as pir_server.cpp draws key seeds (aborts on failure)
void random_bytes(uint8_t* buf, size_t len);

}  // namespace pir_shim
