// pir_server_mac.cpp -- pirClientTagFiles of the pir_server.h shim: the CheckMAC tags
// (client.cpp:29-31) of a caller's own database, recomputed on the GPU by pir_mac_files_rows.
// A unit of its own because pir_server.cpp must link without the entry points newer than its
// own modes (pir_server_internal.h).
#include <stdio.h>
#include <stdlib.h>

#include "../../include/pir_client.h"
#include "pir_server_internal.h"

extern "C" void pirClientTagFiles(client* c) {
  if (!CHECK_MAC) {
    fprintf(stderr, "pir shim: pirClientTagFiles needs a CheckMAC setup (setSystemParams "
                    "checkMac = 1)\n");
    abort();
  }
  if (!c || !c->unencoded_files || !c->macKey) {
    fprintf(stderr, "pir shim: pirClientTagFiles needs an initialised client\n");
    abort();
  }
  const int rc = pir_mac_files_rows(pir_shim::device(), c->unencoded_files, (uint64_t)NUM_FILES,
                                    PAYLOAD_SIZE_BYTES, c->macKey);
  if (rc != PIR_OK) {
    fprintf(stderr, "pir shim: pirClientTagFiles: pir_mac_files_rows failed (%d)\n", rc);
    abort();
  }
}
