// pir_engine_comm.cpp -- the split shard's communicator: attach / detach, the all-gather of the
// per-partition answers and their XOR fold (RCCL has no XOR reduction op).
#include <chrono>
#include <thread>

#include "pir_engine_internal.h"

using namespace eng;

namespace {

// The engine's communicators are non-blocking (ncclConfig_t.blocking = 0), so that a refused or
// stuck rank cannot hang the others inside ncclCommInitRank: a call may return ncclInProgress,
// settled here by polling ncclCommGetAsyncError, bounded by timeout_s.
ncclResult_t rccl_settle(ncclComm_t comm, ncclResult_t r, double timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  while (r == ncclInProgress) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      return ncclInProgress;
    std::this_thread::yield();
    if (ncclCommGetAsyncError(comm, &r) != ncclSuccess) return ncclSystemError;
  }
  return r;
}

// The split-shard combine after the all-gather: d_gather holds nranks blocks of `bytes`
// (rank r's partial answers at r * bytes -- ncclAllGather's layout), d_result[i] = XOR_r of
// them (the XOR assembly of server.cpp:553-562 across partitions; RCCL has no XOR op).
int fold_gathered(const uint8_t* d_gather, int nranks, size_t bytes, uint8_t* d_result,
                  hipStream_t s) {
  HIP_TRY(pir::launch_xor_fold(d_gather, nranks, bytes, d_result, s));
  return PIR_OK;
}

}  // namespace

// Every rank's `bytes` of partial answers (d_part) -> every rank's XOR over ranks (d_result):
// ONE ncclAllGather into d_gather (nranks x bytes) + fold_gathered, on stream s.  A failed or
// timed-out exchange aborts the communicator (an operation may still be in flight on it) and
// marks the engine failed, so that later answers refuse instead of returning partition-only
// partials.
int eng::exchange(pir_engine* e, const uint8_t* d_part, size_t bytes, uint8_t* d_gather,
                  uint8_t* d_result, hipStream_t s) {
  const ncclResult_t r = rccl_settle(
      e->comm, ncclAllGather(d_part, d_gather, bytes, ncclUint8, e->comm, s), e->comm_timeout_s);
  if (r != ncclSuccess) {
    (void)ncclCommAbort(e->comm);
    e->comm = nullptr;
    e->comm_failed = true;
    return fail(PIR_ECOMM, "ncclAllGather of %zu bytes failed: %s (communicator aborted)", bytes,
                r == ncclInProgress ? "timed out" : ncclGetErrorString(r));
  }
  return fold_gathered(d_gather, e->nranks, bytes, d_result, s);
}

extern "C" {

int pir_engine_fold_gathered_dev(pir_engine_t* e, const uint8_t* d_gathered, int nranks,
                                 uint64_t bytes_per_rank, uint8_t* d_result, void* stream) {
  if (!e || !d_gathered || !d_result || nranks < 1) return fail(PIR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  return fold_gathered(d_gathered, nranks, (size_t)bytes_per_rank, d_result, s);
}

int pir_comm_unique_id(uint8_t id[PIR_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == PIR_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  RCCL_TRY(ncclGetUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return PIR_OK;
}

int pir_comm_detach(pir_engine_t* e) {
  if (!e) return fail(PIR_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  // abort, not destroy: a peer that never joined (or already left) cannot block the caller
  if (e->comm) (void)ncclCommAbort(e->comm);
  e->comm = nullptr;
  e->comm_failed = false;
  e->nranks = 1;
  e->rank = 0;
  return PIR_OK;
}

int pir_comm_info(pir_engine_t* e, pir_comm_info_t* out) {
  if (!e || !out) return fail(PIR_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  memset(out, 0, sizeof *out);
  out->attached = e->comm ? 1 : 0;
  out->count = out->user_rank = out->device = -1;
  out->engine_device = e->cfg.device;
  if (e->comm) {
    RCCL_TRY(ncclCommCount(e->comm, &out->count));
    RCCL_TRY(ncclCommUserRank(e->comm, &out->user_rank));
    RCCL_TRY(ncclCommCuDevice(e->comm, &out->device));
  }
  HIP_TRY(hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof out->pci_bus_id, e->cfg.device));
  return PIR_OK;
}

int pir_comm_attach(pir_engine_t* e, const uint8_t id[PIR_COMM_ID_BYTES], int nranks, int rank) {
  if (!e || !id) return fail(PIR_EINVAL, "null argument");
  if (nranks != (1 << e->cfg.log_num_partitions) || rank != e->cfg.partition_index)
    return fail(PIR_EINVAL, "rank %d/%d does not match partition %d of 2^%d", rank, nranks,
                e->cfg.partition_index, e->cfg.log_num_partitions);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  // non-blocking init, bounded: a rank that cannot join (e.g. RCCL refuses the device) fails
  // here with PIR_ECOMM after at most $PIR_COMM_INIT_TIMEOUT seconds (default 120) instead of
  // leaving the other ranks blocked in ncclCommInitRank
  const char* ts = getenv("PIR_COMM_INIT_TIMEOUT");
  const double timeout_s = ts ? atof(ts) : 120.0;
  ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
  cfg.blocking = 0;
  ncclComm_t comm = nullptr;
  ncclResult_t r = ncclCommInitRankConfig(&comm, nranks, u, rank, &cfg);
  if (comm) r = rccl_settle(comm, r, timeout_s);
  if (r != ncclSuccess) {
    if (comm) (void)ncclCommAbort(comm);
    return fail(PIR_ECOMM, "ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks,
                r == ncclInProgress ? "timed out" : ncclGetErrorString(r));
  }
  e->comm = comm;
  e->nranks = nranks;
  e->rank = rank;
  e->comm_failed = false;
  const char* xt = getenv("PIR_COMM_TIMEOUT");  // seconds one exchange may take to enqueue
  if (xt && atof(xt) > 0) e->comm_timeout_s = atof(xt);
  e->d_gather.release();  // a re-attach (after pir_comm_detach)
  return e->d_gather.reserve((size_t)nranks * e->cfg.num_rounds * e->cfg.record_bytes);
}

}  // extern "C"
