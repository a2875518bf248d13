// pir_engine_internal.h -- what the engine's translation units (pir_engine*.cpp) share: struct
// pir_engine, the error helpers, the owned buffers, the answer scope and the helpers that cross
// files.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/pir_client.h"
#include "../../include/pir_engine.h"
#include "pir_coefs.h"
#include "pir_kernels.h"
#include "pir_mac.h"
#include "pir_mp.h"
#include "pir_shamir.h"
#include "pir_woodruff.h"

// everything here is internal to the library: none of it enters the dynamic symbol table
#define PIR_HIDDEN __attribute__((visibility("hidden")))

namespace eng PIR_HIDDEN {

int fail(int code, const char* fmt, ...);  // sets pir_engine_last_error(), returns code

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return eng::fail(PIR_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),     \
                       __FILE__, __LINE__);                                                 \
  } while (0)

#define RCCL_TRY(expr)                                                                        \
  do {                                                                                        \
    ncclResult_t _r = (expr);                                                                 \
    if (_r != ncclSuccess) return eng::fail(PIR_ECOMM, "%s failed: %s", #expr, ncclGetErrorString(_r)); \
  } while (0)

// A growable buffer the engine owns: device memory, or pinned host memory.  reserve() only ever
// grows it and frees before it allocates (the old contents are not kept), so a regrow never
// holds both sizes; the destructor frees.
template <class T, bool kPinned>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;  // bytes
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) release(), p = o.p, cap = o.cap, o.p = nullptr, o.cap = 0;
    return *this;
  }
  ~Buf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  int reserve(size_t bytes) {
    if (bytes <= cap) return PIR_OK;
    release();
    HIP_TRY(kPinned ? hipHostMalloc((void**)&p, bytes) : hipMalloc((void**)&p, bytes));
    cap = bytes;
    return PIR_OK;
  }
};
template <class T = uint8_t>
using DevBuf = Buf<T, false>;
using PinnedBuf = Buf<uint8_t, true>;

// the storage behind a pir::NodeBufs (the kernel-side struct holds the pointers only)
struct NodeStore {
  DevBuf<uint4> s[2];
  DevBuf<uint32_t> t[2];
  uint64_t cap = 0;  // nodes
  // nb->s/t[0..nbuf) with room for `nodes` nodes each
  int reserve(pir::NodeBufs* nb, uint64_t nodes, int nbuf = 2) {
    if (nodes <= cap) return PIR_OK;
    cap = 0;
    for (int i = 0; i < 2; ++i) s[i].release(), t[i].release(), nb->s[i] = nullptr, nb->t[i] = nullptr;
    for (int i = 0; i < nbuf; ++i) {
      if (int rc = s[i].reserve(nodes * sizeof(uint4))) return rc;
      if (int rc = t[i].reserve(nodes * sizeof(uint32_t))) return rc;
      nb->s[i] = s[i], nb->t[i] = t[i];
    }
    cap = nodes;
    return PIR_OK;
  }
};

struct UserBuf {  // pir_engine_alloc_dev
  void* p = nullptr;
  size_t bytes = 0;
};

// Event layout of one profiled answer.  Leaves and scans run as kMaxChunks-way pipelined
// chunks on two streams (tree leaves of chunk j+1 overlap the shard scan of chunk j).
constexpr int kMaxChunks = 8;
enum {
  EV_START = 0, EV_KEY = 1, EV_FRONT = 2,
  EV_LEAF_B = 3, EV_LEAF_E = EV_LEAF_B + kMaxChunks,
  EV_SCAN_B = EV_LEAF_E + kMaxChunks, EV_SCAN_E = EV_SCAN_B + kMaxChunks,
  EV_PRERED = EV_SCAN_E + kMaxChunks, EV_RED, EV_END, kNumEv
};

// The engine's streams and ordering events, a base of pir_engine so that they outlive its
// members: the buffers are freed first, then the events and the streams are destroyed.
struct StreamSet {
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;              // scan stream of the leaves/scan pipeline
  hipEvent_t ev_leaf[kMaxChunks] = {};    // leaves of chunk j written
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_cb_ready[2] = {}, ev_cb_free[2] = {};  // batched answers: share buffers
  // the engine's work buffers (slabs, tree nodes, share buffers, staged keys) are shared by
  // every answer: an answer enqueued on a stream other than the previous answer's waits for
  // that answer's last use of them (ev_ws: recorded after an answer on a caller's stream, and
  // for the engine's own stream when the next answer comes on another one)
  hipEvent_t ev_ws = nullptr;
  hipStream_t ws_stream = nullptr;
  // live updates: the copy that read the pinned term table h_upd[i] has completed (made on first
  // use, pir_engine_update.cpp)
  hipEvent_t ev_upd[2] = {};
  ~StreamSet() {
    for (hipEvent_t ev : ev_leaf)
      if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {ev_cb_ready[0], ev_cb_ready[1], ev_cb_free[0], ev_cb_free[1], ev_fork,
                          ev_join, ev_ws, ev_upd[0], ev_upd[1]})
      if (ev) (void)hipEventDestroy(ev);
    if (aux) (void)hipStreamDestroy(aux);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

}  // namespace eng

struct pir_engine : eng::StreamSet {
  PIR_HIDDEN ~pir_engine() = default;  // frees the buffers; not a symbol of the library
  pir_engine_config cfg{};
  int nrp = 1;
  uint32_t pitch = 0;
  uint64_t rows = 0;  // rows held = 2^(n - G)
  int key_len = 0;
  int num_cus = 256;
  int last_chunks = 1;
  int last_fused = 0;
  bool allow_fused = true;  // $PIR_FUSED=0 forces the 2-kernel path (A/B diagnostics)
  bool allow_query = true;  // $PIR_QUERY=0: frontier + k_fused instead of k_query
  eng::DevBuf<> d_shard;
  // The fold image (pir_kernels.h: launch_fold_image): the shard once more, in the nibble-index
  // form k_scan_t looks up by.  shard_epoch counts the writes to d_shard (eng::ShardWrite);
  // the image is valid only while image_epoch equals it.  A pass that wants the image and finds
  // none notes the epoch in image_wanted; the next one that finds the same epoch builds it
  // (eng::fold_image_for), so a shard rewritten between queries never pays a build
  eng::DevBuf<> d_image;
  uint64_t shard_epoch = 1, image_epoch = 0, image_wanted = 0;
  int fold_image = 1;               // $PIR_FOLD_IMAGE: 0 never, 1 (default) by the rule above and where it fits, 2 required
  uint64_t fold_image_max = ~0ull;  // $PIR_FOLD_IMAGE_MAX_BYTES
  bool fold_image_noroom = false;   // this epoch's image did not fit: not tried again
  bool fold_image_noted = false;    // "no room" was said once
  // live updates (pir_engine_update.cpp): the term table of a batch, in two pinned buffers taken
  // in turn and on the device; the staged deltas of the host forms and the CheckMAC form, and
  // that form's tags.  An update moves shard_epoch without a ShardWrite: a valid image is patched
  // and follows (image_epoch), and image_wanted is carried to the new epoch
  eng::PinnedBuf h_upd[2];
  int upd_next = 0;
  eng::DevBuf<> d_upd, d_upd_delta, d_upd_tags;
  eng::DevBuf<> d_key_raw;          // max_batch keys
  eng::DevBuf<pir::DevKey> d_keys;  // max_batch parsed keys
  int max_batch = 0;
  pir::NodeBufs nodes{};  // tree levels between kernels (ping-pong)
  eng::NodeStore node_store;
  eng::DevBuf<> d_c;
  eng::DevBuf<> d_slabs;
  eng::DevBuf<> d_part;    // nq*efs partition answer
  eng::DevBuf<> d_gather;  // nranks*nq*efs
  // batched answers: interleaved shares of a key group, group answer, batch partition answer
  eng::DevBuf<> d_cb;
  pir::NodeBufs bnodes{};       // upper tree levels of a batch's super-group (FB x max_nodes)
  eng::NodeStore bnode_store;
  eng::DevBuf<> d_gtmp;         // 16*efs
  eng::DevBuf<> d_bpart;        // batch partition answers (split shard)
  eng::DevBuf<> d_bgather;      // nranks x batch answers
  int batch_group = 0;          // keys per shard pass (0: automatic; $PIR_BATCH_G)
  int last_batch_group = 0;
  int stream_share = 1;         // $PIR_STREAM_SHARE: 0 never, 1 stream_share_policy, 2 wherever supported
  int stream_group = 0;         // $PIR_STREAM_G: keys per pass of a shared queue (0: the policy's)
  bool stream_narrow = false;   // $PIR_STREAM_NARROW=1: narrower scans for short groups (diagnostics)
  int wd_share = 1;             // $PIR_WD_SHARE: 0 never, 1 woodruff_share_policy, 2 every queue of >= 2
  int wd_group = 0;             // $PIR_WD_G: keys per pass of a shared Woodruff queue (0: 8)
  int gq_share = 1;             // $PIR_GQ_SHARE: 0 never, 1 group_share_policy, 2 every queue of >= 2
  int gq_group = 0;             // $PIR_GQ_G: key slots per pass of a shared group queue (0: 8 / nrp)
  int sh_share = 1;             // $PIR_SH_SHARE: 0 never, 1 shamir_share_policy, 2 every queue of >= 2
  int sh_group = 0;             // $PIR_SH_G: virtual-key slots per pass of a shared Shamir queue (0: 8)
  int wdd_share = 1;            // $PIR_WDD_SHARE: 0 never, 1 woodruff_deriv_share_policy, 2 every queue of >= 2
  int wdd_group = 0;            // $PIR_WDD_G: key slots per pass of a shared Woodruff derivative queue (0: 8)
  uint64_t gq_key_bytes = 0;    // the longest sqrt(N) key a queue has staged (reserve_group_queue)
  int batch_scan_bpc = 2;       // scan workgroups per CU in batched answers ($PIR_BATCH_SCAN_BPC)
  int batch_k_last = -1;        // levels of the batched leaf stage (-1: make_plan's; $PIR_BATCH_KLAST)
  eng::DevBuf<> d_result;       // nq*efs (host-API staging)
  eng::DevBuf<> d_qscratch;     // k_query super-tile tile inputs
  eng::DevBuf<uint32_t> d_qcnt;  // k_query fused reduce: per-query slab counters (kept zero)
  // k_query's end-of-query work stealing for a lone whole answer (StealArgs, pir_kernels.h):
  // per-workgroup chunk counters + publication flags + last-tile shares, zeroed once; steal_gen
  // numbers the launches that use it ($PIR_QUERY_STEAL=0 turns it off)
  eng::DevBuf<uint32_t> d_steal;
  uint32_t steal_gen = 0;
  int steal = PIR_QUERY_STEAL ? 3 : 0;
  // k_query's in-kernel reduce (no k_reduce launch), $PIR_FUSED_REDUCE: 0 = off (k_reduce);
  // 1 = the last workgroup XORs the slabs (measured slower for a lone 2^20 x 1 KiB query: kernel
  // 0.250 vs 0.218 ms, one workgroup's 256 KiB of cross-XCD sc1 loads outlast a k_reduce
  // launch); 2 = every workgroup adds its partial to the answer with memory-side atomics
  // (answers of efs % 4 == 0 bytes at 4-byte aligned addresses; else k_reduce)
  int fused_reduce = 0;
  eng::DevBuf<> d_coef_stage;  // explicit-coefficient answers: host vectors staged here
  // Shamir answers through the host API: nq x response_len; Woodruff derivative answers too
  eng::DevBuf<> d_shamir_res;
  eng::DevBuf<> d_mpkey;       // multiparty DPF keys: host keys / unaligned device keys
  eng::PinnedBuf h_key, h_res;
  eng::DevBuf<> d_slices;      // pir_engine_answer_slices: T x nq x efs partials
  eng::PinnedBuf h_slices;
  std::vector<eng::UserBuf> user;  // pir_engine_alloc_dev
  std::mutex mu;
  uint64_t byz_counter = 0;
  // profiling: a ring of event sets, one per answer, read back after a sync
  // fused: the path of the slot's answer, which decides the events recorded in it (2: k_query,
  // and with queue set a shared queue of fused == 0: EV_START, EV_SCAN_B, EV_SCAN_E, EV_RED,
  // EV_END; else every event up to `chunks` leaf / scan pairs)
  struct ProfSlot {
    hipEvent_t ev[eng::kNumEv];
    int fused = 0, chunks = 1;
    bool queue = false;
  };
  std::vector<ProfSlot> prof;
  int prof_next = 0, prof_count = 0;
  hipEvent_t* ev = nullptr;  // the current answer's slot (nullptr: profiling off)
  // RCCL
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  bool comm_failed = false;   // an exchange failed: the communicator was aborted, answers refuse
  double comm_timeout_s = 60; // $PIR_COMM_TIMEOUT: bound on one exchange's enqueue
};

namespace eng PIR_HIDDEN {

// One answer's hold on the engine: the constructor takes the engine's lock, makes its device
// current, picks the stream (the caller's, or the engine's own) and orders the answer after the
// previous answer's use of the shared workspace; rc() != 0: nothing was acquired, return it.
// finish(rc) makes the next answer, on whatever stream, wait for this one, and returns rc.  A
// scope left without finish() (an error return after the acquire, when work may already sit on
// the stream) is finished by the destructor, so no exit leaves the workspace unordered.
class AnswerScope {
 public:
  explicit AnswerScope(pir_engine* e, void* stream = nullptr);
  ~AnswerScope() {
    if (held_) (void)finish(PIR_EHIP);
  }
  int rc() const { return rc_; }
  hipStream_t stream() const { return s_; }
  int finish(int rc);
  void synced();  // the caller has waited for the stream: nothing left to order after

 private:
  std::lock_guard<std::mutex> lk_;
  pir_engine* const e_;
  hipStream_t s_ = nullptr;
  int rc_ = PIR_OK;
  bool held_ = false;
};

// Staging for the forms that take host memory (and device keys the kernels cannot read in
// place): grow `buf` and enqueue the copy of n bytes, or of `rows` rows of `width` bytes
// dst_pitch apart, into it on s ...
int stage(DevBuf<>& buf, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s);
int stage2d(DevBuf<>& buf, size_t dst_pitch, const void* src, size_t src_pitch, size_t width,
            size_t rows, hipMemcpyKind kind, hipStream_t s);
// ... and n device bytes back to the caller's memory, waited for: straight into dst, or through
// the pinned `via` (each entry point keeps the route it measured with)
int download(void* dst, const void* d_src, size_t n, hipStream_t s, uint8_t* via = nullptr);

// the arguments every queue form checks first
inline int check_queue_args(const void* e, int num_keys, const void* keys, const void* results) {
  if (!e) return fail(PIR_EINVAL, "null argument");
  if (num_keys < 0) return fail(PIR_EINVAL, "a queue of %d keys", num_keys);
  if (num_keys > 0 && (!keys || !results)) return fail(PIR_EINVAL, "null argument");
  return PIR_OK;
}

// pir_engine.cpp
int check_key_ptr(const void* p);
pir::KeySrc key_src(pir_engine* e, const uint8_t* d_raw);
int steal_args(pir_engine* e, const pir::QueryPlan& qp, int nk, int nslices, hipStream_t s,
               pir::StealArgs* out);
pir::ScanShape group_scan_shape(const pir_engine* e, uint64_t nleaves, int gw, int G, bool* kmaj);
// pir_engine_comm.cpp
int exchange(pir_engine* e, const uint8_t* d_part, size_t bytes, uint8_t* d_gather,
             uint8_t* d_result, hipStream_t s);
// pir_engine_prof.cpp
hipEvent_t* prof_slot(pir_engine* e, int fused, int chunks, bool queue);
// pir_engine_shard.cpp: the fold image's life
// Held, under the engine's lock, by every entry point that writes d_shard: when it goes (on
// every way out: a failed write may have written part) the shard has a new epoch and the image
// of the old one is dropped
struct ShardWrite {
  explicit ShardWrite(pir_engine* e) : e_(e) {}
  ~ShardWrite() {
    ++e_->shard_epoch;
    e_->image_epoch = 0;
    e_->fold_image_noroom = false;
    e_->d_image.release();
  }
  ShardWrite(const ShardWrite&) = delete;
  ShardWrite& operator=(const ShardWrite&) = delete;

 private:
  pir_engine* const e_;
};
// build the image of the current shard on s now (the memory rule applies).  PIR_OK also when it
// was left out for want of room in mode 1 (said once through last_error); mode 2 fails then
int fold_image_build(pir_engine* e, hipStream_t s);
// the image for a k_scan_t pass enqueued on s (or on a stream ordered after s): *img = the valid
// image, else nullptr -- after building it here where the rule says so (struct pir_engine)
int fold_image_for(pir_engine* e, hipStream_t s, const uint8_t** img);
// the image at the engine rows [row0, ..) for a scan of shape sh, nullptr where the pass reads rows
inline int fold_image_at(pir_engine* e, const pir::ScanShape& sh, uint64_t row0, hipStream_t s,
                         const uint8_t** img) {
  *img = nullptr;
  if (!e->fold_image || !sh.tfold || row0 % 4 != 0) return PIR_OK;
  if (int rc = fold_image_for(e, s, img)) return rc;
  if (*img) *img += row0 * e->pitch;
  return PIR_OK;
}
// a reserve call's part: the image now, where queues of shape sh will want it (so that none of
// them allocates)
inline int fold_image_reserve(pir_engine* e, const pir::ScanShape& sh) {
  if (!e->fold_image || !sh.tfold) return PIR_OK;
  if (int rc = fold_image_build(e, e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}
// pir_engine_shamir.cpp
int check_rows(const pir_engine* e, uint64_t row0, uint64_t nrows);
int answer_coefs_locked(pir_engine* e, const uint8_t* src, uint64_t pitch, uint64_t row0,
                        uint64_t nrows, uint8_t* d_result, hipStream_t s);

// a group of G key slots over nrec records: record-major shares (the coefficient kernel writes
// all of a record's bytes at once), whichever scan takes them.  Every group queue's shape
// (answer_group_queue), G * nrp rounds wide
inline pir::ScanShape woodruff_group_shape(const pir_engine* e, uint64_t nrec, int G) {
  bool kmaj = false;
  pir::ScanShape sh = group_scan_shape(e, nrec, G, G, &kmaj);
  sh.ckey = 0;
  sh.ckoff = 0;
  return sh;
}

inline size_t wd_share_bytes(uint64_t nrec, int W) { return ((size_t)nrec * W + 15) & ~(size_t)15; }

// The group loop of every queue whose keys become record-major share rows (the Woodruff queue,
// the explicit-coefficient queue, the sqrt(N) DPF queues): nk keys over the engine rows [row0,
// row0 + nrec), G key slots of nrp bytes per pass (W = G nrp <= 8).  The keys go into ceil(nk / G)
// groups of as equal sizes as possible (20 at G = 8: 7 + 7 + 6), as answer_batch_core's queue
// does; per group, on s alone and with the one share buffer d_cb: write(q0, ng, d_cb, s) writes
// the W-byte share rows of the keys [q0, q0 + ng) (key slot g at bytes [g nrp, (g + 1) nrp) of
// each record; slots past ng and rounds past num_rounds zero), the full-width scan reads the
// shard once, and k_reduce writes straight into the results for a full group with nrp ==
// num_rounds, else into d_gtmp, from where the group's slots and rounds are copied (the empty
// slots' and padded rounds' outputs are dropped, as in answer_batch_core).  d_result: nk x
// num_rounds x record_bytes.  The caller has sized d_cb, the slabs and d_gtmp.  Five-event
// layout with fused = path: "launch" = start -> the first share kernel, "scan" = that -> the end
// of the last scan, "reduce" = the last group's reduce.
template <class Writer>
int answer_group_queue(pir_engine* e, int nk, int G, int path, uint64_t row0, uint64_t nrec,
                       uint8_t* d_result, hipStream_t s, Writer&& write) {
  const auto& c = e->cfg;
  const size_t out_bytes = (size_t)c.num_rounds * c.record_bytes;
  e->ev = nullptr;
  hipEvent_t* ev = nullptr;
  if (!e->prof.empty()) {
    ev = prof_slot(e, path, 1, true);
    HIP_TRY(hipEventRecord(ev[EV_START], s));
  }
  const pir::ScanShape sh = woodruff_group_shape(e, nrec, G);
  const uint8_t* d_img = nullptr;  // the fold image of the rows from row0 (k_scan_t passes)
  if (int rc = fold_image_at(e, sh, row0, s, &d_img)) return rc;
  if (ev) HIP_TRY(hipEventRecord(ev[EV_SCAN_B], s));
  const int ngroups = (nk + G - 1) / G;
  for (int q0 = 0, j = 0, ng = 0; q0 < nk; q0 += ng, ++j) {
    ng = nk / ngroups + (j < nk % ngroups ? 1 : 0);
    HIP_TRY(write(q0, ng, e->d_cb, s));
    HIP_TRY(pir::launch_scan(sh, e->d_shard + row0 * e->pitch, nrec, e->d_cb, e->d_slabs, false, s,
                             d_img));
    if (ev && q0 + ng >= nk) HIP_TRY(hipEventRecord(ev[EV_SCAN_E], s));
    uint8_t* dst = d_result + (size_t)q0 * out_bytes;
    if (e->nrp == c.num_rounds && ng * e->nrp == sh.nq) {
      HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, dst, s));
    } else {
      HIP_TRY(pir::launch_reduce(sh, e->d_slabs, c.record_bytes, e->d_gtmp, s));
      if (e->nrp == c.num_rounds)
        HIP_TRY(hipMemcpyAsync(dst, e->d_gtmp, (size_t)ng * out_bytes, hipMemcpyDeviceToDevice, s));
      else
        HIP_TRY(hipMemcpy2DAsync(dst, out_bytes, e->d_gtmp, (size_t)e->nrp * c.record_bytes,
                                 out_bytes, ng, hipMemcpyDeviceToDevice, s));
    }
  }
  e->last_fused = path;
  if (ev) {
    HIP_TRY(hipEventRecord(ev[EV_RED], s));
    HIP_TRY(hipEventRecord(ev[EV_END], s));
  }
  return PIR_OK;
}

}  // namespace eng
