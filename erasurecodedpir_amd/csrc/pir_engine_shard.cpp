// pir_engine_shard.cpp -- the engine's shard: host rows in and out (staged through pinned memory
// by a crew of host threads), the device-side encoders and fills.
#include <condition_variable>
#include <functional>
#include <thread>

#include "pir_engine_internal.h"

using namespace eng;

namespace {

// Host threads for the staged row copies below ($PIR_GATHER_THREADS; the GPU box grants 16
// CPUs per GPU, OMP_NUM_THREADS says how many)
int gather_threads() {
  if (const char* v = getenv("PIR_GATHER_THREADS")) return std::max(1, atoi(v));
  int n = (int)std::thread::hardware_concurrency();
  if (const char* v = getenv("OMP_NUM_THREADS")) n = std::min(n, std::max(1, atoi(v)));
  return std::max(1, std::min(8, n));
}

// T - 1 host threads kept for the length of one staged copy (a 64 GiB setup is ~1000 chunks:
// spawning a thread team per chunk cost more than some chunks' copies); run(fn) calls fn(t, T)
// on every thread, the caller's as t = 0, and returns when all have.
class Crew {
 public:
  explicit Crew(int T) : T_(T) {
    for (int t = 1; t < T_; ++t) th_.emplace_back([this, t] { loop(t); });
  }
  ~Crew() {
    {
      std::lock_guard<std::mutex> lk(m_);
      quit_ = true;
    }
    go_.notify_all();
    for (auto& x : th_) x.join();
  }
  void run(const std::function<void(int, int)>& fn) {
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = &fn;
      pending_ = T_ - 1;
      ++gen_;
    }
    go_.notify_all();
    fn(0, T_);
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this] { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  void loop(int t) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(int, int)>* job;
      {
        std::unique_lock<std::mutex> lk(m_);
        go_.wait(lk, [&] { return quit_ || gen_ != seen; });
        if (quit_) return;
        seen = gen_;
        job = job_;
      }
      (*job)(t, T_);
      std::lock_guard<std::mutex> lk(m_);
      if (--pending_ == 0) done_.notify_one();
    }
  }
  const int T_;
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable go_, done_;
  const std::function<void(int, int)>* job_ = nullptr;
  uint64_t gen_ = 0;
  int pending_ = 0;
  bool quit_ = false;
};

// [a, b) of n items split into T contiguous slices: slice t
inline void slice_of(uint64_t n, int t, int T, uint64_t& a, uint64_t& b) {
  a = n * (uint64_t)t / (uint64_t)T;
  b = n * (uint64_t)(t + 1) / (uint64_t)T;
}

// dst + i * efs <- rows[i] for i in [a, b), each run of rows that lie back to back in host
// memory (the shim's client files and indexList rows are one block) as one memcpy
inline void gather_rows(uint8_t* dst, const uint8_t* const* rows, uint64_t a, uint64_t b,
                        uint32_t efs) {
  for (uint64_t i = a; i < b;) {
    const uint8_t* s0 = rows[i];
    uint64_t j = i + 1;
    while (j < b && rows[j] == s0 + (j - i) * efs) ++j;
    memcpy(dst + i * efs, s0, (size_t)(j - i) * efs);
    i = j;
  }
}
// the reverse: rows[i] <- src + i * efs
inline void scatter_rows(uint8_t* const* rows, const uint8_t* src, uint64_t a, uint64_t b,
                         uint32_t efs) {
  for (uint64_t i = a; i < b;) {
    uint8_t* d0 = rows[i];
    uint64_t j = i + 1;
    while (j < b && rows[j] == d0 + (j - i) * efs) ++j;
    memcpy(d0, src + i * efs, (size_t)(j - i) * efs);
    i = j;
  }
}

// two pinned staging buffers with an event each; both go with the object, after the caller's
// last wait for the stream
struct PinnedPair {
  PinnedBuf h[2];
  hipEvent_t ev[2] = {nullptr, nullptr};
  int init(size_t bytes) {
    for (int i = 0; i < 2; ++i)
      if (h[i].reserve(bytes) || hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess)
        return fail(PIR_ENOMEM, "pinned staging of %zu bytes", bytes);
    return PIR_OK;
  }
  ~PinnedPair() {
    for (hipEvent_t x : ev)
      if (x) (void)hipEventDestroy(x);
  }
};

// Host rows -> device through two pinned staging buffers of `chunk_bytes`: chunk c is gathered
// by T host threads (fill(c, pinned, t, T)) while the DMA and kernel of chunk c - 1 run
// (issue(c, pinned, stream): its H2D copy and whatever consumes it, enqueued on the engine
// stream); a pinned buffer is refilled only after the copy that read it has completed.  The
// pageable single-threaded gather this replaces moved a 16 GiB shard at a few GB/s.
template <class Fill, class Issue>
int staged_h2d(pir_engine* e, uint64_t nchunks, size_t chunk_bytes, const Fill& fill,
               const Issue& issue) {
  if (!nchunks) return PIR_OK;
  PinnedPair st;  // ev: the copy that read the buffer has completed
  Crew crew(gather_threads());
  int rc = st.init(chunk_bytes);
  for (uint64_t c = 0; c < nchunks && !rc; ++c) {
    const int b = (int)(c & 1);
    if (c >= 2 && hipEventSynchronize(st.ev[b]) != hipSuccess) {
      rc = fail(PIR_EHIP, "staged upload: chunk %llu", (unsigned long long)(c - 2));
      break;
    }
    const std::function<void(int, int)> job = [&](int t, int nt) { fill(c, st.h[b], t, nt); };
    crew.run(job);
    hipError_t err = issue(c, st.h[b], e->stream);
    if (err == hipSuccess) err = hipEventRecord(st.ev[b], e->stream);
    if (err != hipSuccess) rc = fail(PIR_EHIP, "staged upload: %s", hipGetErrorString(err));
  }
  if (hipStreamSynchronize(e->stream) != hipSuccess && !rc) rc = fail(PIR_EHIP, "staged upload sync");
  return rc;
}

// rows per staging chunk: ~64 MiB of `bytes_per_row` ($PIR_STAGE_CHUNK_BYTES: tests use small
// chunks so a small shard crosses several, with a ragged last one)
uint64_t chunk_rows_for(uint64_t bytes_per_row) {
  uint64_t chunk = 64ull << 20;
  if (const char* v = getenv("PIR_STAGE_CHUNK_BYTES")) chunk = std::max<uint64_t>(1, strtoull(v, nullptr, 10));
  return std::max<uint64_t>(1, chunk / std::max<uint64_t>(1, bytes_per_row));
}

}  // namespace

int eng::fold_image_build(pir_engine* e, hipStream_t s) {
  if (e->image_epoch == e->shard_epoch) return PIR_OK;
  const size_t bytes = (size_t)((e->rows + 3) / 4 * 4) * e->pitch;
  if (e->d_image.cap < bytes) {
    // room: under the cap, and a sixteenth of the device's memory stays free afterwards
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes > e->fold_image_max || free_b < bytes || free_b - bytes < total_b / 16) {
      e->fold_image_noroom = true;
      if (e->fold_image == 2)
        return fail(PIR_ENOMEM, "fold image: no room for %zu bytes (free %zu of %zu, cap %llu)", bytes,
                    free_b, total_b, (unsigned long long)e->fold_image_max);
      if (!e->fold_image_noted)
        (void)fail(PIR_OK, "fold image left out: no room for %zu bytes (free %zu of %zu, cap %llu)",
                   bytes, free_b, total_b, (unsigned long long)e->fold_image_max);
      e->fold_image_noted = true;
      return PIR_OK;
    }
    if (e->d_image.reserve(bytes)) return fail(PIR_ENOMEM, "fold image: hipMalloc of %zu bytes", bytes);
  }
  HIP_TRY(pir::launch_fold_image(e->d_shard, e->rows, e->pitch, e->d_image, s));
  e->image_epoch = e->shard_epoch;
  return PIR_OK;
}

int eng::fold_image_for(pir_engine* e, hipStream_t s, const uint8_t** img) {
  *img = nullptr;
  if (!e->fold_image) return PIR_OK;
  // (mode 2 asks again every time, and fails every time, where the image does not fit)
  if (e->image_epoch != e->shard_epoch && (!e->fold_image_noroom || e->fold_image == 2)) {
    if (e->fold_image == 2 || e->image_wanted == e->shard_epoch) {
      if (int rc = fold_image_build(e, s)) return rc;
    } else {
      e->image_wanted = e->shard_epoch;  // wanted once: the next pass over this shard builds it
    }
  }
  if (e->image_epoch == e->shard_epoch) *img = e->d_image;
  return PIR_OK;
}

extern "C" {

int pir_engine_fold_image(pir_engine_t* e, int op, uint64_t* bytes_held) {
  if (!e || op < PIR_FOLD_IMAGE_REPORT || op > PIR_FOLD_IMAGE_DROP) return fail(PIR_EINVAL, "bad argument");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  int rc = PIR_OK;
  if (op == PIR_FOLD_IMAGE_DROP) {
    e->image_epoch = 0;
    e->image_wanted = 0;
    e->d_image.release();
  } else if (op == PIR_FOLD_IMAGE_BUILD) {
    if (!e->fold_image) return fail(PIR_EINVAL, "the fold image is switched off (PIR_FOLD_IMAGE=0)");
    e->fold_image_noroom = false;
    rc = fold_image_build(e, e->stream);
    if (!rc) HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (bytes_held) *bytes_held = e->image_epoch == e->shard_epoch ? e->d_image.cap : 0;
  return rc;
}

int pir_engine_set_shard(pir_engine_t* e, const uint8_t* host, uint64_t row0, uint64_t nrows,
                         uint64_t src_pitch) {
  if (!e || (!host && nrows)) return fail(PIR_EINVAL, "null argument");
  if (row0 + nrows > e->rows) return fail(PIR_EINVAL, "rows [%llu,%llu) beyond %llu",
                                          (unsigned long long)row0,
                                          (unsigned long long)(row0 + nrows),
                                          (unsigned long long)e->rows);
  if (src_pitch < e->cfg.record_bytes) return fail(PIR_EINVAL, "src_pitch < record_bytes");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  // 2-D copy writes record_bytes per row; the pad bytes stay zero from the create memset
  HIP_TRY(hipMemcpy2DAsync(e->d_shard + row0 * e->pitch, e->pitch, host, src_pitch,
                           e->cfg.record_bytes, nrows, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_set_shard_rows(pir_engine_t* e, const uint8_t* const* rows, uint64_t row0,
                              uint64_t nrows) {
  if (!e || (!rows && nrows)) return fail(PIR_EINVAL, "null argument");
  if (row0 + nrows > e->rows) return fail(PIR_EINVAL, "rows beyond shard");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  const uint32_t efs = e->cfg.record_bytes;
  const uint64_t m = chunk_rows_for(efs);
  return staged_h2d(
      e, (nrows + m - 1) / m, (size_t)m * efs,
      [&](uint64_t c, uint8_t* dst, int t, int nt) {
        const uint64_t r0 = c * m, n = std::min(m, nrows - r0);
        uint64_t a, b;
        slice_of(n, t, nt, a, b);
        gather_rows(dst, rows + r0, a, b, efs);
      },
      [&](uint64_t c, const uint8_t* src, hipStream_t s) {
        const uint64_t r0 = c * m, n = std::min(m, nrows - r0);
        // record_bytes per row; the pad bytes stay zero from the create memset
        return hipMemcpy2DAsync(e->d_shard + (row0 + r0) * e->pitch, e->pitch, src, efs, efs, n,
                                hipMemcpyHostToDevice, s);
      });
}

int pir_engine_get_shard_rows(pir_engine_t* e, uint8_t* const* rows, uint64_t row0,
                              uint64_t nrows) {
  if (!e || (!rows && nrows)) return fail(PIR_EINVAL, "null argument");
  if (row0 + nrows > e->rows) return fail(PIR_EINVAL, "rows beyond shard");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const uint32_t efs = e->cfg.record_bytes;
  const uint64_t m = chunk_rows_for(efs), nchunks = (nrows + m - 1) / m;
  // device -> two pinned buffers (DMA of chunk c + 1 while host threads scatter chunk c)
  PinnedPair st;  // ev: the chunk has arrived
  int rc = st.init((size_t)m * efs);
  auto enqueue = [&](uint64_t c) {
    const uint64_t r0 = c * m, n = std::min(m, nrows - r0);
    hipError_t err = hipMemcpy2DAsync(st.h[c & 1], efs, e->d_shard + (row0 + r0) * e->pitch,
                                      e->pitch, efs, n, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipEventRecord(st.ev[c & 1], e->stream);
    return err;
  };
  if (!rc && nchunks && enqueue(0) != hipSuccess) rc = fail(PIR_EHIP, "get_shard_rows: copy");
  Crew crew(gather_threads());
  for (uint64_t c = 0; c < nchunks && !rc; ++c) {
    if (hipEventSynchronize(st.ev[c & 1]) != hipSuccess) {
      rc = fail(PIR_EHIP, "get_shard_rows: chunk %llu", (unsigned long long)c);
      break;
    }
    if (c + 1 < nchunks && enqueue(c + 1) != hipSuccess) {
      rc = fail(PIR_EHIP, "get_shard_rows: copy");
      break;
    }
    const uint64_t r0 = c * m, n = std::min(m, nrows - r0);
    const uint8_t* src = st.h[c & 1];
    const std::function<void(int, int)> job = [&](int t, int nt) {
      uint64_t a, b;
      slice_of(n, t, nt, a, b);
      scatter_rows(rows + r0, src, a, b, efs);
    };
    crew.run(job);
  }
  (void)hipStreamSynchronize(e->stream);
  return rc;
}

int pir_engine_fill_shard_random(pir_engine_t* e, uint64_t seed) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  const uint64_t row0 = (uint64_t)e->cfg.partition_index * e->rows;
  HIP_TRY(pir::launch_fill_shard(e->d_shard, e->rows, e->pitch, e->cfg.record_bytes, row0, seed,
                                 e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

// pir_engine_encode_across_dev; with `key` the synthetic CheckMAC database (d_files == nullptr)
static int encode_across_dev(pir_engine_t* e, const uint8_t* d_files, uint64_t file_pitch,
                             uint64_t num_files, int k, const uint8_t* key) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  if (k < 1 || k > 16) return fail(PIR_EINVAL, "k = %d outside [1,16]", k);
  if (d_files && file_pitch < e->cfg.record_bytes) return fail(PIR_EINVAL, "file_pitch < record_bytes");
  const uint64_t encdb = (num_files + (uint64_t)k - 1) / (uint64_t)k;
  if (encdb > (1ull << e->cfg.log_num_records))
    return fail(PIR_EINVAL, "%llu files over k=%d need %llu rows > 2^%d", (unsigned long long)num_files,
                k, (unsigned long long)encdb, e->cfg.log_num_records);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  const uint64_t row0 = (uint64_t)e->cfg.partition_index * e->rows;
  // CheckMAC: the 257 distinct synthetic payloads (bytes v, and file 1's ramp as entry 256) are
  // materialised once, tagged by k_hmac_sha256_files, and the encode reads the 257 x 32 table
  DevBuf<> d_pay, d_tags;
  const uint32_t payload = key ? e->cfg.record_bytes - PIR_MAC_BYTES : 0;
  int rc = PIR_OK;
  if (key) {
    std::vector<uint8_t> pay((size_t)257 * payload);
    for (uint32_t v = 0; v < 256; ++v) memset(&pay[(size_t)v * payload], (int)v, payload);
    for (uint32_t j = 0; j < payload; ++j) pay[(size_t)256 * payload + j] = (uint8_t)j;
    if (d_pay.reserve(pay.size()) || d_tags.reserve(257 * PIR_MAC_BYTES))
      rc = fail(PIR_ENOMEM, "tag table");
    else if (hipMemcpyAsync(d_pay, pay.data(), pay.size(), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
             hipStreamSynchronize(e->stream) != hipSuccess ||  // pay is pageable and dies here
             pir::launch_hmac_sha256_files(d_pay, payload, 257, payload, pir::hmac_states(key),
                                           d_tags, PIR_MAC_BYTES, e->stream) != hipSuccess)
      rc = fail(PIR_EHIP, "tag table");
  }
  if (!rc && (pir::launch_encode_across(d_files, file_pitch, num_files, k, e->cfg.party_index,
                                        e->d_shard, e->rows, row0, e->pitch, e->cfg.record_bytes,
                                        e->stream, d_tags, payload) != hipSuccess ||
              hipStreamSynchronize(e->stream) != hipSuccess))
    rc = fail(PIR_EHIP, "encode_across: %s", hipGetErrorString(hipGetLastError()));
  return rc;
}

int pir_engine_encode_across_dev(pir_engine_t* e, const uint8_t* d_files, uint64_t file_pitch,
                                 uint64_t num_files, int k) {
  return encode_across_dev(e, d_files, file_pitch, num_files, k, nullptr);
}

int pir_engine_encode_across_synthetic_mac(pir_engine_t* e, uint64_t num_files, int k,
                                           const uint8_t key[16]) {
  if (!e || !key) return fail(PIR_EINVAL, "null argument");
  if (e->cfg.record_bytes <= PIR_MAC_BYTES)
    return fail(PIR_EINVAL, "record_bytes %u leaves no payload before the %d-byte tag",
                e->cfg.record_bytes, PIR_MAC_BYTES);
  return encode_across_dev(e, nullptr, 0, num_files, k, key);
}

int pir_engine_encode_across_rows(pir_engine_t* e, const uint8_t* const* files, uint64_t num_files,
                                  int k) {
  if (!e || (!files && num_files)) return fail(PIR_EINVAL, "null argument");
  if (k < 1 || k > 16) return fail(PIR_EINVAL, "k = %d outside [1,16]", k);
  const uint64_t encdb = (num_files + (uint64_t)k - 1) / (uint64_t)k;
  if (encdb > (1ull << e->cfg.log_num_records))
    return fail(PIR_EINVAL, "%llu files over k=%d need %llu rows > 2^%d", (unsigned long long)num_files,
                k, (unsigned long long)encdb, e->cfg.log_num_records);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  const uint32_t efs = e->cfg.record_bytes;
  const uint64_t prow0 = (uint64_t)e->cfg.partition_index * e->rows;
  // chunk c = this engine's rows [c m, (c + 1) m): its k source files per row staged as k blocks
  // of m rows (block j row r = file encdb j + global row; zero past num_files), so the encode
  // kernel sees k m "files" of which row r takes m j + r -- the encdb of a k m-file database
  const uint64_t m = chunk_rows_for((uint64_t)k * efs), nchunks = (e->rows + m - 1) / m;
  DevBuf<> d_stage[2];
  const size_t sbytes = (size_t)k * m * efs;
  int rc = PIR_OK;
  for (int i = 0; i < 2 && !rc; ++i)
    if (d_stage[i].reserve(sbytes)) rc = fail(PIR_ENOMEM, "encode staging");
  if (!rc)
    rc = staged_h2d(
        e, nchunks, sbytes,
        [&](uint64_t c, uint8_t* dst, int t, int nt) {
          const uint64_t r0 = c * m, n = std::min(m, e->rows - r0), tot = (uint64_t)k * n;
          uint64_t a, b;
          slice_of(tot, t, nt, a, b);  // items i = j n + r: block j, row r
          while (a < b) {
            const uint64_t j = a / n, r = a - j * n, e_r = std::min(n, r + (b - a));  // rows [r, e_r) of block j
            const uint64_t f0 = encdb * j + prow0 + r0;  // the file of row 0 of block j
            uint8_t* d = dst + j * n * efs;
            const uint64_t live = f0 + e_r <= num_files ? e_r : (f0 >= num_files ? 0 : num_files - f0);
            if (live > r) gather_rows(d, files + f0, r, live, efs);
            const uint64_t z0 = std::max(r, live);
            if (e_r > z0) memset(d + z0 * efs, 0, (size_t)(e_r - z0) * efs);
            a += e_r - r;
          }
        },
        [&](uint64_t c, const uint8_t* src, hipStream_t s) {
          const uint64_t r0 = c * m, n = std::min(m, e->rows - r0);
          uint8_t* ds = d_stage[c & 1];
          hipError_t err = hipMemcpyAsync(ds, src, (size_t)k * n * efs, hipMemcpyHostToDevice, s);
          if (err == hipSuccess)
            err = pir::launch_encode_across(ds, efs, (uint64_t)k * n, k, e->cfg.party_index,
                                            e->d_shard + r0 * e->pitch, n, 0, e->pitch, efs, s);
          return err;
        });
  return rc;
}

int pir_engine_encode_within_rows(pir_engine_t* e, const uint8_t* const* files, uint64_t num_files,
                                  uint32_t file_bytes, int k, int party) {
  if (!e || (!files && num_files)) return fail(PIR_EINVAL, "null argument");
  if (k < 1 || k > 16) return fail(PIR_EINVAL, "k = %d outside [1,16]", k);
  if (party < 0 || party > 255) return fail(PIR_EINVAL, "party %d outside [0,255]", party);
  if ((uint64_t)file_bytes > (uint64_t)k * e->cfg.record_bytes)
    return fail(PIR_EINVAL, "file_bytes %u > k * record_bytes (%d * %u)", file_bytes, k,
                e->cfg.record_bytes);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  const uint64_t prow0 = (uint64_t)e->cfg.partition_index * e->rows;
  const uint32_t fb = std::max<uint32_t>(file_bytes, 1);
  // chunk c = this engine's rows [c m, (c + 1) m) = files prow0 + c m + r (one file per row)
  const uint64_t m = chunk_rows_for(fb), nchunks = (e->rows + m - 1) / m;
  DevBuf<> d_stage[2];
  const size_t sbytes = (size_t)m * fb;
  int rc = PIR_OK;
  for (int i = 0; i < 2 && !rc; ++i)
    if (d_stage[i].reserve(sbytes)) rc = fail(PIR_ENOMEM, "encode staging");
  auto nfiles_of = [&](uint64_t r0, uint64_t n) {
    const uint64_t g0 = prow0 + r0;
    return g0 >= num_files ? 0ull : std::min<uint64_t>(n, num_files - g0);
  };
  if (!rc)
    rc = staged_h2d(
        e, nchunks, sbytes,
        [&](uint64_t c, uint8_t* dst, int t, int nt) {
          const uint64_t r0 = c * m, n = std::min(m, e->rows - r0), nf = nfiles_of(r0, n);
          uint64_t a, b;
          slice_of(nf, t, nt, a, b);
          if (file_bytes == fb) {
            gather_rows(dst, files + prow0 + r0, a, b, fb);
          } else {
            for (uint64_t i = a; i < b; ++i) memcpy(dst + i * fb, files[prow0 + r0 + i], file_bytes);
          }
        },
        [&](uint64_t c, const uint8_t* src, hipStream_t s) {
          const uint64_t r0 = c * m, n = std::min(m, e->rows - r0), nf = nfiles_of(r0, n);
          uint8_t* ds = d_stage[c & 1];
          hipError_t err = nf ? hipMemcpyAsync(ds, src, (size_t)nf * fb, hipMemcpyHostToDevice, s)
                              : hipSuccess;
          if (err == hipSuccess)
            err = pir::launch_encode_within(ds, fb, nf, file_bytes, k,
                                            party ? party : e->cfg.party_index,
                                            e->d_shard + r0 * e->pitch, n, 0, e->pitch,
                                            e->cfg.record_bytes, s);
          return err;
        });
  return rc;
}

int pir_engine_encode_within_dev(pir_engine_t* e, const uint8_t* d_files, uint64_t file_pitch,
                                 uint64_t num_files, uint32_t file_bytes, int k, int party) {
  if (!e) return fail(PIR_EINVAL, "null engine");
  if (k < 1 || k > 16) return fail(PIR_EINVAL, "k = %d outside [1,16]", k);
  if (party < 0 || party > 255) return fail(PIR_EINVAL, "party %d outside [0,255]", party);
  if (d_files && file_pitch < file_bytes) return fail(PIR_EINVAL, "file_pitch < file_bytes");
  if ((uint64_t)file_bytes > (uint64_t)k * e->cfg.record_bytes)
    return fail(PIR_EINVAL, "file_bytes %u > k * record_bytes (%d * %u)", file_bytes, k,
                e->cfg.record_bytes);
  if (num_files > (1ull << e->cfg.log_num_records))
    return fail(PIR_EINVAL, "%llu files > 2^%d rows", (unsigned long long)num_files,
                e->cfg.log_num_records);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  ShardWrite sw(e);
  const uint64_t row0 = (uint64_t)e->cfg.partition_index * e->rows;
  HIP_TRY(pir::launch_encode_within(d_files, file_pitch, num_files, file_bytes, k,
                                    party ? party : e->cfg.party_index, e->d_shard, e->rows,
                                    row0, e->pitch,
                                    e->cfg.record_bytes, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_get_shard_row(pir_engine_t* e, uint64_t row, uint8_t* out) {
  if (!e || !out) return fail(PIR_EINVAL, "null argument");
  if (row >= e->rows) return fail(PIR_EINVAL, "row %llu beyond shard", (unsigned long long)row);
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipMemcpyAsync(out, e->d_shard + row * e->pitch, e->cfg.record_bytes,
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

int pir_engine_get_shard(pir_engine_t* e, uint64_t row0, uint64_t nrows, uint8_t* out) {
  if (!e || (!out && nrows)) return fail(PIR_EINVAL, "null argument");
  if (row0 + nrows > e->rows) return fail(PIR_EINVAL, "rows beyond shard");
  std::lock_guard<std::mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipMemcpy2DAsync(out, e->cfg.record_bytes, e->d_shard + row0 * e->pitch, e->pitch,
                           e->cfg.record_bytes, nrows, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return PIR_OK;
}

}  // extern "C"
