// ckpt.cpp -- host-only half of libhdgnn.so: CRC-32C, the TF V2 checkpoint bundle writer
// and its background thread (hdg_crc32c, hdg_bundle_write, hdg_ckpt_writer_*; see
// include/hdgnn.h).  Plain C++17, no HIP header in reach: it also builds stand-alone for
// the host sanitizer runs (tests/host/ckpt_threads.cpp).
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hdgnn.h"
#include "err.h"

using hdg::fail;

extern "C" {

// CRC-32C (Castagnoli, reflected 0x82F63B78), slicing by 8: the checksum of the TF V2
// checkpoint bundle's records (hdgnn.tfckpt; LevelDB / TF masked CRCs)
uint32_t hdg_crc32c(const void* data, size_t n, uint32_t crc) {
  // slicing-by-8 tables, built once (a C++11 function-local static: thread-safe init)
  struct Tab {
    uint32_t t[8][256];
    Tab() {
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
        t[0][i] = c;
      }
      for (uint32_t i = 0; i < 256; ++i)
        for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFFu];
    }
  };
  static const Tab T;
  const auto& tab = T.t;
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint32_t c = crc ^ 0xFFFFFFFFu;
  for (; n >= 8; n -= 8, p += 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = tab[7][lo & 0xFFu] ^ tab[6][(lo >> 8) & 0xFFu] ^ tab[5][(lo >> 16) & 0xFFu] ^
        tab[4][lo >> 24] ^ tab[3][hi & 0xFFu] ^ tab[2][(hi >> 8) & 0xFFu] ^
        tab[1][(hi >> 16) & 0xFFu] ^ tab[0][hi >> 24];
  }
  for (; n; --n, ++p) c = tab[0][(c ^ *p) & 0xFFu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

static uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

static int write_file(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return fail(HDG_EINVAL, "cannot open %s for writing", path);
  const size_t w = n ? fwrite(p, 1, n, f) : 0;
  const int rc = fclose(f);
  if (w != n || rc != 0) return fail(HDG_EINVAL, "short write to %s", path);
  return 0;
}

int hdg_bundle_write(const char* data_path, const char* index_path, const float* state,
                     int64_t n_state, const int32_t* gather, int64_t n_floats,
                     uint8_t* index_img, int64_t index_len, const int64_t* entries,
                     int32_t n_entries, const int64_t* blocks, int32_t n_blocks) {
  if (!data_path || !index_path || !state || n_state < 0 || !gather || n_floats < 0 ||
      !index_img || index_len < 48 || (n_entries && !entries) || (n_blocks && !blocks))
    return fail(HDG_EINVAL, "hdg_bundle_write: bad arguments");
  std::vector<float> blob((size_t)n_floats);
  for (int64_t i = 0; i < n_floats; ++i) {
    if (gather[i] < 0 || gather[i] >= n_state)
      return fail(HDG_EINVAL, "hdg_bundle_write: gather[%lld] = %d outside the %lld-float state",
                  (long long)i, (int)gather[i], (long long)n_state);
    blob[i] = state[gather[i]];
  }
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(blob.data());
  const int64_t nbytes = n_floats * 4;
  for (int32_t e = 0; e < n_entries; ++e) {        // entry proto field 6: masked CRC of bytes
    const int64_t off = entries[3 * e], size = entries[3 * e + 1], pos = entries[3 * e + 2];
    if (off < 0 || size < 0 || off + size > nbytes || pos < 0 || pos + 4 > index_len)
      return fail(HDG_EINVAL, "hdg_bundle_write: entry %d out of range", (int)e);
    const uint32_t c = mask_crc(hdg_crc32c(bytes + off, (size_t)size, 0));
    memcpy(index_img + pos, &c, 4);
  }
  for (int32_t b = 0; b < n_blocks; ++b) {         // block trailer: type byte + masked CRC
    const int64_t off = blocks[2 * b], len = blocks[2 * b + 1];
    if (off < 0 || len < 0 || off + len + 5 > index_len)
      return fail(HDG_EINVAL, "hdg_bundle_write: block %d out of range", (int)b);
    const uint32_t c = mask_crc(hdg_crc32c(index_img + off, (size_t)len + 1, 0));
    memcpy(index_img + off + len + 1, &c, 4);
  }
  // both files under temporary names first, then renamed data before index: a crash or a
  // full disk mid-save never leaves a new .index beside a stale or partial .data
  const std::string dtmp = std::string(data_path) + ".tmp", itmp = std::string(index_path) + ".tmp";
  int rc = write_file(dtmp.c_str(), bytes, (size_t)nbytes);
  if (!rc) rc = write_file(itmp.c_str(), index_img, (size_t)index_len);
  if (!rc && rename(dtmp.c_str(), data_path) != 0)
    rc = fail(HDG_EINVAL, "cannot rename %s to %s", dtmp.c_str(), data_path);
  if (!rc && rename(itmp.c_str(), index_path) != 0)
    rc = fail(HDG_EINVAL, "cannot rename %s to %s", itmp.c_str(), index_path);
  if (rc) {
    remove(dtmp.c_str());
    remove(itmp.c_str());
  }
  return rc;
}

// ---- background checkpoint writer -------------------------------------------------
// saver.save off the training thread: one native thread writes the queued bundles (and the
// small text files that go with them) in submission order, so the training loop's thread
// only copies the state into the job.  The first failure is kept for flush().
struct CkptJob {
  std::vector<float> state;                  // empty: no bundle in this job
  std::string data_path, index_path, removes, text_path, text;
  bool text_append = false;
};
struct hdg_ckpt_writer_s {
  std::vector<int32_t> gather;
  std::vector<uint8_t> image;
  std::vector<int64_t> entries, blocks;
  int64_t n_state = 0;
  std::mutex mu;
  std::condition_variable cv, idle;
  std::deque<CkptJob> q;
  bool busy = false, stop = false;
  int err_code = 0;
  char err[512] = "";
  std::thread th;
};

static int ckpt_run(hdg_ckpt_writer_s* w, CkptJob& j) {
  if (!j.state.empty()) {
    std::vector<uint8_t> img = w->image;     // the CRCs are patched into a private copy
    if (int rc = hdg_bundle_write(j.data_path.c_str(), j.index_path.c_str(), j.state.data(),
                                  (int64_t)j.state.size(), w->gather.data(),
                                  (int64_t)w->gather.size(), img.data(), (int64_t)img.size(),
                                  w->entries.data(), (int32_t)(w->entries.size() / 3),
                                  w->blocks.data(), (int32_t)(w->blocks.size() / 2)))
      return rc;
  }
  size_t a = 0;                              // '\n'-separated paths: missing ones are fine
  while (a < j.removes.size()) {
    size_t e = j.removes.find('\n', a);
    if (e == std::string::npos) e = j.removes.size();
    if (e > a) remove(j.removes.substr(a, e - a).c_str());
    a = e + 1;
  }
  if (!j.text_path.empty()) {
    FILE* f = fopen(j.text_path.c_str(), j.text_append ? "ab" : "wb");
    if (!f) return fail(HDG_EINVAL, "cannot open %s for writing", j.text_path.c_str());
    const size_t n = j.text.size(), wr = n ? fwrite(j.text.data(), 1, n, f) : 0;
    if (fclose(f) != 0 || wr != n) return fail(HDG_EINVAL, "short write to %s", j.text_path.c_str());
  }
  return 0;
}

static void ckpt_loop(hdg_ckpt_writer_s* w) {
  std::unique_lock<std::mutex> lk(w->mu);
  for (;;) {
    w->cv.wait(lk, [&] { return w->stop || !w->q.empty(); });
    if (w->q.empty()) return;                // stop with nothing queued
    CkptJob j = std::move(w->q.front());
    w->q.pop_front();
    w->busy = true;
    lk.unlock();
    const int rc = ckpt_run(w, j);
    lk.lock();
    if (rc && !w->err_code) {
      w->err_code = rc;
      snprintf(w->err, sizeof(w->err), "%s", hdg::g_err);
    }
    w->busy = false;
    if (w->q.empty()) w->idle.notify_all();
  }
}

int hdg_ckpt_writer_create(const int32_t* gather, int64_t n_floats, int64_t n_state,
                           const uint8_t* index_img, int64_t index_len, const int64_t* entries,
                           int32_t n_entries, const int64_t* blocks, int32_t n_blocks,
                           void** writer) {
  if (!writer || !gather || n_floats < 0 || n_state < 0 || !index_img || index_len < 48 ||
      (n_entries && !entries) || (n_blocks && !blocks))
    return fail(HDG_EINVAL, "hdg_ckpt_writer_create: bad arguments");
  for (int64_t i = 0; i < n_floats; ++i)
    if (gather[i] < 0 || gather[i] >= n_state)
      return fail(HDG_EINVAL, "hdg_ckpt_writer_create: gather[%lld] outside the state",
                  (long long)i);
  auto* w = new hdg_ckpt_writer_s;
  w->gather.assign(gather, gather + n_floats);
  w->image.assign(index_img, index_img + index_len);
  w->entries.assign(entries, entries + 3 * (size_t)n_entries);
  w->blocks.assign(blocks, blocks + 2 * (size_t)n_blocks);
  w->n_state = n_state;
  w->th = std::thread(ckpt_loop, w);
  *writer = w;
  return 0;
}

int hdg_ckpt_writer_submit(void* writer, const float* state, const char* data_path,
                           const char* index_path, const char* removes, const char* text_path,
                           const char* text, int32_t text_append) {
  auto* w = static_cast<hdg_ckpt_writer_s*>(writer);
  if (!w || (state && (!data_path || !index_path)) || (text_path && !text))
    return fail(HDG_EINVAL, "hdg_ckpt_writer_submit: bad arguments");
  CkptJob j;
  if (state) {
    j.state.assign(state, state + w->n_state);
    j.data_path = data_path;
    j.index_path = index_path;
  }
  if (removes) j.removes = removes;
  if (text_path) {
    j.text_path = text_path;
    j.text = text;
    j.text_append = text_append != 0;
  }
  {
    std::lock_guard<std::mutex> lk(w->mu);
    w->q.push_back(std::move(j));
  }
  w->cv.notify_one();
  return 0;
}

int hdg_ckpt_writer_flush(void* writer) {
  auto* w = static_cast<hdg_ckpt_writer_s*>(writer);
  if (!w) return fail(HDG_EINVAL, "hdg_ckpt_writer_flush: NULL writer");
  std::unique_lock<std::mutex> lk(w->mu);
  w->idle.wait(lk, [&] { return w->q.empty() && !w->busy; });
  const int rc = w->err_code;
  if (rc) {
    snprintf(hdg::g_err, sizeof(hdg::g_err), "%s", w->err);
    w->err_code = 0;                         // reported once, as a future's exception is
  }
  return rc;
}

int hdg_ckpt_writer_poll(void* writer) {
  auto* w = static_cast<hdg_ckpt_writer_s*>(writer);
  if (!w) return fail(HDG_EINVAL, "hdg_ckpt_writer_poll: NULL writer");
  std::lock_guard<std::mutex> lk(w->mu);
  const int rc = w->err_code;
  if (rc) {
    snprintf(hdg::g_err, sizeof(hdg::g_err), "%s", w->err);
    w->err_code = 0;
  }
  return rc;
}

int hdg_ckpt_writer_destroy(void* writer) {
  auto* w = static_cast<hdg_ckpt_writer_s*>(writer);
  if (!w) return 0;
  const int rc = hdg_ckpt_writer_flush(w);
  {
    std::lock_guard<std::mutex> lk(w->mu);
    w->stop = true;
  }
  w->cv.notify_all();
  w->th.join();
  delete w;
  return rc;
}

}  // extern "C"
