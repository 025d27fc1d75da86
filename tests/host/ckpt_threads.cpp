// Stand-alone driver of the background checkpoint writer (csrc/ckpt.cpp), built with the
// thread sanitizer and with ASan + UBSan by tests/test_host_ckpt.py: no HIP, no Python.
//   ckpt_threads <scratch dir>
// The main thread submits a handful of small jobs (bundles, text lines, removals, and two
// jobs whose files cannot be opened) while the writer's thread works them off, then
// flushes, polls and destroys; the files' bytes and the reported error are checked.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "hdgnn.h"
#include "err.h"

static int g_failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

static bool slurp(const std::string& path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out.clear();
  uint8_t buf[256];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

static uint32_t masked(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

int main(int argc, char** argv) {
  if (argc < 2) return printf("usage: %s <scratch dir>\n", argv[0]), 2;
  const std::string dir = argv[1];
  CHECK(hdg_crc32c("123456789", 9, 0) == 0xE3069283u);   // the CRC-32C check value

  // template: 6 of the state's 8 floats, reversed; one entry CRC, one block trailer
  constexpr int NS = 8, NF = 6, IL = 64, NJ = 6;
  const int32_t gather[NF] = {6, 5, 4, 3, 2, 1};
  uint8_t image[IL];
  for (int i = 0; i < IL; ++i) image[i] = (uint8_t)(3 * i + 1);
  const int64_t entries[3] = {4, 16, 8};     // CRC of data bytes [4, 20) -> image[8..12)
  const int64_t blocks[2] = {16, 20};        // CRC of image [16, 37) -> image[37..41)
  void* w = nullptr;
  CHECK(hdg_ckpt_writer_create(gather, NF, NS, image, IL, entries, 1, blocks, 1, &w) == 0);
  if (!w) return 1;

  const std::string log = dir + "/log.txt", state_txt = dir + "/checkpoint";
  const std::string bad1 = dir + "/no_such_dir_1/ck.data", bad2 = dir + "/no_such_dir_2/t.txt";
  auto data_of = [&](int k) { return dir + "/ck-" + std::to_string(k) + ".data"; };
  auto index_of = [&](int k) { return dir + "/ck-" + std::to_string(k) + ".index"; };
  float state[NS];
  for (int k = 0; k < NJ; ++k) {
    for (int i = 0; i < NS; ++i) state[i] = (float)(10 * k + i);
    const std::string line = "line " + std::to_string(k) + "\n";
    const std::string keep = "latest " + std::to_string(k) + "\n";
    if (k == 2) {
      // a bundle whose data file cannot be opened: the first failure; its text is skipped
      CHECK(hdg_ckpt_writer_submit(w, state, bad1.c_str(), index_of(k).c_str(), nullptr,
                                   log.c_str(), line.c_str(), 1) == 0);
    } else if (k == 4) {
      // text only, into a directory that does not exist: a second failure, not reported
      CHECK(hdg_ckpt_writer_submit(w, nullptr, nullptr, nullptr, nullptr, bad2.c_str(),
                                   line.c_str(), 0) == 0);
    } else {
      // a bundle, the removal of the first job's bundle (and of a missing file) from job 3
      // on, an appended log line; then the replaced state file as a job of its own
      const std::string rm = data_of(0) + "\n" + index_of(0) + "\n" + dir + "/never_there\n";
      CHECK(hdg_ckpt_writer_submit(w, state, data_of(k).c_str(), index_of(k).c_str(),
                                   k >= 3 ? rm.c_str() : nullptr, log.c_str(), line.c_str(),
                                   1) == 0);
      CHECK(hdg_ckpt_writer_submit(w, nullptr, nullptr, nullptr, nullptr, state_txt.c_str(),
                                   keep.c_str(), 0) == 0);
    }
    state[0] = -1.f;   // submit copied the state: later writes of the caller do not show
  }
  CHECK(hdg_ckpt_writer_submit(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) ==
        HDG_EINVAL);

  // flush: the first failure, once
  CHECK(hdg_ckpt_writer_flush(w) == HDG_EINVAL);
  CHECK(strstr(hdg::g_err, "no_such_dir_1") != nullptr);
  CHECK(strstr(hdg::g_err, "no_such_dir_2") == nullptr);
  CHECK(hdg_ckpt_writer_poll(w) == 0);
  CHECK(hdg_ckpt_writer_flush(w) == 0);

  // the files' bytes
  std::vector<uint8_t> got;
  for (int k = 0; k < NJ; ++k) {
    if (k == 2 || k == 4) continue;
    if (k == 0) {   // removed by job 3
      CHECK(!slurp(data_of(k), got) && !slurp(index_of(k), got));
      continue;
    }
    float blob[NF];
    for (int i = 0; i < NF; ++i) blob[i] = (float)(10 * k + gather[i]);
    CHECK(slurp(data_of(k), got) && got.size() == sizeof(blob) &&
          memcmp(got.data(), blob, sizeof(blob)) == 0);
    uint8_t img[IL];
    memcpy(img, image, IL);
    const uint32_t ce = masked(hdg_crc32c((const uint8_t*)blob + 4, 16, 0));
    memcpy(img + 8, &ce, 4);
    const uint32_t cb = masked(hdg_crc32c(img + 16, 21, 0));
    memcpy(img + 37, &cb, 4);
    CHECK(slurp(index_of(k), got) && got.size() == IL && memcmp(got.data(), img, IL) == 0);
    CHECK(!slurp(data_of(k) + ".tmp", got) && !slurp(index_of(k) + ".tmp", got));
  }
  CHECK(!slurp(bad1, got) && !slurp(index_of(2), got) && !slurp(bad2, got));
  const std::string want_log = "line 0\nline 1\nline 3\nline 5\n", want_state = "latest 5\n";
  CHECK(slurp(log, got) && std::string(got.begin(), got.end()) == want_log);
  CHECK(slurp(state_txt, got) && std::string(got.begin(), got.end()) == want_state);

  // a failure after the flush is a new first failure; the jobs behind it still run
  CHECK(hdg_ckpt_writer_submit(w, nullptr, nullptr, nullptr, nullptr, bad2.c_str(), "x", 0) == 0);
  CHECK(hdg_ckpt_writer_submit(w, nullptr, nullptr, nullptr, nullptr, log.c_str(), "tail\n", 1) == 0);
  CHECK(hdg_ckpt_writer_destroy(w) == HDG_EINVAL);   // destroy flushes first
  CHECK(strstr(hdg::g_err, "no_such_dir_2") != nullptr);
  CHECK(slurp(log, got) && std::string(got.begin(), got.end()) == want_log + "tail\n");
  CHECK(hdg_ckpt_writer_destroy(nullptr) == 0);

  if (g_failed) return printf("%d checks failed\n", g_failed), 1;
  printf("all checks passed\n");
  return 0;
}
