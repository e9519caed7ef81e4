// Driver for the AddressSanitizer + UBSan build of radnet_inflate_streams_check (csrc/inflate_plan.cpp; tests/test_inflate_many_host.py
// builds and runs it): the check on exactly-sized heap tables, so a read past the table is caught; an accepted table with gaps,
// every refusal once with the index it names and a message that fits its buffer, offsets near INT64_MAX (no sum may overflow), and
// a message buffer of every small size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "radnet_hip.h"

static int failed = 0, checked = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checked;                                                       \
    if (!(cond)) {                                                   \
      ++failed;                                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
    }                                                                \
  } while (0)

struct Result {
  int rc, bad;
  char msg[256];
};

// the check on a heap copy of exactly streams.size() entries; count: what the call is told
static Result run(const std::vector<radnet_inflate_stream>& streams, int64_t z_len, int64_t out_len, int count = INT32_MIN) {
  const size_t bytes = sizeof(radnet_inflate_stream) * streams.size();
  radnet_inflate_stream* t = (radnet_inflate_stream*)malloc(bytes ? bytes : 1);
  if (bytes) memcpy(t, streams.data(), bytes);
  Result r;
  int32_t bad = -7;
  memset(r.msg, 0, sizeof r.msg);
  r.rc = radnet_inflate_streams_check(t, count == INT32_MIN ? (int32_t)streams.size() : count, z_len, out_len, &bad, r.msg, (int32_t)sizeof r.msg);
  r.bad = bad;
  free(t);
  return r;
}

int main() {
  CHECK(sizeof(radnet_inflate_stream) == 32);
  // three streams with a gap of 1 and of 15 bytes in z, of 0 and of 7 bytes in the output; the second inflates to nothing
  const std::vector<radnet_inflate_stream> good = {{0, 9, 0, 1}, {10, 100, 1, 0}, {125, 3, 8, 40}};
  Result r = run(good, 128, 48);
  CHECK(r.rc == RADNET_OK && r.bad == -1 && r.msg[0] == 0);
  CHECK(run(good, 128, 1000).rc == RADNET_OK);
  CHECK(run({{5, 3, 2, 0}}, 8, 2).rc == RADNET_OK);                        // one stream that ends with both buffers
  std::vector<radnet_inflate_stream> v = good;
  std::swap(v[1], v[2]);
  r = run(v, 128, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 2 && strstr(r.msg, "not sorted"));
  v = good, v[2].out_offset = 0;                                           // sorted in z, unsorted in the output
  r = run(v, 128, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 2 && strstr(r.msg, "not sorted"));
  v = good, v[1].z_offset = 8;
  r = run(v, 128, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 1 && strstr(r.msg, "overlaps"));
  v = good, v[2].out_offset = 1, v[1].expected = 2;                        // disjoint in z, overlapping in the output
  r = run(v, 128, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 2 && strstr(r.msg, "overlaps"));
  r = run(good, 127, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 2 && strstr(r.msg, "outside"));
  r = run(good, 128, 47);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 2 && strstr(r.msg, "outside"));
  v = good, v[0].n = 2;
  r = run(v, 128, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 0 && strstr(r.msg, "3 at least"));
  v = good, v[0].z_offset = -1;
  CHECK(run(v, 128, 48).rc == RADNET_ERR_ARG);
  v = good, v[1].out_offset = -1;
  CHECK(run(v, 128, 48).rc == RADNET_ERR_ARG);
  v = good, v[1].expected = -1;
  CHECK(run(v, 128, 48).rc == RADNET_ERR_ARG);
  // offsets and lengths near INT64_MAX: refused by comparison, never by a sum that wraps
  v = good, v[2].z_offset = INT64_MAX - 1;
  r = run(v, 128, 48);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == 2);
  v = good, v[2].n = INT64_MAX;
  CHECK(run(v, 128, 48).rc == RADNET_ERR_ARG);
  v = good, v[2].expected = INT64_MAX, v[2].out_offset = INT64_MAX;
  CHECK(run(v, 128, 48).rc == RADNET_ERR_ARG);
  // the two size limits, judged before the streams
  r = run(good, (int64_t)1 << 29, 48);
  CHECK(r.rc == RADNET_ERR_UNSUPPORTED && r.bad == -1 && strstr(r.msg, "2^29"));
  CHECK(run(good, ((int64_t)1 << 29) - 1, 48).rc == RADNET_OK);
  r = run(good, 128, (int64_t)1 << 31);
  CHECK(r.rc == RADNET_ERR_UNSUPPORTED && r.bad == -1 && strstr(r.msg, "2^31"));
  CHECK(run(good, 128, ((int64_t)1 << 31) - 1).rc == RADNET_OK);
  // the count: 0, negative, the cap and one above it (a table of exactly the cap entries, three bytes each)
  CHECK(run(good, 128, 48, 0).rc == RADNET_ERR_ARG && run(good, 128, 48, -2).rc == RADNET_ERR_ARG);
  std::vector<radnet_inflate_stream> full;
  for (int k = 0; k < RADNET_INFLATE_MANY_MAX_STREAMS; ++k) full.push_back({3 * (int64_t)k, 3, (int64_t)k, 1});
  CHECK(run(full, 3 * (int64_t)RADNET_INFLATE_MANY_MAX_STREAMS, RADNET_INFLATE_MANY_MAX_STREAMS).rc == RADNET_OK);
  r = run(full, 3 * (int64_t)RADNET_INFLATE_MANY_MAX_STREAMS, RADNET_INFLATE_MANY_MAX_STREAMS, RADNET_INFLATE_MANY_MAX_STREAMS + 1);
  CHECK(r.rc == RADNET_ERR_ARG && r.bad == -1);                            // refused before entry 4096 would be read
  CHECK(radnet_inflate_streams_check(nullptr, 3, 128, 48, nullptr, nullptr, 0) == RADNET_ERR_ARG);
  CHECK(run(good, -1, 48).rc == RADNET_ERR_ARG && run(good, 128, -1).rc == RADNET_ERR_ARG);
  // null bad_stream and msg, and message buffers of 0 .. 40 bytes, each of exactly that size
  CHECK(radnet_inflate_streams_check(good.data(), 3, 127, 48, nullptr, nullptr, 0) == RADNET_ERR_ARG);
  for (int cap = 0; cap <= 40; ++cap) {
    char* m = (char*)malloc(cap ? cap : 1);
    CHECK(radnet_inflate_streams_check(good.data(), 3, 127, 48, nullptr, m, cap) == RADNET_ERR_ARG);
    CHECK(cap == 0 || strlen(m) < (size_t)cap);
    free(m);
  }
  printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
