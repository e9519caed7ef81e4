// Driver for the AddressSanitizer + UBSan build of csrc/deflate_plan.cpp's LZ entries (tests/test_deflate_lz_plan_sanitize.py builds
// and runs it): radnet_deflate_build_codes_lz, radnet_deflate_lz_piece_cap and radnet_deflate_stream_bits on exactly-sized heap
// buffers, so a read past the 286 or the 30 counts or a write past a code table or the header's 168 bytes is caught.
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

static const int kHeaderBytes = 168, kHeaderBits = 1338, kLl = RADNET_DEFLATE_SYMBOLS, kD = RADNET_DEFLATE_DIST_SYMBOLS;
static const int kLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};

static void check_code(const radnet_deflate_code* code, const uint32_t* hist, int n) {
  uint64_t kraft = 0;
  int used = 0;
  for (int s = 0; s < n; ++s) {
    const int l = code[s].length;
    CHECK(l <= 15 && (code[s].bits >> l) == 0);
    CHECK(l > 0 || hist[s] == 0);
    if (l) kraft += 1ull << (15 - l), ++used;
  }
  CHECK(kraft == 1ull << 15);
  CHECK(used >= 2);
}

// builds the codes of the counts in buffers of exactly 286 + 30 counts, 286 + 30 entries and 168 bytes; checks what every pair must
// satisfy, the piece bound and the bit count against a sum made here
static void build(const std::vector<uint32_t>& counts_ll, const std::vector<uint32_t>& counts_d, const char* what) {
  uint32_t* hist_ll = (uint32_t*)malloc(sizeof(uint32_t) * kLl);
  uint32_t* hist_d = (uint32_t*)malloc(sizeof(uint32_t) * kD);
  memcpy(hist_ll, counts_ll.data(), sizeof(uint32_t) * kLl);
  memcpy(hist_d, counts_d.data(), sizeof(uint32_t) * kD);
  radnet_deflate_code* code_ll = (radnet_deflate_code*)malloc(sizeof(radnet_deflate_code) * kLl);
  radnet_deflate_code* code_d = (radnet_deflate_code*)malloc(sizeof(radnet_deflate_code) * kD);
  uint8_t* header = (uint8_t*)malloc(kHeaderBytes);
  memset(code_ll, 0xEE, sizeof(radnet_deflate_code) * kLl);
  memset(code_d, 0xEE, sizeof(radnet_deflate_code) * kD);
  memset(header, 0xEE, kHeaderBytes);
  int32_t nbits = -1;
  CHECK(radnet_deflate_build_codes_lz(hist_ll, hist_d, code_ll, code_d, header, kHeaderBytes, &nbits) == RADNET_OK);
  CHECK(nbits == kHeaderBits);
  check_code(code_ll, hist_ll, kLl);
  check_code(code_d, hist_d, kD);
  CHECK(code_ll[256].length > 0);
  CHECK((header[0] & 7) == 4);                                        // BFINAL 0, BTYPE 10
  CHECK((header[1] >> 0 & 0x1f) == 29);                               // HDIST: bits 8..12
  CHECK((header[kHeaderBytes - 1] >> (kHeaderBits & 7)) == 0);        // the bits behind the header are zero
  int longest = 0;
  for (int s = 0; s < kLl; ++s) longest = code_ll[s].length > longest ? code_ll[s].length : longest;
  const int64_t cap = radnet_deflate_lz_piece_cap(code_ll, code_d, nbits);
  CHECK(cap >= kHeaderBytes + (int64_t)longest * RADNET_DEFLATE_CHUNK / 8 + 16);
  CHECK(cap <= kHeaderBytes + (int64_t)16 * RADNET_DEFLATE_CHUNK / 8 + 16);      // 48 bits on three bytes at the most
  int64_t want = 3ll * nbits, matches = 0;
  for (int s = 0; s < kLl; ++s) {
    want += (int64_t)hist_ll[s] * (code_ll[s].length + (s > 256 ? kLengthExtra[s - 257] : 0));
    if (s > 256) matches += hist_ll[s];
  }
  CHECK(radnet_deflate_stream_bits(hist_ll, nullptr, code_ll, nullptr, 1, nbits, 3) == want + matches);
  for (int s = 0; s < kD; ++s) want += (int64_t)hist_d[s] * (code_d[s].length + (s < 4 ? 0 : s / 2 - 1));
  CHECK(radnet_deflate_stream_bits(hist_ll, hist_d, code_ll, code_d, 0, nbits, 3) == want);
  if (failed) printf("  (while building the codes of the %s histograms)\n", what);
  free(header);
  free(code_d);
  free(code_ll);
  free(hist_d);
  free(hist_ll);
}

int main() {
  std::vector<uint32_t> zero_ll(kLl, 0), zero_d(kD, 0), single_ll(kLl, 0), single_d(kD, 0), single_d0(kD, 0), skewed_ll(kLl, 0), skewed_d(kD, 0);
  std::vector<uint32_t> uniform_ll(kLl, 1000), all_d(kD, 7), maximal_ll(kLl, 0xFFFFFFFFu), maximal_d(kD, 0xFFFFFFFFu);
  single_ll[65] = 12345;
  single_d[17] = 99;
  single_d0[0] = 3;
  uint64_t a = 1, b = 1;                                              // Fibonacci counts: Huffman's own trees are about 45 and 29 deep
  for (int s = 0; s < 45; ++s) {
    skewed_ll[(size_t)(s * 6 % kLl)] = (uint32_t)a;
    if (s < kD) skewed_d[(size_t)s] = (uint32_t)a;
    const uint64_t c = a + b;
    a = b, b = c;
  }
  build(zero_ll, zero_d, "empty");
  build(single_ll, single_d, "single-symbol");
  build(single_ll, single_d0, "single-symbol, distance symbol 0");
  build(skewed_ll, skewed_d, "skewed");
  build(uniform_ll, all_d, "all-30-distances");
  build(maximal_ll, maximal_d, "maximal");
  {                                                                   // refusals: nothing is written
    radnet_deflate_code code_ll[kLl], code_d[kD], before_ll[kLl], before_d[kD];
    uint8_t header[kHeaderBytes], header_before[kHeaderBytes];
    memset(code_ll, 0x5A, sizeof(code_ll));
    memset(code_d, 0x5A, sizeof(code_d));
    memset(header, 0x5A, sizeof(header));
    memcpy(before_ll, code_ll, sizeof(code_ll));
    memcpy(before_d, code_d, sizeof(code_d));
    memcpy(header_before, header, sizeof(header));
    int32_t nbits = -7;
    CHECK(radnet_deflate_build_codes_lz(nullptr, all_d.data(), code_ll, code_d, header, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), nullptr, code_ll, code_d, header, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), all_d.data(), nullptr, code_d, header, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), all_d.data(), code_ll, nullptr, header, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), all_d.data(), code_ll, code_d, nullptr, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), all_d.data(), code_ll, code_d, header, kHeaderBytes, nullptr) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), all_d.data(), code_ll, code_d, header, kHeaderBytes - 1, &nbits) == RADNET_ERR_ARG);
    CHECK(memcmp(before_ll, code_ll, sizeof(code_ll)) == 0 && memcmp(before_d, code_d, sizeof(code_d)) == 0);
    CHECK(memcmp(header_before, header, sizeof(header)) == 0 && nbits == -7);
    CHECK(radnet_deflate_lz_piece_cap(code_ll, code_d, 3) == RADNET_ERR_ARG);      // lengths of 0x5A5A
    CHECK(radnet_deflate_stream_bits(uniform_ll.data(), all_d.data(), code_ll, code_d, 0, 3, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_codes_lz(uniform_ll.data(), all_d.data(), code_ll, code_d, header, kHeaderBytes, &nbits) == RADNET_OK);
    CHECK(radnet_deflate_lz_piece_cap(nullptr, code_d, nbits) == RADNET_ERR_ARG && radnet_deflate_lz_piece_cap(code_ll, nullptr, nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_lz_piece_cap(code_ll, code_d, 2) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_lz_piece_cap(code_ll, code_d, RADNET_DEFLATE_HEADER_MAX_BITS + 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_stream_bits(nullptr, all_d.data(), code_ll, code_d, 0, nbits, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_stream_bits(uniform_ll.data(), all_d.data(), code_ll, nullptr, 0, nbits, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_stream_bits(uniform_ll.data(), nullptr, code_ll, code_d, 0, nbits, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_stream_bits(uniform_ll.data(), all_d.data(), code_ll, code_d, 16, nbits, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_stream_bits(uniform_ll.data(), all_d.data(), code_ll, code_d, 0, nbits, 0) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_stream_bits(uniform_ll.data(), all_d.data(), code_ll, code_d, 0, nbits, 65537) == RADNET_ERR_ARG);
    code_ll[256].length = 0, code_ll[256].bits = 0;
    CHECK(radnet_deflate_lz_piece_cap(code_ll, code_d, nbits) == RADNET_ERR_ARG);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
