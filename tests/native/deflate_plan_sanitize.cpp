// Driver for the AddressSanitizer + UBSan build of csrc/deflate_plan.cpp (tests/test_deflate_plan_sanitize.py builds and runs it):
// radnet_deflate_build_code and radnet_deflate_piece_cap on exactly-sized heap buffers, so a read past the 286 counts or a write past
// the code table or the header's 153 bytes is caught.
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

static const int kHeaderBytes = 153, kHeaderBits = 1222;

// builds the code of `counts` in buffers of exactly 286 counts, 286 entries and 153 bytes; checks what every code must satisfy
static void build(const std::vector<uint32_t>& counts, const char* what) {
  uint32_t* hist = (uint32_t*)malloc(sizeof(uint32_t) * RADNET_DEFLATE_SYMBOLS);
  memcpy(hist, counts.data(), sizeof(uint32_t) * RADNET_DEFLATE_SYMBOLS);
  radnet_deflate_code* code = (radnet_deflate_code*)malloc(sizeof(radnet_deflate_code) * RADNET_DEFLATE_SYMBOLS);
  uint8_t* header = (uint8_t*)malloc(kHeaderBytes);
  memset(code, 0xEE, sizeof(radnet_deflate_code) * RADNET_DEFLATE_SYMBOLS);
  memset(header, 0xEE, kHeaderBytes);
  int32_t nbits = -1;
  CHECK(radnet_deflate_build_code(hist, code, header, kHeaderBytes, &nbits) == RADNET_OK);
  CHECK(nbits == kHeaderBits);
  uint64_t kraft = 0;
  int used = 0, longest = 0;
  for (int s = 0; s < RADNET_DEFLATE_SYMBOLS; ++s) {
    const int l = code[s].length;
    CHECK(l <= 15 && (code[s].bits >> l) == 0);
    CHECK(l > 0 || hist[s] == 0);
    if (l) kraft += 1ull << (15 - l), ++used;
    longest = l > longest ? l : longest;
  }
  CHECK(kraft == 1ull << 15);
  CHECK(used >= 2 && code[256].length > 0);
  CHECK((header[0] & 7) == 4);                                        // BFINAL 0, BTYPE 10
  CHECK((header[kHeaderBytes - 1] >> (kHeaderBits & 7)) == 0);        // the bits behind the header are zero
  const int64_t cap = radnet_deflate_piece_cap(code, nbits, 1);
  CHECK(cap >= kHeaderBytes + (int64_t)longest * RADNET_DEFLATE_CHUNK / 8 + 16);
  if (failed) printf("  (while building the code of the %s histogram)\n", what);
  free(header);
  free(code);
  free(hist);
}

int main() {
  static_assert(sizeof(radnet_deflate_code) == 4, "radnet_deflate_code is 4 bytes");
  const int n = RADNET_DEFLATE_SYMBOLS;
  std::vector<uint32_t> zero(n, 0), single(n, 0), eob_only(n, 0), skewed(n, 0), uniform(n, 1000), maximal(n, 0xFFFFFFFFu), two(n, 0);
  single[65] = 12345;
  eob_only[256] = 3;
  two[0] = 1, two[256] = 1;
  uint64_t a = 1, b = 1;                                              // Fibonacci counts: Huffman's own tree is about 45 deep
  for (int s = 0; s < 45; ++s) {
    skewed[(size_t)(s * 6 % n)] = (uint32_t)a;
    const uint64_t c = a + b;
    a = b, b = c;
  }
  build(zero, "zero");
  build(single, "single-symbol");
  build(eob_only, "end-of-block only");
  build(two, "two-symbol");
  build(skewed, "skewed");
  build(uniform, "uniform");
  build(maximal, "maximal");
  {                                                                   // a mix of huge and tiny counts: the sums need 64 bits
    std::vector<uint32_t> mixed(n, 1);
    for (int s = 0; s < n; s += 3) mixed[(size_t)s] = 0xFFFFFFFFu - (uint32_t)s;
    build(mixed, "mixed");
  }
  {                                                                   // refusals: nothing is written
    radnet_deflate_code code[RADNET_DEFLATE_SYMBOLS], before[RADNET_DEFLATE_SYMBOLS];
    uint8_t header[kHeaderBytes], header_before[kHeaderBytes];
    memset(code, 0x5A, sizeof(code));
    memset(header, 0x5A, sizeof(header));
    memcpy(before, code, sizeof(code));
    memcpy(header_before, header, sizeof(header));
    int32_t nbits = -7;
    CHECK(radnet_deflate_build_code(nullptr, code, header, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_code(uniform.data(), nullptr, header, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_code(uniform.data(), code, nullptr, kHeaderBytes, &nbits) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_code(uniform.data(), code, header, kHeaderBytes, nullptr) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_build_code(uniform.data(), code, header, kHeaderBytes - 1, &nbits) == RADNET_ERR_ARG);
    CHECK(memcmp(before, code, sizeof(code)) == 0 && memcmp(header_before, header, sizeof(header)) == 0 && nbits == -7);
    CHECK(radnet_deflate_piece_cap(nullptr, 3, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_piece_cap(code, 3, 1) == RADNET_ERR_ARG);    // lengths of 0x5A5A
    CHECK(radnet_deflate_build_code(uniform.data(), code, header, kHeaderBytes, &nbits) == RADNET_OK);
    CHECK(radnet_deflate_piece_cap(code, 2, 1) == RADNET_ERR_ARG && radnet_deflate_piece_cap(code, RADNET_DEFLATE_HEADER_MAX_BITS + 1, 1) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_piece_cap(code, nbits, -1) == RADNET_ERR_ARG && radnet_deflate_piece_cap(code, nbits, 16) == RADNET_ERR_ARG);
    CHECK(radnet_deflate_piece_cap(code, nbits, 1) == kHeaderBytes + 9 * RADNET_DEFLATE_CHUNK / 8 + 16);      // 286 equal counts: lengths 8 and 9
    code[256].length = 0, code[256].bits = 0;
    CHECK(radnet_deflate_piece_cap(code, nbits, 1) == RADNET_ERR_ARG);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
