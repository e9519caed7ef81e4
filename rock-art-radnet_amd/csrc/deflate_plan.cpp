// ---- host side of the device deflate (deflate.hip, deflate_lz.hip): the codes of an image, their dynamic block header, sizes -----
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).
#include <algorithm>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "radnet_hip.h"

namespace {

constexpr int kSymbols = RADNET_DEFLATE_SYMBOLS, kEob = 256, kMaxLen = 15;
constexpr int kDistSymbols = RADNET_DEFLATE_DIST_SYMBOLS;
constexpr int kHeaderBits = 3 + 5 + 5 + 4 + 19 * 3 + (kSymbols + 1) * 4;      // 1222
constexpr int kHeaderBitsLz = 3 + 5 + 5 + 4 + 19 * 3 + (kSymbols + kDistSymbols) * 4;      // 1338

struct BitWriter {
  uint8_t* out;
  int n = 0;
  void put(unsigned value, int bits) {          // least significant bit first
    for (int k = 0; k < bits; ++k, ++n)
      if ((value >> k) & 1) out[n >> 3] |= (uint8_t)(1u << (n & 7));
  }
  void put_code(unsigned code, int bits) {      // a Huffman code: most significant bit first
    for (int k = bits - 1; k >= 0; --k, ++n)
      if ((code >> k) & 1) out[n >> 3] |= (uint8_t)(1u << (n & 7));
  }
};

// Huffman depths of the symbols with weight[s] > 0 (at least two of them) out of n
void huffman_depths(const uint64_t* weight, int n, int* depth) {
  struct Node {
    uint64_t w;
    int left, right;
  };
  std::vector<Node> nodes;
  typedef std::pair<uint64_t, int> Item;          // weight, node; ties go to the lower node index, so the tree is a function of the counts
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  for (int s = 0; s < n; ++s)
    if (weight[s]) {
      nodes.push_back(Node{weight[s], -1 - s, 0});
      heap.push(Item(weight[s], (int)nodes.size() - 1));
    }
  while (heap.size() > 1) {
    const Item a = heap.top();
    heap.pop();
    const Item b = heap.top();
    heap.pop();
    nodes.push_back(Node{a.first + b.first, a.second, b.second});
    heap.push(Item(a.first + b.first, (int)nodes.size() - 1));
  }
  std::vector<std::pair<int, int>> stack(1, std::make_pair(heap.top().second, 0));
  while (!stack.empty()) {
    const std::pair<int, int> t = stack.back();
    stack.pop_back();
    const Node& nd = nodes[(size_t)t.first];
    if (nd.left < 0) {
      depth[-1 - nd.left] = t.second;
    } else {
      stack.push_back(std::make_pair(nd.left, t.second + 1));
      stack.push_back(std::make_pair(nd.right, t.second + 1));
    }
  }
}

// A complete canonical code of at most kMaxLen bits for the n symbols with weight[s] > 0 (at least two of them, n <= kSymbols):
// Huffman's lengths, and where the tree is deeper than kMaxLen, shortened and repaired to a Kraft sum of 1
void limited_code(const uint64_t* weight, int n, int* length, radnet_deflate_code* code) {
  int depth[kSymbols] = {0};
  huffman_depths(weight, n, depth);
  // at most kMaxLen bits: fold the deeper levels into the last one, then move leaves down until the Kraft sum is 1 again
  int per_len[kMaxLen + 1] = {0};
  for (int s = 0; s < n; ++s)
    if (weight[s]) ++per_len[std::min(depth[s], kMaxLen)];
  uint32_t kraft = 0;
  for (int l = 1; l <= kMaxLen; ++l) kraft += (uint32_t)per_len[l] << (kMaxLen - l);
  while (kraft > (1u << kMaxLen)) {               // each round frees 2^-15: one leaf of the last level pairs with a leaf moved down from above
    --per_len[kMaxLen];
    for (int l = kMaxLen - 1; l > 0; --l)
      if (per_len[l]) {
        --per_len[l];
        per_len[l + 1] += 2;
        break;
      }
    --kraft;
  }
  // the shortest lengths to the heaviest symbols; among equal weights the lower symbol first
  int order[kSymbols], m = 0;
  for (int s = 0; s < n; ++s)
    if (weight[s]) order[m++] = s;
  std::stable_sort(order, order + m, [&](int a, int b) { return weight[a] > weight[b]; });
  for (int s = 0; s < n; ++s) length[s] = 0;
  for (int l = 1, k = 0; l <= kMaxLen; ++l)
    for (int c = 0; c < per_len[l]; ++c) length[order[k++]] = l;
  // canonical codes (RFC 1951, 3.2.2)
  unsigned next[kMaxLen + 2] = {0}, c = 0;
  for (int l = 1; l <= kMaxLen; ++l) {
    c = (c + (unsigned)per_len[l - 1]) << 1;
    next[l] = c;
  }
  for (int s = 0; s < n; ++s) code[s] = radnet_deflate_code{(uint16_t)(length[s] ? next[length[s]]++ : 0), (uint16_t)length[s]};
}

// the literal/length weights of a histogram: end-of-block always counts; with fewer than two used symbols literal 0 joins them
void literal_weights(const uint32_t* hist, uint64_t* weight) {
  int used = 0;
  for (int s = 0; s < kSymbols; ++s) {
    weight[s] = hist[s];
    if (s == kEob && !weight[s]) weight[s] = 1;
    used += weight[s] != 0;
  }
  if (used < 2) weight[0] = 1;                    // end-of-block alone: literal 0 joins it
}

// BFINAL 0, BTYPE 10, HLIT 29, HDIST, HCLEN 15 and the code-length code that gives 4 bits to each of 0..15 and none to 16..18
void header_front(BitWriter& w, int hdist) {
  w.put(0, 1);                                    // BFINAL
  w.put(2, 2);                                    // BTYPE 10
  w.put(kSymbols - 257, 5);                       // HLIT
  w.put((unsigned)hdist, 5);                      // HDIST
  w.put(15, 4);                                   // HCLEN: all 19 lengths of the code-length code follow
  static const int kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 19; ++i) w.put(kOrder[i] < 16 ? 4 : 0, 3);
}

// RFC 1951, 3.2.5: the extra bits of length symbol 257 + k and of distance symbol k
const int kLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const int kDistExtra[kDistSymbols] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

bool legal_code(const radnet_deflate_code* code, int n) {
  for (int s = 0; s < n; ++s)
    if (code[s].length > kMaxLen || (code[s].bits >> code[s].length) != 0) return false;
  return true;
}

}  // namespace

extern "C" int radnet_deflate_build_code(const uint32_t* hist, radnet_deflate_code* code, uint8_t* header, int32_t header_cap, int32_t* header_nbits) {
  if (!hist || !code || !header || !header_nbits || header_cap < (kHeaderBits + 7) / 8) return RADNET_ERR_ARG;
  uint64_t weight[kSymbols];
  literal_weights(hist, weight);
  int length[kSymbols];
  limited_code(weight, kSymbols, length, code);
  for (int i = 0; i < (kHeaderBits + 7) / 8; ++i) header[i] = 0;
  BitWriter w{header};
  header_front(w, 0);
  for (int s = 0; s < kSymbols; ++s) w.put_code((unsigned)length[s], 4);      // 16 codes of 4 bits: the canonical code of v is v
  w.put_code(1, 4);                               // the distance code: symbol 0 alone, one bit
  *header_nbits = w.n;
  return RADNET_OK;
}

extern "C" int64_t radnet_deflate_piece_cap(const radnet_deflate_code* code, int32_t header_nbits, int32_t dist_nbits) {
  if (!code || header_nbits < 3 || header_nbits > RADNET_DEFLATE_HEADER_MAX_BITS || dist_nbits < 0 || dist_nbits > 15) return RADNET_ERR_ARG;
  int longest = 0, longest_match = 0;
  for (int s = 0; s < kSymbols; ++s) {
    const int l = code[s].length;
    if (l > kMaxLen || (code[s].bits >> l) != 0) return RADNET_ERR_ARG;
    longest = std::max(longest, l);
    if (s > kEob) longest_match = std::max(longest_match, l);
  }
  if (code[kEob].length == 0) return RADNET_ERR_ARG;
  const int w = std::max(longest, (longest_match + 5 + dist_nbits + 2) / 3);
  return (int64_t)((header_nbits + 7) / 8) + ((int64_t)w * RADNET_DEFLATE_CHUNK + 7) / 8 + 16;
}

extern "C" int radnet_deflate_build_codes_lz(const uint32_t* hist_ll, const uint32_t* hist_d, radnet_deflate_code* code_ll, radnet_deflate_code* code_d,
                                             uint8_t* header, int32_t header_cap, int32_t* header_nbits) {
  if (!hist_ll || !hist_d || !code_ll || !code_d || !header || !header_nbits || header_cap < (kHeaderBitsLz + 7) / 8) return RADNET_ERR_ARG;
  uint64_t weight[kSymbols];
  literal_weights(hist_ll, weight);
  int length_ll[kSymbols], length_d[kDistSymbols];
  limited_code(weight, kSymbols, length_ll, code_ll);
  int used = 0, only = 0;
  for (int s = 0; s < kDistSymbols; ++s) {
    weight[s] = hist_d[s];
    if (weight[s]) ++used, only = s;
  }
  if (used == 0) weight[0] = weight[1] = 1;       // no match at all: a complete code of two one-bit symbols nothing uses
  if (used == 1) weight[only == 0 ? 1 : 0] = 1;   // one distance symbol: symbol 0 (or 1) joins it
  limited_code(weight, kDistSymbols, length_d, code_d);
  for (int i = 0; i < (kHeaderBitsLz + 7) / 8; ++i) header[i] = 0;
  BitWriter w{header};
  header_front(w, kDistSymbols - 1);
  for (int s = 0; s < kSymbols; ++s) w.put_code((unsigned)length_ll[s], 4);
  for (int s = 0; s < kDistSymbols; ++s) w.put_code((unsigned)length_d[s], 4);
  *header_nbits = w.n;
  return RADNET_OK;
}

extern "C" int64_t radnet_deflate_lz_piece_cap(const radnet_deflate_code* code_ll, const radnet_deflate_code* code_d, int32_t header_nbits) {
  if (!code_ll || !code_d || header_nbits < 3 || header_nbits > RADNET_DEFLATE_HEADER_MAX_BITS) return RADNET_ERR_ARG;
  if (!legal_code(code_ll, kSymbols) || !legal_code(code_d, kDistSymbols) || code_ll[kEob].length == 0) return RADNET_ERR_ARG;
  int longest = 0, longest_match = 0;
  for (int s = 0; s < kSymbols; ++s) longest = std::max(longest, (int)code_ll[s].length);
  for (int s = kEob + 1; s < kSymbols; ++s)
    for (int d = 0; d < kDistSymbols; ++d)
      longest_match = std::max(longest_match, code_ll[s].length + kLengthExtra[s - 257] + code_d[d].length + kDistExtra[d]);
  const int w = std::max(longest, (longest_match + 2) / 3);
  return (int64_t)((header_nbits + 7) / 8) + ((int64_t)w * RADNET_DEFLATE_CHUNK + 7) / 8 + 16;
}

extern "C" int64_t radnet_deflate_stream_bits(const uint32_t* hist_ll, const uint32_t* hist_d, const radnet_deflate_code* code_ll,
                                              const radnet_deflate_code* code_d, int32_t dist_nbits, int32_t header_nbits, int64_t chunks) {
  if (!hist_ll || !code_ll || (hist_d != nullptr) != (code_d != nullptr) || header_nbits < 3 || header_nbits > RADNET_DEFLATE_HEADER_MAX_BITS ||
      dist_nbits < 0 || dist_nbits > kMaxLen || chunks < 1 || chunks > 65536)
    return RADNET_ERR_ARG;
  if (!legal_code(code_ll, kSymbols) || (code_d && !legal_code(code_d, kDistSymbols))) return RADNET_ERR_ARG;
  int64_t bits = chunks * header_nbits, matches = 0;
  for (int s = 0; s < kSymbols; ++s) {
    bits += (int64_t)hist_ll[s] * (code_ll[s].length + (s > kEob ? kLengthExtra[s - 257] : 0));
    if (s > kEob) matches += hist_ll[s];
  }
  if (!hist_d) return bits + matches * dist_nbits;
  for (int s = 0; s < kDistSymbols; ++s) bits += (int64_t)hist_d[s] * (code_d[s].length + kDistExtra[s]);
  return bits;
}
