// ---- the unit decoder of the device inflate: ONE kernel body for inflate.hip (run-length streams) and inflate_lz.hip (any stream) ----
// A workgroup is one wave and takes one unit; the compressed bytes pass through a window in LDS, the code tables stand in LDS (a
// direct table for codes of at most kPrimaryBits bits, the canonical count / sorted-symbol walk for longer ones), lane 0 decodes a
// batch of tokens, the wave sums their lengths by prefix and all lanes expand them.  kEmit: measure (a record per unit, no output)
// or emit (the bytes of the chained units).  kLz: false takes matches of distance 1 alone (another distance is NOT_RLE) and writes
// bytes; true takes the distance whole (RFC 1951 3.2.5), measures reach / far_matches and emits literals into `out` and, for every
// byte, the position it copies into `src` (contract: include/radnet_hip.h).  wave64, integers only, no inline assembly, no waits
// between workgroups.  Everything stands in an unnamed namespace: each unit that includes this gets kernels of its own.
#pragma once
#include "radnet_internal.h"

namespace {

constexpr int kWave = 64, kBatch = 64, kPrimaryBits = 10, kLit = 288, kDist = 32;
constexpr int kWinBytes = 4096;      // the window; refilled when fewer than kWinSlack bytes of it lie behind the position
constexpr int kWinSlack = 768;       // more than the longest dynamic header (14 + 57 + 316 * 14 bits) and than a batch (64 * 48 bits)
constexpr unsigned kMaxSymbols = RADNET_INFLATE_UNIT_MAX_SYMBOLS;
__constant__ unsigned char kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

typedef unsigned long long u64;

// at least 25 bits of the stream from bit `pos` on, zero beyond it: byte loads, so z needs no alignment
struct GlobalBits {
  const uint8_t* z;
  long long n;
  __device__ __forceinline__ unsigned peek(u64 pos) const {
    const long long b = (long long)(pos >> 3);
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (b + k < n) v |= (unsigned)z[b + k] << (8 * k);
    return v >> (pos & 7);
  }
};

// 32 bits from bit `pos` on out of the LDS window, whose word 0 holds the stream from bit base_bit on
struct WindowBits {
  const unsigned* win;
  u64 base_bit;
  __device__ __forceinline__ unsigned peek(u64 pos) const {
    const unsigned r = (unsigned)(pos - base_bit), w = r >> 5;
    const u64 v = ((u64)win[w + 1] << 32) | win[w];
    return (unsigned)(v >> (r & 31));
  }
};

// The dynamic block header behind BFINAL and BTYPE, by zlib's rule (include/radnet_hip.h, radnet_inflate_find_blocks): RADNET_INFLATE_OK,
// BAD_HEADER or PAST_END; sink(i, length) receives the lengths of the literal/length symbols i < nlen and of the distance symbols
// i - nlen in order.  Nothing is kept in an array: the code-length code's lengths are packed 3 bits per symbol, its counts 8 bits per
// length, and a code is complete when its Kraft sum says so.
template <class Bits, class Sink>
__device__ __forceinline__ int parse_dynamic(const Bits& bits, u64& pos, u64 nbits, Sink&& sink, int& nlen, int& ndist) {
  unsigned v = bits.peek(pos);
  pos += 14;
  if (pos > nbits) return RADNET_INFLATE_PAST_END;
  nlen = 257 + (int)(v & 31), ndist = 1 + (int)((v >> 5) & 31);
  const int ncode = 4 + (int)((v >> 10) & 15);
  if (nlen > 286 || ndist > 30) return RADNET_INFLATE_BAD_HEADER;
  u64 cl = 0, cnt = 0;
  unsigned kraft = 0;
  for (int i = 0; i < ncode; ++i) {
    const unsigned l = bits.peek(pos) & 7;
    pos += 3;
    cl |= (u64)l << (3 * kClOrder[i]);
    if (l) kraft += 128u >> l, cnt += 1ull << (8 * l);
  }
  if (pos > nbits) return RADNET_INFLATE_PAST_END;
  if (kraft != 128u) return RADNET_INFLATE_BAD_HEADER;
  const int total = nlen + ndist;
  int have = 0, prev = 0, eob = 0;
  unsigned kraft_lit = 0, kraft_dist = 0;
  int used_lit = 0, used_dist = 0, max_lit = 0, max_dist = 0;
  while (have < total) {
    v = bits.peek(pos);
    int code = 0, first = 0, sym = -1, l = 1;
    for (; l <= 7; ++l) {                        // the canonical walk: codes of length l are numbered from `first`
      code |= (int)((v >> (l - 1)) & 1);
      const int c = (int)((cnt >> (8 * l)) & 255);
      if (code - c < first) {
        int k = code - first;
        for (int s = 0; s < 19; ++s)
          if ((int)((cl >> (3 * s)) & 7) == l && k-- == 0) {
            sym = s;
            break;
          }
        break;
      }
      first = (first + c) << 1;
      code <<= 1;
    }
    if (sym < 0) return RADNET_INFLATE_BAD_HEADER;      // not reached: the code is complete
    pos += l;
    if (pos > nbits) return RADNET_INFLATE_PAST_END;
    int rep = 1, val = sym;
    if (sym >= 16) {
      if (sym == 16 && have == 0) return RADNET_INFLATE_BAD_HEADER;
      const int eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
      rep = (sym == 18 ? 11 : 3) + (int)(bits.peek(pos) & ((1u << eb) - 1));
      pos += eb;
      if (pos > nbits) return RADNET_INFLATE_PAST_END;
      val = sym == 16 ? prev : 0;
      if (have + rep > total) return RADNET_INFLATE_BAD_HEADER;
    }
    prev = val;
    for (int r = 0; r < rep; ++r, ++have) {
      sink(have, val);
      if (!val) continue;
      if (have < nlen) {
        kraft_lit += 32768u >> val, ++used_lit, max_lit = max(max_lit, val);
        if (have == 256) eob = val;
      } else {
        kraft_dist += 32768u >> val, ++used_dist, max_dist = max(max_dist, val);
      }
    }
  }
  if (!eob) return RADNET_INFLATE_BAD_HEADER;
  if (kraft_lit != 32768u && !(used_lit == 1 && max_lit == 1)) return RADNET_INFLATE_BAD_HEADER;
  if (kraft_dist != 32768u && used_dist != 0 && !(used_dist == 1 && max_dist == 1)) return RADNET_INFLATE_BAD_HEADER;
  return RADNET_INFLATE_OK;
}

enum { kActHeader = 0, kActStored, kActTable, kActTokens, kActAfter, kActDone };

struct UnitShared {
  unsigned win[kWinBytes / 4 + 2];
  unsigned short primary[1 << kPrimaryBits];      // symbol | length << 9 for the codes of at most kPrimaryBits bits, by their reversed bits; 0: none
  unsigned short lsorted[kLit], lcode[kLit], lcount[16], dcount[16], work[32];
  unsigned char llen[kLit], dlen[kDist], dsorted[kDist];
  unsigned char tok_byte[kBatch];
  unsigned short tok_len[kBatch];
  unsigned short tok_dist[kBatch];                // kLz: a match's distance - 1 (32768 does not fit 15 bits, 32767 does); a literal has tok_len 1
  unsigned tok_end[kBatch];
  u64 pos;
  long long wbase, stored_src;
  int act, status, fixed, bfinal, n_tok, stored_len;
};

// what lane 0 alone keeps of a unit
struct UnitState {
  unsigned symbols = 0, blocks = 0, flags = 0, last = 0, prev = 0;
  unsigned reach = 0, far_matches = 0;            // kLz
  u64 produced = 0;
  bool seen = false;
};

// one symbol of a canonical code from the bits v (first bit of the code in bit 0): the symbol and its length, or -1
template <class T>
__device__ __forceinline__ int walk_code(unsigned v, const unsigned short* count, const T* sorted, int& len) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((v >> (l - 1)) & 1);
    const int c = count[l];
    if (code - c < first) {
      len = l;
      return sorted[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// lane 0: up to kBatch tokens of the current block into sh.tok_*; RADNET_INFLATE_OK or the status that ends the unit
template <bool kLz>
__device__ __forceinline__ int decode_batch(UnitShared& sh, const WindowBits& bits, u64& pos, u64 nbits, UnitState& st, int& n_tok, bool& eob) {
  int nt = 0;
  eob = false;
  n_tok = 0;
  while (nt < kBatch) {
    if (st.symbols >= kMaxSymbols) return RADNET_INFLATE_TOO_LONG;
    unsigned v = bits.peek(pos);
    const unsigned e = sh.primary[v & ((1u << kPrimaryBits) - 1)];
    int sym, l;
    if (e) {
      sym = (int)(e & 511), l = (int)(e >> 9);
    } else {
      sym = walk_code(v, sh.lcount, sh.lsorted, l);
      if (sym < 0) return pos + 15 > nbits ? RADNET_INFLATE_PAST_END : RADNET_INFLATE_BAD_CODE;
    }
    pos += l;
    if (pos > nbits) return RADNET_INFLATE_PAST_END;
    ++st.symbols;
    if (sym < 256) {
      sh.tok_byte[nt] = (unsigned char)sym, sh.tok_len[nt] = 1, ++nt;
      st.prev = st.last = (unsigned)sym, st.flags |= RADNET_INFLATE_FLAG_LAST_KNOWN, st.seen = true, ++st.produced;
      continue;
    }
    if (sym == 256) {
      eob = true;
      break;
    }
    if (sym >= 286) return RADNET_INFLATE_BAD_CODE;
    const int s = sym - 257;                      // RFC 1951, 3.2.5
    int base, eb;
    if (s < 8) base = 3 + s, eb = 0;
    else if (s == 28) base = 258, eb = 0;
    else eb = (s - 4) >> 2, base = 3 + ((4 + (s & 3)) << eb);
    const int length = base + (int)(bits.peek(pos) & ((1u << eb) - 1));
    pos += eb;
    if (pos > nbits) return RADNET_INFLATE_PAST_END;
    v = bits.peek(pos);
    int dl;
    const int d = walk_code(v, sh.dcount, sh.dsorted, dl);
    if (d < 0) return pos + 15 > nbits ? RADNET_INFLATE_PAST_END : RADNET_INFLATE_BAD_CODE;
    pos += dl;
    if (pos > nbits) return RADNET_INFLATE_PAST_END;
    if (d >= 30) return RADNET_INFLATE_BAD_CODE;
    if (kLz) {
      const int deb = d < 4 ? 0 : (d - 2) >> 1;   // distance symbols 0..29: 1..4 without extra bits, then two symbols per width up to 13
      const int dist = (d < 4 ? d + 1 : 1 + ((2 + (d & 1)) << deb)) + (int)(bits.peek(pos) & ((1u << deb) - 1));
      pos += deb;
      if (pos > nbits) return RADNET_INFLATE_PAST_END;
      if ((u64)dist > st.produced) st.reach = max(st.reach, (unsigned)((u64)dist - st.produced));
      st.far_matches += dist != 1;
      sh.tok_len[nt] = (unsigned short)length, sh.tok_dist[nt] = (unsigned short)(dist - 1), ++nt;
    } else {
      if (d != 0) return RADNET_INFLATE_NOT_RLE;
      if (!st.seen) st.seen = true, st.flags |= RADNET_INFLATE_FLAG_LEAD_MATCH;
      sh.tok_byte[nt] = (unsigned char)st.prev, sh.tok_len[nt] = (unsigned short)length, ++nt;
    }
    st.produced += (unsigned)length;
  }
  n_tok = nt;
  return RADNET_INFLATE_OK;
}

// The zlib stream a unit belongs to, as the body sees it: the n bytes at z, whose bit 0 is bit `bit_base` of what the caller's
// start_bit / end_bit count in, and whose inflated bytes are [out_base, out_end) of `out` / `src`.  One stream alone (inflate.hip,
// inflate_lz.hip): {z, n, 0, 0, out_len}.  One of many (inflate_many.hip): the table entry that holds the unit's start; a start
// that no stream holds gets n = 0 and bit_base = the start itself, which the reading rule ends with PAST_END before any byte is read.
struct UnitSpan {
  const uint8_t* z;
  long long n;
  unsigned bit_base;
  long long out_base, out_end;
};

// the bit the caller gave unit u (measure: its record, emit: its link), in the caller's count
template <bool kEmit, bool kLz>
__device__ __forceinline__ unsigned unit_start_bit(const void* units, const radnet_inflate_link* links, int u) {
  if (kEmit) return links[u].start_bit;
  return kLz ? static_cast<const radnet_inflate_lz_unit*>(units)[u].start_bit : static_cast<const radnet_inflate_unit*>(units)[u].start_bit;
}

// One unit by one wave, the whole body.  units: radnet_inflate_unit (kLz: radnet_inflate_lz_unit) records, measure only; links, out:
// emit only; src: kLz emit only.  Everything read lies in span.z[0 .. span.n), everything written in [span.out_base, span.out_end).
template <bool kEmit, bool kLz>
__device__ __forceinline__ void inflate_unit(UnitShared& sh, const UnitSpan span, void* __restrict__ units, const radnet_inflate_link* __restrict__ links,
                                             uint8_t* __restrict__ out, uint32_t* __restrict__ src) {
  const uint8_t* __restrict__ z = span.z;
  const long long n = span.n;
  const int lane = (int)threadIdx.x, u = (int)blockIdx.x;
  const u64 nbits = 8ull * (u64)n;
  UnitState st;
  const unsigned start = unit_start_bit<kEmit, kLz>(units, links, u) - span.bit_base;      // from here on bits count inside the stream
  long long out_pos = 0, out_stop = 0;            // emit: where the next byte goes and where the unit's bytes end; every lane keeps them
  if (kEmit) {
    const radnet_inflate_link link = links[u];
    out_pos = link.out_offset;
    out_stop = min(link.out_offset + (long long)link.out_bytes, span.out_end);
    if (out_pos < span.out_base || out_pos > out_stop) return;      // a table no chain gives: nothing is written
    st.prev = link.prev_byte & 255u;
  }
  if (lane == 0) {
    sh.pos = start, sh.wbase = -1, sh.act = kActHeader, sh.status = RADNET_INFLATE_OK, sh.fixed = 0, sh.bfinal = 0, sh.n_tok = 0;
    if ((u64)start >= nbits) sh.status = RADNET_INFLATE_PAST_END, sh.act = kActDone;
  }
  __syncthreads();
  for (;;) {
    const int act = sh.act;
    u64 pos = sh.pos;
    long long wbase = sh.wbase;
    __syncthreads();                              // every lane holds the state; lane 0 may write it again
    if (act == kActDone) break;
    const long long byte = (long long)(pos >> 3);
    if (act != kActStored && (wbase < 0 || byte < wbase || byte + kWinSlack > wbase + kWinBytes)) {
      wbase = byte;
      uint8_t* win8 = reinterpret_cast<uint8_t*>(sh.win);
      for (int i = lane; i < kWinBytes + 8; i += kWave) win8[i] = wbase + i < n ? z[wbase + i] : (uint8_t)0;
      if (lane == 0) sh.wbase = wbase;
      __syncthreads();
    }
    const WindowBits bits{sh.win, 8ull * (u64)wbase};
    int status = RADNET_INFLATE_OK;
    if (act == kActHeader) {
      if (lane == 0) {
        unsigned v = bits.peek(pos);
        pos += 3;
        int next = kActTable;
        if (pos > nbits) {
          status = RADNET_INFLATE_PAST_END;
        } else {
          const int btype = (int)((v >> 1) & 3);
          sh.bfinal = (int)(v & 1), sh.fixed = btype == 1;
          if (btype == 0) {
            pos = (pos + 7) & ~7ull;
            v = bits.peek(pos);
            pos += 32;
            const unsigned len = v & 0xffffu;
            if (pos > nbits) status = RADNET_INFLATE_PAST_END;
            else if (len != ((v >> 16) ^ 0xffffu)) status = RADNET_INFLATE_STORED_MISMATCH;
            else {
              sh.stored_src = (long long)(pos >> 3), sh.stored_len = (int)len;
              pos += 8ull * len;
              if (pos > nbits) status = RADNET_INFLATE_PAST_END;
              next = kActStored;
            }
          } else if (btype == 2) {
            for (int i = 0; i < kLit; ++i) sh.llen[i] = 0;
            for (int i = 0; i < kDist; ++i) sh.dlen[i] = 0;
            int nlen = 0, ndist = 0;
            unsigned char* llen = sh.llen;
            unsigned char* dlen = sh.dlen;
            const int* nl = &nlen;
            status = parse_dynamic(bits, pos, nbits, [llen, dlen, nl](int i, int l) {
              if (i < *nl) llen[i] = (unsigned char)l; else dlen[i - *nl] = (unsigned char)l;
            }, nlen, ndist);
          } else if (btype == 3) {
            status = RADNET_INFLATE_BAD_HEADER;
          }
        }
        sh.pos = pos, sh.act = status ? kActDone : next, sh.status = status;
      }
    } else if (act == kActStored) {
      const long long from = sh.stored_src;
      const int len = sh.stored_len;
      if (kEmit) {
        const long long t = min((long long)len, out_stop - out_pos);
        for (long long j = lane; j < t; j += kWave) {
          out[out_pos + j] = z[from + j];
          if (kLz) src[out_pos + j] = (uint32_t)(out_pos + j);
        }
        out_pos += len;
      }
      if (lane == 0) {
        if (len > 0) {
          st.prev = st.last = z[from + len - 1];
          st.flags |= RADNET_INFLATE_FLAG_LAST_KNOWN, st.seen = true, st.produced += (unsigned)len;
        }
      }
      __syncthreads();                            // the lengths read above are lane 0's to write again
      if (lane == 0) sh.act = kActAfter;
    } else if (act == kActTable) {
      if (sh.fixed) {                             // RFC 1951, 3.2.6
        for (int s = lane; s < kLit; s += kWave) sh.llen[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        if (lane < kDist) sh.dlen[lane] = 5;
      }
      for (int i = lane; i < (1 << kPrimaryBits); i += kWave) sh.primary[i] = 0;
      __syncthreads();
      if (lane == 0) {
        unsigned short* offs = sh.work;           // where the symbols of a length start in the sorted list
        unsigned short* next = sh.work + 16;      // the next canonical code of a length (RFC 1951, 3.2.2)
        for (int l = 0; l < 16; ++l) sh.lcount[l] = sh.dcount[l] = 0;
        for (int s = 0; s < kLit; ++s) ++sh.lcount[sh.llen[s]];
        for (int s = 0; s < kDist; ++s) ++sh.dcount[sh.dlen[s]];
        sh.lcount[0] = sh.dcount[0] = 0;
        unsigned code = 0;
        offs[0] = offs[1] = 0, next[0] = 0;
        for (int l = 1; l < 16; ++l) {
          code = (code + sh.lcount[l - 1]) << 1;
          next[l] = (unsigned short)code;
          if (l > 1) offs[l] = (unsigned short)(offs[l - 1] + sh.lcount[l - 1]);
        }
        for (int s = 0; s < kLit; ++s) {
          const int l = sh.llen[s];
          if (l) sh.lsorted[offs[l]++] = (unsigned short)s, sh.lcode[s] = next[l]++;
        }
        offs[0] = offs[1] = 0;
        for (int l = 2; l < 16; ++l) offs[l] = (unsigned short)(offs[l - 1] + sh.dcount[l - 1]);
        for (int s = 0; s < kDist; ++s) {
          const int l = sh.dlen[s];
          if (l) sh.dsorted[offs[l]++] = (unsigned char)s;
        }
      }
      __syncthreads();
      for (int s = lane; s < kLit; s += kWave) {
        const int l = sh.llen[s];
        if (l && l <= kPrimaryBits) {
          const unsigned rev = __brev((unsigned)sh.lcode[s]) >> (32 - l);
          for (unsigned k = rev; k < (1u << kPrimaryBits); k += 1u << l) sh.primary[k] = (unsigned short)(s | (l << 9));
        }
      }
      if (lane == 0) sh.act = kActTokens;
    } else if (act == kActTokens) {
      if (lane == 0) {
        int n_tok = 0;
        bool eob = false;
        status = decode_batch<kLz>(sh, bits, pos, nbits, st, n_tok, eob);
        sh.n_tok = status ? 0 : n_tok;
        sh.pos = pos, sh.status = status, sh.act = status ? kActDone : eob ? kActAfter : kActTokens;
      }
      __syncthreads();
      if (kEmit) {
        const int nt = sh.n_tok;
        unsigned incl = lane < nt ? sh.tok_len[lane] : 0u;
        for (int d = 1; d < kWave; d <<= 1) {
          const unsigned o = __shfl_up(incl, d, kWave);
          if (lane >= d) incl += o;
        }
        sh.tok_end[lane] = incl;
        const long long total = (long long)__shfl(incl, kWave - 1, kWave);
        __syncthreads();
        const long long t = min(total, out_stop - out_pos);
        for (long long j = lane; j < t; j += kWave) {
          int lo = 0, hi = nt - 1;                // the first token whose end lies behind j
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sh.tok_end[mid] > (unsigned)j) hi = mid; else lo = mid + 1;
          }
          if (!kLz) {
            out[out_pos + j] = sh.tok_byte[lo];
          } else {
            const long long p = out_pos + j;      // span.out_base <= p < out_stop <= span.out_end < 2^31
            const unsigned len = sh.tok_len[lo];
            if (len == 1) {
              out[p] = sh.tok_byte[lo], src[p] = (uint32_t)p;
            } else {                              // byte k of a match that begins at m copies m - dist + k % dist: a run points in front of itself directly
              const unsigned k = (unsigned)j - (sh.tok_end[lo] - len), dist = (unsigned)sh.tok_dist[lo] + 1u;
              const long long from = out_pos + (long long)(sh.tok_end[lo] - len) - (long long)dist + (long long)(k % dist);
              src[p] = (uint32_t)(from < span.out_base ? p : from);      // a chained unit never reaches in front of its stream (RADNET_INFLATE_CHAIN_REACH)
            }
          }
        }
        out_pos += total;
      }
    } else {                                      // kActAfter: a block is done
      if (lane == 0) {
        ++st.blocks;
        if (sh.bfinal) {
          st.flags |= RADNET_INFLATE_FLAG_FINAL;
          sh.act = kActDone;
        } else {
          const unsigned v = bits.peek(pos);
          sh.act = (pos + 3 <= nbits && ((v >> 1) & 3) == 2) ? kActDone : kActHeader;      // the next dynamic header begins another unit
        }
      }
    }
    __syncthreads();
  }
  if (!kEmit && lane == 0) {
    const int status = sh.status;
    if (kLz) {
      radnet_inflate_lz_unit r = {start + span.bit_base, 0u, 0u, 0u, 0u, (uint32_t)status, 0u, 0u, 0u, 0u};
      if (status == RADNET_INFLATE_OK) {
        r.end_bit = (uint32_t)sh.pos + span.bit_base, r.out_bytes = (uint32_t)st.produced, r.symbols = st.symbols, r.blocks = st.blocks;
        r.flags = st.flags & RADNET_INFLATE_FLAG_FINAL, r.reach = st.reach, r.far_matches = st.far_matches;
      }
      static_cast<radnet_inflate_lz_unit*>(units)[u] = r;
    } else {
      radnet_inflate_unit r = {start + span.bit_base, 0u, 0u, 0u, 0u, (uint32_t)status, 0u, 0u};
      if (status == RADNET_INFLATE_OK) {
        r.end_bit = (uint32_t)sh.pos + span.bit_base, r.out_bytes = (uint32_t)st.produced, r.symbols = st.symbols, r.blocks = st.blocks;
        r.flags = st.flags, r.last_byte = (st.flags & RADNET_INFLATE_FLAG_LAST_KNOWN) ? st.last : 0u;
      }
      static_cast<radnet_inflate_unit*>(units)[u] = r;
    }
  }
}

// one stream alone: the kernel of inflate.hip and inflate_lz.hip
template <bool kEmit, bool kLz>
__global__ void __launch_bounds__(kWave) inflate_units_kernel(const uint8_t* __restrict__ z, long long n, void* __restrict__ units,
                                                              const radnet_inflate_link* __restrict__ links, uint8_t* __restrict__ out,
                                                              uint32_t* __restrict__ src, long long out_len) {
  __shared__ UnitShared sh;
  inflate_unit<kEmit, kLz>(sh, UnitSpan{z, n, 0u, 0ll, out_len}, units, links, out, src);
}

// Whether a dynamic block header that zlib's inflate accepts begins at bit p of the stream `bits` reads, nbits long (the rule:
// include/radnet_hip.h, radnet_inflate_find_blocks).  Three offsets in four end at BTYPE, HLIT or HDIST.
template <class Bits>
__device__ __forceinline__ bool dynamic_header_at(const Bits& bits, u64 p, u64 nbits) {
  const unsigned v = bits.peek(p);
  if (((v >> 1) & 3) != 2 || ((v >> 3) & 31) > 29 || ((v >> 8) & 31) > 29) return false;
  u64 pos = p + 3;
  int nlen, ndist;
  return parse_dynamic(bits, pos, nbits, [](int, int) {}, nlen, ndist) == RADNET_INFLATE_OK;
}

int check_stream(radnet_ctx* ctx, const char* what, const void* z, int64_t n) {
  if (!z || n < 3) RADNET_FAIL(ctx, RADNET_ERR_ARG, "%s: a null stream or one of %lld bytes (3 at least)", what, (long long)n);
  if (n >= (1ll << 29)) RADNET_FAIL(ctx, RADNET_ERR_UNSUPPORTED, "%s: %lld bytes (a bit offset could pass 2^32)", what, (long long)n);
  return RADNET_OK;
}

}  // namespace
