// ---- host side of the painters of draw.hip: the tables' validation -------------------------------------------------------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h, draw_check.h).  One walk
// over a radnet_prim table in the dialect of its entry point -- radnet_draw_list_u8's or radnet_draw_scene_u8's, whose exported form
// is radnet_draw_scene_check -- and one over radnet_draw_rects_u8's table; the entries call them before they launch, and
// tests/native/draw_scene_check_sanitize.cpp runs them under ASan + UBSan on exactly sized tables.
#include <stdarg.h>
#include <stdio.h>
#include "draw_check.h"

namespace {

constexpr int kFontFirst = 0x20, kFontLast = 0x7E;      // the codes csrc/draw_font.h has (radnet_draw_glyph_rows refuses the others)

struct Refusal {      // where a refusal goes: the entry it names, and the message
  int32_t* bad_entry;
  char* msg;
  int32_t msg_cap;
  __attribute__((format(printf, 3, 4))) int at(int32_t i, const char* fmt, ...) const {
    if (bad_entry) *bad_entry = i;
    if (msg && msg_cap > 0) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(msg, (size_t)msg_cap, fmt, ap);
      va_end(ap);
    }
    return RADNET_ERR_ARG;
  }
};

bool beyond(int32_t v) { return v < -RADNET_DRAW_SCENE_MAX_COORD || v > RADNET_DRAW_SCENE_MAX_COORD; }

}  // namespace

int radnet_draw_prims_check(const DrawDialect& d, const radnet_prim* prims, int32_t count, const uint8_t* chars, int32_t n_chars, int32_t* bad_entry,
                            char* msg, int32_t msg_cap, int* has_text) {
  const Refusal no = {bad_entry, msg, msg_cap};
  if (msg && msg_cap > 0) msg[0] = 0;
  if (has_text) *has_text = 0;
  if (count < 0) return no.at(-1, "%s: %d entries", d.name, count);
  if (count == 0) return RADNET_OK;
  if (!prims) return no.at(-1, "%s: a null table of %d entries", d.name, count);
  if (n_chars < 0 || (n_chars > 0 && !chars)) return no.at(-1, "%s: a character pool of %d bytes at %p", d.name, n_chars, (const void*)chars);
  for (int32_t i = 0; i < count; ++i) {
    const radnet_prim& p = prims[i];
    if (!d.tau && (p.bgr < 0 || p.bgr > 0xFFFFFF)) return no.at(i, "%s: entry %d has the colour 0x%08X", d.name, i, (unsigned)p.bgr);
    switch (p.kind >= 0 && p.kind < 32 && (d.kinds >> p.kind & 1) ? p.kind : -1) {
      case RADNET_PRIM_RECT:
        if (p.a == 0) return no.at(i, "%s: entry %d is a rectangle of thickness 0", d.name, i);
        break;
      case RADNET_PRIM_TEXT:
        if (p.x2 < 1 || p.x2 > RADNET_DRAW_TEXT_MAX_SCALE) return no.at(i, "%s: entry %d has the text scale %d", d.name, i, p.x2);
        if (p.y2 != 0) return no.at(i, "%s: entry %d is text with y2 = %d, not 0", d.name, i, p.y2);
        if (p.a < 0 || p.b < 0 || (int64_t)p.a + p.b > n_chars)
          return no.at(i, "%s: entry %d takes %d characters at offset %d of a pool of %d", d.name, i, p.b, p.a, n_chars);
        for (int32_t k = 0; k < p.b; ++k) {
          const int code = chars[(int64_t)p.a + k];
          if (code < kFontFirst || code > kFontLast) return no.at(i, "%s: entry %d has the byte 0x%02X as character %d", d.name, i, code, k);
        }
        if (has_text) *has_text = 1;
        break;
      case RADNET_PRIM_LINE:
        if (p.a < 1) return no.at(i, "%s: entry %d is a line of thickness %d", d.name, i, p.a);
        if (p.b != 0 && ((p.b & 0xFFFF) == 0 || ((p.b >> 16) & 0xFFFF) == 0))
          return no.at(i, "%s: entry %d has the dash %d on, %d off", d.name, i, p.b & 0xFFFF, (p.b >> 16) & 0xFFFF);
        if (beyond(p.x1) || beyond(p.y1) || beyond(p.x2) || beyond(p.y2))
          return no.at(i, "%s: entry %d is a line from (%d, %d) to (%d, %d), beyond +-%d", d.name, i, p.x1, p.y1, p.x2, p.y2, RADNET_DRAW_SCENE_MAX_COORD);
        break;
      case RADNET_PRIM_DISC:
        if (p.a == 0) return no.at(i, "%s: entry %d is a disc of thickness 0", d.name, i);
        if (p.x2 < 0) return no.at(i, "%s: entry %d is a disc of radius %d", d.name, i, p.x2);
        if (p.y2 != 0 || p.b != 0) return no.at(i, "%s: entry %d is a disc with y2 = %d and b = %d, not 0", d.name, i, p.y2, p.b);
        if (beyond(p.x1) || beyond(p.y1) || beyond(p.x2))
          return no.at(i, "%s: entry %d is a disc at (%d, %d) of radius %d, beyond +-%d", d.name, i, p.x1, p.y1, p.x2, RADNET_DRAW_SCENE_MAX_COORD);
        break;
      default:
        return no.at(i, "%s: entry %d is of the unknown kind %d", d.name, i, p.kind);
    }
  }
  return RADNET_OK;
}

extern "C" int radnet_draw_scene_check(const radnet_prim* prims, int32_t count, const uint8_t* chars, int32_t n_chars, int32_t* bad_entry,
                                       char* msg, int32_t msg_cap) {
  return radnet_draw_prims_check(kDrawSceneDialect, prims, count, chars, n_chars, bad_entry, msg, msg_cap, nullptr);
}

int radnet_draw_rects_check(const radnet_rect* rects, int32_t count, int32_t* bad_entry, char* msg, int32_t msg_cap) {
  const Refusal no = {bad_entry, msg, msg_cap};
  if (msg && msg_cap > 0) msg[0] = 0;
  for (int32_t i = 0; i < count; ++i) {
    const radnet_rect& r = rects[i];
    if (r.thickness == 0) return no.at(i, "draw_rects: rectangle %d has thickness 0", i);
    if (r.b < 0 || r.b > 255 || r.g < 0 || r.g > 255 || r.r < 0 || r.r > 255)
      return no.at(i, "draw_rects: rectangle %d has the colour (%d, %d, %d)", i, r.b, r.g, r.r);
  }
  return RADNET_OK;
}
