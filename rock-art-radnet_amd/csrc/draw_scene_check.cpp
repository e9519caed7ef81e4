// ---- host side of the scene painter (draw_scene.hip): the table's validation ------------------------------------------------------
// No device call and no HIP header: compiled by g++, runs without a GPU (contract: include/radnet_hip.h).  radnet_draw_scene_u8
// calls this before it launches; tests/native/draw_scene_check_sanitize.cpp runs it under ASan + UBSan on exactly sized tables.
#include <stdarg.h>
#include <stdio.h>
#include "radnet_hip.h"

namespace {

constexpr int kFontFirst = 0x20, kFontLast = 0x7E;      // the codes csrc/draw_font.h has (radnet_draw_glyph_rows refuses the others)

int refuse(int32_t i, int32_t* bad_entry, char* msg, int32_t msg_cap, const char* fmt, ...) {
  if (bad_entry) *bad_entry = i;
  if (msg && msg_cap > 0) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, (size_t)msg_cap, fmt, ap);
    va_end(ap);
  }
  return RADNET_ERR_ARG;
}

bool beyond(int32_t v) { return v < -RADNET_DRAW_SCENE_MAX_COORD || v > RADNET_DRAW_SCENE_MAX_COORD; }

}  // namespace

extern "C" int radnet_draw_scene_check(const radnet_prim* prims, int32_t count, const uint8_t* chars, int32_t n_chars, int32_t* bad_entry,
                                       char* msg, int32_t msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (count < 0) return refuse(-1, bad_entry, msg, msg_cap, "draw_scene: %d entries", count);
  if (count == 0) return RADNET_OK;
  if (!prims) return refuse(-1, bad_entry, msg, msg_cap, "draw_scene: a null table of %d entries", count);
  if (n_chars < 0 || (n_chars > 0 && !chars))
    return refuse(-1, bad_entry, msg, msg_cap, "draw_scene: a character pool of %d bytes at %p", n_chars, (const void*)chars);
  for (int32_t i = 0; i < count; ++i) {
    const radnet_prim& p = prims[i];
    switch (p.kind) {
      case RADNET_PRIM_RECT:
        if (p.a == 0) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a rectangle of thickness 0", i);
        break;
      case RADNET_PRIM_TEXT:
        if (p.x2 < 1 || p.x2 > RADNET_DRAW_TEXT_MAX_SCALE) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d has the text scale %d", i, p.x2);
        if (p.y2 != 0) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is text with y2 = %d, not 0", i, p.y2);
        if (p.a < 0 || p.b < 0 || (int64_t)p.a + p.b > n_chars)
          return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d takes %d characters at offset %d of a pool of %d", i, p.b, p.a, n_chars);
        for (int32_t k = 0; k < p.b; ++k) {
          const int code = chars[(int64_t)p.a + k];
          if (code < kFontFirst || code > kFontLast)
            return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d has the byte 0x%02X as character %d", i, code, k);
        }
        break;
      case RADNET_PRIM_LINE:
        if (p.a < 1) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a line of thickness %d", i, p.a);
        if (p.b != 0 && ((p.b & 0xFFFF) == 0 || ((p.b >> 16) & 0xFFFF) == 0))
          return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d has the dash %d on, %d off", i, p.b & 0xFFFF, (p.b >> 16) & 0xFFFF);
        if (beyond(p.x1) || beyond(p.y1) || beyond(p.x2) || beyond(p.y2))
          return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a line from (%d, %d) to (%d, %d), beyond +-%d", i, p.x1, p.y1, p.x2, p.y2,
                        RADNET_DRAW_SCENE_MAX_COORD);
        break;
      case RADNET_PRIM_DISC:
        if (p.a == 0) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a disc of thickness 0", i);
        if (p.x2 < 0) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a disc of radius %d", i, p.x2);
        if (p.y2 != 0 || p.b != 0) return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a disc with y2 = %d and b = %d, not 0", i, p.y2, p.b);
        if (beyond(p.x1) || beyond(p.y1) || beyond(p.x2))
          return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is a disc at (%d, %d) of radius %d, beyond +-%d", i, p.x1, p.y1, p.x2,
                        RADNET_DRAW_SCENE_MAX_COORD);
        break;
      default:
        return refuse(i, bad_entry, msg, msg_cap, "draw_scene: entry %d is of the unknown kind %d", i, p.kind);
    }
  }
  return RADNET_OK;
}
