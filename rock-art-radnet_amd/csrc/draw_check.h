// The painters' table validation (draw_scene_check.cpp), for the entries of draw.hip and for the sanitizer driver under
// tests/native.  Host only: no HIP header, g++ compiles it alone.  Internal to the library: nothing here is exported.
#pragma once
#include "radnet_hip.h"

#define RADNET_DRAW_INTERNAL __attribute__((visibility("hidden")))

struct DrawDialect {      // what one entry point admits in a radnet_prim table
  const char* name;       // the prefix of its messages
  unsigned kinds;         // bit k: kind k exists
  bool tau;               // bits 24..31 of bgr carry the transparency; otherwise bgr lies in 0..0xFFFFFF
};
constexpr DrawDialect kDrawListDialect = {"draw_list", 1u << RADNET_PRIM_RECT | 1u << RADNET_PRIM_TEXT, false};
constexpr DrawDialect kDrawSceneDialect = {"draw_scene", kDrawListDialect.kinds | 1u << RADNET_PRIM_LINE | 1u << RADNET_PRIM_DISC, true};

// radnet_draw_scene_check's contract (include/radnet_hip.h) in the dialect `d`; *has_text, if given, says whether a text entry was seen.
RADNET_DRAW_INTERNAL int radnet_draw_prims_check(const DrawDialect& d, const radnet_prim* prims, int32_t count, const uint8_t* chars, int32_t n_chars,
                                                 int32_t* bad_entry, char* msg, int32_t msg_cap, int* has_text);

// The same for radnet_draw_rects_u8's table: thickness 0 and a colour value outside 0..255 are refused.
RADNET_DRAW_INTERNAL int radnet_draw_rects_check(const radnet_rect* rects, int32_t count, int32_t* bad_entry, char* msg, int32_t msg_cap);
