// Driver for the AddressSanitizer + UBSan build of csrc/draw_scene_check.cpp (tests/test_draw_scene_check_sanitize.py builds and runs
// it): radnet_draw_scene_check, the list dialect of the same walk (what radnet_draw_list_u8 calls) and the check of
// radnet_draw_rects_u8's table, on exactly-sized heap tables, pools and message buffers, so a read past the last entry, past a run's
// last byte or a write past msg_cap is caught; the arithmetic at the ends of int32 runs under UBSan.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../rock-art-radnet_amd/csrc/draw_check.h"

static int failed = 0, checked = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checked;                                                       \
    if (!(cond)) {                                                   \
      ++failed;                                                      \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
    }                                                                \
  } while (0)

static const int kMsg = 96;

// the check on heap copies of exactly the table's and the pool's size; returns its code, *bad the entry it names, *said the message.
// dialect: null for the exported radnet_draw_scene_check, else the internal walk in that dialect
static int run(const std::vector<radnet_prim>& prims, const std::vector<uint8_t>& pool, int32_t* bad, int msg_cap = kMsg, const DrawDialect* dialect = nullptr,
               std::string* said = nullptr) {
  radnet_prim* table = (radnet_prim*)malloc(sizeof(radnet_prim) * (prims.size() ? prims.size() : 1));
  uint8_t* chars = (uint8_t*)malloc(pool.size() ? pool.size() : 1);
  char* msg = (char*)malloc((size_t)(msg_cap > 0 ? msg_cap : 1));
  if (prims.size()) memcpy(table, prims.data(), sizeof(radnet_prim) * prims.size());
  if (pool.size()) memcpy(chars, pool.data(), pool.size());
  *bad = -7;
  int has_text = -7, texts = 0;
  for (const radnet_prim& p : prims) texts |= p.kind == RADNET_PRIM_TEXT;
  const int rc = dialect ? radnet_draw_prims_check(*dialect, prims.size() ? table : nullptr, (int32_t)prims.size(), pool.size() ? chars : nullptr,
                                                   (int32_t)pool.size(), bad, msg_cap > 0 ? msg : nullptr, msg_cap, &has_text)
                         : radnet_draw_scene_check(prims.size() ? table : nullptr, (int32_t)prims.size(), pool.size() ? chars : nullptr, (int32_t)pool.size(), bad,
                                                   msg_cap > 0 ? msg : nullptr, msg_cap);
  if (msg_cap > 0) CHECK(memchr(msg, 0, (size_t)msg_cap) != nullptr);      // always terminated inside its buffer
  if (rc == RADNET_OK && msg_cap > 0) CHECK(msg[0] == 0);
  if (rc == RADNET_OK && dialect) CHECK(has_text == texts);                // what the entries stage the font by
  if (said) *said = msg_cap > 0 ? msg : "";
  free(msg);
  free(chars);
  free(table);
  return rc;
}

// the same for radnet_draw_rects_u8's table
static int run_rects(const std::vector<radnet_rect>& rects, int32_t* bad, int msg_cap = kMsg, std::string* said = nullptr) {
  radnet_rect* table = (radnet_rect*)malloc(sizeof(radnet_rect) * (rects.size() ? rects.size() : 1));
  char* msg = (char*)malloc((size_t)(msg_cap > 0 ? msg_cap : 1));
  if (rects.size()) memcpy(table, rects.data(), sizeof(radnet_rect) * rects.size());
  *bad = -7;
  const int rc = radnet_draw_rects_check(table, (int32_t)rects.size(), bad, msg_cap > 0 ? msg : nullptr, msg_cap);
  if (msg_cap > 0) CHECK(memchr(msg, 0, (size_t)msg_cap) != nullptr);
  if (rc == RADNET_OK && msg_cap > 0) CHECK(msg[0] == 0);
  if (said) *said = msg_cap > 0 ? msg : "";
  free(msg);
  free(table);
  return rc;
}

static bool names(const std::string& said, const char* prefix, const char* noun, int entry) {      // "<prefix>: ... <noun> <entry> ..."
  return said.rfind(prefix, 0) == 0 && said.find(std::string(noun) + " " + std::to_string(entry) + " ") != std::string::npos;
}

static radnet_prim prim(int kind, int x1, int y1, int x2, int y2, int a, int b, int bgr) { return radnet_prim{kind, x1, y1, x2, y2, a, b, bgr}; }

int main() {
  static_assert(sizeof(radnet_prim) == 32, "radnet_prim is 32 bytes");
  const int M = RADNET_DRAW_SCENE_MAX_COORD;
  int32_t bad;
  const std::vector<uint8_t> pool = {'o', 'k', ':', ' ', '1', 'g', 'y'};
  const std::vector<radnet_prim> good = {prim(RADNET_PRIM_RECT, 2, 2, 9, 9, 8, 0, 0x030201),
                                         prim(RADNET_PRIM_TEXT, 3, 12, 1, 0, 0, 5, 0xFF00FF),
                                         prim(RADNET_PRIM_LINE, 1, 1, 20, 9, 2, 3 | 2 << 16, (int)0x80090909u),
                                         prim(RADNET_PRIM_DISC, 8, 8, 4, 0, -1, 0, 0),
                                         prim(RADNET_PRIM_DISC, 15, 10, 5, 0, 2, 0, 0x63070707),
                                         prim(RADNET_PRIM_TEXT, 1, 18, 1, 0, 5, 2, -1)};      // a run that ends at the pool's last byte
  CHECK(run(good, pool, &bad) == RADNET_OK && bad == -7);
  CHECK(run({}, {}, &bad) == RADNET_OK && bad == -7);
  CHECK(run(good, pool, &bad, 0) == RADNET_OK);                                               // no message buffer at all
  CHECK(radnet_draw_scene_check(nullptr, 0, nullptr, 0, nullptr, nullptr, 0) == RADNET_OK);
  CHECK(radnet_draw_scene_check(nullptr, 3, nullptr, 0, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_draw_scene_check(good.data(), -1, nullptr, 0, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_draw_scene_check(good.data(), 1, nullptr, -1, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_draw_scene_check(good.data(), 1, nullptr, 4, &bad, nullptr, 0) == RADNET_ERR_ARG && bad == -1);
  CHECK(radnet_draw_scene_check(good.data(), 1, nullptr, 0, nullptr, nullptr, 0) == RADNET_OK);      // a rectangle needs no pool

  struct Case {
    int entry, field, value;
  };
  // field: the index of the int32 in radnet_prim (kind, x1, y1, x2, y2, a, b, bgr)
  const Case cases[] = {{3, 0, 4},       {0, 0, -1},       {0, 0, INT_MAX}, {0, 0, INT_MIN}, {0, 5, 0},        {1, 3, 0},         {5, 3, 65},       {1, 3, INT_MIN},
                        {5, 4, 1},       {1, 5, -1},       {5, 6, -1},      {5, 6, 3},       {1, 5, INT_MAX},  {1, 6, INT_MAX},   {2, 5, 0},        {2, 5, -1},
                        {2, 5, INT_MIN}, {2, 6, 3 << 16},  {2, 6, 3},       {2, 6, INT_MIN}, {2, 1, M + 1},    {2, 2, -M - 1},    {2, 3, INT_MIN},  {2, 4, INT_MAX},
                        {3, 5, 0},       {4, 3, -1},       {3, 3, INT_MIN}, {3, 4, 1},       {4, 6, 1},        {3, 1, M + 1},     {4, 2, INT_MIN},  {3, 3, M + 1}};
  for (const Case& c : cases) {
    std::vector<radnet_prim> t = good;
    ((int32_t*)&t[(size_t)c.entry])[c.field] = c.value;
    CHECK(run(t, pool, &bad) == RADNET_ERR_ARG && bad == c.entry);
    CHECK(run(t, pool, &bad, 1) == RADNET_ERR_ARG && bad == c.entry);                          // a message buffer of one byte
    CHECK(run(t, pool, &bad, 9) == RADNET_ERR_ARG && bad == c.entry);
    if (failed) printf("  (entry %d, field %d = %d)\n", c.entry, c.field, c.value);
  }
  {                                                                   // a byte outside the font inside a run, and outside every run
    std::vector<uint8_t> p = pool;
    p[6] = 0x7F;
    CHECK(run(good, p, &bad) == RADNET_ERR_ARG && bad == 5);
    p[6] = 'y', p[4] = 0x1F;
    CHECK(run(good, p, &bad) == RADNET_ERR_ARG && bad == 1);
    p = pool;
    p.push_back(0xFF);
    CHECK(run(good, p, &bad) == RADNET_OK);
    p.pop_back(), p.pop_back();                                       // the last run no longer fits
    CHECK(run(good, p, &bad) == RADNET_ERR_ARG && bad == 5);
  }
  {                                                                   // everything at the bound, at the ends of int32 where that is allowed
    const std::vector<radnet_prim> edge = {prim(RADNET_PRIM_LINE, M, -M, -M, M, INT_MAX, (int)0xFFFFFFFFu, INT_MIN),
                                           prim(RADNET_PRIM_DISC, -M, M, M, 0, INT_MAX, 0, -1), prim(RADNET_PRIM_DISC, M, -M, 0, 0, INT_MIN, 0, 0),
                                           prim(RADNET_PRIM_RECT, INT_MIN, INT_MIN, INT_MAX, INT_MAX, INT_MIN, 12345, INT_MAX),
                                           prim(RADNET_PRIM_TEXT, INT_MAX, INT_MIN, RADNET_DRAW_TEXT_MAX_SCALE, 0, 7, 0, 0)};      // an empty run at the pool's end
    CHECK(run(edge, pool, &bad) == RADNET_OK);
  }
  {                                                                   // a long table: the first bad entry is the one named
    std::vector<radnet_prim> many;
    for (int i = 0; i < 1000; ++i) many.push_back(good[(size_t)(i % 5)]);
    CHECK(run(many, pool, &bad) == RADNET_OK);
    many[998].kind = 9, many[640].a = 0;
    CHECK(run(many, pool, &bad) == RADNET_ERR_ARG && bad == 640);
  }
  {                                                                   // the list dialect: tests/test_gpu_draw_list.py::test_count_zero_and_refusals
    const DrawDialect* L = &kDrawListDialect;
    std::string said;
    const std::vector<radnet_prim> list = {prim(RADNET_PRIM_RECT, 2, 2, 9, 9, 8, 0, 0x030201), prim(RADNET_PRIM_TEXT, 3, 12, 1, 0, 0, 5, 0xFF00FF),
                                           prim(RADNET_PRIM_RECT, 1, 1, 5, 5, -1, 0, 0), prim(RADNET_PRIM_TEXT, 1, 18, 1, 0, 5, 2, 0x090909)};
    CHECK(run(list, pool, &bad, kMsg, L) == RADNET_OK && bad == -7);
    CHECK(run(list, pool, &bad, 0, L) == RADNET_OK);
    CHECK(run({}, {}, &bad, kMsg, L) == RADNET_OK && bad == -7);
    CHECK(run({list[0], list[2]}, {}, &bad, kMsg, L) == RADNET_OK);                            // rectangles need no pool; no text is seen
    CHECK(run(good, pool, &bad, kMsg, L, &said) == RADNET_ERR_ARG && bad == 2 && names(said, "draw_list:", "entry", 2));      // the scene's table
    const Case list_cases[] = {{2, 0, RADNET_PRIM_LINE}, {2, 0, RADNET_PRIM_DISC}, {0, 0, -1},      {0, 0, 4},        {0, 0, INT_MAX}, {0, 0, INT_MIN}, {2, 5, 0},
                               {1, 3, 0},                {3, 3, 65},               {1, 3, -1},      {3, 4, 1},        {1, 5, -1},      {3, 6, -1},      {3, 6, 3},
                               {0, 7, 1 << 24},          {3, 7, -1},               {1, 7, INT_MIN}, {2, 7, 0x1000000}};
    for (const Case& c : list_cases) {
      std::vector<radnet_prim> t = list;
      ((int32_t*)&t[(size_t)c.entry])[c.field] = c.value;
      CHECK(run(t, pool, &bad, kMsg, L, &said) == RADNET_ERR_ARG && bad == c.entry && names(said, "draw_list:", "entry", c.entry));
      CHECK(run(t, pool, &bad, 1, L) == RADNET_ERR_ARG && bad == c.entry);
      CHECK(run(t, pool, &bad, 9, L) == RADNET_ERR_ARG && bad == c.entry);
      if (failed) printf("  (list entry %d, field %d = %d: %s)\n", c.entry, c.field, c.value, said.c_str());
    }
    std::vector<radnet_prim> t = list;                                // an offset past the pool; offset + length past int32
    t[1].a = 8, t[1].b = 0;
    CHECK(run(t, pool, &bad, kMsg, L, &said) == RADNET_ERR_ARG && bad == 1 && names(said, "draw_list:", "entry", 1));
    t[1].a = INT_MAX, t[1].b = INT_MAX;
    CHECK(run(t, pool, &bad, kMsg, L, &said) == RADNET_ERR_ARG && bad == 1 && names(said, "draw_list:", "entry", 1));
    const struct { int byte, value, entry; } bytes[] = {{2, 0x1F, 1}, {6, 0x7F, 3}, {0, 0xE5, 1}};      // a control code, DEL, a byte above ASCII
    for (const auto& b : bytes) {
      std::vector<uint8_t> p = pool;
      p[(size_t)b.byte] = (uint8_t)b.value;
      CHECK(run(list, p, &bad, kMsg, L, &said) == RADNET_ERR_ARG && bad == b.entry && names(said, "draw_list:", "entry", b.entry));
    }
    std::vector<uint8_t> p = pool;                                    // a byte outside the font that no run refers to is nobody's business
    p.push_back(0x00), p.push_back(0xFF);
    CHECK(run(list, p, &bad, kMsg, L) == RADNET_OK);
    t = list;                                                         // the colour is looked at before the kind
    t[0].kind = 9, t[0].bgr = -1;
    CHECK(run(t, pool, &bad, kMsg, L, &said) == RADNET_ERR_ARG && bad == 0 && said.find("colour") != std::string::npos);
  }
  {                                                                   // radnet_draw_rects_u8's table: tests/test_gpu_png_write.py::test_draw_rects_count_zero_and_refusals
    static_assert(sizeof(radnet_rect) == 32, "radnet_rect is 32 bytes");
    std::string said;
    const std::vector<radnet_rect> rects = {radnet_rect{2, 2, 9, 9, 8, 1, 2, 3}, radnet_rect{4, 4, 12, 12, -1, 255, 0, 255}, radnet_rect{1, 1, 5, 5, 1, 0, 0, 0},
                                            radnet_rect{INT_MIN, INT_MAX, INT_MAX, INT_MIN, INT_MIN, 0, 255, 0}};
    CHECK(run_rects(rects, &bad) == RADNET_OK && bad == -7);
    CHECK(run_rects(rects, &bad, 0) == RADNET_OK);
    CHECK(run_rects({}, &bad) == RADNET_OK && bad == -7);
    // field: the index of the int32 in radnet_rect (x1, y1, x2, y2, thickness, b, g, r)
    const Case rect_cases[] = {{1, 4, 0}, {2, 5, 256}, {0, 6, -1}, {2, 7, 1000}, {3, 5, INT_MIN}, {3, 7, INT_MAX}};
    for (const Case& c : rect_cases) {
      std::vector<radnet_rect> t = rects;
      ((int32_t*)&t[(size_t)c.entry])[c.field] = c.value;
      CHECK(run_rects(t, &bad, kMsg, &said) == RADNET_ERR_ARG && bad == c.entry && names(said, "draw_rects:", "rectangle", c.entry));
      CHECK(run_rects(t, &bad, 1) == RADNET_ERR_ARG && bad == c.entry);
      CHECK(run_rects(t, &bad, 9) == RADNET_ERR_ARG && bad == c.entry);
    }
    std::vector<radnet_rect> t = rects;                               // the first bad rectangle is the one named
    t[2].thickness = 0, t[1].g = 300;
    CHECK(run_rects(t, &bad) == RADNET_ERR_ARG && bad == 1);
  }
  printf("%d checks, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
