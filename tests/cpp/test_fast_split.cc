// Where csrc/vsf_fast_split.h cuts FAST's list of full cells, checked on the CPU against work lists as the library builds
// them (vsf_debug_fast_work; tests/test_fast_split.py writes them into the file this program reads):
//   shapes
//   then per shape:  width height nlevels nfull
//                    nlevels lines  x_lo x_hi y_lo y_hi fast_a0 nbands nstrips
//                    nfull words    level << 24 | band << 16 | strip
// For every Le in 0 .. nlevels + 2: the head [0, n_early(Le)) holds exactly the full-width cells of levels < Le, each once,
// and nothing behind it is a full-width cell of such a level; n_early(0) == 0; n_early is monotone; beyond the last level
// that has a full-width cell it stays what it is.  Exit status 0 and a line "ok ..." when everything holds.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_fast_split.h"

static int fails = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (fails++ < 20) {                      \
        std::printf("FAIL %s: ", #cond);       \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

struct Level {
  int x_lo, x_hi, y_lo, y_hi, a0, nbands, nstrips;
};

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_fast_split <work lists>\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  int shapes = 0;
  long cuts = 0;
  if (std::fscanf(f, "%d", &shapes) != 1 || shapes < 1) return 2;
  for (int s = 0; s < shapes; s++) {
    int w, h, nlevels, nfull;
    if (std::fscanf(f, "%d %d %d %d", &w, &h, &nlevels, &nfull) != 4 || nlevels < 1 || nlevels > 64 || nfull < 0) return 2;
    std::vector<Level> lv((size_t)nlevels);
    for (Level& L : lv)
      if (std::fscanf(f, "%d %d %d %d %d %d %d", &L.x_lo, &L.x_hi, &L.y_lo, &L.y_hi, &L.a0, &L.nbands, &L.nstrips) != 7) return 2;
    std::vector<uint32_t> units((size_t)nfull);
    for (uint32_t& u : units)
      if (std::fscanf(f, "%u", &u) != 1) return 2;
    // a full-width cell, by the level table alone
    auto full_width = [&](uint32_t u) {
      const Level& L = lv[u >> 24];
      return vsf_fast_cell_lanes(L.a0, L.x_hi, (int)((u >> 16) & 0xFF)) >= 64;
    };
    const int split_levels = vsf_fast_split_levels(lv.data(), nlevels);
    int last_full_level = -1;
    for (uint32_t u : units)
      if (full_width(u) && (int)(u >> 24) > last_full_level) last_full_level = (int)(u >> 24);
    CHECK(split_levels == last_full_level + 1, "%dx%d: split levels %d, last level with a full-width cell %d", w, h, split_levels,
          last_full_level);
    CHECK(vsf_fast_n_early(lv.data(), nlevels, 0) == 0, "%dx%d: n_early(0)", w, h);
    int prev = 0;
    for (int Le = 0; Le <= nlevels + 2; Le++, cuts++) {
      const int n = vsf_fast_n_early(lv.data(), nlevels, Le);
      CHECK(n >= prev && n <= nfull, "%dx%d Le %d: n_early %d after %d, %d full items", w, h, Le, n, prev, nfull);
      if (Le > split_levels) CHECK(n == prev, "%dx%d Le %d: grows past the last level with a full-width cell", w, h, Le);
      prev = n;
      if (n > nfull) continue;
      // the cells the head must hold: by the level table
      std::set<uint32_t> want, got;
      for (int l = 0; l < Le && l < nlevels; l++)
        for (int st = 0; st < lv[l].nstrips; st++)
          for (int b = 0; b < lv[l].nbands; b++)
            if (vsf_fast_cell_lanes(lv[l].a0, lv[l].x_hi, b) >= 64) want.insert(((uint32_t)l << 24) | ((uint32_t)b << 16) | (uint32_t)st);
      for (int i = 0; i < n; i++) {
        CHECK((int)(units[i] >> 24) < Le, "%dx%d Le %d: item %d of the head is of level %u", w, h, Le, i, units[i] >> 24);
        CHECK(full_width(units[i]), "%dx%d Le %d: item %d of the head is a narrow cell", w, h, Le, i);
        CHECK(got.insert(units[i]).second, "%dx%d Le %d: item %d twice", w, h, Le, i);
      }
      CHECK(got == want, "%dx%d Le %d: the head holds %zu cells, the levels have %zu", w, h, Le, got.size(), want.size());
      for (int i = n; i < nfull; i++)
        CHECK(!((int)(units[i] >> 24) < Le && full_width(units[i])), "%dx%d Le %d: item %d behind the head belongs to it", w, h, Le, i);
    }
    // the per-level count against the table's own bands and strips
    for (int l = 0; l < nlevels; l++) {
      int full = 0;
      for (int b = 0; b < lv[l].nbands; b++) full += vsf_fast_cell_lanes(lv[l].a0, lv[l].x_hi, b) >= 64;
      CHECK(vsf_fast_full_cells(lv[l].x_lo, lv[l].x_hi, lv[l].y_lo, lv[l].y_hi) == full * lv[l].nstrips, "%dx%d level %d", w, h, l);
    }
  }
  std::fclose(f);
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok %d shapes, %ld cuts\n", shapes, cuts);
  return 0;
}
