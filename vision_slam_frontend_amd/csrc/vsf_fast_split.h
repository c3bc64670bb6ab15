// vsf_fast_split.h -- what the host and the tests share of FAST's work list: which cells of a level are one wave each
// ("full" cells: a band wide enough for every lane), and where the list of full cells may be cut so that its head holds
// the cells of the first levels only.  Plain C++ (tests/cpp/test_fast_split.cc compiles it with g++).
//
// build_geometry (vsf_geometry.hip) pushes the full cells level by level, strip by strip, band by band, and behind them
// the narrow cells that were left alone in their wave (one-cell bins of the packing, of any level).  The head
// [0, vsf_fast_n_early(levels, n, Le)) of that list is exactly the full cells of levels < Le: levels 0 .. Le - 1 exist
// before the rest of the pyramid does, so a pipelined call may start FAST on them early (vsf_api.hip extract_on).
#ifndef VSF_FAST_SPLIT_H_
#define VSF_FAST_SPLIT_H_

#define VSF_FAST_SPLIT_BAND_COLS 248  // = VSF_FAST_BAND_COLS (vsf_internal.h checks)
#define VSF_FAST_SPLIT_STRIP_ROWS 32  // = VSF_FAST_STRIP_ROWS

// Lanes of the cell of band `band`: four columns per lane plus the two halo lanes; 64 = a full cell.
inline int vsf_fast_cell_lanes(int fast_a0, int x_hi, int band) {
  const int bx0 = fast_a0 + VSF_FAST_SPLIT_BAND_COLS * band;
  const int end = x_hi < bx0 + VSF_FAST_SPLIT_BAND_COLS ? x_hi : bx0 + VSF_FAST_SPLIT_BAND_COLS;
  return (end - bx0 + 3) / 4 + 2;
}

// Full cells of a level whose keypoints sit at x_lo <= x < x_hi, y_lo <= y < y_hi.
inline int vsf_fast_full_cells(int x_lo, int x_hi, int y_lo, int y_hi) {
  if (x_hi <= x_lo || y_hi <= y_lo) return 0;
  const int a0 = x_lo & ~3;
  const int nbands = (x_hi - a0 + VSF_FAST_SPLIT_BAND_COLS - 1) / VSF_FAST_SPLIT_BAND_COLS;
  const int nstrips = (y_hi - y_lo + VSF_FAST_SPLIT_STRIP_ROWS - 1) / VSF_FAST_SPLIT_STRIP_ROWS;
  int full = 0;
  for (int b = 0; b < nbands; b++) full += vsf_fast_cell_lanes(a0, x_hi, b) >= 64;
  return full * nstrips;
}

// Levels that may go early at most: one past the last level that has a full cell (0: none has).
template <class Level>
inline int vsf_fast_split_levels(const Level* lv, int nlevels) {
  int n = 0;
  for (int l = 0; l < nlevels; l++)
    if (vsf_fast_full_cells(lv[l].x_lo, lv[l].x_hi, lv[l].y_lo, lv[l].y_hi) > 0) n = l + 1;
  return n;
}

// Length of the head of the full-cell list that holds the full cells of levels < early_levels (clamped to
// [0, vsf_fast_split_levels]); 0: no split.  `Level`: anything with x_lo, x_hi, y_lo, y_hi (VsfLevel).
template <class Level>
inline int vsf_fast_n_early(const Level* lv, int nlevels, int early_levels) {
  const int le = early_levels < nlevels ? early_levels : nlevels;
  int n = 0;
  for (int l = 0; l < le; l++) n += vsf_fast_full_cells(lv[l].x_lo, lv[l].x_hi, lv[l].y_lo, lv[l].y_hi);
  return n;
}

#endif  // VSF_FAST_SPLIT_H_
