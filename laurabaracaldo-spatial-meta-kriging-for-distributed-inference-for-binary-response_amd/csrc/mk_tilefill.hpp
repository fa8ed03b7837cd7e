// Which tiles of a tiled session's test sites a result sink's buffer holds, and over which kept window:
// the record behind the missing-tile error of the results entries.  A sink's tile replay calls
// begin() before its launch and mark() once the kernels ran and the stream went idle; the results entry asks
// first_missing().  Standard headers only, so the bookkeeping is tested on the host (tests/tilefill_test.cpp).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace mk {

struct TileFill {
  std::vector<char> done;   // per tile: replayed over the window (lo, n) since the sink was attached
  int tile = 0;             // test sites per tile (the last tile may hold fewer)
  int lo = -1, n = -1;      // the kept window those replays ran over (-1: none yet)

  // A sink attached to n_test_all sites in tiles of pred_tile: no tile filled, no window.
  void attach(int n_test_all, int pred_tile) {
    done.assign((size_t)((n_test_all + pred_tile - 1) / pred_tile), 0);
    tile = pred_tile;
    lo = n = -1;
  }
  // A tile replay over kept states [win_lo, win_lo + n_kept) begins: the tiles filled over another window
  // do not go with it.
  void begin(int win_lo, int n_kept) {
    if (lo == win_lo && n == n_kept) return;
    std::fill(done.begin(), done.end(), 0);
    lo = win_lo;
    n = n_kept;
  }
  // The tile that starts at test site t0 is filled.
  void mark(int t0) { done[(size_t)(t0 / tile)] = 1; }
  // The first tile the buffer does not hold for the window (win_lo, n_kept) -- every tile when the buffer
  // holds another window's -- or -1.
  long first_missing(int win_lo, int n_kept) const {
    const bool stale = lo != win_lo || n != n_kept;
    for (size_t t = 0; t < done.size(); ++t)
      if (stale || !done[t]) return (long)t;
    return -1;
  }
};

// The error text for a missing tile t of n_test_all sites in tiles of pred_tile: what names the sink
// ("posterior maps"), attached what was attached ("the maps were attached").
inline std::string tile_missing_msg(const char* what, const char* attached, long t, int pred_tile, int n_test_all) {
  const long a = t * pred_tile, b = std::min<long>(a + pred_tile, n_test_all) - 1;
  return std::string(what) + ": tile " + std::to_string(t) + " (test sites " + std::to_string(a) + " .. " +
         std::to_string(b) + ") has not been replayed over this kept window since " + attached +
         " (mk_session_outputs, mk_session_tile_grids)";
}

}  // namespace mk
