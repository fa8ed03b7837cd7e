// Host test of the tile-fill record (csrc/mk_tilefill.hpp): which tiles a result sink's buffer holds, over
// which kept window, and the text of the missing-tile error.  Built by test_tilefill_host.py with the host
// compiler and -fsanitize=address,undefined; prints the first failed check and exits 1, else "ok".
#include <cstdio>
#include <string>
#include "mk_tilefill.hpp"

static int failed = 0;
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      std::printf("line %d: %s is false\n", __LINE__, #x); \
      failed = 1;                                           \
    }                                                       \
  } while (0)

int main() {
  using mk::TileFill;
  using mk::tile_missing_msg;
  // sizes: 24 sites in tiles of 16 (the last ragged), 16 in 16, one site
  TileFill f;
  f.attach(24, 16);
  CHECK(f.done.size() == 2 && f.lo == -1 && f.n == -1);
  TileFill one_tile, one_site;
  one_tile.attach(16, 16);
  CHECK(one_tile.done.size() == 1);
  one_site.attach(1, 16);
  CHECK(one_site.done.size() == 1);
  one_site.begin(0, 48);
  one_site.mark(0);
  CHECK(one_site.first_missing(0, 48) == -1);
  // a fresh record misses tile 0, whatever the window asked about
  CHECK(f.first_missing(0, 48) == 0);
  CHECK(f.first_missing(-1, -1) == 0);
  // tiles are marked one by one; the ragged tile starts at site 16
  f.begin(0, 48);
  CHECK(f.first_missing(0, 48) == 0);
  f.mark(0);
  CHECK(f.first_missing(0, 48) == 1);
  f.begin(0, 48);   // the same window again: nothing forgotten
  CHECK(f.first_missing(0, 48) == 1);
  f.mark(16);
  CHECK(f.first_missing(0, 48) == -1);
  // asked about another window, every tile is stale although every tile is marked
  CHECK(f.first_missing(3, 41) == 0);
  CHECK(f.first_missing(0, 41) == 0);
  CHECK(f.first_missing(3, 48) == 0);
  CHECK(f.done[0] && f.done[1]);
  // a replay over another window forgets both
  f.begin(3, 41);
  CHECK(!f.done[0] && !f.done[1] && f.lo == 3 && f.n == 41);
  CHECK(f.first_missing(3, 41) == 0);
  f.mark(16);   // the second tile first
  CHECK(f.first_missing(3, 41) == 0);
  f.mark(0);
  CHECK(f.first_missing(3, 41) == -1);
  CHECK(f.first_missing(0, 48) == 0);
  // attaching anew forgets tiles and window
  f.attach(24, 16);
  CHECK(f.first_missing(3, 41) == 0 && f.lo == -1 && !f.done[1]);
  // the three sinks' messages for tile 1 of 24 sites in tiles of 16, as they were written out in
  // mk_session_maps, mk_session_scores and mk_session_pairs before they shared this function
  const std::string maps = tile_missing_msg("posterior maps", "the maps were attached", 1, 16, 24);
  const std::string scores = tile_missing_msg("held-out scores", "the validation data were attached", 1, 16, 24);
  const std::string pairs = tile_missing_msg("cross-outcome prediction", "the pairs were attached", 1, 16, 24);
  CHECK(maps ==
        "posterior maps: tile 1 (test sites 16 .. 23) has not been replayed over this kept window since the maps were "
        "attached (mk_session_outputs, mk_session_tile_grids)");
  CHECK(scores ==
        "held-out scores: tile 1 (test sites 16 .. 23) has not been replayed over this kept window since the validation "
        "data were attached (mk_session_outputs, mk_session_tile_grids)");
  CHECK(pairs ==
        "cross-outcome prediction: tile 1 (test sites 16 .. 23) has not been replayed over this kept window since the "
        "pairs were attached (mk_session_outputs, mk_session_tile_grids)");
  for (const std::string* m : {&maps, &scores, &pairs}) CHECK(m->find("tile 1 (test sites 16 .. 23)") != std::string::npos);
  // a full first tile, and the single site of a one-site session
  CHECK(tile_missing_msg("posterior maps", "the maps were attached", 0, 16, 24).find("tile 0 (test sites 0 .. 15)") !=
        std::string::npos);
  CHECK(tile_missing_msg("posterior maps", "the maps were attached", 0, 16, 1).find("tile 0 (test sites 0 .. 0)") !=
        std::string::npos);
  if (!failed) std::printf("ok\n");
  return failed;
}
