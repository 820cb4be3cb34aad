// tile_slots_main.cpp - the staging-slot sources of the two-ring tiles (thetis_amd/csrc/swe2d_tiles.h: slot_src / slot_first), checked on the
// host: tests/test_tile_slots.py compiles this with the address and undefined-behaviour sanitizers and runs it per mesh.
//
//   tile_slots_main IN
//
// IN: the input of tests/tile_tables_main.cpp (int32: nfacets = 3, stride, n_cells, has_order, has_start; neighbour codes [3][stride];
// order; start flags).  Builds the 'triple' tables as swe2d_api_fuse.hip does and checks what the three-stage kernel's gather relies on:
//   * a tile's slots are 0 .. n_slots-1, n_slots <= SWE_FUSE3_MAX_OUT (224), and slot_first is their running sum;
//   * every slot is named by exactly one facet field of the tile (bit 9 set), so it has exactly one source;
//   * that source is the neighbour code the connectivity holds for the naming cell's facet: (neighbour << 2) | the neighbour's facet.
// Prints "tiles N max_slots M total T" and returns 0; a violated check: its message on stderr, status 3.
#include "../thetis_amd/csrc/swe2d_tiles.h"

#include <cstdio>

using namespace swe2d_impl;

static bool read_ints(FILE *f, std::vector<int> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(int), n, f) == n;
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 3; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s IN\n", argv[0]); return 1; }
    const TileSpec spec{3, 2, 256, 256, -1, 224, true};       // kTripleTiles of swe2d_api_fuse.hip
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    std::vector<int> head, nbr, order, start32;
    if (!read_ints(in, head, 5) || head[0] != 3 || head[1] < head[2] || head[2] < 0) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t stride = (size_t)head[1];
    const int n = head[2];
    if (!read_ints(in, nbr, 3*stride) || !read_ints(in, order, head[3] ? n : 0) || !read_ints(in, start32, head[4] ? n : 0)) {
        fprintf(stderr, "short input\n");
        return 1;
    }
    fclose(in);
    std::vector<unsigned char> start(start32.begin(), start32.end());
    TileTable t;
    std::string err;
    if (build_tiles(nbr.data(), stride, n, order.empty() ? nullptr : order.data(), start.empty() ? nullptr : start.data(), spec, t, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 2;
    }
    const int n_tiles = (int)t.n_inner.size();
    CHECK((int)t.slot_first.size() == n_tiles + 1 && t.slot_first[0] == 0, "slot_first: %zu entries for %d tiles", t.slot_first.size(), n_tiles);
    CHECK(t.slot_first[n_tiles] == (int)t.slot_src.size(), "slot_first ends at %d, %zu sources", t.slot_first[n_tiles], t.slot_src.size());
    int max_slots = 0;
    for (int tile = 0; tile < n_tiles; tile++) {
        const int first = t.slot_first[tile], ns = t.slot_first[tile + 1] - first;
        CHECK(ns >= 0 && ns <= spec.max_out, "tile %d: %d slots", tile, ns);
        std::vector<int> named((size_t)ns, 0);
        for (int l = 0; l < spec.wg; l++) {
            const int c = t.cell[(size_t)tile*spec.wg + l];
            for (int f = 0; f < 3; f++) {
                const unsigned w = t.facet[((size_t)tile*spec.wg + l)*3 + f];
                if (c < 0) { CHECK(w == 0u, "tile %d lane %d: a padding lane with a facet field", tile, l); continue; }
                if (!(w & kTileOutside)) continue;
                const int s = (int)(w & 0x1ffu);
                CHECK(s < ns, "tile %d lane %d facet %d: slot %d of %d", tile, l, f, s, ns);
                named[s]++;
                const int code = nbr[(size_t)f*stride + c];
                CHECK(code >= 0, "tile %d lane %d facet %d: a boundary facet with a staging slot", tile, l, f);
                CHECK(t.slot_src[first + s] == code, "tile %d slot %d: source %d, the connectivity says %d", tile, s, t.slot_src[first + s], code);
                const int nb = code >> 2, g = code & 3;
                CHECK(nb < n && g < 3 && (nbr[(size_t)g*stride + nb] >> 2) == c, "tile %d slot %d: cell %d facet %d does not lead back to cell %d", tile, s, nb, g, c);
            }
        }
        for (int s = 0; s < ns; s++) CHECK(named[s] == 1, "tile %d slot %d: named by %d facets", tile, s, named[s]);
        if (ns > max_slots) max_slots = ns;
    }
    printf("tiles %d max_slots %d total %zu\n", n_tiles, max_slots, t.slot_src.size());
    return 0;
}
