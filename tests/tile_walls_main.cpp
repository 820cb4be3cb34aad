// tile_walls_main.cpp - TileSpec::group_walls of the tile-table builder (thetis_amd/csrc/swe2d_tiles.h: build_tiles), checked on the host:
// tests/test_tile_walls.py compiles this with the address and undefined-behaviour sanitizers and runs it per mesh.
//
//   tile_walls_main IN
//
// IN: the input of tests/tile_records_main.cpp.  Builds the 'triple' tables twice, in the order the builder had before (group_walls off)
// and with the wall cells - the cells with a boundary facet - on consecutive roles, decodes the lane records of both and checks, tile
// by tile:
//   * counts, rotation and the number of staging slots are the same, and the roles of each class (interior, ring 1, ring 2) hold the
//     same cells: a permutation inside the class;
//   * a tile without a wall cell has the same cell on every lane;
//   * every cell's record says what it said: vertex offsets and bmarkers equal; per facet and trace word an address inside the planes
//     names the same plane (the neighbour's node) and a lane that holds the same cell, an address in the staging area a slot whose two
//     byte offsets (its source cell and nodes) are the same;
//   * the wall cells of each class take consecutive roles;
//   * the (wave, stage) pairs that hold a wall cell (wall_wave_stages) are no more than before.
// Prints "tiles N wall_tiles W moved M pairs_before A pairs_after B max_slots S" and returns 0; a difference: its message on stderr,
// status 3.
#include "../thetis_amd/csrc/swe2d_tiles.h"

#include <algorithm>
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
    const TileSpec before{3, 2, 256, 256, -1, 224, true}, after{3, 2, 256, 256, -1, 224, true, true};   // kTripleTiles of swe2d_api_fuse.hip
    const int WG = 256, XG = 9*WG;                             // SWE_FUSE_WG, SWE_FUSE3_XG of swe2d_fuse.h
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    std::vector<int> head, nbr, order, start32, cv, tail;
    if (!read_ints(in, head, 5) || head[0] != 3 || head[1] < head[2] || head[2] < 0) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t stride = (size_t)head[1];
    const int n = head[2];
    if (!read_ints(in, nbr, 3*stride) || !read_ints(in, order, head[3] ? n : 0) || !read_ints(in, start32, head[4] ? n : 0) ||
        !read_ints(in, cv, 3*stride) || !read_ints(in, tail, 1)) {
        fprintf(stderr, "short input\n");
        return 1;
    }
    fclose(in);
    std::vector<unsigned char> start(start32.begin(), start32.end());
    TileTable t0, t1;
    std::string err;
    if (build_tiles(nbr.data(), stride, n, order.empty() ? nullptr : order.data(), start.empty() ? nullptr : start.data(), before, t0, err) ||
        build_tiles(nbr.data(), stride, n, order.empty() ? nullptr : order.data(), start.empty() ? nullptr : start.data(), after, t1, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 2;
    }
    LaneRecords r0, r1;
    build_lane_records(t0, nbr.data(), cv.data(), stride, WG, 8u*(unsigned)XG, (unsigned)tail[0], r0);
    build_lane_records(t1, nbr.data(), cv.data(), stride, WG, 8u*(unsigned)XG, (unsigned)tail[0], r1);
    auto wall = [&](int c) { return nbr[c] < 0 || nbr[stride + c] < 0 || nbr[2*stride + c] < 0; };
    const int n_tiles = (int)t0.n_inner.size();
    CHECK((int)t1.n_inner.size() == n_tiles && t0.slot_first == t1.slot_first && t0.ring[0] == t1.ring[0] && t0.ring[1] == t1.ring[1],
          "the two tables differ in their tiles, rings or slot counts");
    long long pairs0 = 0, pairs1 = 0;
    int wall_tiles = 0, moved = 0, max_slots = 0;
    std::vector<int> lane0((size_t)n, -1);                    // the lane of a cell in the tile at hand, old order
    for (int tile = 0; tile < n_tiles; tile++) {
        const int ni = t0.n_inner[tile], nm = t0.n_mid[tile], rot = t0.rot[tile];
        CHECK(t1.n_inner[tile] == ni && t1.n_mid[tile] == nm && t1.rot[tile] == rot, "tile %d: counts or rotation differ", tile);
        const int ns = t0.slot_first[tile + 1] - t0.slot_first[tile];
        max_slots = std::max(max_slots, ns);
        auto at = [&](const TileTable &t, int role) { return t.cell[(size_t)tile*WG + ((role + 64*rot) & (WG - 1))]; };
        int nt = 0;
        while (nt < WG && at(t0, nt) >= 0) nt++;
        bool has_wall = false, same = true;
        for (int role = 0; role < WG; role++) {
            CHECK((at(t0, role) >= 0) == (role < nt) && (at(t1, role) >= 0) == (role < nt), "tile %d role %d: padding inside the roles", tile, role);
            if (role < nt) { has_wall = has_wall || wall(at(t0, role)); same = same && at(t0, role) == at(t1, role); }
        }
        CHECK(has_wall || same, "tile %d has no wall cell and its roles moved", tile);
        wall_tiles += has_wall;
        moved += !same;
        const int bound[4] = {0, ni, nm, nt};
        for (int cls = 0; cls < 3; cls++) {
            std::vector<int> a, b;
            for (int role = bound[cls]; role < bound[cls + 1]; role++) { a.push_back(at(t0, role)); b.push_back(at(t1, role)); }
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            CHECK(a == b, "tile %d class %d: not a permutation of the class", tile, cls);
            int first = -1, last = -1, count = 0;
            for (int role = bound[cls]; role < bound[cls + 1]; role++)
                if (wall(at(t1, role))) { if (first < 0) first = role; last = role; count++; }
            CHECK(count == 0 || last - first + 1 == count, "tile %d class %d: wall cells on roles %d .. %d, %d of them", tile, cls, first, last, count);
        }
        for (int l = 0; l < WG; l++) if (t0.cell[(size_t)tile*WG + l] >= 0) lane0[t0.cell[(size_t)tile*WG + l]] = l;
        for (int l = 0; l < WG; l++) {
            const int c = t1.cell[(size_t)tile*WG + l];
            if (c < 0) continue;
            const int l0 = lane0[c];
            CHECK(l0 >= 0, "tile %d lane %d: cell %d was not in the tile", tile, l, c);
            const int *a1 = &r1.lane[((size_t)(2*tile + 0)*WG + l)*4], *b1 = &r1.lane[((size_t)(2*tile + 1)*WG + l)*4];
            const int *a0 = &r0.lane[((size_t)(2*tile + 0)*WG + l0)*4], *b0 = &r0.lane[((size_t)(2*tile + 1)*WG + l0)*4];
            CHECK(a1[0] == c && a0[0] == c, "tile %d lane %d: the record's cell", tile, l);
            CHECK(b1[0] == b0[0] && b1[1] == b0[1] && b1[2] == b0[2] && b1[3] == b0[3], "tile %d cell %d: vertex offsets or bmarkers differ", tile, c);
            for (int f = 0; f < 3; f++)
                for (int half = 0; half < 2; half++) {
                    const unsigned w1 = ((unsigned)a1[1 + f] >> (16*half)) & 0xffffu, w0 = ((unsigned)a0[1 + f] >> (16*half)) & 0xffffu;
                    const bool out1 = w1 >= 8u*(unsigned)XG, out0 = w0 >= 8u*(unsigned)XG;
                    CHECK(out1 == out0, "tile %d cell %d facet %d: inside in one table, outside in the other", tile, c, f);
                    if (out1) {
                        const unsigned s1 = (w1 - 8u*XG)/48u, s0 = (w0 - 8u*XG)/48u;
                        CHECK((w1 - 8u*XG)%48u == (w0 - 8u*XG)%48u && (int)s1 < ns && (int)s0 < ns, "tile %d cell %d facet %d: staging address", tile, c, f);
                        const unsigned *o1 = &r1.slot[2*(size_t)(t1.slot_first[tile] + s1)], *o0 = &r0.slot[2*(size_t)(t0.slot_first[tile] + s0)];
                        CHECK(o1[0] == o0[0] && o1[1] == o0[1] && t1.slot_src[t1.slot_first[tile] + s1] == t0.slot_src[t0.slot_first[tile] + s0],
                              "tile %d cell %d facet %d: the slot's source moved", tile, c, f);
                    } else {
                        const unsigned p1 = w1/(8u*WG), p0 = w0/(8u*WG), n1 = (w1%(8u*WG))/8u, n0 = (w0%(8u*WG))/8u;
                        CHECK(p1 == p0 && p1 < 3u && w1%8u == 0u, "tile %d cell %d facet %d: the neighbour's node moved", tile, c, f);
                        CHECK(t1.cell[(size_t)tile*WG + n1] == t0.cell[(size_t)tile*WG + n0] && t1.cell[(size_t)tile*WG + n1] >= 0,
                              "tile %d cell %d facet %d: lane %u holds another cell than lane %u held", tile, c, f, n1, n0);
                    }
                }
        }
        for (int l = 0; l < WG; l++) if (t0.cell[(size_t)tile*WG + l] >= 0) lane0[t0.cell[(size_t)tile*WG + l]] = -1;
        const long long p0 = wall_wave_stages(t0, nbr.data(), stride, 3, WG, tile), p1 = wall_wave_stages(t1, nbr.data(), stride, 3, WG, tile);
        CHECK(p1 <= p0 && (has_wall ? p1 >= 1 : p0 == 0), "tile %d: %lld (wave, stage) pairs with a wall cell, %lld before", tile, p1, p0);
        pairs0 += p0; pairs1 += p1;
    }
    CHECK(pairs0 == wall_wave_stages(t0, nbr.data(), stride, 3, WG) && pairs1 == wall_wave_stages(t1, nbr.data(), stride, 3, WG), "the table's total");
    printf("tiles %d wall_tiles %d moved %d pairs_before %lld pairs_after %lld max_slots %d\n", n_tiles, wall_tiles, moved, pairs0, pairs1, max_slots);
    return 0;
}
