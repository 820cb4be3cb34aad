// tile_layout_main.cpp - the third plane of the lane records and the plane layout of the staging area (thetis_amd/csrc/swe2d_tiles.h:
// LaneRecords::lane_slot, kStagingPlanes), checked on the host: tests/test_tile_layout.py compiles this with the address and
// undefined-behaviour sanitizers and runs it per mesh.
//
//   tile_layout_main IN
//
// IN: the input of tests/tile_records_main.cpp (header, neighbour codes [3][stride], order, start flags, vertex ids [3][stride], the
// byte length of a state plane).  Builds the 'triple' tables and the records twice, with the [slot][6] staging area of the eight-argument
// call and with kStagingPlanes, as swe2d_api_fuse.hip does, and checks for every tile
//   * the slot plane: lane 64*(s & 3) + (s >> 2) carries the {ob, oa} of slot s as the old arrays hold them (slot_first / slot), every
//     other lane - padding lanes among them - the sentinel {~0u, ~0u}, and no real offset is the sentinel;
//   * every OUTSIDE tr word of the plane layout: its slot s (read from the old layout's word, which is checked by tile_records_main)
//     is gathered by lane L = 64*(s & 3) + (s >> 2), whose writer fills index L of plane 3c (node f + 1) and 3c + 1 (node f) of P1 with
//     component c - so the word must be {P1 + 8 L, P1 + 8*256 + 8 L}, and with the component step 3*256*8 of SWE_TR_BYTES_INSIDE all six
//     addresses lie in planes 0, 1, 3, 4, 6, 7 of P1, below its end, at an index a writer of this tile fills (s < the tile's slots);
//     two slots of a tile never share an index;
//   * every INSIDE word, the cell, the vertex offsets and bmarkers: the same in both layouts, and so are the slot arrays.
// Prints "tiles N real R padding P rotations MASK max_slots M min_slots m slots T outside O" and returns 0; a difference: its message on
// stderr, status 3.
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
    const TileSpec spec{3, 2, 256, 256, -1, 224, true, true};  // kTripleTiles of swe2d_api_fuse.hip
    const int WG = 256, XG = 9*WG;                             // SWE_FUSE_WG, SWE_FUSE3_XG of swe2d_fuse.h: the staging area is P1
    const unsigned P1 = 8u*(unsigned)XG, P1_END = P1 + 9u*8u*(unsigned)WG, PLANE = 8u*(unsigned)WG, STEP = 3u*PLANE;
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
    const unsigned S8 = (unsigned)tail[0];
    std::vector<unsigned char> start(start32.begin(), start32.end());
    TileTable t;
    std::string err;
    if (build_tiles(nbr.data(), stride, n, order.empty() ? nullptr : order.data(), start.empty() ? nullptr : start.data(), spec, t, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 2;
    }
    LaneRecords r0, r1;
    build_lane_records(t, nbr.data(), cv.data(), stride, WG, P1, S8, r0);
    build_lane_records(t, nbr.data(), cv.data(), stride, WG, P1, S8, r1, kStagingPlanes);
    const int n_tiles = (int)t.n_inner.size();
    CHECK(r1.lane.size() == r0.lane.size() && r0.lane.size() == (size_t)n_tiles*2*WG*4, "lane records: %zu and %zu words", r0.lane.size(), r1.lane.size());
    CHECK(r0.slot == r1.slot && r0.slot.size() == 2*t.slot_src.size(), "the slot arrays depend on the layout");
    CHECK(r0.lane_slot == r1.lane_slot && r1.lane_slot.size() == (size_t)n_tiles*WG*2, "slot plane: %zu words for %d tiles", r1.lane_slot.size(), n_tiles);
    long long n_real = 0, n_pad = 0, n_outside = 0;
    int rotations = 0, max_slots = 0, min_slots = 1 << 30;
    for (int tile = 0; tile < n_tiles; tile++) {
        rotations |= 1 << t.rot[tile];
        const int first = t.slot_first[tile], ns = t.slot_first[tile + 1] - first;
        if (ns > max_slots) max_slots = ns;
        if (ns < min_slots) min_slots = ns;
        CHECK(ns >= 0 && ns <= spec.max_out, "tile %d: %d slots", tile, ns);
        // the slot plane against the old arrays under the slot -> lane map
        std::vector<int> slot_of(WG, -1);
        for (int s = 0; s < ns; s++) {
            const int L = 64*(s & 3) + (s >> 2);
            CHECK(L < WG && slot_of[L] < 0, "tile %d slot %d: lane %d twice", tile, s, L);
            slot_of[L] = s;
        }
        for (int lane = 0; lane < WG; lane++) {
            const unsigned *ls = &r1.lane_slot[((size_t)tile*WG + lane)*2];
            if (slot_of[lane] < 0) {
                CHECK(ls[0] == kNoSlot && ls[1] == kNoSlot, "tile %d lane %d: no slot, but the plane says %u %u", tile, lane, ls[0], ls[1]);
                continue;
            }
            const unsigned *so = &r0.slot[2*(size_t)(first + slot_of[lane])];
            CHECK(ls[0] == so[0] && ls[1] == so[1], "tile %d lane %d slot %d: %u %u, the slot arrays say %u %u", tile, lane, slot_of[lane], ls[0], ls[1], so[0], so[1]);
            CHECK(ls[0] != kNoSlot, "tile %d lane %d: an offset that is the sentinel", tile, lane);
        }
        // the lane records
        std::vector<unsigned char> read_at(WG, 0);
        for (int lane = 0; lane < WG; lane++) {
            const int *a0 = &r0.lane[((size_t)(2*tile + 0)*WG + lane)*4], *a1 = &r1.lane[((size_t)(2*tile + 0)*WG + lane)*4];
            const int *b0 = &r0.lane[((size_t)(2*tile + 1)*WG + lane)*4], *b1 = &r1.lane[((size_t)(2*tile + 1)*WG + lane)*4];
            CHECK(a0[0] == a1[0] && b0[0] == b1[0] && b0[1] == b1[1] && b0[2] == b1[2] && b0[3] == b1[3], "tile %d lane %d: cell, vertices or bmarkers depend on the layout", tile, lane);
            if (a0[0] < 0) {
                n_pad++;
                CHECK(a1[0] == -1 && !a1[1] && !a1[2] && !a1[3], "tile %d lane %d: a padding lane with a record", tile, lane);
                CHECK(slot_of[lane] >= 0 || r1.lane_slot[((size_t)tile*WG + lane)*2] == kNoSlot, "tile %d lane %d: padding lane, slot word", tile, lane);
                continue;
            }
            n_real++;
            for (int f = 0; f < 3; f++) {
                const unsigned w0 = (unsigned)a0[1 + f], w1 = (unsigned)a1[1 + f];
                const unsigned fw = t.facet[((size_t)tile*WG + lane)*3 + f];
                if (!(fw & kTileOutside)) {
                    CHECK(w0 == w1, "tile %d lane %d facet %d: an inside word changed, 0x%x -> 0x%x", tile, lane, f, w0, w1);
                    CHECK((w1 & 0xffffu) < P1 && (w1 >> 16) + 2u*STEP < P1, "tile %d lane %d facet %d: an inside word outside P0", tile, lane, f);
                    continue;
                }
                n_outside++;
                // the slot, from the old layout's word: P1 + 48 s | (P1 + 24 + 48 s) << 16
                const unsigned ab0 = w0 & 0xffffu, s = (ab0 - P1)/48u;
                CHECK(ab0 >= P1 && (ab0 - P1) % 48u == 0u && s == (fw & 0x1ffu) && (w0 >> 16) == ab0 + 24u, "tile %d lane %d facet %d: old word 0x%x", tile, lane, f, w0);
                CHECK((int)s < ns, "tile %d lane %d facet %d: slot %u of %d", tile, lane, f, s, ns);
                const unsigned L = 64u*(s & 3u) + (s >> 2);
                CHECK(slot_of[L] == (int)s, "tile %d lane %d facet %d: slot %u has no writer on lane %u", tile, lane, f, s, L);
                const unsigned ab = w1 & 0xffffu, aa = w1 >> 16;
                CHECK(ab == P1 + 8u*L && aa == P1 + PLANE + 8u*L, "tile %d lane %d facet %d: word 0x%x, the writer of slot %u fills index %u", tile, lane, f, w1, s, L);
                for (unsigned c = 0; c < 3; c++) {
                    const unsigned pb = (ab + c*STEP - P1)/PLANE, pa = (aa + c*STEP - P1)/PLANE;
                    CHECK(pb == 3u*c && pa == 3u*c + 1u && (ab + c*STEP - P1) % PLANE == 8u*L && (aa + c*STEP - P1) % PLANE == 8u*L,
                          "tile %d lane %d facet %d component %u: planes %u %u", tile, lane, f, c, pb, pa);
                    CHECK(ab + c*STEP + 8u <= P1_END && aa + c*STEP + 8u <= P1_END, "tile %d lane %d facet %d component %u: beyond P1", tile, lane, f, c);
                }
                CHECK(!read_at[L], "tile %d: two facets read the slot on lane %u", tile, L);
                read_at[L] = 1;
            }
        }
        for (int s = 0; s < ns; s++) CHECK(read_at[64*(s & 3) + (s >> 2)], "tile %d slot %d: gathered and never read", tile, s);
    }
    if (n_tiles == 0) min_slots = 0;
    printf("tiles %d real %lld padding %lld rotations %d max_slots %d min_slots %d slots %zu outside %lld\n", n_tiles, n_real, n_pad, rotations,
           max_slots, min_slots, t.slot_src.size(), n_outside);
    return 0;
}
