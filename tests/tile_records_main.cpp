// tile_records_main.cpp - the lane records of the three-stage kernel (thetis_amd/csrc/swe2d_tiles.h: build_lane_records), checked on the
// host: tests/test_tile_records.py compiles this with the address and undefined-behaviour sanitizers and runs it per mesh.
//
//   tile_records_main IN
//
// IN: the input of tests/tile_tables_main.cpp (int32: nfacets = 3, stride, n_cells, has_order, has_start; neighbour codes [3][stride];
// order; start flags), then the vertex ids [3][stride] and one int32, the byte length of a state plane.  Builds the 'triple' tables and
// the records as swe2d_api_fuse.hip does and compares EVERY field of every lane and slot with the value the kernel's prologue formed
// before the records existed, restated here from that prologue: the connectivity through swe_conn_pack / swe_conn_unpack with the wide
// record behind an escape, bmarkers from the neighbour codes, per facet the 10-bit field of the packed tile word, f2 / f2a, the outside
// test and the two byte addresses, per vertex 8 * id, per slot scode >> 2, scode & 3 and the two selects.
// Prints "tiles N real R padding P escapes E corners C rotations MASK max_slots M slots T" and returns 0; a difference: its message on
// stderr, status 3.
#include "../thetis_amd/csrc/swe2d_conn.h"
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
    const int WG = 256, FBITS = 10, XG = 9*WG;                 // SWE_FUSE_WG, SWE_FUSE_FBITS, SWE_FUSE3_XG of swe2d_fuse.h
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
    LaneRecords r;
    build_lane_records(t, nbr.data(), cv.data(), stride, WG, 8u*(unsigned)XG, S8, r);
    const int n_tiles = (int)t.n_inner.size();
    CHECK(r.lane.size() == (size_t)n_tiles*2*WG*4, "lane records: %zu words for %d tiles", r.lane.size(), n_tiles);
    CHECK(r.slot.size() == 2*t.slot_src.size(), "slot records: %zu words for %zu slots", r.slot.size(), t.slot_src.size());
    long long n_real = 0, n_pad = 0, n_escape = 0, n_corner = 0;
    int rotations = 0, max_slots = 0;
    for (int tile = 0; tile < n_tiles; tile++) {
        rotations |= 1 << t.rot[tile];
        const int ns = t.slot_first[tile + 1] - t.slot_first[tile];
        if (ns > max_slots) max_slots = ns;
        for (int lane = 0; lane < WG; lane++) {
            const int *ra = &r.lane[((size_t)(2*tile + 0)*WG + lane)*4], *rb = &r.lane[((size_t)(2*tile + 1)*WG + lane)*4];
            // the int2 record the kernel read: {cell, w0 | w1 << 10 | w2 << 20}
            const unsigned *fw = &t.facet[((size_t)tile*WG + lane)*3];
            const int tl_x = t.cell[(size_t)tile*WG + lane], tl_y = (int)(fw[0] | (fw[1] << FBITS) | (fw[2] << (2*FBITS)));
            if (tl_x < 0) {
                n_pad++;
                CHECK(ra[0] == -1 && !ra[1] && !ra[2] && !ra[3] && !rb[0] && !rb[1] && !rb[2] && !rb[3], "tile %d lane %d: a padding lane with a record", tile, lane);
                continue;
            }
            n_real++;
            const int k = tl_x;
            CHECK(ra[0] == k, "tile %d lane %d: cell %d, the table says %d", tile, lane, ra[0], k);
            // swe_conn_load: the 16-B record, the wide ones behind an escape
            const int wide_nb[3] = {nbr[k], nbr[stride + k], nbr[2*stride + k]}, wide_v[3] = {cv[k], cv[stride + k], cv[2*stride + k]};
            int nb[3], vid[3];
            if (swe_conn_unpack(swe_conn_pack(k, wide_nb, wide_v), k, nb, vid)) {
                n_escape++;
                for (int i = 0; i < 3; i++) { nb[i] = wide_nb[i]; vid[i] = wide_v[i]; }
            }
            const int bmarkers = (nb[0] < 0 ? -nb[0] : 0) | (nb[1] < 0 ? (-nb[1]) << 8 : 0) | (nb[2] < 0 ? (-nb[2]) << 16 : 0);
            CHECK(rb[3] == bmarkers, "tile %d lane %d: bmarkers 0x%x, the prologue formed 0x%x", tile, lane, rb[3], bmarkers);
            if ((nb[0] < 0) + (nb[1] < 0) + (nb[2] < 0) >= 2) n_corner++;
            for (int f = 0; f < 3; f++) {
                const int nbf = nb[f];
                const unsigned w = ((unsigned)tl_y >> (FBITS*f)) & 0x3ffu;
                const bool outside = (w & 0x200u) != 0u;
                const unsigned at = w & 0x1ffu;
                const int f2 = nbf >= 0 ? (nbf & 3) : f, f2a = f2 == 2 ? 0 : f2 + 1;
                const unsigned ab = outside ? (unsigned)(8*XG) + 48u*at : (unsigned)(8*WG*f2) + 8u*at;
                const unsigned aa = outside ? (unsigned)(8*XG + 24) + 48u*at : (unsigned)(8*WG*f2a) + 8u*at;
                const unsigned tr = ab | (aa << 16);
                CHECK((unsigned)ra[1 + f] == tr, "tile %d lane %d facet %d: trace word 0x%x, the prologue formed 0x%x", tile, lane, f, (unsigned)ra[1 + f], tr);
                CHECK(ab < 65536u && aa < 65536u && (outside ? (int)at < ns : (int)at < WG), "tile %d lane %d facet %d: address out of its field", tile, lane, f);
                if (nbf < 0) CHECK(!outside && (int)at == lane, "tile %d lane %d facet %d: a boundary facet that does not point at the lane", tile, lane, f);
                const unsigned v8 = (unsigned)vid[f]*8u;
                CHECK((unsigned)rb[f] == v8, "tile %d lane %d vertex %d: offset %u, the prologue formed %u", tile, lane, f, (unsigned)rb[f], v8);
            }
        }
        for (int s = 0; s < ns; s++) {
            const int scode = t.slot_src[t.slot_first[tile] + s];
            const unsigned kn8 = (unsigned)(scode >> 2)*8u;
            const int g2 = scode & 3;
            const unsigned ob = kn8 + (g2 == 0 ? 0u : (g2 == 1 ? S8 : 2u*S8));
            const unsigned oa = kn8 + (g2 == 0 ? S8 : (g2 == 1 ? 2u*S8 : 0u));
            const unsigned *so = &r.slot[2*(size_t)(t.slot_first[tile] + s)];
            CHECK(so[0] == ob && so[1] == oa, "tile %d slot %d: offsets %u %u, the prologue formed %u %u", tile, s, so[0], so[1], ob, oa);
        }
    }
    printf("tiles %d real %lld padding %lld escapes %lld corners %lld rotations %d max_slots %d slots %zu\n", n_tiles, n_real, n_pad, n_escape,
           n_corner, rotations, max_slots, t.slot_src.size());
    return 0;
}
