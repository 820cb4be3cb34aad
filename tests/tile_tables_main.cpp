// tile_tables_main.cpp - runs the tile-table builder of the fused stage kernels (thetis_amd/csrc/swe2d_tiles.h) by itself, on the host:
// tests/test_tile_tables.py compiles it with the address and undefined-behaviour sanitizers and reads what it writes.
//
//   tile_tables_main pair|quad|triple IN OUT
//
// IN (int32, native order): nfacets, stride, n_cells, has_order, has_start; the packed neighbour codes [nfacets][stride] as swe2d_create
// packs them ((neighbour << 2) | its facet, or -marker); n_cells of order if has_order; n_cells of start flags if has_start.
// OUT (int32): n_tiles, wg, nfacets, ring 1 cells, ring 2 cells; cell[n_tiles*wg]; facet[n_tiles*wg*nfacets]; n_inner, n_mid, rot [n_tiles] each.
// Exit status 2 with the builder's message on stderr when it declines the mesh.
#include "../thetis_amd/csrc/swe2d_tiles.h"

#include <cstdio>
#include <cstring>

using namespace swe2d_impl;

static bool read_ints(FILE *f, std::vector<int> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(int), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s pair|quad|triple IN OUT\n", argv[0]); return 1; }
    // the caps of thetis_amd/csrc/swe2d_fuse.h (SWE_FUSE_WG, _INNER, _RING, _MAX_OUT; SWE_QFUSE_*; SWE_FUSE3_MAX_OUT), as swe2d_api_fuse.hip hands them in
    TileSpec spec;
    if (!strcmp(argv[1], "pair")) spec = TileSpec{3, 1, 256, 192, 64, 128, false};
    else if (!strcmp(argv[1], "quad")) spec = TileSpec{4, 1, 256, 192, 64, 192, false};
    else if (!strcmp(argv[1], "triple")) spec = TileSpec{3, 2, 256, 256, -1, 224, true};
    else { fprintf(stderr, "unknown kind %s\n", argv[1]); return 1; }
    FILE *in = fopen(argv[2], "rb");
    if (!in) { perror(argv[2]); return 1; }
    std::vector<int> head, nbr, order, start32;
    if (!read_ints(in, head, 5) || head[0] != spec.nfacets || head[1] < head[2] || head[2] < 0) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t stride = (size_t)head[1];
    const int n = head[2];
    if (!read_ints(in, nbr, (size_t)spec.nfacets*stride) || !read_ints(in, order, head[3] ? n : 0) || !read_ints(in, start32, head[4] ? n : 0)) {
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
    FILE *out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 1; }
    const int h[5] = {(int)t.n_inner.size(), spec.wg, spec.nfacets, (int)t.ring[0], (int)t.ring[1]};
    fwrite(h, sizeof(int), 5, out);
    fwrite(t.cell.data(), sizeof(int), t.cell.size(), out);
    fwrite(t.facet.data(), sizeof(unsigned), t.facet.size(), out);
    fwrite(t.n_inner.data(), sizeof(int), t.n_inner.size(), out);
    fwrite(t.n_mid.data(), sizeof(int), t.n_mid.size(), out);
    fwrite(t.rot.data(), sizeof(int), t.rot.size(), out);
    return fclose(out) == 0 ? 0 : 1;
}
