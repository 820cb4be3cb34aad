// swe2d_tiles.h - the tile tables of the fused stage kernels (swe2d_fuse.h): which cells a workgroup holds, on which lane, and where
// each facet finds its neighbour.  Host integer logic only: no HIP header, no handle (tests/tile_tables_main.cpp runs it by itself).
//
// A tile = consecutive cells of an order (the interior) + ring 1, every cell that shares a facet with an interior cell + (two-ring
// tiles) ring 2, the facet neighbours of ring 1.  The interior grows cell by cell while the caps of the TileSpec hold - and, where the
// caller marks positions of the order as tile starts, up to the next mark.  ROLES are numbered [interior in the order added | ring 1 |
// ring 2], each ring in the order of discovery without the cells that moved inwards later; the rest of the wg lanes is padding.
// (TileSpec::group_walls: inside each of the three classes the cells with a boundary facet take consecutive roles, see build_tiles.)
// Per role and facet the table holds a 10-bit field: the lane of the neighbour in the tile (a boundary facet: the lane itself) or,
// with bit 9 set, the staging slot of a neighbour outside the tile - only facets of the outermost ring lead there, slots are counted
// per tile in role order.  How the fields are packed into device records is the caller's (swe2d_api_fuse.hip).
// Next to the fields, per tile, the SOURCE of every staging slot: the neighbour code of the facet that names the slot ((neighbour << 2) |
// the neighbour's facet g: its nodes g and (g + 1) % 3 lie on the shared facet), slot after slot - slot_src[slot_first[tile] + slot],
// slot_first[n_tiles] = the total.  A kernel that gathers the traces from outside the tile slot by slot needs nothing else.
//
// Lanes: role r sits on the physical lane (r + 64*rot) & (wg - 1); rot = 0 unless the spec rotates.  In the three-stage kernel the wave
// that holds the last 64 roles runs two stage bodies, the other three run three; which wave that is follows from rot, and rot from the
// tile number by SWE_FUSE3_ROT - a host-side policy, the kernel reads it from its counts.  Not tile & 3: the XCD-chunked block map and
// the dealing of workgroups over the compute units of an XCD can hand one compute unit tiles of a single residue.  The top two bits of
// tile x 2^32/phi instead: every arithmetic progression of tile numbers meets the four values equally often.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#ifndef SWE_FUSE3_ROT
#define SWE_FUSE3_ROT(tile) ((int)(((unsigned)(tile)*0x9E3779B1u) >> 30))
#endif

namespace swe2d_impl {

constexpr unsigned kTileOutside = 0x200u;             // facet field: bits [8:0] are a staging slot, not a lane

struct TileSpec {
    int nfacets;              // 3 | 4 facets per cell
    int rings;                // 1 | 2
    int wg;                   // lanes of a tile: the cap of interior + rings
    int max_inner;            // cap of the interior
    int max_ring1;            // cap of ring 1; < 0: only the total is bounded
    int max_out;              // staging slots: (nfacets - 1) per cell of the outermost ring must fit
    bool rotate;              // rot of tile t = SWE_FUSE3_ROT(t), else 0
    bool group_walls = false; // the cells with a boundary facet of a tile on consecutive roles, see build_tiles (the three-stage kernel)
};

struct TileTable {
    std::vector<int> cell;                 // [n_tiles*wg] cell or -1, by physical lane
    std::vector<unsigned> facet;           // [n_tiles*wg*nfacets] 10-bit fields, by physical lane
    std::vector<int> n_inner, n_mid, rot;  // [n_tiles]: roles below n_inner are interior, below n_mid ring 1
    long long ring[2] = {0, 0};            // cells of ring 1 / ring 2 over all tiles
    std::vector<int> slot_src;             // neighbour code of every staging slot, tile after tile
    std::vector<int> slot_first;           // [n_tiles + 1]: where a tile's slots start in slot_src
};

// nbr: packed neighbour codes [nfacets][stride], (neighbour << 2) | its facet, or -marker on the boundary.  order: a permutation of
// the cells, or null for the numbering.  start: [n_cells] 1 = a tile begins at this position of the order, or null.
// Returns 0, or 1 with the reason in err (the mesh does not fit the caps, or the bookkeeping found itself wrong).
inline int build_tiles(const int *nbr, size_t stride, int n_cells, const int *order, const unsigned char *start,
                       const TileSpec &sp, TileTable &t, std::string &err)
{
    const int n = n_cells, nf = sp.nfacets, wg = sp.wg;
    const char *who = sp.rings == 2 ? "fused stages: " : "fused stage pair: ";
    t = TileTable();
    std::vector<unsigned char> state((size_t)n, 0);                // 0 outside | 1 interior | 2 ring 1 | 3 ring 2, of the tile being built
    std::vector<int> lane_of((size_t)n, -1), touched, inner;
    std::vector<std::pair<int, unsigned char>> undo;
    int count[4] = {0, 0, 0, 0};
    t.slot_first.push_back(0);
    auto set = [&](int c, unsigned char ns) {
        undo.push_back({c, state[c]});
        if (state[c] == 0) touched.push_back(c);
        count[state[c]]--; state[c] = ns; count[ns]++;
    };
    for (int pos = 0; pos < n;) {
        inner.clear(); touched.clear();
        count[1] = count[2] = count[3] = 0;
        while (pos < n && (int)inner.size() < sp.max_inner) {
            if (start && start[pos] && !inner.empty()) break;      // the caller's tiles: compact patches
            const int kk = order ? order[pos] : pos;
            undo.clear();
            const size_t touched_before = touched.size();
            set(kk, 1);
            for (int f = 0; f < nf; f++) {
                const int code = nbr[(size_t)f*stride + kk];
                if (code < 0) continue;
                const int c1 = code >> 2;
                if (state[c1] == 0 || state[c1] == 3) {
                    set(c1, 2);
                    for (int g = 0; sp.rings == 2 && g < nf; g++) {
                        const int code2 = nbr[(size_t)g*stride + c1];
                        if (code2 >= 0 && state[code2 >> 2] == 0) set(code2 >> 2, 3);
                    }
                }
            }
            if (count[1] + count[2] + count[3] > wg || (sp.max_ring1 >= 0 && count[2] > sp.max_ring1) || (nf - 1)*count[sp.rings + 1] > sp.max_out) {
                if (inner.empty()) {
                    err = std::string(who) + (sp.rings == 2 ? "a cell whose two rings do not fit a tile" : "a cell with more neighbours than a ring holds");
                    return 1;
                }
                for (size_t i = undo.size(); i-- > 0;) { count[state[undo[i].first]]--; state[undo[i].first] = undo[i].second; count[undo[i].second]++; }
                touched.resize(touched_before);
                break;
            }
            inner.push_back(kk);
            pos++;
        }
        // roles: the interior in the order it was added, ring 1, ring 2 (in the order of discovery)
        std::vector<int> cells(inner);
        for (int want = 2; want <= 3; want++)
            for (int c : touched) if (state[c] == want) cells.push_back(c);
        const int ni = (int)inner.size(), nm = ni + count[2], nt = (int)cells.size();
        // group_walls: a wave with a wall cell among its lanes runs the boundary pass of swe_tri_finish (once, twice with a corner cell), in
        // every stage that is active on it - stage 1 on every role, stage 2 below nm, stage 3 below ni.  In the order above the wall cells
        // of a patch at the wall lie all over its roles, so nearly every wave of the tile pays.  Here the wall cells of each class take
        // consecutive roles, inside the group and around it the order above.  Where the group sits in its class is chosen so that the
        // fewest (wave, stage) pairs hold a wall cell - waves are 64 consecutive roles, whatever the rotation: first choice the END of
        // the interior and the START of each ring (one run across ni, the bound of stage 3), else a place at an end of the class or
        // against a multiple of 64 that does better (a group that would straddle a wave it need not touch).  A tile without a wall cell
        // keeps its roles, and so does one - none known - that no such placement serves as well as the order above.  The rings' caps, the
        // counts and the slots (numbered in role order below) do not look at the order.
        if (sp.group_walls) {
            auto wall = [&](int c) { for (int f = 0; f < nf; f++) if (nbr[(size_t)f*stride + c] < 0) return true; return false; };
            const int bound[4] = {0, ni, nm, nt}, limit[3] = {nt, nm, ni};
            std::vector<int> walls[3], rest[3];
            for (int cls = 0; cls < 3; cls++)
                for (int l = bound[cls]; l < bound[cls + 1]; l++) (wall(cells[l]) ? walls[cls] : rest[cls]).push_back(cells[l]);
            auto pairs_of = [&](const unsigned char *is_wall) {          // is_wall[role]
                int pairs = 0;
                for (int st = 0; st < 3; st++) {
                    unsigned waves = 0u;
                    for (int r = 0; r < limit[st]; r++) if (is_wall[r]) waves |= 1u << (r >> 6);
                    for (; waves; waves &= waves - 1) pairs++;
                }
                return pairs;
            };
            if (!walls[0].empty() || !walls[1].empty() || !walls[2].empty()) {
                std::vector<unsigned char> mark((size_t)nt + 1, 0);
                for (int l = 0; l < nt; l++) mark[l] = wall(cells[l]);
                int best = pairs_of(mark.data()) + 1, best_off[3] = {-1, -1, -1};     // (+ 1: a tie with the order above goes to the grouping)
                std::vector<int> cand[3];
                for (int cls = 0; cls < 3; cls++) {
                    const int w = (int)walls[cls].size(), room = (int)rest[cls].size();
                    cand[cls].push_back(cls == 0 ? room : 0);
                    cand[cls].push_back(cls == 0 ? 0 : room);
                    for (int edge = 64; edge < wg && w > 0; edge += 64)
                        for (int o : {edge - bound[cls], edge - w - bound[cls]}) if (o > 0 && o < room) cand[cls].push_back(o);
                }
                for (int o0 : cand[0]) for (int o1 : cand[1]) for (int o2 : cand[2]) {
                    const int off[3] = {o0, o1, o2};
                    std::fill(mark.begin(), mark.end(), 0);
                    for (int cls = 0; cls < 3; cls++)
                        for (int l = 0; l < (int)walls[cls].size(); l++) mark[bound[cls] + off[cls] + l] = 1;
                    const int pairs = pairs_of(mark.data());
                    if (pairs < best) { best = pairs; best_off[0] = o0; best_off[1] = o1; best_off[2] = o2; }
                }
                if (best_off[0] >= 0) {
                    std::vector<int> sorted;
                    for (int cls = 0; cls < 3; cls++) {
                        sorted.insert(sorted.end(), rest[cls].begin(), rest[cls].begin() + best_off[cls]);
                        sorted.insert(sorted.end(), walls[cls].begin(), walls[cls].end());
                        sorted.insert(sorted.end(), rest[cls].begin() + best_off[cls], rest[cls].end());
                    }
                    cells.swap(sorted);
                }
            }
        }
        if (nt != count[1] + count[2] + count[3] || ni != count[1] || nt > wg) { err = std::string(who) + "tile bookkeeping"; return 1; }
        const int tile = (int)t.n_inner.size();
        const int rot = sp.rotate ? SWE_FUSE3_ROT(tile) & 3 : 0;
        auto phys = [rot, wg](int role) { return (role + 64*rot) & (wg - 1); };
        for (int l = 0; l < nt; l++) lane_of[cells[l]] = phys(l);
        const size_t base = (size_t)tile*wg;
        t.cell.resize(base + wg, -1);
        t.facet.resize((base + wg)*nf, 0u);
        const int outermost = sp.rings == 2 ? nm : ni;             // the first role that may have a neighbour outside the tile
        int n_out = 0;
        for (int l = 0; l < nt; l++) {
            const int c = cells[l];
            t.cell[base + phys(l)] = c;
            for (int f = 0; f < nf; f++) {
                const int code = nbr[(size_t)f*stride + c];
                unsigned field;
                if (code < 0) field = (unsigned)phys(l);                             // boundary facet: the cell itself
                else if (state[code >> 2] != 0) field = (unsigned)lane_of[code >> 2];
                else {
                    if (l < outermost || n_out >= sp.max_out) { err = std::string(who) + "ring bookkeeping"; return 1; }
                    field = kTileOutside | (unsigned)n_out++;
                    t.slot_src.push_back(code);
                }
                t.facet[(base + phys(l))*nf + f] = field;
            }
        }
        t.n_inner.push_back(ni); t.n_mid.push_back(nm); t.rot.push_back(rot);
        t.ring[0] += count[2]; t.ring[1] += count[3];
        t.slot_first.push_back((int)t.slot_src.size());
        for (int c : cells) { state[c] = 0; lane_of[c] = -1; }
    }
    return 0;
}

// How many (wave, stage) pairs of a two-ring table hold a cell with a boundary facet: stage 1 runs every role, stage 2 the roles below
// n_mid, stage 3 those below n_inner, and a wave is 64 consecutive PHYSICAL lanes.  Each such pair is one execution of the boundary
// pass of swe_tri_finish that a wave without a wall cell branches round.  tile < 0: summed over the table.
inline long long wall_wave_stages(const TileTable &t, const int *nbr, size_t stride, int nfacets, int wg, int tile = -1)
{
    long long pairs = 0;
    const int n_tiles = (int)t.n_inner.size();
    for (int tl = tile < 0 ? 0 : tile; tl < (tile < 0 ? n_tiles : tile + 1); tl++) {
        unsigned waves[3] = {0u, 0u, 0u};
        for (int l = 0; l < wg; l++) {
            const int c = t.cell[(size_t)tl*wg + l];
            if (c < 0) continue;
            bool wall = false;
            for (int f = 0; f < nfacets; f++) wall = wall || nbr[(size_t)f*stride + c] < 0;
            if (!wall) continue;
            const int role = (l - 64*t.rot[tl]) & (wg - 1);
            waves[0] |= 1u << (l >> 6);
            if (role < t.n_mid[tl]) waves[1] |= 1u << (l >> 6);
            if (role < t.n_inner[tl]) waves[2] |= 1u << (l >> 6);
        }
        for (int s = 0; s < 3; s++) for (unsigned w = waves[s]; w; w &= w - 1) pairs++;
    }
    return pairs;
}

// ---- the lane records of the three-stage kernel (swe2d_fuse.h: swe_fuse123_kernel) ---------------------------------------------------
// Everything a lane of a tile derives from the mesh and the table before its first load of the state, decoded once here instead of in
// every lane of every step: the kernel reads the words and issues its loads.  Two planes of wg int4 per tile, by physical lane:
//   lane[((2*tile + 0)*wg + l)*4 ..] = {cell or -1, tr[0], tr[1], tr[2]}: per facet f the BYTE address in LDS of component 0's trace at
//       the neighbour's node on my node f + 1, | the same on my node f << 16.  The neighbour traverses the shared facet backwards: its
//       node g sits on my node f + 1, its node (g + 1) % 3 on my node f, g = the low two bits of the neighbour code (a boundary facet:
//       g = f, and the table's field is the lane itself).  A neighbour in the tile on lane `at`: plane g of the 8-byte planes of wg
//       lanes, plane_g*8*wg + 8*at; outside, in staging slot `at`: xg_bytes + 48*at and 24 further ([slot][6] doubles);
//   lane[((2*tile + 1)*wg + l)*4 ..] = {8*vertex 0, 8*vertex 1, 8*vertex 2, bmarkers}: the byte offsets of the cell's vertices in the
//       coordinate arrays, and 8 bits of marker per boundary facet (marker of facet f << 8 f, 0 for a facet with a neighbour).
// A padding lane: {-1, 0, 0, 0}, {0, 0, 0, 0}.
// Per staging slot, slot[2*(slot_first[tile] + s) ..] = {ob, oa}: the byte offsets into the three state planes of one component
// (plane length s8 bytes) of the slot's source cell at its node g and at its node (g + 1) % 3, source = slot_src = (cell << 2) | g.
// The arithmetic is the unsigned 32-bit arithmetic the kernel did: the words are the bits it formed.
//
// A third plane, by physical lane again (round 22): lane_slot[(tile*wg + l)*2 ..] = the {ob, oa} of the staging slot that lane l of the
// tile gathers - slot s is the work of lane lane_of_slot(s, wg) = (wg/4)*(s & 3) + (s >> 2), the slots dealt round over the four waves -
// or {kNoSlot, kNoSlot} for a lane without one (no offset into a state plane is that large: the planes hold 8-byte values).  A lane
// reads its own word next to its record, with an address that depends on the tile and the lane alone: one trip to memory, where the
// per-tile {first, count} and then slot[first + s] were two.
//
// kStagingPlanes (round 22) lays the staging area out like the state planes: planes of wg 8-byte values behind xg_bytes, component c of
// a slot's value on the reader's node f + 1 in plane 3c, the value on its node f in plane 3c + 1, and slot s at index lane_of_slot(s) -
// the lane that gathers it, which therefore writes its six values where it writes its own state, one plane on: 8-byte stride over the
// lanes of a wave, no bank conflict (at index s the lanes of a wave would be 32 B apart, four to a bank; [slot][6] had them 192 B
// apart, sixteen to a bank).  The outside tr words then have the form of the inside ones - component step 3*wg*8 bytes, the two nodes
// one plane apart - and 8 planes are touched: 3c + 1 <= 7, and lane_of_slot < wg.
constexpr unsigned kNoSlot = 0xffffffffu;
enum StagingLayout { kStagingSlot6 = 0, kStagingPlanes = 1 };
inline unsigned lane_of_slot(unsigned s, int wg) { return (unsigned)(wg/4)*(s & 3u) + (s >> 2); }

struct LaneRecords {
    std::vector<int> lane;                 // [n_tiles][2][wg] int4
    std::vector<unsigned> slot;            // [slot_first[n_tiles]] uint2
    std::vector<unsigned> lane_slot;       // [n_tiles][wg] uint2
};

// nbr, cv: [3][stride] neighbour codes and vertex ids (triangles).  xg_bytes: where the staging area starts in LDS; s8: the byte length
// of a state plane.  staging: how the outside tr words address the staging area.
inline void build_lane_records(const TileTable &t, const int *nbr, const int *cv, size_t stride, int wg, unsigned xg_bytes, unsigned s8,
                               LaneRecords &r, StagingLayout staging = kStagingSlot6)
{
    const size_t n_tiles = t.n_inner.size();
    r.lane.assign(n_tiles*2*(size_t)wg*4, 0);
    r.slot.assign(2*t.slot_src.size(), 0u);
    r.lane_slot.assign(n_tiles*(size_t)wg*2, kNoSlot);
    const unsigned plane = 8u*(unsigned)wg;
    for (size_t tile = 0; tile < n_tiles; tile++) {
        for (int l = 0; l < wg; l++) {
            int *a = &r.lane[((2*tile + 0)*wg + l)*4], *b = &r.lane[((2*tile + 1)*wg + l)*4];
            const int c = t.cell[tile*wg + l];
            a[0] = c;
            if (c < 0) { a[0] = -1; continue; }
            unsigned bm = 0u;
            for (int f = 0; f < 3; f++) {
                const int code = nbr[(size_t)f*stride + c];
                const unsigned w = t.facet[(tile*wg + l)*3 + f], at = w & 0x1ffu;
                const unsigned g = code >= 0 ? (unsigned)(code & 3) : (unsigned)f, ga = g == 2u ? 0u : g + 1u;
                const bool outside = (w & kTileOutside) != 0u;
                unsigned ab = outside ? xg_bytes + 48u*at : plane*g + 8u*at;
                unsigned aa = outside ? xg_bytes + 24u + 48u*at : plane*ga + 8u*at;
                if (outside && staging == kStagingPlanes) { ab = xg_bytes + 8u*lane_of_slot(at, wg); aa = ab + plane; }
                a[1 + f] = (int)(ab | (aa << 16));
                if (code < 0) bm |= (unsigned)(-code) << (8*f);
                b[f] = (int)((unsigned)cv[(size_t)f*stride + c]*8u);
            }
            b[3] = (int)bm;
        }
    }
    for (size_t s = 0; s < t.slot_src.size(); s++) {
        const unsigned code = (unsigned)t.slot_src[s], kn8 = (code >> 2)*8u, g = code & 3u;
        r.slot[2*s] = kn8 + (g == 0u ? 0u : (g == 1u ? s8 : 2u*s8));
        r.slot[2*s + 1] = kn8 + (g == 0u ? s8 : (g == 1u ? 2u*s8 : 0u));
    }
    for (size_t tile = 0; tile < n_tiles; tile++)
        for (int s = t.slot_first[tile]; s < t.slot_first[tile + 1]; s++) {
            unsigned *ls = &r.lane_slot[(tile*wg + lane_of_slot((unsigned)(s - t.slot_first[tile]), wg))*2];
            ls[0] = r.slot[2*(size_t)s]; ls[1] = r.slot[2*(size_t)s + 1];
        }
}

}  // namespace swe2d_impl
