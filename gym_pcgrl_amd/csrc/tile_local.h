// The local half of helper.py for any tile set (helper.py:37-137): get_floor_dist with _calc_dist_floor's value of every cell,
// get_type_grouping with _calc_group_value's, get_changes, and a count of every tile 0..31 -- what ONE LANE of the lanes that share a
// map does, over the map's tile bytes wherever they are (an LDS stage, or the caller's global memory).
//
// The choices.
//   * Lanes on columns.  A lane owns the columns lane, lane + nlanes, ... and walks each from the bottom row up, carrying the row of
//     the nearest floor tile at or below (the floor rule is that scan) and the tile below (the vertical changes).  The left neighbour
//     and the cells at the caller's offsets are read from the bytes again: LDS in the staged form, L2 in the other.  Consecutive lanes
//     hold consecutive cells of a row, so a row of either per-cell output is one contiguous run of stores across the lanes and a row
//     of bytes one contiguous run of loads; a lane never holds two adjacent cells, so there is nothing to widen within a lane.
//   * Lanes share nothing but the bytes: the sums behind the scalars are per-lane partial sums (TlLane) that the caller adds up over
//     its lanes -- a DPP reduction on the device (kernels_tile_local.h), a loop in tests/hostsim/sim_tile_local.cpp, which runs the
//     lanes one after the other.  No atomics but the status word's.
//   * The tile counts are a second walk, cell by cell, into sixteen words of two 16-bit counters each -- a lane's share of the largest
//     map a handle exists for is a few thousand cells; whoever adds the lanes up does so in 32 bits where the map has 32 768 cells
//     or more -- and no array indexed by the tile, which would live in scratch.
//   * What is computed follows from what is asked for (TlWant, from the descriptor's pointers: uniform over the launch): a call for
//     the changes alone does no floor scan and reads no offsets.
//   * CHECK: the lane also notes a byte >= 32 (the form without a stage, whose bytes nobody has looked at yet).
//
// Plain functions of (bytes, lane, nlanes): the device and the CPU simulator compile the same text.
#pragma once
#include "pcgrl_common.h"
#include "../../include/pcgrl_hip.h"

struct TlWant {
    bool floor, group, changes, counts;
};
PCGRL_HD TlWant tl_want(const pcgrl_tile_local_desc& D) {
    return {D.floor_dist_out || D.floor_map_out, D.grouping_out || D.group_map_out, D.changes_out != nullptr, D.counts_out != nullptr};
}

// a lane's partial sums over its cells
struct TlLane {
    int floor_dist, grouping, changes_h, changes_v, bad;
};

PCGRL_HD uint32_t tl_bit(unsigned t) { return t < 32 ? 1u << t : 0u; }

// The columns lane, lane + nlanes, ... of one map: floor_map / group_map (NULL: not stored) are the map's own [H, W] outputs.
template <bool CHECK>
PCGRL_HD void tl_lane_cells(const uint8_t* __restrict__ tiles, const pcgrl_tile_local_desc& D, const TlWant want, int W, int H, int lane, int nlanes,
                            int16_t* __restrict__ floor_map, int8_t* __restrict__ group_map, TlLane& a) {
    const int noff = want.group ? D.noffsets : 0;
    for (int x = lane; x < W; x += nlanes) {
        int near = -1;                  // the row of the nearest floor tile at or below, -1: none yet
        unsigned below = 0;
        for (int y = H - 1; y >= 0; y--) {
            const int c = y * W + x;
            const unsigned t = tiles[c];
            const uint32_t bit = tl_bit(t);
            if (CHECK && t >= 32) a.bad = 1;
            if (want.floor) {
                if (D.floor_tiles & bit) near = y;
                const int d = near >= 0 ? near - y - 1 : H - 1;
                if (floor_map) floor_map[c] = (int16_t)d;
                if (D.from_tiles & bit) a.floor_dist += d;
            }
            if (want.changes) {
                if (y + 1 < H && t != below) a.changes_v++;
                if (x > 0 && t != tiles[c - 1]) a.changes_h++;
                below = t;
            }
            if (want.group) {
                const bool own = (D.group_tiles & bit) != 0;
                if (group_map || own) {         // (the scalar alone: only a group tile's own value matters)
                    int v = 0;
                    for (int k = 0; k < noff; k++) {
                        const int nx = x + D.offsets[k][0], ny = y + D.offsets[k][1];
                        if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
                        v += (D.group_tiles & tl_bit(tiles[ny * W + nx])) != 0;
                    }
                    if (group_map) group_map[c] = (int8_t)v;
                    if (own && v >= D.group_min && v <= D.group_max) a.grouping++;
                }
            }
        }
    }
}

// The cells lane, lane + nlanes, ... of one map into p[k] = (cells of tile 2k) | (cells of tile 2k + 1) << 16
template <bool CHECK>
PCGRL_HD void tl_lane_counts(const uint8_t* __restrict__ tiles, int cells, int lane, int nlanes, uint32_t (&p)[16], TlLane& a) {
#pragma unroll
    for (int k = 0; k < 16; k++) p[k] = 0;
    for (int c = lane; c < cells; c += nlanes) {
        const unsigned t = tiles[c];
        const uint32_t bit = tl_bit(t);
        if (CHECK && t >= 32) a.bad = 1;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t two = (bit >> (2 * k)) & 3u;          // 0, 1 (tile 2k) or 2 (tile 2k + 1)
            p[k] += (two | (two << 15)) & 0x10001u;
        }
    }
}
