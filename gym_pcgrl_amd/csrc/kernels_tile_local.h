// pcgrl_tile_local: the local half of helper.py (helper.py:37-137) for any tile set on the caller's maps -- get_floor_dist,
// get_type_grouping, get_changes, their per-cell maps and the tile counts (tile_local.h has the per-lane algorithm and the choices).
// Part of the single translation unit pcgrl_abi.hip.
//   k_tile_local<G, STAGED>   one launch per call, G lanes per map, grid-stride over `count`; lanes on columns.
//       STAGED   maps of at most 64 x 64: k_tile_graph's frame -- the caller's bytes, as they are (eval_stage_map<false>, which also
//                reports a byte >= 32) -> the lane group's LDS stage; the neighbour reads come out of LDS.  Sixteen lanes a map, four
//                maps a wavefront, for maps of at most 16 columns (a lane per column: wider lane groups would idle), else a wavefront.
//                The lane group follows from the map's width, not from the handle's row-bitboard form: smb's and the other problems'
//                handles take the same kernel for the same shape.
//       else     every other shape (smb's 114 x 14, maps beyond 64 x 64): a wavefront per map on the caller's bytes in global memory.
//                A row is read coalesced across the lanes, neighbours come out of L2; the lanes look for bytes >= 32 themselves.
//   Every output is optional (NULL: neither computed nor stored; the checks are on kernel arguments, wave-uniform: TlWant), every
//   element of a requested one is stored exactly once: the per-cell values by the lane that owns the column, the scalars by lane 0
//   after a reduction of the lanes' partial sums over the lane group (DevGroup::sum).
#pragma once
#include "tile_local.h"

#define TL_STAGE_SIDE 64          /* the staged form: maps of at most this many rows and columns */
#define TL_NARROW 16              /* ... with sixteen lanes a map up to this many columns */
__host__ __device__ constexpr bool tl_staged(int W, int H) { return W <= TL_STAGE_SIDE && H <= TL_STAGE_SIDE; }
__host__ __device__ constexpr int tl_group(int W, int H) { return tl_staged(W, H) && W <= TL_NARROW ? 16 : 64; }

template <int G, bool STAGED>
__global__ __launch_bounds__(PCGRL_BLOCK) void k_tile_local(int W, int H, pcgrl_tile_local_desc D, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // STAGED: per lane group the tile bytes of its map
    constexpr int GPW = 64 / G, WPB = PCGRL_BLOCK / 64;
    DevGroup<G, uint32_t> g;
    const int lane64 = threadIdx.x & 63, wv = threadIdx.x >> 6, gw = lane64 / G;
    const int cells = W * H, count = D.count;
    const TlWant want = tl_want(D);
    uint8_t* stage = smem + (size_t)(wv * GPW + gw) * reset_tile_bytes(cells);
    // (MapLanes::each's loop and `have` rule: the groups of a wavefront go round together)
    for (long long base = ((long long)blockIdx.x * WPB + wv) * GPW; base < count; base += (long long)gridDim.x * WPB * GPW) {
        const long long m = base + gw;
        const bool have = m < count;
        const uint8_t* tiles = D.maps + (size_t)(have ? m : 0) * cells;
        if (STAGED) {
            if (have) eval_stage_map<false>(D.maps, m, cells, 32, stage, g.lane, G, status);
            __builtin_amdgcn_wave_barrier();
            tiles = stage;
        }
        TlLane a = {0, 0, 0, 0, 0};
        uint32_t packed[16];
        if (have) {
            if (want.floor || want.group || want.changes)
                tl_lane_cells<!STAGED>(tiles, D, want, W, H, g.lane, G, D.floor_map_out ? D.floor_map_out + (size_t)m * cells : nullptr,
                                       D.group_map_out ? D.group_map_out + (size_t)m * cells : nullptr, a);
            if (want.counts) tl_lane_counts<!STAGED>(tiles, cells, g.lane, G, packed, a);
        }
        if (STAGED) __builtin_amdgcn_wave_barrier();                    // (the stage is free for the next round)
        if (!have) continue;
        if (!STAGED && a.bad) atomicOr(status, PCGRL_STATUS_BAD_TILE);
        if (want.floor && D.floor_dist_out) {
            const int v = g.sum(a.floor_dist);
            if (g.lane == 0) D.floor_dist_out[m] = v;
        }
        if (want.group && D.grouping_out) {
            const int v = g.sum(a.grouping);
            if (g.lane == 0) D.grouping_out[m] = v;
        }
        if (want.changes) {
            const int hz = g.sum(a.changes_h), vt = g.sum(a.changes_v);
            if (g.lane == 0) { D.changes_out[2 * m] = hz; D.changes_out[2 * m + 1] = vt; }
        }
        if (want.counts) {
            int32_t* row = D.counts_out + (size_t)m * 32;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                int even, odd;
                if (cells < 32768) {                                    // two sums in one reduction where both fit sixteen bits and the word stays a positive int
                    const int v = g.sum((int)packed[k]);
                    even = v & 0xFFFF; odd = v >> 16;
                } else { even = g.sum((int)(packed[k] & 0xFFFFu)); odd = g.sum((int)(packed[k] >> 16)); }
                if (g.lane == 0) { row[2 * k] = even; row[2 * k + 1] = odd; }
            }
        }
    }
}
