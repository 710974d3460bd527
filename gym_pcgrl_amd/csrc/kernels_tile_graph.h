// pcgrl_tile_graph: helper.py (helper.py:170-296) for any tile set on the caller's maps (tile_graph.h has the set rule).
// Part of the single translation unit pcgrl_abi.hip.
//   k_tile_graph  k_get_stats' shape (MapLanes, kernels_evaluate.h), with the preamble and the loop written out here: under MapLanes::each
//                 the + dist call on 64 x 64 maps measured 0.5 - 0.8 % slower than this form in two sessions (profiles/readout_frame/NOTES.md).
//                 A lane group per map, grid-stride over `count`; the caller's bytes, as they are (eval_stage_map<false>), -> the LDS
//                 stage -> the pass / source / reach planes in registers,
//                 built from three 32-bit tile sets (the problem's own tiles and planes_from_tiles are not used: tiles 0..31 are legal,
//                 a byte >= 32 is in no set and reported).  The label and distance planes live in registers: no LDS beyond the stage,
//                 no workspace per map.  Every output is optional (NULL: neither computed nor stored; the checks are on kernel
//                 arguments, wave-uniform), every element of a requested one is stored exactly once: the scalars by lane 0, the source by
//                 the lane that owns it, a map's row by the lane that holds it.
#pragma once
#include "tile_graph.h"

// row `lane` of a map's [H, W] i16 output from its NP planes, 32 columns of plane words at a time
template <int NP, class MaskT>
__device__ __forceinline__ void tg_store_row(int16_t* __restrict__ out, const MaskT* p, MaskT valid, int lane, int W, int H) {
    if (lane >= H) return;
    int16_t* row = out + (size_t)lane * W;
#pragma unroll
    for (int half = 0; half < (int)sizeof(MaskT) / 4; half++) {
        uint32_t w[NP];
#pragma unroll
        for (int k = 0; k < NP; k++) w[k] = (uint32_t)(p[k] >> (half * 32));
        const uint32_t v = (uint32_t)(valid >> (half * 32));
        const int n = W - half * 32 < 32 ? W - half * 32 : 32;
#pragma nounroll
        for (int x = 0; x < n; x++) row[half * 32 + x] = (int16_t)tg_cell<NP>(w, v, x);
    }
}

template <int G, class MaskT>
__global__ __launch_bounds__(PCGRL_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_tile_graph(PcgrlParams P, pcgrl_tile_graph_desc D, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // per lane group the tile bytes of its map
    constexpr int GPW = 64 / G, WPB = PCGRL_BLOCK / 64, NP = tg_planes(G, 8 * (int)sizeof(MaskT));
    DevGroup<G, MaskT> g;
    const int lane64 = threadIdx.x & 63, wv = threadIdx.x >> 6, gw = lane64 / G;
    const int W = P.width, H = P.height, cells = W * H, count = D.count;
    uint8_t* tiles = smem + (size_t)(wv * GPW + gw) * reset_tile_bytes(cells);
    const bool want_scalars = D.regions_out || D.longest_out, want_sweep = D.dist_out || D.reach_out;
    // (MapLanes::each's loop and `have` rule)
    for (long long base = ((long long)blockIdx.x * WPB + wv) * GPW; base < count; base += (long long)gridDim.x * WPB * GPW) {
        const long long m = base + gw;
        const bool have = m < count;
        if (have) eval_stage_map<false>(D.maps, m, cells, 32, tiles, g.lane, G, status);      // (a byte no set can name is reported)
        __builtin_amdgcn_wave_barrier();
        MaskT pass = 0, srcs = 0, goal = 0;
        if (have && g.lane < H) {
            const uint8_t* row = tiles + g.lane * W;
#pragma nounroll
            for (int x = 0; x < W; x++) {
                const unsigned t = row[x];
                const uint32_t bit = t < 32 ? 1u << t : 0u;
                pass |= (MaskT)((D.passable & bit) != 0) << x;
                srcs |= (MaskT)((D.source_tiles & bit) != 0) << x;
                goal |= (MaskT)((D.reach_tiles & bit) != 0) << x;
            }
        }
        __builtin_amdgcn_wave_barrier();                                // (the stage is free for the next round)
        if (!have) continue;
        if (want_scalars) {
            int regions, path;
            regions_and_longest_path(g, pass, regions, path);
            if (g.lane == 0) {
                if (D.regions_out) D.regions_out[m] = regions;
                if (D.longest_out) D.longest_out[m] = path;
            }
        }
        if (D.labels_out) {
            MaskT lp[NP];
            tg_labels<NP>(g, pass, lp);
            tg_store_row<NP>(D.labels_out + (size_t)m * cells, lp, pass, g.lane, W, H);
        }
        if (want_sweep || D.source_out) {
            // the source: the caller's cell, or the first cell of source_tiles (_get_certain_tiles(locs, [start_value])[0])
            MaskT src;
            if (D.sources) {
                int c = D.sources[m];
                if (c < -1 || c >= cells) { if (g.lane == 0) atomicOr(status, PCGRL_STATUS_BAD_ACTION); c = -1; }     // outside the map: none, reported
                src = (c >= 0 && g.lane == c / W) ? (MaskT)1 << (c % W) : (MaskT)0;
            } else src = g.first_bit(srcs);
            if (D.source_out) {
                const bool none = !g.any(src);                          // (asked of the whole group: one lane stores)
                if (src != 0) D.source_out[m] = g.lane * W + (sizeof(MaskT) == 4 ? __builtin_ctz((unsigned)src) : __builtin_ctzll((unsigned long long)src));
                else if (g.lane == 0 && none) D.source_out[m] = -1;
            }
            if (want_sweep) {
                MaskT dp[NP], reached;
                tg_dist<NP>(g, src, pass, dp, reached);
                if (D.dist_out) tg_store_row<NP>(D.dist_out + (size_t)m * cells, dp, reached, g.lane, W, H);
                if (D.reach_out) {
                    const int n = g.popcount_sum(goal & reached);
                    if (g.lane == 0) D.reach_out[m] = n;
                }
            }
        }
    }
}
