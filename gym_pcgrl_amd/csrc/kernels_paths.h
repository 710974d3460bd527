// pcgrl_get_paths: the cells of the paths behind binary's `path-length` and zelda's `path-length` / `nearest-enemy` (path_trace.h).
// Part of the single translation unit pcgrl_abi.hip.
//   k_get_paths   k_get_stats' frame (MapLanes, kernels_evaluate.h): a lane group per map, grid-stride over `count`; the caller's bytes
//                 -> the LDS stage -> row planes in registers -> compute_item_stats for the row -> the legs.  The distance classes of a sweep and the walk-back live in registers:
//                 no LDS beyond the stage, no workspace per map.  Every element of a map's [legs, max_len] cells is stored exactly
//                 once: the cells by the lane that owns each, then -1 from the end of the leg to the end of the row.
#pragma once

#define PATHS_MAX_LEGS 3
__host__ __device__ constexpr int paths_legs(int prob) { return prob == PCGRL_PROB_BINARY ? 1 : (prob == PCGRL_PROB_ZELDA ? PATHS_MAX_LEGS : 0); }

// path_trace.h's Sink on the device: `row` is the leg's row of cells_out, `lane` the map row this lane holds
template <class MaskT>
struct DevPathSink {
    int16_t* base;
    int16_t* row;
    int max_len, W, lane;
    __device__ __forceinline__ void leg(int l) { row = base + (size_t)l * max_len; }
    __device__ __forceinline__ void put(MaskT cur, int i) const {
        if (cur != 0 && i < max_len) row[i] = (int16_t)(lane * W + (sizeof(MaskT) == 4 ? __builtin_ctz((unsigned)cur) : __builtin_ctzll((unsigned long long)cur)));
    }
};

template <int PROB, int G, class MaskT>
__global__ __launch_bounds__(PCGRL_BLOCK) void k_get_paths(PcgrlParams P, const uint8_t* __restrict__ maps, int count, int max_len, int16_t* __restrict__ cells_out,
                                                            int32_t* __restrict__ length_out, int32_t* __restrict__ rows_out, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // per lane group the tile bytes of its map
    constexpr int LEGS = paths_legs(PROB);
    const MapLanes<G, MaskT> L(smem, P.width * P.height);
    const auto& g = L.g;
    const int W = P.width;
    const MaskT rowmask = row_valid<MaskT>(g.lane, W, P.height);
    L.each(count, [&](long long m, bool have) {
        MaskT b0, b1, b2;
        L.planes(P, maps, m, have, b0, b1, b2, status);
        if (!have) return;
        int32_t s[PCGRL_MAX_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
        compute_item_stats<PROB>(g, P, b0, b1, b2, rowmask, s, status);
        if (g.lane == 0 && rows_out) store_stats_row<PROB>(rows_out + (size_t)m * 8, s);
        DevPathSink<MaskT> sink = {cells_out + (size_t)m * LEGS * max_len, nullptr, max_len, W, g.lane};
        sink.leg(0);
        int len[PATHS_MAX_LEGS] = {-1, -1, -1};
        if (PROB == PCGRL_PROB_BINARY) len[0] = binary_longest_leg(g, (MaskT)(~b0 & rowmask), s[1], sink);
        else zelda_legs(g, b0, b1, b2, rowmask, s, sink, len);
#pragma unroll
        for (int l = 0; l < LEGS; l++) {
            sink.leg(l);
            const int n = len[l] < 0 ? 0 : (len[l] + 1 < max_len ? len[l] + 1 : max_len);
            for (int i = n + g.lane; i < max_len; i += G) sink.row[i] = (int16_t)-1;
            if (g.lane == 0) length_out[(size_t)m * LEGS + l] = len[l];
        }
    });
}
