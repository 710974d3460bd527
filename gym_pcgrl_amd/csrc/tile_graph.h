// helper.py for any tile set, as row-bitboard programs over a lane group (pcgrl_algos.h): the two maps the reference computes and
// throws away -- calc_num_regions' color_map (helper.py:170-207) and run_dikjstra's distance map (helper.py:222-237) -- kept as
// bit-sliced planes in registers.  The scalars beside them (calc_num_regions, calc_longest_path, helper.py:197-207, 250-264) are
// regions_and_longest_path of pcgrl_algos.h, calc_num_reachable_tile (helper.py:288-296) is a popcount over the reached cells.
//
// The set rule.  The reference's helpers take a LIST of passable values and _get_certain_tiles (helper.py:150-154) orders cells by list
// position first and row-major second, so calc_longest_path's double sweep starts elsewhere in a component, and the color_map is
// numbered differently, for [0, 1] than for [1, 0].  Here a passable argument is a SET: every result is the reference's on the level
// in which every passable tile has been renamed to one single value.  A component's first sweep starts at its first cell in row-major
// order and regions are numbered 1, 2, ... by the row-major order of their first cell.  For one passable value that is the reference
// exactly; for several, the region count, the distance map and the reachable count are still exactly the reference's (they do not
// depend on the order), the longest path and the numbering of the labels are the merged-tile ones.
//
// A value of up to NP bits per cell is NP row masks: plane k holds bit k of every cell's value.  A BFS level, or a component, is ORed
// into the planes its number has a bit in; tg_cell reads one cell back.  tg_planes(lanes, bits): the planes that hold every distance
// (at most cells - 1) and every label (at most cells / 2, a checkerboard) of a lanes x bits map.
//
// A template over the same backends as pcgrl_algos.h: the device (kernels_tile_graph.h) and tests/hostsim/sim_tile_graph.cpp.
#pragma once
#include "pcgrl_algos.h"

PCGRL_HD constexpr int tg_planes(int lanes, int bits) {
    int n = 0;
    while ((1 << n) < lanes * bits) n++;
    return n;
}

// cell x of a row whose plane words are p[0..NP): its value, -1 outside `valid`
template <int NP, class W>
PCGRL_HD int tg_cell(const W* p, W valid, int x) {
    if (!((valid >> x) & 1)) return -1;
    int v = 0;
#pragma unroll
    for (int k = 0; k < NP; k++) v |= (int)((p[k] >> x) & 1) << k;
    return v;
}

// run_dikjstra(src; pass): dp[0..NP) = the distance planes, reached = the cells with a distance (dikjstra_map >= 0).  src: one cell or
// none; a source outside `pass` reaches nothing, like the reference's first pop.
template <int NP, class B>
PCGRL_D void tg_dist(B& g, typename B::mask_t src, typename B::mask_t pass, typename B::mask_t* dp, typename B::mask_t& reached) {
    typedef typename B::mask_t M;
    const M zero = pass ^ pass;
#pragma unroll
    for (int k = 0; k < NP; k++) dp[k] = zero;
    M fresh = src & pass;
    reached = fresh;
    int it = 0;
    for (;;) {
        const M n = pcg_neighbours(g, fresh) & pass & ~reached;
        if (!g.any(n)) break;                       // group-uniform, like bfs_dist
        ++it;
#pragma unroll
        for (int k = 0; k < NP; k++) dp[k] = dp[k] | (((it >> k) & 1) ? n : zero);
        reached = reached | n;
        fresh = n;
    }
}

// calc_num_regions' color_map under the set rule: lp[0..NP) = the label planes over `pass` (1 .. regions, in the order of the regions'
// first cells), returns the number of regions.  The regions are taken one at a time from the first cell of what is left; a cell
// without a passable neighbour is its own region and needs no fill.
template <int NP, class B>
PCGRL_D int tg_labels(B& g, typename B::mask_t pass, typename B::mask_t* lp) {
    typedef typename B::mask_t M;
    const M zero = pass ^ pass;
#pragma unroll
    for (int k = 0; k < NP; k++) lp[k] = zero;
    M rest = pass;
    int label = 0;
    if (!g.any(rest)) return 0;
    const M lone = pass & ~pcg_neighbours(g, pass);
    const PcgFillCtx<B> ctx = pcg_fill_ctx(g, pass);    // components never touch, so the full mask is safe
    while (g.any(rest)) {
        const M seed = g.first_bit(rest);
        M comp = seed;
        if (!g.any(seed & lone)) comp = pcg_component(g, seed, ctx);
        rest = rest & ~comp;
        ++label;
#pragma unroll
        for (int k = 0; k < NP; k++) lp[k] = lp[k] | (((label >> k) & 1) ? comp : zero);
    }
    return label;
}
