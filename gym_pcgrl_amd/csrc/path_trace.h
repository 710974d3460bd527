// The paths behind the path-length statistics, as row-bitboard programs over a lane group (pcgrl_algos.h): the cells of binary's
// longest shortest path (helper.py:250-264 calc_longest_path) and of zelda's player -> key, key -> door and player -> nearest enemy
// routes (zelda_prob.py:91-110), which the reference's run_dikjstra maps (helper.py:222-237) define and its get_stats throws away.
//
// The rule, on a run_dikjstra map D from a start cell: the leg to a cell t with D[t] >= 0 is built backwards from t; the predecessor
// of a cell c with D[c] > 0 is the FIRST neighbour n of c in run_dikjstra's own order -- (dx, dy) = (-1,0), (1,0), (0,-1), (0,1):
// left, right, up, down -- with D[n] == D[c] - 1.  "First" among cells is row-major (np.argmax, get_tile_locations): first_bit.
//
// No distance map is kept: neighbouring cells of a BFS differ by at most 1 in distance, so D mod 3 names the predecessor class
// exactly.  A sweep (pt_sweep) leaves (D mod 3) + 1 of every reached cell as a two-bit code in two row masks (00 = not reached); the
// walk-back (pt_walk_back) is mask work on a one-bit `cur`: bit x is column x, so the left neighbour is cur >> 1, the right one
// cur << 1, the one above g.down(cur) (row r receives row r + 1: the bit moves to row r - 1) and the one below g.up(cur).
//
// A template over the same backends as pcgrl_algos.h, plus a `Sink` that receives the cells:
//   sink.put(cur, i)   cell i of the leg is the single bit of `cur` (zero in every lane but the one of its row)
// On the device the lane that owns the bit stores y * W + x (kernels_paths.h); tests/hostsim/sim_paths.cpp has the CPU form.
#pragma once
#include "pcgrl_algos.h"

// BFS from the single cell `src` (a cell of `pass`) through `pass`, one level per round.  STOP: the sweep ends at the first level
// that reaches a cell of `stop` -- found = true, hit = those cells, returns their distance; otherwise (and always without STOP) it
// runs until nothing new is reached -- found = false, hit = the last frontier (src itself at eccentricity 0), returns the eccentricity.
// p0 / p1: bit 0 / bit 1 of (D mod 3) + 1 for every cell reached so far.
template <bool STOP, class B>
PCGRL_D int pt_sweep(B& g, typename B::mask_t src, typename B::mask_t pass, typename B::mask_t stop, typename B::mask_t& p0,
                     typename B::mask_t& p1, typename B::mask_t& hit, bool& found) {
    typedef typename B::mask_t M;
    M reached = src, fresh = src;
    p0 = src; p1 = src ^ src;
    int it = 0, code = 1;
    found = false;
    for (;;) {
        const M n = pcg_neighbours(g, fresh) & pass & ~reached;
        if (!g.any(n)) break;                       // group-uniform, like bfs_dist
        ++it;
        code = code == 3 ? 1 : code + 1;
        if (code & 1) p0 = p0 | n;
        if (code & 2) p1 = p1 | n;
        reached = reached | n;
        fresh = n;
        if (STOP) {
            const M h = n & stop;
            if (g.any(h)) { found = true; fresh = h; break; }
        }
    }
    hit = fresh;
    return it;
}

// The leg that ends on `target` (one bit, D[target] = d in the sweep that left p0 / p1), start -> target: cell d is the target, cell
// k - 1 the first neighbour of cell k -- left, right, up, down -- in the class of distance k - 1.
template <class B, class Sink>
PCGRL_D void pt_walk_back(B& g, typename B::mask_t target, int d, typename B::mask_t p0, typename B::mask_t p1, Sink& sink) {
    typedef typename B::mask_t M;
    const M zero = target ^ target;
    const M c1 = p0 & ~p1, c2 = p1 & ~p0, c3 = p0 & p1;      // D mod 3 == 0, 1, 2
    M cur = target;
    int code = d % 3 + 1;
    for (int k = d;; --k) {
        sink.put(cur, k);
        if (k == 0) break;
        code = code == 1 ? 3 : code - 1;
        const M cls = code == 1 ? c1 : (code == 2 ? c2 : c3);
        const M l = (cur >> 1) & cls, r = (cur << 1) & cls;
        M nx = g.msel_ne(l, zero, l, r);            // (both in the row of cur: left before right)
        if (!g.any(nx)) {
            nx = g.down(cur) & cls;                 // the cell above
            if (!g.any(nx)) nx = g.up(cur) & cls;   // the cell below
        }
        cur = nx;
    }
}

// One leg of zelda: run_dikjstra(src; pass), the first cell of `dst` at the smallest positive distance, the walk-back to it.
// Returns that distance, -1 when no cell of dst is reached (nothing is put then).  src is one cell and not in dst.
template <class B, class Sink>
PCGRL_D int pt_leg(B& g, typename B::mask_t src, typename B::mask_t dst, typename B::mask_t pass, Sink& sink) {
    typedef typename B::mask_t M;
    M p0, p1, hit;
    bool found;
    const int d = pt_sweep<true>(g, src, pass, dst, p0, p1, hit, found);
    if (!found) return -1;
    pt_walk_back(g, g.first_bit(hit), d, p0, p1, sink);
    return d;
}

// binary, the leg "longest" (helper.py:250-264): the regions of `pass` in the order of their first cell; for each the sweep from that
// cell, (mx, my) = the first cell at the largest distance, the second map D2 from there.  The region is the first whose D2.max()
// equals `path` (the reference updates on `>` only: the first region to reach the final value keeps it); the leg runs from (mx, my)
// to the first arg-max of D2.  A region of k cells holds no shortest path beyond k - 1, and a second eccentricity is at most twice
// the first: such regions are passed over without their sweeps.  Returns the length, -1 without a passable cell.
// (`path` is regions_and_longest_path's value for this mask; this is NOT its champion: that function sweeps the largest region first.)
template <class B, class Sink>
PCGRL_D int binary_longest_leg(B& g, typename B::mask_t pass, int path, Sink& sink) {
    typedef typename B::mask_t M;
    M rest = pass;
    if (!g.any(rest)) return -1;
    const PcgFillCtx<B> ctx = pcg_fill_ctx(g, pass);    // components never touch, so the full mask is safe
    while (g.any(rest)) {
        const M seed = g.first_bit(rest);
        const M comp = pcg_component(g, seed, ctx);
        rest = rest & ~comp;
        if (g.popcount_sum(comp) - 1 < path) continue;
        M last;
        const int e1 = bfs_levels(g, seed, comp, last);
        if (2 * e1 < path) continue;
        M p0, p1, hit;
        bool found;
        const int e2 = pt_sweep<false>(g, g.first_bit(last), comp, comp ^ comp, p0, p1, hit, found);
        if (e2 != path) continue;
        pt_walk_back(g, g.first_bit(hit), e2, p0, p1, sink);
        return e2;
    }
    return -1;      // (not reached with the map's own path-length: some region attains it)
}

// zelda, the legs "key", "door", "enemy" (zelda_prob.py:91-110) from the statistics row `s` of the same map (zelda_stats): their
// conditions and passable sets are the reference's.  len[leg] = the leg's length, -1 where it does not exist.  sink.leg(i) is called
// before the cells of leg i.
template <class B, class Sink>
PCGRL_D void zelda_legs(B& g, typename B::mask_t b0, typename B::mask_t b1, typename B::mask_t b2, typename B::mask_t valid,
                        const int32_t* s, Sink& sink, int* len) {
    typedef typename B::mask_t M;
    len[0] = -1; len[1] = -1; len[2] = -1;
    if (!(s[0] == 1 && s[4] == 1)) return;                      // one player, one region (:91)
    const ZeldaMasks<M> z = zelda_masks(b0, b1, b2, valid);
    const M walk = z.empty | z.player | z.key | z.enemy;
    if (s[1] == 1 && s[2] == 1) {                               // :104-110
        sink.leg(0);
        len[0] = pt_leg(g, z.player, z.key, walk, sink);
        sink.leg(1);
        len[1] = pt_leg(g, z.key, z.door, walk | z.door, sink);       // -1: the door is walled off
    }
    if (s[3] > 0) {                                             // :97-103 (the key is not passable here)
        sink.leg(2);
        len[2] = pt_leg(g, z.player, z.enemy, z.empty | z.player | z.enemy, sink);
    }
}
