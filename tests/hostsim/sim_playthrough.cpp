// The traced MiniDungeons and Dangerous Dave searches of gym_pcgrl_amd/csrc (PlayTrace: mdungeon_solver.h, mdungeon_fast.h,
// ddave_solver.h, ddave_fast.h) instantiated on the CPU, with the walk-back that k_get_moves does (kernels_moves.h): the
// four agents of _run_game in its order, the moves of the first winner or -- when nobody wins -- those to the BFS agent's best node.
// Built by tests/test_playthrough_host.py:  g++ -O2 -std=c++17 -fPIC -shared -o libsim_playthrough.so sim_playthrough.cpp
// and, with -DSIM_PLAYTHROUGH_MAIN -fsanitize=address,undefined, as a stand-alone program that runs a few built-in levels through
// every traced search and walk-back.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gym_pcgrl_amd/csrc/sokoban_solver.h"
#include "../../gym_pcgrl_amd/csrc/sokoban_fast.h"
#include "../../gym_pcgrl_amd/csrc/mdungeon_solver.h"
#include "../../gym_pcgrl_amd/csrc/mdungeon_fast.h"
#include "../../gym_pcgrl_amd/csrc/ddave_solver.h"
#include "../../gym_pcgrl_amd/csrc/ddave_fast.h"

extern "C" {

int sim_mdf_maxi() { return MDF_MAXI; }
int sim_ddf_maxd() { return DDF_MAXD; }
// things on the floor (mdungeon) / diamonds (ddave): what decides between the compact and the generic search
int sim_play_things(int prob, const uint8_t* map, int h, int w) {
    if (prob == 0) { MdLevel L; MdNode root; MdFastLevel F; md_build_level(map, w, h, L, root); return mdf_level(L, root, F); }
    DdLevel L; DdNode root; DdFastLevel F; dd_build_level(map, w, h, L, root); return ddf_level(L, F);
}

// prob 0 = mdungeon, 1 = ddave.  fast = 1: the compact search (-2 if the level has more than MDF_MAXI things / DDF_MAXD diamonds),
// fast = 0: the generic one.  moves[max_len] gets the first min(length, max_len) moves and -1 beyond; *length: the depth of the node
// the game's result comes from; iters[4]: the pops of every agent that ran (no exhausted-agent shortcut: the counts are the
// reference's); *winner: -1 = no agent won; res[5]: mdungeon dist-win, sol-length, col-potions, col-treasures, col-enemies; ddave
// dist-win, sol-length, num-jumps, col-diamonds.
int sim_playthrough(int prob, const uint8_t* map, int h, int w, int power, int fast, int max_len, int8_t* moves, int* length, int* winner, int* iters,
                    int* res) {
    if ((w + 2) * (h + 2) > 256 || power > SOK_LDS_POWER) return -1;
    MdLevel ML; MdNode mroot, mwork; MdFastLevel MF;
    DdLevel DL; DdNode droot, dwork; DdFastLevel DF;
    int things;
    if (prob == 0) { md_build_level(map, w, h, ML, mroot); things = mdf_level(ML, mroot, MF); }
    else { dd_build_level(map, w, h, DL, droot); things = ddf_level(DL, DF); }
    if (fast && things > (prob == 0 ? MDF_MAXI : DDF_MAXD)) return -2;
    const size_t nodes = 4 * (size_t)power + 4;
    std::vector<MdNode> pool(nodes);                    // (a DdNode is as large; the compact searches use it as 16-byte nodes)
    std::vector<uint32_t> heap(nodes), trace(nodes);
    const int tsize = SOK_LDS_TABLE;
    std::vector<uint64_t> table(tsize);                 // (the generic search uses it as tsize 32-bit slots)
    const int KS[4] = {2, 1, 0, -1};
    for (int i = 0; i < max_len; i++) moves[i] = -1;
    for (int a = 0; a < 4; a++) iters[a] = 0;
    for (int i = 0; i < 5; i++) res[i] = 0;
    *length = 0; *winner = -1;
    for (int a = 0; a < 4; a++) {
        memset(table.data(), 0, table.size() * sizeof(uint64_t));
        memset(trace.data(), 0xEE, trace.size() * 4);   // (a word the agent did not write cannot pass for one it wrote)
        bool exhausted = false, win;
        int node = -1, depth = 0;
        const PlayTrace tr = {trace.data(), &node};
        const bool in_node = prob == 0 && fast;         // the compact mdungeon search keeps its trace word in the node
        if (prob == 0) {
            if (fast) {
                MdFastNode cache[4];
                uint64_t key = 0; int hh = 0, dd = 0;
                const PlayTraceInNode trn = {&node};
                win = md_search_fast_traced(ML, MF, reinterpret_cast<MdFastNode*>(pool.data()), heap.data(), table.data(), tsize - 1, cache, mroot, KS[a], power,
                                            key, hh, dd, iters[a], exhausted, SokNoHook(), MdKidsSerial(), trn);
                mdf_result(MF, key, hh, dd, win, res);
                depth = dd;
            } else {
                win = md_search(ML, pool.data(), heap.data(), reinterpret_cast<uint32_t*>(table.data()), tsize - 1, mwork, mroot, KS[a], power, iters[a], exhausted,
                                SokNoHook(), tr);
                md_result(ML, mroot, mwork, win, res);
                depth = mwork.depth;
            }
        } else {
            if (fast) {
                DdFastNode cache[4];
                uint64_t key = 0; int hh = 0, dd = 0, jj = 0;
                win = dd_search_fast_traced(DL, DF, reinterpret_cast<DdFastNode*>(pool.data()), heap.data(), table.data(), tsize - 1, cache, droot, KS[a], power,
                                            key, hh, dd, jj, iters[a], exhausted, SokNoHook(), DdKidsSerial(), tr);
                ddf_result(DF, key, hh, dd, jj, win, res);
                depth = dd;
            } else {
                win = dd_search(DL, reinterpret_cast<DdNode*>(pool.data()), heap.data(), reinterpret_cast<uint32_t*>(table.data()), tsize - 1, dwork, droot, KS[a],
                                power, iters[a], exhausted, SokNoHook(), tr);
                dd_result(DL, dwork, win, res);
                depth = dwork.depth;
            }
        }
        if (win || a == 3) {
            *length = depth; *winner = win ? a : -1;
            if (in_node) mdf_walk_back(reinterpret_cast<const MdFastNode*>(pool.data()), (int)nodes, node, depth, moves, max_len);
            else play_walk_back(trace.data(), (int)nodes, node, depth, moves, max_len);
            break;
        }
    }
    return 0;
}

}  // extern "C"

#ifdef SIM_PLAYTHROUGH_MAIN
// A handful of built-in levels through every traced search and walk-back, for a sanitizer build.  Prints one line per run; exit
// status 0 when the compact and the generic search agree on every level and every truncated row is a prefix of the full one.
static int run_level(int prob, const uint8_t* m, int h, int w, int power) {
    int8_t full[2][64 + 2];
    int len[2], win[2], it[2][4], res[2][5];
    for (int fast = 0; fast < 2; fast++) {
        memset(full[fast], 77, sizeof(full[fast]));
        if (sim_playthrough(prob, m, h, w, power, fast, 64, full[fast], &len[fast], &win[fast], it[fast], res[fast]) != 0) return 1;
        if (full[fast][64] != 77 || full[fast][65] != 77) return 2;
        printf("prob %d %dx%d power %d fast %d: winner %d length %d pops %d %d %d %d\n", prob, h, w, power, fast, win[fast], len[fast], it[fast][0], it[fast][1],
               it[fast][2], it[fast][3]);
    }
    if (len[0] != len[1] || win[0] != win[1] || memcmp(full[0], full[1], 64) != 0 || memcmp(it[0], it[1], sizeof(it[0])) != 0 ||
        memcmp(res[0], res[1], sizeof(res[0])) != 0) return 3;
    const int lens[3] = {1, 4, len[0] > 0 ? len[0] : 1};
    for (int q = 0; q < 3; q++)
        for (int fast = 0; fast < 2; fast++) {
            std::vector<int8_t> row((size_t)lens[q] + 2, 77);
            int l, wn, its[4], rs[5];
            if (sim_playthrough(prob, m, h, w, power, fast, lens[q], row.data(), &l, &wn, its, rs) != 0) return 4;
            if (l != len[0] || row[lens[q]] != 77 || row[lens[q] + 1] != 77 || memcmp(row.data(), full[0], lens[q] < 64 ? lens[q] : 64) != 0) return 5;
        }
    return 0;
}
int main() {
    // mdungeon tiles: 0 empty 1 solid 2 player 3 exit 4 potion 5 treasure 6 goblin 7 ogre
    static const uint8_t md_a[1 * 6] = {2, 0, 5, 6, 0, 3};
    static const uint8_t md_b[5 * 5] = {2, 0, 0, 5, 0,  0, 1, 1, 6, 0,  4, 0, 7, 0, 0,  0, 1, 1, 1, 0,  5, 0, 6, 0, 3};
    static const uint8_t md_c[3 * 4] = {2, 7, 7, 3,  1, 1, 1, 1,  0, 5, 0, 0};           // three ogres' worth of health is not there: nobody wins
    // ddave tiles: 0 empty 1 solid 2 player 3 exit 4 diamond 5 key 6 spike
    static const uint8_t dd_a[1 * 5] = {2, 0, 5, 4, 3};
    static const uint8_t dd_b[5 * 5] = {0, 0, 4, 0, 3,  0, 0, 1, 1, 1,  2, 0, 0, 4, 5,  1, 1, 0, 1, 1,  0, 0, 0, 6, 0};
    static const uint8_t dd_c[2 * 6] = {2, 0, 4, 0, 6, 3,  1, 1, 1, 1, 1, 1};            // no key: nobody wins
    int rc = 0;
    rc |= run_level(0, md_a, 1, 6, 5000);
    rc |= run_level(0, md_b, 5, 5, 5000);
    rc |= run_level(0, md_b, 5, 5, 7);
    rc |= run_level(0, md_c, 3, 4, 300);
    rc |= run_level(1, dd_a, 1, 5, 5000);
    rc |= run_level(1, dd_b, 5, 5, 5000);
    rc |= run_level(1, dd_b, 5, 5, 9);
    rc |= run_level(1, dd_c, 2, 6, 300);
    printf(rc ? "FAILED %d\n" : "ok\n", rc);
    return rc ? 1 : 0;
}
#endif
