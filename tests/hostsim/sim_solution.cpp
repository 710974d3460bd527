// The traced sokoban searches of gym_pcgrl_amd/csrc (SokTrace: sokoban_solver.h, sokoban_fast.h) instantiated on the CPU, with the
// walk-back that k_get_moves does (kernels_moves.h): the four agents of _run_game in its order, the moves of the first winner.
// Built by tests/test_solution_host.py:  g++ -O2 -std=c++17 -fPIC -shared -o libsim_solution.so sim_solution.cpp
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../gym_pcgrl_amd/csrc/sokoban_solver.h"
#include "../../gym_pcgrl_amd/csrc/sokoban_fast.h"

extern "C" {

int sim_sokf_maxc() { return SOKF_MAXC; }

// fast = 1: the compact search (sok_search_fast<1> up to 64 bordered cells, <4> beyond; -2 if the level has more than SOKF_MAXC
// crates), fast = 0: the generic one.  moves[max_len] gets the first min(length, max_len) moves and -1 beyond; iters[4]: the pops of
// every agent that ran (no exhausted-BFS shortcut: the counts are the reference's); *winner: -1 = no agent won.
int sim_sokoban_solution(const uint8_t* map, int h, int w, int power, int fast, int max_len, int8_t* moves, int* length, int* winner, int* iters) {
    SokLevel L; SokNode root;
    const int ncr = sok_build_level(map, w, h, L, root);
    if (ncr > SOK_MAXC) return -1;
    if (fast && L.nc > SOKF_MAXC) return -2;
    sok_init_deadlocks(L);
    root.h = (uint16_t)sok_heuristic(L, root.crate);
    std::vector<SokNode> pool(4 * (size_t)power + 4);
    std::vector<uint32_t> heap(4 * (size_t)power + 4);
    int tsize = 1024; while (tsize < 2 * power) tsize <<= 1;
    if (power <= SOK_LDS_POWER) tsize = SOK_LDS_TABLE;
    std::vector<uint64_t> table(tsize);                 // (the generic search uses it as tsize 32-bit slots)
    const int KS[4] = {-1, 2, 1, 0};
    for (int i = 0; i < max_len; i++) moves[i] = -1;
    for (int a = 0; a < 4; a++) iters[a] = 0;
    *length = 0; *winner = -1;
    for (int a = 0; a < 4; a++) {
        memset(table.data(), 0, table.size() * sizeof(uint64_t));
        bool exhausted = false, win;
        int hh = 0, dd = 0, widx = -1;
        const SokTrace tr = {&widx};
        if (fast) {
            SokFastNode* fp = reinterpret_cast<SokFastNode*>(pool.data());
            SokFastNode cache[4];
            if (L.cells <= 64)
                win = sok_search_fast_traced<1>(L, fp, heap.data(), table.data(), tsize - 1, cache, root, KS[a], power, hh, dd, iters[a], exhausted, SokNoHook(), SokKidsSerial(), tr);
            else
                win = sok_search_fast_traced<4>(L, fp, heap.data(), table.data(), tsize - 1, cache, root, KS[a], power, hh, dd, iters[a], exhausted, SokNoHook(), SokKidsSerial(), tr);
            if (win) sokf_walk_back(fp, widx, dd, moves, max_len);
        } else {
            SokNode work;
            win = sok_search(L, pool.data(), heap.data(), reinterpret_cast<uint32_t*>(table.data()), tsize - 1, work, root, KS[a], power, hh, dd, iters[a], exhausted, SokNoHook(), tr);
            if (win) sok_walk_back(pool.data(), widx, dd, moves, max_len);
        }
        if (win) { *length = dd; *winner = a; break; }
    }
    return 0;
}

}  // extern "C"
