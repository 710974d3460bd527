// k_mdungeon / k_ddave: the planner jobs that k_stats / k_reset parked for the mdungeon and ddave problems (mdungeon_solver.h,
// ddave_solver.h), one wavefront per search.  One body for both, written against SearchGame<PROB> (search_game.h).  Part of the
// single translation unit pcgrl_abi.hip.
//
// _run_game (mdungeon_prob.py:110-126, ddave_prob.py:111-127) runs A*(1), A*(0.5), A*(0) and BFS one after the other and stops
// at the first winner.  The agents are independent searches from the same root, so only the *selection* is
// sequential: here the four agents of a level are four tickets (handed out with an atomic counter on a word the host
// zeroes before the launch) and run concurrently in different workgroups.  Every agent records (win, h, depth, what
// was collected / jumped); the last of the four to finish selects exactly what the sequential loop would have returned -- the
// first winner in agent order, else the BFS agent's best node -- and finishes the environment's step.  An agent whose
// result cannot be selected any more is abandoned at its next poll (SearchGame::stopped):
//   * an earlier agent has won (level 3 - a in the low byte of the environment's stop word), or
//   * mdungeon only: some A* agent ran out of states without a win (bit 8): then no agent can win or reach the cap (the exact
//     shortcut of md_run_game) and only the BFS agent's best node matters, so the other A* agents stop.  (A ddave agent that
//     exhausts says nothing about the others: ddave_solver.h.)
// Nobody waits for anybody: a level with one player, one exit and one region (mdungeon_prob.py:152) is usually won by
// A*(1) within a few dozen pops, and the other three agents then stop at their first poll.
#pragma once

// Agent a of environment e is done.  The fourth report selects the result and finishes the item.
template <int PROB>
__device__ __forceinline__ void agents4_report(const PcgrlParams& P, const DevBufs& B, int e, int a, bool win, bool exhausted, const int* res,
                                               int mode, int parity, int rst_list) {
    typedef SearchGame<PROB> G;
    int32_t* r = B.sok_res + ((size_t)e * 4 + a) * 4;
    __hip_atomic_store(r + 0, win ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(r + 1, res[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(r + 2, res[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(r + 3, G::encode(res), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    G::stop_update(B.sok_stop + e, a, win, exhausted);
    __threadfence();
    if (atomicAdd(B.sok_cnt + e, 1) != 3) return;
    __threadfence();
    int chosen = 3;
    for (int k = 2; k >= 0; k--) if (sok_ld(B.sok_res + ((size_t)e * 4 + k) * 4)) chosen = k;
    const int32_t* q = B.sok_res + ((size_t)e * 4 + chosen) * 4;
    int sel[G::NRES] = {sok_ld(q + 1), sok_ld(q + 2)};
    G::decode(sok_ld(q + 3), sel);
    B.sok_cnt[e] = 0;      // ready for the next job of this environment (a later launch)
    B.sok_stop[e] = 0;
    finish_search_item<PROB>(P, B, e, sel, mode, parity, true, rst_list);
}

// Jobs = list_a (mode_a) followed by list_b (mode_b); list_b < 0: none.  Environments that finish their episode here
// go to `rst_list`.  only_agent >= 0: just that agent runs (mdungeon's md_only_agent switch).
// Two wavefronts per block: the search wavefront (everything below) and the heap server of its A* searches (sokoban_fast.h).
template <int PROB>
__device__ __forceinline__ void agents4_body(const PcgrlParams& P, const DevBufs& B, int list_a, int mode_a, int list_b, int mode_b, int parity,
                                             int rst_list, int32_t* sync, int clear_parity, int only_agent) {
    typedef SearchGame<PROB> G;
    extern __shared__ __attribute__((aligned(16))) uint32_t a4_lds[];
    __shared__ int s_pref_a[WL_NSHARD + 1], s_pref_b[WL_NSHARD + 1];
    __shared__ typename G::Shared s_game;            // level + node workspace in LDS: they are indexed dynamically
    __shared__ SokDuoBox s_box;
    if (clear_parity >= 0 && blockIdx.x == 0) wl_clear(B, clear_parity);
    const int lane = threadIdx.x & 63;
    const int n_a = wl_load_prefix(B, parity, list_a, s_pref_a);
    const int n_b = list_b >= 0 ? wl_load_prefix(B, parity, list_b, s_pref_b) : 0;
    const int n = n_a + n_b;
    if (threadIdx.x >= 64) { sok_duo_server(a4_lds, &s_box, lane); return; }
    SokDuoBox* const duo = B.sok_use_lds ? &s_box : nullptr;       // (the heap has to be the LDS one)
    void* pool = B.sok_pool + (size_t)blockIdx.x * B.sok_pool_stride;
    uint32_t* g_heap = B.sok_use_lds ? nullptr : B.sok_heap + (size_t)blockIdx.x * B.sok_heap_stride;
    uint32_t* g_table = B.sok_use_lds ? nullptr : B.sok_table + (size_t)blockIdx.x * B.sok_table_size;
    const int tsize = B.sok_use_lds ? SOK_LDS_TABLE : B.sok_table_size;
    for (;;) {
        int t = 0;
        if (lane == 0) t = atomicAdd(sync + SOK_SY_TICKET_A, 1);
        t = __shfl(t, 0, 64);
        if (t >= 4 * n) break;
        const int job = t >> 2, a = t & 3;
        int e, mode;
        if (job < n_a) { e = wl_get(B, list_a, s_pref_a, job); mode = mode_a; }
        else { e = wl_get(B, list_b, s_pref_b, job - n_a); mode = mode_b; }
        const SearchPollHook<PROB> hook = {B.sok_stop + e, a};
        int skip = 0;
        if (lane == 0) skip = (hook(0) || (only_agent >= 0 && only_agent != a)) ? 1 : 0;   // already decided before this agent started
        skip = __shfl(skip, 0, 64);
        if (!skip) G::build(P, B, B.map + (size_t)e * P.width * P.height, s_game, lane);
        __threadfence_block();
        const int fast = skip ? 0 : s_game.fast;
        if (!skip) search_clear_table(B, a4_lds, g_table, tsize, fast, lane);
        __threadfence_block();
        // the compact search runs on lanes 0..3 (uniform except for the four children of a pop), the generic one on lane 0
        if (lane < (fast ? 4 : 1)) {
            int it = 0, res[G::NRES] = {};
            bool exhausted = false, win = false;
            if (!skip) win = search_agent<PROB>(B, s_game, a, pool, a4_lds, g_heap, g_table, tsize, fast, P.solver_power, lane, res, it, exhausted, hook, duo);
            if (lane == 0) agents4_report<PROB>(P, B, e, a, win, exhausted, res, mode, parity, rst_list);
        }
        __threadfence_block();
    }
    s_box.session = 0;          // the heap server leaves with us
    sok_duo_sync();
}

// (templates only so that every part of the library can include this header: instantiated where they are launched)
template <int PART_TAG>
__global__ __launch_bounds__(128) void k_mdungeon(PcgrlParams P, DevBufs B, int list_a, int mode_a, int list_b, int mode_b, int parity,
                                                 int rst_list, int32_t* sync, int clear_parity) {
    agents4_body<PCGRL_PROB_MDUNGEON>(P, B, list_a, mode_a, list_b, mode_b, parity, rst_list, sync, clear_parity, B.md_only_agent);
}
template <int PART_TAG>
__global__ __launch_bounds__(128) void k_ddave(PcgrlParams P, DevBufs B, int list_a, int mode_a, int list_b, int mode_b, int parity,
                                              int rst_list, int32_t* sync, int clear_parity) {
    agents4_body<PCGRL_PROB_DDAVE>(P, B, list_a, mode_a, list_b, mode_b, parity, rst_list, sync, clear_parity, -1);
}
