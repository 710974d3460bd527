// pcgrl_get_solution / pcgrl_get_playthrough: the moves behind the planner's statistics.  Part of the single translation unit
// pcgrl_abi.hip.
//   sokoban            SokobanProblem.get_stats(map)["solution"] (sokoban_prob.py:133-145): the moves of the first agent of _run_game
//                      (:104-122) that wins, Node.getActions (engine.py:38-44).  Nobody wins: nothing is written.
//   mdungeon / ddave   _run_game (mdungeon_prob.py:100-138, ddave_prob.py:92-127) asks its agents for node.getActions()
//                      (mdungeon/engine.py:43-49) and keeps only len(sol) and the game status of the returned state; this kernel keeps
//                      the moves: the first winner's, or -- when nobody wins -- those that lead to the BFS agent's best node, the state
//                      the statistics row is taken from.
// The job list is the one k_get_stats<PROB> makes (kernels_evaluate.h); k_get_moves is k_get_stats_search with the traced searches
// (SokTrace, sokoban_solver.h; PlayTrace, mdungeon_solver.h): a chunk ticket, eight wavefronts try the jobs in the small regions,
// wavefront 0 redoes what the small limit stopped in the full region with the full solver_power.  Sokoban's searches record parent and
// move in free bits of their nodes, and so does the compact mdungeon search (MdFastNode's free `pad`).  For the three searches whose
// nodes have no room every block has, beside its node pool, as many trace words (parent | move << 30), cut from the caller's workspace
// and indexed like the pool; sokoban is launched without them.  Right after the agent that ends a game returns, while that
// wavefront's pool and trace words still hold the search, one lane walks the parent chain from the returned node and writes the row.
// Only a run whose result is accepted writes: a try that was "not final" leaves row, length and agent as they are.
// The rows are filled with -1, the lengths with 0 and the agents with -2 before the launch (moves_call / get_moves, pcgrl_abi.hip): a level whose
// planner does not run is never seen here.
// The trace store is one global store per filed child that nothing waits for before the walk (the __threadfence() in front of it):
// it is not on the search's chain of dependent pops.
// moves_game_run and k_get_moves repeat search_game_run (search_game.h) and k_get_stats_search (kernels_evaluate.h) on purpose: one
// body with an agent / finish policy for the untraced side as well was tried and changed the machine code of k_step_solver and
// k_get_stats_search (the compiler schedules the inlined loop differently), and those kernels have to stay what they are.  So the
// loop exists twice, there and here: a change to the ticket, the small tries or the redo there has to be made here as well.  The
// traced searches are instantiated in this kernel only.
#pragma once

struct SolOut { int8_t* moves; int32_t* length; int8_t* agent; int max_len; };

// The traced agents of SearchGame<PROB> (search_game.h agent_fast / agent_generic): res[] as there; `node`: the returned node's index
// in the pool and the trace words, `depth`: the number of moves that lead to it.  walks_without_winner: whether the agent that ends a
// game without winning has a node to walk back from (the BFS agent's best node) -- sokoban's searches return one only when they win.
template <int PROB>
struct TracedAgents;

template <>
struct TracedAgents<PCGRL_PROB_SOKOBAN> {
    typedef SearchGame<PCGRL_PROB_SOKOBAN> G;
    static constexpr bool walks_without_winner = false;
    // (the trace is in the nodes: `trace` is not used.  The compact search has no `duo` parameter: a traced search is the
    //  one-wavefront loop.)
    static __device__ __forceinline__ bool fast(G::Shared& S, int a, void* pool, uint32_t*, uint32_t* lds, int toff, int tsize, int power, int lane, int* res,
                                                int& it, bool& exhausted, int& node, int& depth) {
        const SokKidsLanes kids = {lane, sokf_dir(lane & 3, S.L.w)};
        uint64_t* tab = reinterpret_cast<uint64_t*>(lds + toff);
        SokFastNode* fp = reinterpret_cast<SokFastNode*>(pool);
        const SokTrace tr = {&node};
        int hh = 0, dd = 0;
        bool w;
        if (S.L.cells <= 64) w = sok_search_fast_traced<1>(S.L, fp, lds, tab, tsize - 1, S.cache, S.root, G::ks(a), power, hh, dd, it, exhausted, SokNoHook(), kids, tr);
        else w = sok_search_fast_traced<4>(S.L, fp, lds, tab, tsize - 1, S.cache, S.root, G::ks(a), power, hh, dd, it, exhausted, SokNoHook(), kids, tr);
        res[0] = w ? 0 : hh; res[1] = w ? dd : 0;
        depth = res[1];
        return w;
    }
    template <class HP, class TP>
    static __device__ __forceinline__ bool generic(G::Shared& S, int a, void* pool, uint32_t*, HP heap, TP table, int tsize, int power, int* res, int& it,
                                                   bool& exhausted, int& node, int& depth) {
        const SokTrace tr = {&node};
        int hh = 0, dd = 0;
        const bool w = sok_search(S.L, reinterpret_cast<SokNode*>(pool), heap, table, tsize - 1, S.work, S.root, G::ks(a), power, hh, dd, it, exhausted, SokNoHook(), tr);
        res[0] = w ? 0 : hh; res[1] = w ? dd : 0;
        depth = res[1];
        return w;
    }
    static __device__ __forceinline__ void walk(int fast, const void* pool, const uint32_t*, int, int node, int depth, int8_t* row, int max_len) {
        if (fast) sokf_walk_back(reinterpret_cast<const SokFastNode*>(pool), node, depth, row, max_len);
        else sok_walk_back(reinterpret_cast<const SokNode*>(pool), node, depth, row, max_len);
    }
};

template <>
struct TracedAgents<PCGRL_PROB_MDUNGEON> {
    typedef SearchGame<PCGRL_PROB_MDUNGEON> G;
    static constexpr bool walks_without_winner = true;
    static __device__ __forceinline__ bool fast(G::Shared& S, int a, void* pool, uint32_t* trace, uint32_t* lds, int toff, int tsize, int power, int lane,
                                                int* res, int& it, bool& exhausted, int& node, int& depth) {
        const MdKidsLanes kids = {lane};
        const PlayTraceInNode tr = {&node};           // (the trace word is in the node's `pad`: `trace` is not used)
        uint64_t key = 0;
        int hh = 0, dd = 0;
        const bool w = md_search_fast_traced(S.L, S.F, reinterpret_cast<MdFastNode*>(pool), lds, reinterpret_cast<uint64_t*>(lds + toff), tsize - 1, S.cache,
                                             S.root, G::ks(a), power, key, hh, dd, it, exhausted, SokNoHook(), kids, tr);
        mdf_result(S.F, key, hh, dd, w, res);
        depth = dd;
        return w;
    }
    template <class HP, class TP>
    static __device__ __forceinline__ bool generic(G::Shared& S, int a, void* pool, uint32_t* trace, HP heap, TP table, int tsize, int power, int* res, int& it,
                                                   bool& exhausted, int& node, int& depth) {
        const PlayTrace tr = {trace, &node};
        const bool w = md_search(S.L, reinterpret_cast<MdNode*>(pool), heap, table, tsize - 1, S.work, S.root, G::ks(a), power, it, exhausted, SokNoHook(), tr);
        md_result(S.L, S.root, S.work, w, res);
        depth = S.work.depth;
        return w;
    }
    static __device__ __forceinline__ void walk(int fast, const void* pool, const uint32_t* trace, int cap, int node, int depth, int8_t* row, int max_len) {
        if (fast) mdf_walk_back(reinterpret_cast<const MdFastNode*>(pool), cap, node, depth, row, max_len);
        else play_walk_back(trace, cap, node, depth, row, max_len);
    }
};

template <>
struct TracedAgents<PCGRL_PROB_DDAVE> {
    typedef SearchGame<PCGRL_PROB_DDAVE> G;
    static constexpr bool walks_without_winner = true;
    static __device__ __forceinline__ bool fast(G::Shared& S, int a, void* pool, uint32_t* trace, uint32_t* lds, int toff, int tsize, int power, int lane,
                                                int* res, int& it, bool& exhausted, int& node, int& depth) {
        const DdKidsLanes kids = {lane};
        const PlayTrace tr = {trace, &node};
        uint64_t key = 0;
        int hh = 0, dd = 0, jj = 0;
        const bool w = dd_search_fast_traced(S.L, S.F, reinterpret_cast<DdFastNode*>(pool), lds, reinterpret_cast<uint64_t*>(lds + toff), tsize - 1, S.cache,
                                             S.root, G::ks(a), power, key, hh, dd, jj, it, exhausted, SokNoHook(), kids, tr);
        ddf_result(S.F, key, hh, dd, jj, w, res);
        depth = dd;
        return w;
    }
    template <class HP, class TP>
    static __device__ __forceinline__ bool generic(G::Shared& S, int a, void* pool, uint32_t* trace, HP heap, TP table, int tsize, int power, int* res, int& it,
                                                   bool& exhausted, int& node, int& depth) {
        const PlayTrace tr = {trace, &node};
        const bool w = dd_search(S.L, reinterpret_cast<DdNode*>(pool), heap, table, tsize - 1, S.work, S.root, G::ks(a), power, it, exhausted, SokNoHook(), tr);
        dd_result(S.L, S.work, w, res);
        depth = S.work.depth;
        return w;
    }
    static __device__ __forceinline__ void walk(int, const void*, const uint32_t* trace, int cap, int node, int depth, int8_t* row, int max_len) {
        play_walk_back(trace, cap, node, depth, row, max_len);
    }
};

// search_game_run (search_game.h) with traced agents.  res[] as there; `winner` (lane 0): the agent that won, -1 = none; `length`
// (lane 0): the depth of the node whose moves were written, 0 when none were.  The moves are in the level's row of `out` when this
// returns "final".  `trace`: `trace_cap` words beside `pool`.
template <int PROB>
__device__ __forceinline__ bool moves_game_run(const PcgrlParams& P, const DevBufs& B, typename SearchGame<PROB>::Shared& S, uint32_t* heap, int table_off,
                                               int tsize, int power, void* pool, uint32_t* trace, int trace_cap, int lane, int* res, int& winner, int& length,
                                               const SolOut& out, int m) {
    typedef SearchGame<PROB> G;
    typedef TracedAgents<PROB> A;
    G::build(P, B, B.map, S, lane);
    __threadfence_block();
    const int fast = S.fast;
    int final = 1;
    winner = -1;
    length = 0;
    for (int a = 0; a < 4;) {
        for (int i = lane; i < (fast ? 2 : 1) * tsize; i += 64) heap[table_off + i] = 0;      // 64-bit keys on the fast path
        __threadfence_block();
        int next = a + 1;
        if (lane < (fast ? 4 : 1)) {
            int it = 0, node = 0, depth = 0;
            bool exhausted = false;
            const bool w = fast ? A::fast(S, a, pool, trace, heap, table_off, tsize, power, lane, res, it, exhausted, node, depth)
                                : A::generic(S, a, pool, trace, heap, heap + table_off, tsize, power, res, it, exhausted, node, depth);
            if (!w && !exhausted && power < P.solver_power) { final = 0; next = 4; }        // stopped by the reduced limit
            else {
                next = G::next(a, w, exhausted);
                if (next == 4 && (w || A::walks_without_winner)) {
                    // this agent ends the game with a node to walk back from: a winner, or (mdungeon, ddave) the BFS agent after
                    // nobody won -- res[] is its node's.  (The compact search's lanes 0..3 all stored every node and trace word:
                    // what lane 0 reads it wrote itself; the fence orders the stores in front of the walk's loads all the same.)
                    __threadfence();
                    if (lane == 0) {
                        winner = w ? a : -1;
                        length = depth;
                        A::walk(fast, pool, trace, trace_cap, node, depth, out.moves + (size_t)m * out.max_len, out.max_len);
                    }
                }
            }
        }
        a = __shfl(next, 0, 64);
        __threadfence_block();
    }
    return __shfl(final, 0, 64) != 0;
}

// what a finished game leaves: the planner's columns of the statistics row (as k_get_stats_search), the length, the winner
template <int PROB>
__device__ __forceinline__ void moves_finish(int32_t* rows_out, const SolOut& out, int m, const int* res, int winner, int length) {
    SearchGame<PROB>::pack(rows_out + (size_t)m * 8, res);
    out.length[m] = length;
    if (out.agent) out.agent[m] = (int8_t)winner;
}

// `traces`: per block `trace_stride` words, indexed like the block's pool (a small try's words start at wv * SS_SMALL_NODES);
// sokoban: NULL and 0
template <int PROB>
__global__ __launch_bounds__(SS_THREADS) void k_get_moves(PcgrlParams P, DevBufs Bs, const uint8_t* __restrict__ maps, int32_t* __restrict__ rows_out,
                                                           SolOut out, int32_t* head, const int32_t* __restrict__ jobs, SokNode* pools, int pool_stride,
                                                           uint32_t* traces, int trace_stride) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ss_lds[];     // the full search region; the small ones are carved out of it
    typedef SearchGame<PROB> Game;
    typedef typename Game::Shared GameShared;
    __shared__ GameShared s_game0;
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[SS_SEARCH_WAVES][EVAL_STAGE_BYTES];
    __shared__ int s_big[EVAL_CHUNK];
    __shared__ int s_nbig, s_base;
    const int tid = (int)threadIdx.x, lane64 = tid & 63, wv = tid >> 6;
    const int cells = P.width * P.height;
    const int njobs = __hip_atomic_load(head + EVAL_HEAD_NJOBS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SokNode* pool = pools + (size_t)blockIdx.x * pool_stride;
    uint32_t* trace = traces + (size_t)blockIdx.x * trace_stride;
    const int small_power = P.solver_power < SS_SMALL_POPS ? P.solver_power : SS_SMALL_POPS;
    GameShared* small_games = reinterpret_cast<GameShared*>(ss_lds + SS_SEARCH_WAVES * SS_SMALL_WORDS);
    DevBufs B = Bs;
    B.map = s_stage[wv < SS_SEARCH_WAVES ? wv : 0];
    for (;;) {
        if (tid == 0) { s_base = atomicAdd(head + EVAL_HEAD_TICKET, EVAL_CHUNK); s_nbig = 0; }
        __syncthreads();
        const int base = s_base;
        if (base >= njobs) break;                                           // block-uniform
        const int n = njobs - base < EVAL_CHUNK ? njobs - base : EVAL_CHUNK;
        if (wv < SS_SEARCH_WAVES) {
            for (int j = wv; j < n; j += SS_SEARCH_WAVES) {
                const int m = jobs[base + j];
                eval_stage_map(maps, m, cells, P.ntiles, s_stage[wv], lane64, 64, B.status);
                __builtin_amdgcn_wave_barrier();
                __threadfence_block();
                int res[Game::NRES] = {};
                int winner = -1, length = 0;
                const bool final = moves_game_run<PROB>(P, B, small_games[wv], ss_lds + wv * SS_SMALL_WORDS, SS_SMALL_HEAP, SS_SMALL_TABLE, small_power,
                                                        pool + (size_t)wv * SS_SMALL_NODES, trace + (size_t)wv * SS_SMALL_NODES, SS_SMALL_NODES, lane64, res,
                                                        winner, length, out, m);
                if (lane64 == 0) {
                    if (final) moves_finish<PROB>(rows_out, out, m, res, winner, length);
                    else s_big[atomicAdd(&s_nbig, 1)] = m;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        if (wv == 0) {
            const int nbig = s_nbig;
            for (int q = 0; q < nbig; q++) {
                const int m = s_big[q];
                eval_stage_map(maps, m, cells, P.ntiles, s_stage[0], lane64, 64, B.status);
                __builtin_amdgcn_wave_barrier();
                __threadfence_block();
                int res[Game::NRES] = {};
                int winner = -1, length = 0;
                moves_game_run<PROB>(P, B, s_game0, ss_lds, SOK_LDS_HEAP, SOK_LDS_TABLE, P.solver_power, pool, trace, trace_stride, lane64, res, winner, length,
                                     out, m);
                if (lane64 == 0) moves_finish<PROB>(rows_out, out, m, res, winner, length);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}
