// pcgrl_get_solution: SokobanProblem.get_stats(map)["solution"] (sokoban_prob.py:133-145) -- the moves of the first agent of
// _run_game (:104-122) that wins, Node.getActions (engine.py:38-44) -- for the caller's maps.  Part of the single translation unit
// pcgrl_abi.hip.  The job list is the one k_get_stats<sokoban> makes (kernels_evaluate.h); k_get_solution is k_get_stats_search with
// the traced searches (SokTrace, sokoban_solver.h): a chunk ticket, eight wavefronts try the jobs in the small regions, wavefront 0
// redoes what the small limit stopped in the full region with the full solver_power.  Right after the agent that ends a game returns,
// while that wavefront's pool still holds the search, one lane walks the parent chain from the winning node and writes the moves.
// Only a run whose result is accepted writes: a try that was "not final" has no winner, so it has nothing to write.
// The rows are filled with -1, the lengths with 0 and the agents with -2 before the launch (pcgrl_get_solution): a level whose
// planner does not run is never seen here.
// solution_game_run and k_get_solution repeat search_game_run (search_game.h) and k_get_stats_search (kernels_evaluate.h) on purpose:
// one body with an agent / finish policy was tried and changed the machine code of k_step_solver and k_get_stats_search (the
// compiler schedules the inlined loop differently), and those kernels have to stay what they are.  A change to the ticket, the small
// tries or the redo there has to be made here as well.
#pragma once

struct SolOut { int8_t* moves; int32_t* length; int8_t* agent; int max_len; };

// search_game_run (search_game.h) for sokoban with traced agents.  res[] as there; `winner` (lane 0): the agent that won, -1 = none.
// The winner's moves are in the level's row of `out` when this returns "final".
__device__ __forceinline__ bool solution_game_run(const PcgrlParams& P, const DevBufs& B, SearchGame<PCGRL_PROB_SOKOBAN>::Shared& S, uint32_t* heap, int table_off,
                                                  int tsize, int power, void* pool, int lane, int* res, int& winner, const SolOut& out, int m) {
    typedef SearchGame<PCGRL_PROB_SOKOBAN> G;
    G::build(P, B, B.map, S, lane);
    __threadfence_block();
    const int fast = S.fast;
    int final = 1;
    winner = -1;
    for (int a = 0; a < 4;) {
        for (int i = lane; i < (fast ? 2 : 1) * tsize; i += 64) heap[table_off + i] = 0;      // 64-bit keys on the fast path
        __threadfence_block();
        int next = a + 1;
        if (lane < (fast ? 4 : 1)) {
            int it = 0, widx = 0;
            bool exhausted = false;
            const bool w = fast ? G::agent_fast_traced(S, a, pool, heap, table_off, tsize, power, lane, res, it, exhausted, widx)
                                : G::agent_generic_traced(S, a, pool, heap, heap + table_off, tsize, power, res, it, exhausted, widx);
            if (!w && !exhausted && power < P.solver_power) { final = 0; next = 4; }        // stopped by the reduced limit
            else next = G::next(a, w, exhausted);
            if (w) {
                // (the compact search's lanes 0..3 all stored every node: what lane 0 reads it wrote itself; the fence orders the
                //  stores in front of the walk's loads all the same)
                __threadfence();
                if (lane == 0) {
                    winner = a;
                    int8_t* row = out.moves + (size_t)m * out.max_len;
                    if (fast) sokf_walk_back(reinterpret_cast<const SokFastNode*>(pool), widx, res[1], row, out.max_len);
                    else sok_walk_back(reinterpret_cast<const SokNode*>(pool), widx, res[1], row, out.max_len);
                }
            }
        }
        a = __shfl(next, 0, 64);
        __threadfence_block();
    }
    return __shfl(final, 0, 64) != 0;
}

// what a finished game leaves: the planner's columns of the statistics row (as k_get_stats_search), the length, the winner
__device__ __forceinline__ void solution_finish(int32_t* rows_out, const SolOut& out, int m, const int* res, int winner) {
    SearchGame<PCGRL_PROB_SOKOBAN>::pack(rows_out + (size_t)m * 8, res);
    out.length[m] = res[1];
    if (out.agent) out.agent[m] = (int8_t)winner;
}

// (a template like k_get_reward<0>: only the part that launches it holds an instance)
template <int UNUSED>
__global__ __launch_bounds__(SS_THREADS) void k_get_solution(PcgrlParams P, DevBufs Bs, const uint8_t* __restrict__ maps, int32_t* __restrict__ rows_out,
                                                              SolOut out, int32_t* head, const int32_t* __restrict__ jobs, SokNode* pools, int pool_stride) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ss_lds[];     // the full search region; the small ones are carved out of it
    typedef SearchGame<PCGRL_PROB_SOKOBAN> Game;
    typedef typename Game::Shared GameShared;
    __shared__ GameShared s_game0;
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[SS_SEARCH_WAVES][EVAL_STAGE_BYTES];
    __shared__ int s_big[EVAL_CHUNK];
    __shared__ int s_nbig, s_base;
    const int tid = (int)threadIdx.x, lane64 = tid & 63, wv = tid >> 6;
    const int cells = P.width * P.height;
    const int njobs = __hip_atomic_load(head + EVAL_HEAD_NJOBS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SokNode* pool = pools + (size_t)blockIdx.x * pool_stride;
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
                int winner = -1;
                const bool final = solution_game_run(P, B, small_games[wv], ss_lds + wv * SS_SMALL_WORDS, SS_SMALL_HEAP, SS_SMALL_TABLE, small_power,
                                                     pool + (size_t)wv * SS_SMALL_NODES, lane64, res, winner, out, m);
                if (lane64 == 0) {
                    if (final) solution_finish(rows_out, out, m, res, winner);
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
                int winner = -1;
                solution_game_run(P, B, s_game0, ss_lds, SOK_LDS_HEAP, SOK_LDS_TABLE, P.solver_power, pool, lane64, res, winner, out, m);
                if (lane64 == 0) solution_finish(rows_out, out, m, res, winner);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}
