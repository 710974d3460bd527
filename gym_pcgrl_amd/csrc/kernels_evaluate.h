// pcgrl_get_stats / pcgrl_get_reward: Problem.get_stats, get_reward and get_episode_over as pure functions of the caller's maps and
// statistics rows -- no episode, no handle state but the sticky status word.  Part of the single translation unit pcgrl_abi.hip.
//   k_get_stats          a lane group per map (four maps a wavefront at <= 16 rows, a wavefront per map beyond), grid-stride over
//                        `count`: the caller's bytes -> an LDS stage -> row planes in registers -> compute_item_stats -> the row.
//                        A map that needs the planner gets its partial row and a place on the job list (counter + indices in `work`).
//   k_get_stats_search   sokoban / mdungeon / ddave: persistent blocks shaped like the search phase of k_step_solver -- eight
//                        wavefronts try a chunk of jobs in small private regions, wavefront 0 redoes what was stopped by the small
//                        limit in the full region with the full solver_power.  The job count is read from device memory.  What a job
//                        is comes from a source: EvalMaps here, ChangeJobs for pcgrl_get_changes (kernels_changes.h).
//   k_get_reward         a thread per row: compute_reward + episode_over (pcgrl_algos.h).
#pragma once

// words of the workspace's head: the job counter k_get_stats appends with, the chunk ticket of k_get_stats_search
enum { EVAL_HEAD_NJOBS = 0, EVAL_HEAD_TICKET = 1 };
#define EVAL_JOBS_PER_WAVE 8                                       /* jobs a wavefront of k_get_stats_search tries per chunk */
#define EVAL_CHUNK (SS_SEARCH_WAVES * EVAL_JOBS_PER_WAVE)          /* jobs a block takes per ticket */
#define EVAL_STAGE_BYTES 256                                       /* a compact search level has at most 256 bordered cells */

// a tile id beyond the last counts as the last one: the one rule of every pass that reads the caller's bytes (eval_stage_map, k_changes_finish)
__device__ __forceinline__ uint8_t eval_tile_clamped(uint8_t t, int ntiles) { return t >= ntiles ? (uint8_t)(ntiles - 1) : t; }
// the caller's tile bytes of map m into the group's LDS stage: a tile id from `ntiles` on is reported in the status word and, with
// CLAMP, clamped here (the caller's map stays as it is); without, the byte is staged as it is (k_tile_graph: it is in no tile set)
template <bool CLAMP = true>
__device__ __forceinline__ void eval_stage_map(const uint8_t* __restrict__ maps, long long m, int cells, int ntiles, uint8_t* stage, int lane, int nlanes,
                                               int32_t* status) {
    const uint8_t* src = maps + (size_t)m * cells;
    for (int c = lane; c < cells; c += nlanes) {
        const uint8_t t = src[c];
        if (t >= ntiles) atomicOr(status, PCGRL_STATUS_BAD_TILE);
        stage[c] = CLAMP ? eval_tile_clamped(t, ntiles) : t;
    }
}

// The frame of the kernels with a lane group per caller-supplied map (k_get_stats, k_get_paths; k_tile_graph has it written out, see
// there; map_grid in pcgrl_abi.hip is its launch shape): four maps a wavefront at <= 16 rows, a wavefront per map beyond; `smem` holds
// a stage of tile bytes per group.
template <int G, class MaskT>
struct MapLanes {
    DevGroup<G, MaskT> g;
    int wv, gw;                                                         // the wavefront in the block, the group in the wavefront
    uint8_t* tiles;                                                     // the group's LDS stage
    __device__ __forceinline__ MapLanes(uint8_t* smem, int cells) {
        wv = threadIdx.x >> 6;
        gw = (threadIdx.x & 63) / G;
        tiles = smem + (size_t)(wv * (64 / G) + gw) * reset_tile_bytes(cells);
    }
    // f(m, have) for the group's maps, grid-stride over `count`.  A wave-uniform loop: the groups of a wavefront go round together, a
    // group beyond `count` sits the round out (have = false: a whole lane group; the loop bound is the wavefront's)
    template <class F>
    __device__ __forceinline__ void each(int count, F f) const {
        constexpr int GPW = 64 / G, WPB = PCGRL_BLOCK / 64;
        for (long long base = ((long long)blockIdx.x * WPB + wv) * GPW; base < count; base += (long long)gridDim.x * WPB * GPW) {
            const long long m = base + gw;
            f(m, m < count);
        }
    }
    // map m's bytes -> the stage -> this lane's words of the row planes; on return the stage is free for the next round
    __device__ __forceinline__ void planes(const PcgrlParams& P, const uint8_t* __restrict__ maps, long long m, bool have, MaskT& b0, MaskT& b1, MaskT& b2,
                                           int32_t* status) const {
        if (have) eval_stage_map(maps, m, P.width * P.height, P.ntiles, tiles, g.lane, G, status);
        __builtin_amdgcn_wave_barrier();
        planes_from_tiles<MaskT>(P, tiles, (MaskT*)nullptr, have ? g.lane : -1, b0, b1, b2, false);
        __builtin_amdgcn_wave_barrier();
    }
};
// a statistics row as the caller gets it: the problem's columns, zeros behind them (binary: the champion flag and bound of slots 2, 3
// stay inside)
template <int PROB>
__device__ __forceinline__ void store_stats_row(int32_t* row, const int32_t* s) {
#pragma unroll
    for (int k = 0; k < 8; k++) row[k] = k < num_stats(PROB) ? s[k] : 0;
}

template <int PROB, int G, class MaskT>
__global__ __launch_bounds__(PCGRL_BLOCK) void k_get_stats(PcgrlParams P, const uint8_t* __restrict__ maps, int count, int32_t* __restrict__ rows_out,
                                                            int32_t* status, int32_t* head, int32_t* jobs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // per lane group the tile bytes of its map
    const MapLanes<G, MaskT> L(smem, P.width * P.height);
    const auto& g = L.g;
    const MaskT rowmask = row_valid<MaskT>(g.lane, P.width, P.height);
    L.each(count, [&](long long m, bool have) {
        MaskT b0, b1, b2;
        L.planes(P, maps, m, have, b0, b1, b2, status);
        int32_t s[PCGRL_MAX_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool need_solver = false;
        if (have) need_solver = compute_item_stats<PROB>(g, P, b0, b1, b2, rowmask, s, status);
        if (g.lane == 0 && have) {
            store_stats_row<PROB>(rows_out + (size_t)m * 8, s);
            if (need_solver) jobs[atomicAdd(head + EVAL_HEAD_NJOBS, 1)] = (int32_t)m;
        }
    });
}

// `Bs`: what search_game_run reads of a DevBufs -- status, sok_use_lds, sok_fast_maxc (SearchGame<PROB>::build) and `map`, which every
// wavefront points at its own clamped LDS copy of the job's map (environment 0 of a one-map batch): the agents work on the level
// that build() left in LDS and on the regions and pools they are handed, nothing else of the struct is dereferenced.
// `Src`: what a job is -- stage(j, P, cells, stage, lane, status) fills a wavefront's stage with job j's level (the wave barrier follows
// here), row(j) is where its row goes.  EvalMaps: job j is map j of the caller's (pcgrl_get_stats); ChangeJobs (kernels_changes.h): a
// level with one cell set to a tile.
struct EvalMaps {
    const uint8_t* __restrict__ maps;
    int32_t* __restrict__ rows_out;
    __device__ __forceinline__ void stage(int m, const PcgrlParams& P, int cells, uint8_t* stage, int lane, int32_t* status) const {
        eval_stage_map(maps, m, cells, P.ntiles, stage, lane, 64, status);
    }
    __device__ __forceinline__ int32_t* row(int m) const { return rows_out + (size_t)m * 8; }
};
template <int PROB, class Src>
__global__ __launch_bounds__(SS_THREADS) void k_get_stats_search(PcgrlParams P, DevBufs Bs, Src src,
                                                                  int32_t* head, const int32_t* __restrict__ jobs, SokNode* pools, int pool_stride) {
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
                src.stage(m, P, cells, s_stage[wv], lane64, B.status);
                __builtin_amdgcn_wave_barrier();
                __threadfence_block();
                int res[Game::NRES] = {};
                const bool final = search_game_run<PROB>(P, B, 0, small_games[wv], ss_lds + wv * SS_SMALL_WORDS, SS_SMALL_HEAP, SS_SMALL_TABLE, small_power,
                                                         pool + (size_t)wv * SS_SMALL_NODES, lane64, res);
                if (lane64 == 0) {
                    if (final) Game::pack(src.row(m), res);
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
                src.stage(m, P, cells, s_stage[0], lane64, B.status);
                __builtin_amdgcn_wave_barrier();
                __threadfence_block();
                int res[Game::NRES] = {};
                search_game_run<PROB>(P, B, 0, s_game0, ss_lds, SOK_LDS_HEAP, SOK_LDS_TABLE, P.solver_power, pool, lane64, res);
                if (lane64 == 0) Game::pack(src.row(m), res);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

// Problem.get_reward(new, old) and Problem.get_episode_over(new, start) over rows: `ref` is both the old and the start statistics
// (a template like k_smb<0>: only the part that launches it holds an instance)
template <int UNUSED>
__global__ __launch_bounds__(256) void k_get_reward(PcgrlParams P, const int32_t* __restrict__ rows, const int32_t* __restrict__ ref, int count,
                                                    double* __restrict__ reward_out, uint8_t* __restrict__ over_out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        int32_t n[PCGRL_MAX_STATS], o[PCGRL_MAX_STATS];
#pragma unroll
        for (int k = 0; k < PCGRL_MAX_STATS; k++) { n[k] = rows[(size_t)i * 8 + k]; o[k] = ref[(size_t)i * 8 + k]; }
        if (reward_out) reward_out[i] = compute_reward(P, n, o, P.prob);
        if (over_out) over_out[i] = episode_over(P, n, o, P.prob) ? 1 : 0;
    }
}
