// SearchGame<PROB>: what a search problem's _run_game is (sokoban_prob.py:104-122, mdungeon_prob.py:110-126, ddave_prob.py:111-127),
// written once per problem for every kernel that plays it -- the concurrent four-agent kernels (kernels_sokoban.h,
// kernels_agents4.h), the sequential search_game_run below (kernels_step_solver.h) and the resumable one (kernels_search_async.h).
// Device only, part of the single translation unit pcgrl_abi.hip; everything here is chosen at compile time.
//   Shared        the level, the root and work nodes, the compact level and node cache, the `fast` flag (LDS)
//   build         the level by the 64 lanes of a wavefront (level_build_wave.h) and whether the compact search takes it
//   KS / NRES     the agents in the reference's order (-1 = BFS, else A* with weight k / 2); how many values get_stats takes
//   agent_fast    agent a by the compact search (*_fast.h): lanes 0..3, LDS heap at `lds`, 64-bit-key table at lds + toff
//   agent_generic agent a by the generic search (*_solver.h): lane 0, heap and table in LDS or in the global arena
//   next          the agent that runs after agent a in the sequential loop (4 = none)
//   pack          the agent's values into the stats row
// and for the kernels that run the four agents side by side: encode / decode (word 3 of an agent's record in sok_res), stop_update
// (what a finished agent tells the others through sok_stop) and stopped (whether agent a may give up on seeing that word).
#pragma once

#define MD_STOP_EXHAUSTED 256          /* sok_stop, mdungeon: an A* agent ran out of states without a win */

__device__ __forceinline__ int sok_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The four children of a pop, one per lane (lanes 0..3 run the search in lockstep; everything else in it is
// uniform across them).  The results come back through v_readlane, i.e. as scalars.
struct SokKidsLanes {
    int lane, dir;      // dir: this lane's move as a cell offset (sokf_dir(lane & 3, level width)), made once per search
    // this lane's child only (two-wavefront searches: each lane files its own child)
    template <int NW>
    __device__ __forceinline__ SokChild mine(const SokFastLevel<NW>& F, uint64_t cr, const uint64_t* cb, int player, int h) const {
        return sokf_child_dir<NW>(F, cr, cb, player, h, dir);
    }
    template <int NW>
    __device__ __forceinline__ void operator()(const SokFastLevel<NW>& F, uint64_t cr, const uint64_t* cb, int player, int h, SokChild* out) const {
        const SokChild mine = sokf_child_dir<NW>(F, cr, cb, player, h, dir);
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine.cr, d);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine.cr >> 32), d);
            out[d].cr = ((uint64_t)hi << 32) | lo;
            out[d].np = __builtin_amdgcn_readlane(mine.np, d);
            out[d].h = __builtin_amdgcn_readlane(mine.h, d);
            out[d].ok = __builtin_amdgcn_readlane(mine.ok, d);
        }
    }
};

// The four children of a pop, one per lane (lanes 0..3 run the compact search in lockstep; everything else in it is
// uniform across them).  The results come back through v_readlane, i.e. as scalars.
struct MdKidsLanes {
    int lane;
    // this lane's child only (two-wavefront searches: each lane files its own child)
    template <class TP>
    __device__ __forceinline__ MdChild mine(const MdLevel& L, const MdFastLevel& F, TP table, int table_mask, uint64_t key, uint64_t alive,
                                            int player, int health) const {
        return mdf_child(L, F, table, table_mask, key, alive, player, health, lane & 3);
    }
    template <class TP>
    __device__ __forceinline__ void operator()(const MdLevel& L, const MdFastLevel& F, TP table, int table_mask, uint64_t key, uint64_t alive,
                                               int player, int health, MdChild* out) const {
        const MdChild mine = mdf_child(L, F, table, table_mask, key, alive, player, health, lane & 3);
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine.key, d);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine.key >> 32), d);
            out[d].key = ((uint64_t)hi << 32) | lo;
            out[d].h = __builtin_amdgcn_readlane(mine.h, d);
            out[d].drop = __builtin_amdgcn_readlane(mine.drop, d);
        }
    }
};

// The four children of a pop, one per lane (lanes 0..3 run the compact search in lockstep).
struct DdKidsLanes {
    int lane;
    // this lane's child only (two-wavefront searches: each lane files its own child)
    template <class TP>
    __device__ __forceinline__ DdChild mine(const DdLevel& L, const DdFastLevel& F, TP table, int table_mask, uint64_t key, int aj, bool ground,
                                            bool ceiling) const {
        return ddf_child(L, F, table, table_mask, key, aj, ground, ceiling, lane & 3);
    }
    template <class TP>
    __device__ __forceinline__ void operator()(const DdLevel& L, const DdFastLevel& F, TP table, int table_mask, uint64_t key, int aj, bool ground,
                                               bool ceiling, DdChild* out) const {
        const DdChild mine = ddf_child(L, F, table, table_mask, key, aj, ground, ceiling, lane & 3);
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine.key, d);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine.key >> 32), d);
            out[d].key = ((uint64_t)hi << 32) | lo;
            out[d].h = __builtin_amdgcn_readlane(mine.h, d);
            out[d].aj = __builtin_amdgcn_readlane(mine.aj, d);
            out[d].drop = __builtin_amdgcn_readlane(mine.drop, d);
        }
    }
};

template <int PROB>
struct SearchGame;

template <>
struct SearchGame<PCGRL_PROB_SOKOBAN> {
    struct Shared { SokLevel L; SokNode root, work; SokFastNode cache[4]; int fast; uint8_t scratch[64]; };
    static constexpr int NRES = 2;                                                  // dist-win, sol-length
    static __device__ __forceinline__ int ks(int a) { const int KS[4] = {-1, 2, 1, 0}; return KS[a]; }   // BFS, A*(1), A*(0.5), A*(0)
    // the compact search: levels of at most sok_fast_maxc crates (PCGRL_SOK_GENERIC=1 makes that -1: tests); it needs the LDS heap
    static __device__ __forceinline__ void build(const PcgrlParams& P, const DevBufs& B, const uint8_t* map, Shared& S, int lane) {
        const int ncr = sok_build_level_wave(map, P.width, P.height, S.L, S.root, lane);
        sok_init_deadlocks_wave(S.L, S.scratch, lane);
        if (lane == 0) {
            if (ncr > SOK_MAXC) atomicOr(B.status, 1);
            S.root.h = (uint16_t)sok_heuristic(S.L, S.root.crate);
            S.fast = (B.sok_use_lds && B.sok_fast_maxc >= 0 && S.L.nc <= B.sok_fast_maxc) ? 1 : 0;
        }
    }
    template <class Hook, class RSP = SokNoResume>
    static __device__ __forceinline__ bool agent_fast(Shared& S, int a, void* pool, uint32_t* lds, int toff, int tsize, int power, int lane, int* res,
                                                      int& it, bool& exhausted, Hook hook, SokDuoBox* duo = nullptr, RSP rsp = RSP()) {
        const SokKidsLanes kids = {lane, sokf_dir(lane & 3, S.L.w)};
        uint64_t* tab = reinterpret_cast<uint64_t*>(lds + toff);
        SokFastNode* fp = reinterpret_cast<SokFastNode*>(pool);
        int hh = 0, dd = 0;
        bool w;
        if (S.L.cells <= 64) w = sok_search_fast<1>(S.L, fp, lds, tab, tsize - 1, S.cache, S.root, ks(a), power, hh, dd, it, exhausted, hook, kids, duo, rsp);
        else w = sok_search_fast<4>(S.L, fp, lds, tab, tsize - 1, S.cache, S.root, ks(a), power, hh, dd, it, exhausted, hook, kids, duo, rsp);
        res[0] = w ? 0 : hh; res[1] = w ? dd : 0;
        return w;
    }
    template <class HP, class TP, class Hook>
    static __device__ __forceinline__ bool agent_generic(Shared& S, int a, void* pool, HP heap, TP table, int tsize, int power, int* res, int& it,
                                                         bool& exhausted, Hook hook) {
        int hh = 0, dd = 0;
        const bool w = sok_search(S.L, reinterpret_cast<SokNode*>(pool), heap, table, tsize - 1, S.work, S.root, ks(a), power, hh, dd, it, exhausted, hook);
        res[0] = w ? 0 : hh; res[1] = w ? dd : 0;
        return w;
    }
    // (the same two agents traced: TracedAgents<PCGRL_PROB_SOKOBAN>, kernels_moves.h)
    // first winner, or the exact exhausted-BFS shortcut (sokoban_solver.h)
    static __device__ __forceinline__ int next(int a, bool win, bool exhausted) { return (win || (a == 0 && exhausted) || a == 3) ? 4 : a + 1; }
    static __device__ __forceinline__ void pack(int32_t* s, const int* res) { s[4] = res[0]; s[5] = res[1]; }
    // agents after `a` are not needed once a wins (or BFS has expanded every reachable state): stop level 3 - a
    static __device__ __forceinline__ void stop_update(int32_t* stop, int a, bool win, bool exhausted) {
        if (win || (a == 0 && exhausted)) atomicMax(stop, 3 - a);
    }
    static __device__ __forceinline__ bool stopped(int v, int a) { return v >= 4 - a; }
};

template <>
struct SearchGame<PCGRL_PROB_MDUNGEON> {
    struct Shared { MdLevel L; MdNode root, work; MdFastLevel F; MdFastNode cache[4]; int fast; };
    static constexpr int NRES = 5;                                                  // dist-win, sol-length, col-potions, col-treasures, col-enemies
    static __device__ __forceinline__ int ks(int a) { const int KS[4] = {2, 1, 0, -1}; return KS[a]; }   // A*(1), A*(0.5), A*(0), BFS
    // the compact search (mdungeon_fast.h): levels with few things; PCGRL_SOK_GENERIC=1 switches it off (tests); it needs the LDS heap
    static __device__ __forceinline__ void build(const PcgrlParams& P, const DevBufs& B, const uint8_t* map, Shared& S, int lane) {
        const int nthings = md_build_level_wave(map, P.width, P.height, S.L, S.root, S.F, lane);
        if (lane == 0) S.fast = (B.sok_use_lds && B.sok_fast_maxc >= 0 && nthings <= MDF_MAXI) ? 1 : 0;
    }
    template <class Hook, class RSP = SokNoResume>
    static __device__ __forceinline__ bool agent_fast(Shared& S, int a, void* pool, uint32_t* lds, int toff, int tsize, int power, int lane, int* res,
                                                      int& it, bool& exhausted, Hook hook, SokDuoBox* duo = nullptr, RSP rsp = RSP()) {
        const MdKidsLanes kids = {lane};
        uint64_t key = 0;
        int hh = 0, dd = 0;
        const bool w = md_search_fast(S.L, S.F, reinterpret_cast<MdFastNode*>(pool), lds, reinterpret_cast<uint64_t*>(lds + toff), tsize - 1, S.cache,
                                      S.root, ks(a), power, key, hh, dd, it, exhausted, hook, kids, duo, rsp);
        mdf_result(S.F, key, hh, dd, w, res);
        return w;
    }
    template <class HP, class TP, class Hook>
    static __device__ __forceinline__ bool agent_generic(Shared& S, int a, void* pool, HP heap, TP table, int tsize, int power, int* res, int& it,
                                                         bool& exhausted, Hook hook) {
        const bool w = md_search(S.L, reinterpret_cast<MdNode*>(pool), heap, table, tsize - 1, S.work, S.root, ks(a), power, it, exhausted, hook);
        md_result(S.L, S.root, S.work, w, res);
        return w;
    }
    // md_run_game: an A* agent that ran out of states without a win sends the game straight to BFS -- no agent can win or reach the cap
    static __device__ __forceinline__ int next(int a, bool win, bool exhausted) { return (win || a == 3) ? 4 : ((a < 3 && exhausted) ? 3 : a + 1); }
    static __device__ __forceinline__ void pack(int32_t* s, const int* res) { md_pack(s, res); }
    static __device__ __forceinline__ int encode(const int* res) { return (res[2] & 255) | ((res[3] & 255) << 8) | ((res[4] & 255) << 16); }
    static __device__ __forceinline__ void decode(int w, int* res) { res[2] = w & 255; res[3] = (w >> 8) & 255; res[4] = (w >> 16) & 255; }
    // an earlier winner stops the later agents (level 3 - a in the low byte); an exhausted A* agent stops the other A* agents
    static __device__ __forceinline__ void stop_update(int32_t* stop, int a, bool win, bool exhausted) {
        if (win) atomicMax(stop, 3 - a);
        else if (a < 3 && exhausted) atomicOr(stop, MD_STOP_EXHAUSTED);
    }
    static __device__ __forceinline__ bool stopped(int v, int a) { return (v & 255) >= 4 - a || (a < 3 && (v & MD_STOP_EXHAUSTED)); }
};

template <>
struct SearchGame<PCGRL_PROB_DDAVE> {
    struct Shared { DdLevel L; DdNode root, work; DdFastLevel F; DdFastNode cache[4]; int fast; };
    static constexpr int NRES = 4;                                                  // dist-win, sol-length, num-jumps, col-diamonds
    static __device__ __forceinline__ int ks(int a) { const int KS[4] = {2, 1, 0, -1}; return KS[a]; }   // A*(1), A*(0.5), A*(0), BFS
    // the compact search (ddave_fast.h): levels with few diamonds; PCGRL_SOK_GENERIC=1 switches it off (tests); it needs the LDS heap
    static __device__ __forceinline__ void build(const PcgrlParams& P, const DevBufs& B, const uint8_t* map, Shared& S, int lane) {
        const int nd = dd_build_level_wave(map, P.width, P.height, S.L, S.root, S.F, lane);
        if (lane == 0) S.fast = (B.sok_use_lds && B.sok_fast_maxc >= 0 && nd <= DDF_MAXD) ? 1 : 0;
    }
    template <class Hook, class RSP = SokNoResume>
    static __device__ __forceinline__ bool agent_fast(Shared& S, int a, void* pool, uint32_t* lds, int toff, int tsize, int power, int lane, int* res,
                                                      int& it, bool& exhausted, Hook hook, SokDuoBox* duo = nullptr, RSP rsp = RSP()) {
        const DdKidsLanes kids = {lane};
        uint64_t key = 0;
        int hh = 0, dd = 0, jj = 0;
        const bool w = dd_search_fast(S.L, S.F, reinterpret_cast<DdFastNode*>(pool), lds, reinterpret_cast<uint64_t*>(lds + toff), tsize - 1, S.cache,
                                      S.root, ks(a), power, key, hh, dd, jj, it, exhausted, hook, kids, duo, rsp);
        ddf_result(S.F, key, hh, dd, jj, w, res);
        return w;
    }
    template <class HP, class TP, class Hook>
    static __device__ __forceinline__ bool agent_generic(Shared& S, int a, void* pool, HP heap, TP table, int tsize, int power, int* res, int& it,
                                                         bool& exhausted, Hook hook) {
        const bool w = dd_search(S.L, reinterpret_cast<DdNode*>(pool), heap, table, tsize - 1, S.work, S.root, ks(a), power, it, exhausted, hook);
        dd_result(S.L, S.work, w, res);
        return w;
    }
    // this engine's visited key ignores the air time, so the states an agent gets to see depend on its own order of exploration:
    // an agent that exhausts says nothing about the others (ddave_solver.h)
    static __device__ __forceinline__ int next(int a, bool win, bool) { return (win || a == 3) ? 4 : a + 1; }
    static __device__ __forceinline__ void pack(int32_t* s, const int* res) { dd_pack(s, res); }
    static __device__ __forceinline__ int encode(const int* res) { return (res[2] & 0xFFFF) | ((res[3] & 255) << 16); }
    static __device__ __forceinline__ void decode(int w, int* res) { res[2] = w & 0xFFFF; res[3] = (w >> 16) & 255; }
    static __device__ __forceinline__ void stop_update(int32_t* stop, int a, bool win, bool) { if (win) atomicMax(stop, 3 - a); }
    static __device__ __forceinline__ bool stopped(int v, int a) { return (v & 255) >= 4 - a; }
};

// Agent a of the concurrent kernels looks at its environment's stop word every SOK_POLL_MASK + 1 pops and gives up once its
// result cannot be selected any more.
template <int PROB>
struct SearchPollHook {
    const int32_t* stop; int a;
    __device__ __forceinline__ bool operator()(int it) const { return (it & SOK_POLL_MASK) == 0 && SearchGame<PROB>::stopped(sok_ld(stop), a); }
};

// Agent a in a block's search region, the way the level (S.fast) and the launch (B.sok_use_lds) ask for it: the compact search with
// heap and 64-bit-key table in LDS (lanes 0..3 call), else the generic one with both in LDS or both in the global arena (lane 0
// calls).  Two generic instantiations: LDS pointers compile to ds_* instructions.
template <int PROB, class Hook>
__device__ __forceinline__ bool search_agent(const DevBufs& B, typename SearchGame<PROB>::Shared& S, int a, void* pool, uint32_t* lds, uint32_t* g_heap,
                                             uint32_t* g_table, int tsize, int fast, int power, int lane, int* res, int& it, bool& exhausted, Hook hook,
                                             SokDuoBox* duo) {
    typedef SearchGame<PROB> G;
    if (fast) return G::agent_fast(S, a, pool, lds, SOK_LDS_HEAP, tsize, power, lane, res, it, exhausted, hook, duo);
    if (B.sok_use_lds) return G::agent_generic(S, a, pool, lds, lds + SOK_LDS_HEAP, tsize, power, res, it, exhausted, hook);
    return G::agent_generic(S, a, pool, g_heap, g_table, tsize, power, res, it, exhausted, hook);
}
// ... and the clearing of its visited table in front of it, by the 64 lanes
__device__ __forceinline__ void search_clear_table(const DevBufs& B, uint32_t* lds, uint32_t* g_table, int tsize, int fast, int lane) {
    if (fast) { for (int i = lane; i < 2 * tsize; i += 64) lds[SOK_LDS_HEAP + i] = 0; }   // 64-bit keys
    else if (B.sok_use_lds) { for (int i = lane; i < tsize; i += 64) lds[SOK_LDS_HEAP + i] = 0; }
    else { for (int i = lane; i < tsize; i += 64) g_table[i] = 0; }
}

// The end of a search job (one lane): the row that k_stats / k_reset parked, the solver's columns from res[], and the end of the
// step or reset the job belongs to (finalize_item; to_list: an environment whose episode ends here goes to rst_list).  Returns
// whether the episode ended.
template <int PROB>
__device__ __forceinline__ bool finish_search_item(const PcgrlParams& P, const DevBufs& B, int e, const int* res, int mode, int parity, bool to_list,
                                                   int rst_list) {
    int32_t s[PCGRL_MAX_STATS];
    const int32_t* park = (mode == MODE_STEP) ? B.info + (size_t)e * 10 : B.stats + (size_t)e * 8;
    for (int k = 0; k < 8; k++) s[k] = park[k];
    SearchGame<PROB>::pack(s, res);
    return finalize_item<PROB>(P, B, e, s, mode, parity, e & (WL_NSHARD - 1), to_list, rst_list);
}

// _run_game of one level by one wavefront with the agents in sequence, inside a given search region (`heap`, `table` of `tsize`
// slots at `heap + table_off` words) and with at most `power` pops per agent; res[] (lane 0): what the last agent that ran found.
// Returns (on every lane) whether the result is final: with power < solver_power an agent that is stopped by the limit makes the
// whole job "not final" -- it is then run again with the full region and the full power.  A search that ends by winning or by
// running out of states before the limit gives what the full search gives (the table size only changes the probe sequences).
template <int PROB>
__device__ __forceinline__ bool search_game_run(const PcgrlParams& P, const DevBufs& B, int e, typename SearchGame<PROB>::Shared& S, uint32_t* heap,
                                                int table_off, int tsize, int power, void* pool, int lane, int* res) {
    typedef SearchGame<PROB> G;
    G::build(P, B, B.map + (size_t)e * P.width * P.height, S, lane);
    __threadfence_block();
    const int fast = S.fast;
    int final = 1;
    for (int a = 0; a < 4;) {
        for (int i = lane; i < (fast ? 2 : 1) * tsize; i += 64) heap[table_off + i] = 0;      // 64-bit keys on the fast path
        __threadfence_block();
        int next = a + 1;
        if (lane < (fast ? 4 : 1)) {
            int it = 0;
            bool exhausted = false;
            const bool w = fast ? G::agent_fast(S, a, pool, heap, table_off, tsize, power, lane, res, it, exhausted, SokNoHook())
                                : G::agent_generic(S, a, pool, heap, heap + table_off, tsize, power, res, it, exhausted, SokNoHook());
            if (!w && !exhausted && power < P.solver_power) { final = 0; next = 4; }        // stopped by the reduced limit
            else next = G::next(a, w, exhausted);
        }
        a = __shfl(next, 0, 64);
        __threadfence_block();
    }
    return __shfl(final, 0, 64) != 0;
}
