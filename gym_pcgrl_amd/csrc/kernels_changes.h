// pcgrl_get_changes: the statistics row, reward and episode end of a level with one cell set to each of the problem's tiles, for a
// list of cells per level -- what a representation's action, a mutation or a "which tiles matter" map asks.  A pure function like
// pcgrl_get_stats (kernels_evaluate.h): no episode, no handle state but the sticky status word.  Part of the single translation unit
// pcgrl_abi.hip.
//   k_get_changes        a lane group per work item = (level, chunk of its cells), grid-stride over the items with k_get_stats' launch
//                        shape (map_grid: four levels a wavefront at <= 16 rows, a wavefront a level beyond).  Per item the level is
//                        staged and its row planes are built ONCE, and the level's own row is computed once; per cell and tile the
//                        lane that owns the cell's row sets the cell's three plane bits in its registers (planes_set_cell,
//                        pcgrl_algos.h), compute_item_stats runs on the edited planes, and the planes are taken back from the kept
//                        originals (a copy in LDS: see the kernel).  Entry (level, cell, tile) = the row; the tile the cell already holds is the level's own row with
//                        reward 0 and is not computed again: a cell takes T - 1 turns, and in each every group of the wavefront has a tile.  binary, zelda: the reward (new = the entry's row, old = the level's own)
//                        and `over` (against the start row, by default the level's own) leave in the same pass.
//                        sokoban, mdungeon, ddave: the partial row, and the entries (and levels) that need the planner go on the job list.
//   ChangeJobs           the job source of k_get_stats_search for those: job j < entries is "level m with cell c set to tile t", a job
//                        beyond is the level itself (its own row).
//   k_changes_finish     the search problems' trailing pass, a thread per entry over the finished rows: the no-op entries take the
//                        level's own row, every entry its reward and `over` (k_get_reward's body with the level's row as `old`).
#pragma once

// the cell of entry column `col` = m * ncells + k: the caller's list (clamped into the map and reported like an action outside the action space)
// or, without one, every cell in row-major order
__device__ __forceinline__ int changes_cell(const int32_t* __restrict__ cells, int col, int ncells, int map_cells, int32_t* status) {
    if (!cells) return col % ncells;                                     // (col = m * ncells + k)
    int c = cells[col];
    if (c < 0 || c >= map_cells) {
        if (status) atomicOr(status, PCGRL_STATUS_BAD_ACTION);           // (NULL: the later passes, which do not report it again)
        c = c < 0 ? 0 : map_cells - 1;
    }
    return c;
}

// `chunk` cells an item, `nchunks` items a level (the host's choice: launch_get_changes).  `head` / `jobs`: the search problems' job
// counter and list (entries first, then entries + m for the level's own row); NULL for binary and zelda.
// Registers: the kernel is held to the eight wavefronts a SIMD that k_get_stats runs at (at most 64 vector registers: the second launch
// bound).  What lives across the statistics of an entry and is read again only after them waits in LDS behind the group's stage for
// that: the level's own row, the start row and the level's `over` (lane 0's), and every lane's words of the level's own planes -- with
// those in registers the forms with 64-bit row masks spilled 11 to 40 dwords a lane at this budget.  The edit itself is in registers.
// Sixteen lanes with 64-bit masks still kept 4 to 9 dwords in scratch: the launcher gives such maps a wavefront a level (changes_group,
// pcgrl_abi.hip), so that form is not instantiated.
#define CHANGES_KEEP_BYTES 80      /* per lane group: the level's own row [0,8), the start row [8,16), its `over` [16], the item's column and cells [17,19) */
__host__ __device__ constexpr int changes_group_bytes(int map_cells, int group, int mask_bytes) {      // a lane group's LDS: stage, rows, planes
    return reset_tile_bytes(map_cells) + CHANGES_KEEP_BYTES + 3 * group * mask_bytes;
}
template <int PROB, int G, class MaskT>
__global__ __launch_bounds__(PCGRL_BLOCK, 8) void k_get_changes(PcgrlParams P, const uint8_t* __restrict__ maps, int count, const int32_t* __restrict__ cells,
                                                              int ncells, int chunk, int nchunks, const int32_t* __restrict__ start_rows,
                                                              int32_t* __restrict__ base_rows_out, int32_t* __restrict__ rows_out, double* __restrict__ reward_out,
                                                              uint8_t* __restrict__ over_out, int32_t* status, int32_t* head, int32_t* jobs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // per lane group: changes_group_bytes
    constexpr int GPW = 64 / G, WPB = PCGRL_BLOCK / 64;
    constexpr bool SEARCH = PROB != PCGRL_PROB_BINARY && PROB != PCGRL_PROB_ZELDA;
    constexpr bool ONE_PLANE = PROB == PCGRL_PROB_BINARY;
    DevGroup<G, MaskT> g;
    const int lane64 = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), gw = lane64 / G;      // (wv: scalar -- with 64 lanes the item is too)
    const int W = P.width, H = P.height, map_cells = W * H, T = P.ntiles;
    // a group's LDS: the kept words, the kept planes, then the stage -- the first two at offsets the compiler knows
    int32_t* own = reinterpret_cast<int32_t*>(smem + (size_t)(wv * GPW + gw) * changes_group_bytes(map_cells, G, (int)sizeof(MaskT)));
    volatile MaskT* keep = reinterpret_cast<MaskT*>(own + CHANGES_KEEP_BYTES / 4) + g.lane;      // plane p of this lane's row: keep[p * G]
    uint8_t* tiles = reinterpret_cast<uint8_t*>(own) + CHANGES_KEEP_BYTES + 3 * G * sizeof(MaskT);
    volatile int32_t* item = own + 17;                                   // the item's first entry column and its number of cells (read per entry)
    const int items = count * nchunks, entries = count * ncells * T;     // (pcgrl_get_changes_bytes: entries + count fit 31 bits)
    // wave-uniform loops: the groups of a wavefront go round together -- a group beyond the items sits the round out, one whose chunk is
    // shorter sits its last cells out; inside a turn only whole groups are switched off
    for (int base = (blockIdx.x * WPB + wv) * GPW; base < items; base += (int)gridDim.x * WPB * GPW) {
        const int it = base + gw;
        const bool have = it < items;
        const int m = have ? it / nchunks : 0;
        const int k0 = have ? (it - m * nchunks) * chunk : 0;
        const int kn = !have ? 0 : (ncells - k0 < chunk ? ncells - k0 : chunk);
        if (have) eval_stage_map(maps, m, map_cells, T, tiles, g.lane, G, status);
        __builtin_amdgcn_wave_barrier();
        {
            MaskT o0, o1, o2;                                            // the level's own planes: kept for the whole item
            planes_from_tiles<MaskT>(P, tiles, (MaskT*)nullptr, have ? g.lane : -1, o0, o1, o2, false);
            keep[0] = o0;
            if (!ONE_PLANE) { keep[G] = o1; keep[2 * G] = o2; }
            int32_t sb[PCGRL_MAX_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
            bool base_needs = false;
            if (have) base_needs = compute_item_stats<PROB>(g, P, o0, o1, o2, row_valid<MaskT>(g.lane, W, H), sb, status);
            if (g.lane == 0) { item[0] = m * ncells + k0; item[1] = kn; }
            if (g.lane == 0 && have) {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    own[k] = k < num_stats(PROB) ? sb[k] : 0;            // (store_stats_row's rule, column by column beside the start row)
                    own[8 + k] = (start_rows && !SEARCH) ? start_rows[(size_t)m * 8 + k] : own[k];
                }
                if (!SEARCH) own[16] = episode_over(P, own, own + 8, PROB) ? 1 : 0;
                if (k0 == 0 && base_rows_out) {                          // (the item with the level's first chunk)
#pragma unroll
                    for (int k = 0; k < 8; k++) base_rows_out[(size_t)m * 8 + k] = own[k];
                    if (SEARCH && base_needs) jobs[atomicAdd(head + EVAL_HEAD_NJOBS, 1)] = entries + m;
                }
            }
        }
        // per cell the T - 1 tiles other than the one it holds, in a turn each: every group of the wavefront has an entry to compute in
        // every turn, whatever tiles their cells hold (a loop over the tile ids would leave the groups whose cell holds tile t idle in
        // turn t: with binary's two tiles half of every turn).  The no-op entry is lane 0's, before the turns.
        for (int k = 0; k < chunk; k++) {
            const bool havek = k < item[1];
            int cell = 0;                                                // y | x << 8 | the tile it holds << 16
            if (havek) {
                const int c = changes_cell(cells, item[0] + k, ncells, map_cells, status), y = c / W;
                cell = y | ((c - y * W) << 8) | ((int)tiles[c] << 16);
            }
            if (G == 64) cell = __builtin_amdgcn_readfirstlane(cell);    // (a wavefront a level: the same in every lane, and so a scalar)
            if (!SEARCH && g.lane == 0 && havek) {                       // (the search problems' no-op entries: k_changes_finish, once the level's row is whole)
                const size_t e = (size_t)((item[0] + k) * T + (cell >> 16));
                if (rows_out) {
#pragma unroll
                    for (int q = 0; q < 8; q++) rows_out[e * 8 + q] = own[q];
                }
                if (reward_out) reward_out[e] = 0.0;
                if (over_out) over_out[e] = (uint8_t)own[16];
            }
            for (int u = 0; u + 1 < T; u++) {
                const int t = u < (cell >> 16) ? u : u + 1;
                int32_t s[PCGRL_MAX_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
                bool need_solver = false;
                if (havek) {
                    MaskT b0 = keep[0], b1 = ONE_PLANE ? (MaskT)0 : keep[G], b2 = ONE_PLANE ? (MaskT)0 : keep[2 * G];
                    if (g.lane == (cell & 255)) planes_set_cell(b0, b1, b2, (cell >> 8) & 255, t);
                    need_solver = compute_item_stats<PROB>(g, P, b0, b1, b2, row_valid<MaskT>(g.lane, W, H), s, status);
                }
                if (g.lane == 0 && havek) {
                    const size_t e = (size_t)((item[0] + k) * T + t);
#pragma unroll
                    for (int q = num_stats(PROB); q < 8; q++) s[q] = 0;  // (store_stats_row's rule, here before the reward reads the row)
                    if (rows_out) {
#pragma unroll
                        for (int q = 0; q < 8; q++) rows_out[e * 8 + q] = s[q];
                    }
                    if (SEARCH) {
                        if (need_solver) jobs[atomicAdd(head + EVAL_HEAD_NJOBS, 1)] = (int32_t)e;
                    } else {
                        if (reward_out) reward_out[e] = compute_reward(P, s, own, PROB);
                        if (over_out) over_out[e] = episode_over(P, s, own + 8, PROB) ? 1 : 0;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                                // (the stage is free for the next round)
    }
}

// k_get_stats_search's job source for pcgrl_get_changes: see the head of this file
struct ChangeJobs {
    const uint8_t* maps;
    const int32_t* cells;
    int32_t* rows;
    int32_t* base_rows;
    int ncells, entries;
    __device__ __forceinline__ void stage(int j, const PcgrlParams& P, int map_cells, uint8_t* stage, int lane, int32_t* status) const {
        const int ntiles = P.ntiles;
        if (j >= entries) { eval_stage_map(maps, j - entries, map_cells, ntiles, stage, lane, 64, status); return; }
        const int t = j % ntiles, col = j / ntiles;
        eval_stage_map(maps, col / ncells, map_cells, ntiles, stage, lane, 64, status);
        const int c = changes_cell(cells, col, ncells, map_cells, nullptr);
        if ((c & 63) == lane) stage[c] = (uint8_t)t;                     // (the lane that staged the byte overwrites it)
    }
    __device__ __forceinline__ int32_t* row(int j) const { return j >= entries ? base_rows + (size_t)(j - entries) * 8 : rows + (size_t)j * 8; }
};

// the search problems' job counter and chunk ticket, zeroed in stream order by a launch (the call issues no memset)
// (templates like k_get_reward<0>: only the part that launches them holds an instance)
template <int UNUSED>
__global__ void k_changes_clear(int32_t* head) {
    if (threadIdx.x == 0) { head[EVAL_HEAD_NJOBS] = 0; head[EVAL_HEAD_TICKET] = 0; }
}

template <int UNUSED>
__global__ __launch_bounds__(256) void k_changes_finish(PcgrlParams P, const uint8_t* __restrict__ maps, const int32_t* __restrict__ cells, int ncells, int entries,
                                                        const int32_t* __restrict__ start_rows, const int32_t* __restrict__ base_rows, int32_t* __restrict__ rows,
                                                        double* __restrict__ reward_out, uint8_t* __restrict__ over_out) {
    const int T = P.ntiles, map_cells = P.width * P.height;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < entries; e += (long long)gridDim.x * 256) {
        const int t = (int)(e % T), col = (int)(e / T), m = col / ncells;
        const int c = changes_cell(cells, col, ncells, map_cells, nullptr);
        const int cur = eval_tile_clamped(maps[(size_t)m * map_cells + c], T);
        int32_t n[PCGRL_MAX_STATS], o[PCGRL_MAX_STATS], sv[PCGRL_MAX_STATS];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            o[q] = base_rows[(size_t)m * 8 + q];
            sv[q] = start_rows ? start_rows[(size_t)m * 8 + q] : o[q];
        }
        if (t == cur) {
#pragma unroll
            for (int q = 0; q < 8; q++) rows[(size_t)e * 8 + q] = n[q] = o[q];
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) n[q] = rows[(size_t)e * 8 + q];
        }
        if (reward_out) reward_out[e] = t == cur ? 0.0 : compute_reward(P, n, o, P.prob);
        if (over_out) over_out[e] = episode_over(P, n, sv, P.prob) ? 1 : 0;
    }
}
