// pcgrl_get_smb_play: the play that smb's jumps / jumps-dist / dist-win describe.  SMBProblem._run_game (smb_prob.py:90-124) asks
// AStarAgent with balance 1 and -- if its node does not win -- with balance 0 for node.getActions() (smb/engine.py:43-49) and keeps the
// game status of the last node returned; this kernel keeps that node's moves (0 stay, 1 right, 2 jump, 3 right + jump: the index
// into engine.directions), its depth and who won (0: balance 1, 1: balance 0, -1: nobody -- the row then leads to the second
// agent's best node, the state dist-win is measured from).  Part of the single translation unit pcgrl_abi.hip.
// k_smb_play is k_smb (kernels_smb.h) outside an episode: persistent blocks of as many wavefronts as the LDS holds, a ticket per
// level, the column masks built from the caller's byte map (tile ids clamped like pcgrl_set_maps / pcgrl_get_stats clamp them), the
// five map statistics, then traced versions of the two searches; while the wavefront's arena still holds the search, lane 0 walks
// the returned node's chain back and writes the row.  It writes nothing of the handle's but the status word.
// What the trace needs on top of the searches:
//  * smb_search_two_label: which of the four children an item is -- different moves often give the same state (right against a
//    wall = stay, a jump without ground = no jump) and the reference returns the move of the child heapq popped first, so the popped
//    item itself carries it: bit 7 (x <= 127 on this path: W + 6 <= 128) and bit 31 (the parent's expansion number needs 14 bits:
//    solver_power < SMB_ROOT_PAR).  The walk over the expansion log that recovers the jump columns stores the moves as well.
//  * smb_search: the children of expansion k are pool nodes 1 + 4k .. 4 + 4k, so node i was made by move (i - 1) & 3 of expansion
//    (i - 1) >> 2; what is missing is that expansion's own node: a log of 16-bit pool indices (a heap word holds no more) beside
//    the arena, and the pool index of the best node.
// The two search bodies repeat smb_search_two_label and smb_search on purpose, for the reason kernels_moves.h gives: k_smb sits
// at its register limit, and one body with a trace policy does not leave its machine code alone.  A change to the searches there has
// to be made here as well.  The traced searches are instantiated in this kernel only.
#pragma once

// bytes of smb_search's expansion log beside one wavefront's arena (host: the workspace plan of pcgrl_get_smb_play)
__host__ __device__ __forceinline__ size_t smb_play_log_bytes(int power) { return ((size_t)power * 2 + 255) & ~(size_t)255; }

// where a walk stores: moves[d] for d < max_len only (the host fills the rows with -1 before the launch)
struct SmbPlayRow { int8_t* moves; int max_len; };

// smb_search (kernels_smb.h) with the log `elog[expansion] = pool index of the expanded node`; node / depth: the returned node's
// pool index and depth.  Lanes 0..3, everything uniform across them.
__device__ __forceinline__ void smb_search_traced(const SmbCols& C, int h, int exit_x, const SmbState& root, int balance, int power, uint2* pool, const SmbHeap& H,
                                                  uint32_t* visited, uint16_t* elog, SmbResult& out, int& node, int& depth, int lane) {
    const int ky = h + SMB_YOFF + 1;
    int npool = 1, heapn = 1, iterations = 0, nexp = 0;
    pool[0] = smb_pack(root);
    H.set(0, ((uint32_t)(exit_x - root.x) << 16) | 0u);
    bool have_best = false, win = false;
    SmbState best = root;
    int best_idx = 0;
    uint2 ahead = pool[0];
    int ahead_idx = 0;
    uint2 kid0 = ahead, kid1 = ahead, kid2 = ahead, kid3 = ahead;
    int kid_base = -8;
    while (iterations < power && heapn > 0) {
        iterations++;
        const uint32_t top = H.get(0), last = H.get(--heapn);
        const int cur = (int)(top & 0xFFFFu);
        uint2 raw;
        const unsigned kd = (unsigned)(cur - kid_base);
        if (cur == ahead_idx) raw = ahead;
        else if (kd < 4u) raw = kd == 0 ? kid0 : (kd == 1 ? kid1 : (kd == 2 ? kid2 : kid3));
        else raw = pool[cur];
        ahead_idx = -1;
        if (heapn > 0) {
            H.set(0, last);
            smb_siftup_root(H, heapn);
            ahead_idx = (int)(H.get(0) & 0xFFFFu);
            const unsigned ka = (unsigned)(ahead_idx - kid_base);
            ahead = ka < 4u ? (ka == 0 ? kid0 : (ka == 1 ? kid1 : (ka == 2 ? kid2 : kid3))) : pool[ahead_idx];
        }
        raw.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw.x);
        raw.y = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw.y);
        const SmbState s = smb_unpack(raw);
        if (s.y >= h) continue;                                       // checkLose
        if (s.x >= exit_x) { win = true; best = s; best_idx = cur; break; }   // checkWin
        const int key = (s.x * ky + (s.y + SMB_YOFF)) * 5 + s.air;
        const uint32_t bit = 1u << (key & 31);
        const uint32_t word = visited[key >> 5];
        if (word & bit) continue;
        visited[key >> 5] = word | bit;
        const int hh = exit_x - s.x, bh = exit_x - best.x;
        if (!have_best || hh < bh || (hh == bh && s.depth < best.depth)) { have_best = true; best = s; best_idx = cur; }
        kid_base = npool;                                             // = 1 + 4 * nexp
        elog[nexp++] = (uint16_t)cur;                                 // (nexp < power: one expansion per pop at most)
        uint32_t wx, wx1;
        smb_window<4>(C, s.x, s.y, wx, wx1);
        const uint2 mine = smb_pack(smb_child_win(s, lane & 3, wx, wx1, h));
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint2 pk;
            pk.x = (uint32_t)__builtin_amdgcn_readlane((int)mine.x, d);
            pk.y = (uint32_t)__builtin_amdgcn_readlane((int)mine.y, d);
            if (d == 0) kid0 = pk; else if (d == 1) kid1 = pk; else if (d == 2) kid2 = pk; else kid3 = pk;
            pool[npool] = pk;
            const int cx = (int)(pk.x & 255u), cdepth = (int)(pk.x >> 17);
            H.set(heapn, ((uint32_t)((exit_x - cx) + balance * cdepth) << 16) | (uint32_t)npool);
            heapn++;
            smb_siftdown(H, heapn - 1);
            npool++;
        }
    }
    out.won = win ? 1 : 0;
    out.jumps = best.jumps; out.prev_jump_x = best.prev_jump_x; out.max_gap = best.max_gap; out.x = best.x; out.iters = iterations;
    node = best_idx; depth = best.depth;
}
// node.getActions() of pool node `node` (depth `depth`) of the search above, by one lane: every index read was written by that
// search (a child's index gives its expansion, the log that expansion's node), the chain ends at pool node 0 after `depth` steps
__device__ __forceinline__ void smb_play_walk_pool(const uint16_t* elog, int node, int depth, const SmbPlayRow& row) {
    for (int d = depth - 1; d >= 0 && node > 0; d--) {
        if (d < row.max_len) row.moves[d] = (int8_t)((node - 1) & 3);
        node = (int)elog[(node - 1) >> 2];
    }
}

// smb_search_two_label (kernels_smb.h) whose items carry their move -- bit 7: right, bit 31: jump; x is bits 0..6, the parent bits
// 17..30 --, and whose closing walk over the ancestors stores the moves (lane 0) beside counting the jumps.  depth: the result's.
#define SMB_PLAY_X(item) ((int)((item) & 127u))
#define SMB_PLAY_PAR(item) (((item) >> 17) & SMB_ROOT_PAR)
__device__ __forceinline__ int smb_search_two_label_traced(const SmbCols& C, int h, int exit_x, int root_x, int root_y, int power, const SmbItems& ent, int cap,
                                                           uint32_t* visited, uint32_t* log, SmbResult& out, int& res_depth, const SmbPlayRow& row, int lane) {
    const int ky = h + SMB_YOFF + 1;
    SmbLab lab = {0u, 0u};
    int n = 1, u = 1, iterations = 0, nexp = 0, fmin = exit_x - root_x;
    const uint32_t root = (uint32_t)root_x | ((uint32_t)(root_y + SMB_YOFF) << 8) | (SMB_ROOT_PAR << 17);
    if (lane == 0) ent.lds[1] = root;
    bool have_best = false;
    int status = 0, best_x = root_x, best_depth = 0;
    uint32_t res = root;
    while (iterations < power && n > 0) {
        iterations++;
        uint32_t rp = ent.lds[1];
        const uint32_t lastp = ent.get(n);
        const bool relabel = (smb_lab_word(lab, 0) & 2u) != 0;
        if (relabel) { lab.a = 0u; lab.b = 0u; fmin++; }
        const int ll = smb_lab_get(lab, n);
        const int nold = n;
        n--;
        if (n > 0) {
            if (relabel) u = smb_rightmost_leaf(1, n);
            else if (u == nold) u = smb_chain_remove_end(lab, nold, n);
            const int leaf = ll ? smb_rightmost_leaf(u, n) : u, k = 31 - __builtin_clz(leaf);
            uint32_t mv = lastp;
            const bool act = lane < k;
            if (act) mv = ent.get(leaf >> (k - lane - 1));
            __builtin_amdgcn_wave_barrier();
            if (act) ent.lds[leaf >> (k - lane)] = mv;
            if (lane == 0) ent.set(leaf, lastp);
            if (ll) {
                smb_lab_set(lab, u, 1, lane);
                u = smb_chain_remove_end(lab, u, n);
            }
        } else {
            u = 0;
        }
        rp = (uint32_t)__builtin_amdgcn_readfirstlane((int)rp);
        const int x = SMB_PLAY_X(rp), y = (int)((rp >> 8) & 63u) - SMB_YOFF, air = (int)((rp >> 14) & 7u);
        if (y >= h) continue;                                                   // checkLose
        const int depth = fmin - (exit_x - x);                                  // the popped item's label is 0
        if (x >= exit_x) { status = 1; res = rp; best_depth = depth; break; }   // checkWin
        const int key = (x * ky + (y + SMB_YOFF)) * 5 + air;
        const uint32_t bit = 1u << (key & 31);
        const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)visited[key >> 5]);
        if (word & bit) continue;
        if (lane == 0) visited[key >> 5] = word | bit;
        const int hh = exit_x - x, bh = exit_x - best_x;
        if (!have_best || hh < bh || (hh == bh && depth < best_depth)) { have_best = true; best_x = x; best_depth = depth; res = rp; }
        if (n + 4 > cap) { status = 2; break; }
        if (lane == 0) log[nexp] = rp;
        uint32_t wx, wx1;
        smb_window<2>(C, x, y, wx, wx1);
        SmbState s = {x, y, air, 0, 0, 0, 0};
        const int d = lane & 3;
        s = smb_child_win(s, d, wx, wx1, h);
        const uint32_t mine = (uint32_t)s.x | ((uint32_t)(d & 1) << 7) | ((uint32_t)(s.y + SMB_YOFF) << 8) | ((uint32_t)s.air << 14) | ((uint32_t)nexp << 17) |
                              ((uint32_t)(d >> 1) << 31);
        nexp++;
        if (lane < 4) ent.set(n + 1 + lane, mine);
        const bool canr = !((wx1 >> 1) & 1u);
        {
            const int q0 = n + 1, sh = q0 & 31, w0 = q0 >> 5;
            const uint64_t msk = 0xFull << sh, pat = (canr ? 0x5ull : 0xFull) << sh;
            const uint32_t m_lo = (uint32_t)msk, m_hi = (uint32_t)(msk >> 32), p_lo = (uint32_t)pat, p_hi = (uint32_t)(pat >> 32);
            const bool own0 = lane == (w0 & 63), own1 = lane == ((w0 + 1) & 63);
            const uint32_t c0 = own0 ? m_lo : 0u, s0 = own0 ? p_lo : 0u, c1 = own1 ? m_hi : 0u, s1 = own1 ? p_hi : 0u;
            const bool a0 = w0 < 64, a1 = w0 + 1 < 64;
            lab.a = (lab.a & ~((a0 ? c0 : 0u) | (a1 ? c1 : 0u))) | (a0 ? s0 : 0u) | (a1 ? s1 : 0u);
            lab.b = (lab.b & ~((a0 ? 0u : c0) | (a1 ? 0u : c1))) | (a0 ? 0u : s0) | (a1 ? 0u : s1);
        }
        n += 4;
        if (canr) {
            u = smb_chain_add(u, smb_climb(lab, ent, n - 2, (uint32_t)__builtin_amdgcn_readlane((int)mine, 1), lane));
            u = smb_chain_add(u, smb_climb(lab, ent, n, (uint32_t)__builtin_amdgcn_readlane((int)mine, 3), lane));
        }
    }
    // the result's ancestors, newest first: jump_locs as in smb_search_two_label, and -- for a winner: the play of a first agent that
    // does not win is never the one returned -- the move that made each of them at its depth.
    // Every log index read is a parent field that an expansion of this search wrote (< nexp); the chain ends at the root's
    // SMB_ROOT_PAR after best_depth steps.
    int jumps = 0, later = -1, max_gap = 0, prev_jump_x = 0;
    if (status != 2) {
        __threadfence_block();
        uint32_t node = res;
        for (int d = best_depth - 1; d >= 0; d--) {
            const uint32_t par = SMB_PLAY_PAR(node);
            if (par == SMB_ROOT_PAR || par >= (uint32_t)nexp) break;
            const uint32_t pe = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&log[par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (lane == 0 && status == 1 && d < row.max_len) row.moves[d] = (int8_t)(((node >> 7) & 1u) | ((node >> 31) << 1));
            if (((node >> 14) & 7u) == 4u) {
                const int jx = SMB_PLAY_X(pe);
                jumps++;
                if (later < 0) prev_jump_x = jx;
                else max_gap = later - jx > max_gap ? later - jx : max_gap;
                later = jx;
            }
            node = pe;
        }
        if (later > max_gap) max_gap = later;
    }
    out.won = status == 1; out.jumps = jumps; out.prev_jump_x = prev_jump_x; out.max_gap = max_gap; out.x = SMB_PLAY_X(res); out.iters = iterations;
    res_depth = best_depth;
    return status;
}

// One level by one wavefront: smb_job (kernels_smb.h) without an episode around it.  `m`: the caller's tile bytes.
__device__ __forceinline__ void smb_play_job(const PcgrlParams& P, const SmbWave& S, uint16_t* elog, const uint8_t* __restrict__ m, int32_t* status_word, int32_t* row_out,
                                             const SmbPlayRow& row, int32_t* length_out, int8_t* agent_out, int lane) {
    const int W = P.width, Hh = P.height, cells = W * Hh;
    const int ew = W + 6;
    const int exit_x = Hh > 3 ? W + 4 : -1;
    const int top_tile = P.ntiles - 1;
#define SMB_PLAY_TILE(c) ((int)m[c] > top_tile ? top_tile : (int)m[c])
    // ---- the five statistics of the byte map, as smb_job computes them
    int c_floor = 0, c_tubes = 0, c_enemy = 0, c_empty = 0, c_noise = 0;
    bool bad = false;
    for (int c = lane; c < cells; c += 64) {
        const int y = c / W, x = c - y * W;
        bad |= (int)m[c] > top_tile;
        const int tl = SMB_PLAY_TILE(c);
        c_empty += tl == 0;
        c_enemy += tl == 2;
        if (x > 0) c_noise += tl != SMB_PLAY_TILE(c - 1);
        if (y > 0) c_noise += tl != SMB_PLAY_TILE(c - W);
        if (tl == 6) {
            const int v = (x > 0 && SMB_PLAY_TILE(c - 1) == 6) + (x < W - 1 && SMB_PLAY_TILE(c + 1) == 6);
            c_tubes += v == 1;
        }
        if (tl == 2) {
            int r = Hh - 1;
            for (int dy = 0; y + dy < Hh; dy++) {
                const int tb = SMB_PLAY_TILE(c + dy * W);
                if (tb == 1 || tb == 3 || tb == 4) { r = dy - 1; break; }
            }
            c_floor += r;
        }
    }
    if (bad) atomicOr(status_word, PCGRL_STATUS_BAD_TILE);
    for (int o = 32; o > 0; o >>= 1) {
        c_floor += __shfl_xor(c_floor, o, 64); c_tubes += __shfl_xor(c_tubes, o, 64); c_enemy += __shfl_xor(c_enemy, o, 64);
        c_empty += __shfl_xor(c_empty, o, 64); c_noise += __shfl_xor(c_noise, o, 64);
    }
    // ---- the engine's grid as column masks: lane l holds columns l + 64 k
    SmbCols C;
    {
        uint64_t col[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int ex = 64 * k + lane;
            uint64_t c = ~0ull << (Hh + SMB_YOFF);
            if (ex < ew) {
                for (int y = 0; y < Hh; y++) {
                    bool sol;
                    if (ex < 3) sol = y > Hh - 3;
                    else if (ex >= W + 3) sol = y > Hh - 3 || (y == Hh - 3 && ex == W + 4);
                    else { const int tl = SMB_PLAY_TILE(y * W + ex - 3); sol = tl == 1 || tl == 3 || tl == 4 || tl == 6; }
                    c |= (uint64_t)sol << (y + SMB_YOFF);
                }
            } else {
                c = ~0ull << SMB_YOFF;
            }
            col[k] = c;
        }
        C.c0 = col[0]; C.c1 = col[1]; C.c2 = col[2]; C.c3 = col[3];
    }
#undef SMB_PLAY_TILE
    // ---- SMBProblem._run_game
    const bool two_label = ew <= 128 && P.solver_power < (int)SMB_ROOT_PAR;
    uint2* pool = reinterpret_cast<uint2*>(S.arena);
    const SmbHeap HP = {S.heap, reinterpret_cast<uint32_t*>(S.arena + (4 * (size_t)P.solver_power + 4) * 8), S.lds_heap_n};
    const SmbItems items = {S.heap, HP.glob, S.lds_heap_n};
    const int cap = S.lds_heap_n >= 2048 ? 4095 : S.lds_heap_n - 1;
    SmbResult res = {0, 0, 0, 0, 1, 0};
    int length = 0, winner = -1;
#pragma clang loop unroll(disable)
    for (int agent = 0; agent < 2 && !res.won; agent++) {
        for (int i = lane; i < S.vis_words; i += 64) S.visited[i] = 0;
        __threadfence_block();
        int status = 2;
        if (agent == 0 && two_label) {
            status = smb_search_two_label_traced(C, Hh, exit_x, 1, Hh - 3, P.solver_power, items, cap, S.visited, reinterpret_cast<uint32_t*>(S.arena), res, length, row, lane);
            __threadfence_block();
            if (status == 2) {
                for (int i = lane; i < S.vis_words; i += 64) S.visited[i] = 0;
                __threadfence_block();
            }
        }
        if (status == 2) {
            int node = 0;
            if (lane < 4) {
                const SmbState root = {1, Hh - 3, 0, 0, 0, 0, 0};
                smb_search_traced(C, Hh, exit_x, root, agent == 0 ? 1 : 0, P.solver_power, pool, HP, S.visited, elog, res, node, length, lane);
                if (lane == 0 && (res.won || agent == 1)) smb_play_walk_pool(elog, node, length, row);
            }
            res.won = __shfl(res.won, 0, 64); res.jumps = __shfl(res.jumps, 0, 64); res.prev_jump_x = __shfl(res.prev_jump_x, 0, 64);
            res.max_gap = __shfl(res.max_gap, 0, 64); res.x = __shfl(res.x, 0, 64); res.iters = __shfl(res.iters, 0, 64);
            length = __shfl(length, 0, 64);
            __threadfence_block();
        }
        if (res.won) winner = agent;
    }
    if (lane == 0) {
        const int dist_win = res.won ? 0 : exit_x - res.x;
        const int tail = P.prob_width - res.prev_jump_x;              // smb_prob.py:145
        const int jumps_dist = res.max_gap > tail ? res.max_gap : tail;
        row_out[0] = c_floor; row_out[1] = c_tubes; row_out[2] = c_enemy; row_out[3] = c_empty; row_out[4] = c_noise;
        row_out[5] = res.jumps; row_out[6] = jumps_dist; row_out[7] = dist_win;
        *length_out = length;
        if (agent_out) *agent_out = (int8_t)winner;
    }
}

// `ticket` (zeroed by the host) hands the levels out, a wavefront at a time.  arenas: `wave_stride` bytes per wavefront of the
// launch (wavefront wv of block b: number b * waves_per_block + wv) = smb_wave_arena_bytes, then smb_play_log_bytes for the log.
template <int PART_TAG>
__global__ __launch_bounds__(SMB_MAX_WAVES * 64) void k_smb_play(PcgrlParams P, const uint8_t* __restrict__ maps, int count, int32_t* __restrict__ rows_out, SolOut out,
                                                                 int32_t* status, int32_t* ticket, uint8_t* arenas, size_t wave_stride, int waves_per_block,
                                                                 int lds_heap_n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smb_lds[];       // per wavefront: heap (lds_heap_n words), then the visited bitmap
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cells = P.width * P.height;
    const int vis_words = ((P.width + 6) * (P.height + SMB_YOFF + 1) * 5 + 31) / 32;
    uint32_t* my_lds = smb_lds + (size_t)wv * (lds_heap_n + ((vis_words + 3) & ~3));
    uint8_t* arena = arenas + ((size_t)blockIdx.x * waves_per_block + wv) * wave_stride;
    const SmbWave S = {my_lds, my_lds + lds_heap_n, arena, lds_heap_n, vis_words};
    uint16_t* elog = reinterpret_cast<uint16_t*>(arena + smb_wave_arena_bytes(P.solver_power));
    for (;;) {
        int t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1);
        t = __shfl(t, 0, 64);
        if (t >= count) break;
        const SmbPlayRow row = {out.moves + (size_t)t * out.max_len, out.max_len};
        smb_play_job(P, S, elog, maps + (size_t)t * cells, status, rows_out + (size_t)t * 8, row, out.length + t, out.agent ? out.agent + t : nullptr, lane);
        __builtin_amdgcn_wave_barrier();
    }
}
