/*
 * pcgrl_hip.h -- C ABI of the MI355X batched PCGRL environment (libpcgrl_hip.so).
 *
 * The reference (amidos2006/gym-pcgrl) has no FFI of its own: its hot path sits behind a Python
 * class.  This ABI is what a replacement for that path binds.  Each entry point names the
 * reference interface it replaces (paths relative to gym_pcgrl/envs/):
 *
 *   pcgrl_create / pcgrl_configure   PcgrlEnv.__init__ pcgrl_env.py:27-42, adjust_param :106-115,
 *                                    Problem/Representation.adjust_param (probs/problem.py:66-72,
 *                                    binary_prob.py:49-59, zelda_prob.py:59-71, sokoban_prob.py:60-73, mdungeon_prob.py:68-84,
 *                                    ddave_prob.py:67-82, smb_prob.py:40-53,
 *                                    reps/representation.py:53-54, narrow_rep.py:86-88, turtle_rep.py:42-44)
 *   pcgrl_seed                       PcgrlEnv.seed pcgrl_env.py:54-57 (host passes MT19937 keys)
 *   pcgrl_reset                      PcgrlEnv.reset pcgrl_env.py:66-76 for every environment
 *   pcgrl_step                       PcgrlEnv.step pcgrl_env.py:129-150 for every environment, plus the
 *                                    vector-env auto-reset the reference delegates to SubprocVecEnv (utils.py:60-71)
 *   pcgrl_set_tile_probs             Problem.adjust_param(probs=...) probs/problem.py:68-72
 *   pcgrl_set_maps                   direct assignment of Representation._map (tests, curriculum loaders)
 *   pcgrl_get_stats / pcgrl_get_reward   Problem.get_stats / get_reward / get_episode_over called on any level, outside an episode
 *   pcgrl_get_solution               SokobanProblem.get_stats(map)["solution"] sokoban_prob.py:133-145: the planner's moves
 *   pcgrl_get_playthrough            the moves of the play _run_game scores, mdungeon_prob.py:100-138 / ddave_prob.py:92-127
 *   pcgrl_get_smb_play               the same for smb's two agents, smb_prob.py:90-124
 *   pcgrl_get_paths                  the cells of the paths that binary's path-length (helper.py:250-264) and zelda's path-length /
 *                                    nearest-enemy (zelda_prob.py:91-110) measure, from the run_dikjstra maps (helper.py:222-237)
 *   pcgrl_tile_graph                 helper.py:170-296 for any tile set: calc_num_regions with its color_map, calc_longest_path,
 *                                    run_dikjstra's map, calc_num_reachable_tile -- what a custom Problem builds its get_stats from
 *   pcgrl_tile_local                 helper.py:37-137 for any tile set: get_floor_dist, get_type_grouping, get_changes with their
 *                                    per-cell maps, on every map size and problem
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * PCGRL_E* code (no exceptions cross the ABI); all device buffers are OWNED BY THE CALLER (hipMalloc,
 * or a torch tensor's data_ptr()) and described by pcgrl_layout; launches are asynchronous on the
 * given hipStream_t (passed as void*); one handle per GPU, one host thread per handle.
 * There is no CPU fallback: without a HIP device every launch returns PCGRL_EHIP.
 */
#ifndef PCGRL_HIP_H
#define PCGRL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: + pcgrl_bind_episode_stats.  3: planes buffer laid out [N,group,nplanes] (was [N,nplanes,group]); + pcgrl_seed_words.
 * 4: + the mdungeon problem: pcgrl_config grew (max_potions, max_treasures, target_col_enemies, rewards[12]).
 * 5: + the ddave problem: pcgrl_config grew (max_diamonds, min_spikes, target_jumps).  6: + pcgrl_rollout.
 * 7: + the smb problem: pcgrl_config grew (min_empty, min_enemies, min_jumps; `reserved_` is gone); pcgrl_status reports
 *    clamped actions.  10: + pcgrl_tuning / pcgrl_set_tuning (the library reads no environment variables any more); pcgrl_config
 *    grew (prob_width, prob_height); maps up to 255 x 255, search levels up to 16 384 bordered cells, solver_power up to 1 000 000.
 * 15: without auto_reset the heat map holds 32-bit counts (an episode goes on past done); max_changes beyond 65 535 there.
 *     Still 15: + pcgrl_row / pcgrl_bind_row -- purely additive (one struct, one entry point; no existing struct or signature
 *     changed), so the number stays; a caller detects the feature by the symbol pcgrl_bind_row.
 *     Still 15: + pcgrl_render_desc / pcgrl_render -- additive in the same way; a caller detects it by the symbol pcgrl_render.
 *     Still 15: + pcgrl_get_stats_bytes / pcgrl_get_stats / pcgrl_get_reward -- additive in the same way (three entry points, no struct);
 *     a caller detects them by the symbol pcgrl_get_stats.
 *     Still 15: + pcgrl_get_solution_bytes / pcgrl_get_solution -- additive in the same way; detected by the symbol pcgrl_get_solution.
 *     Still 15: + pcgrl_get_playthrough_bytes / pcgrl_get_playthrough -- additive in the same way; detected by the symbol
 *     pcgrl_get_playthrough.
 *     Still 15: + pcgrl_get_smb_play_bytes / pcgrl_get_smb_play -- additive in the same way; detected by the symbol pcgrl_get_smb_play.
 *     Still 15: + pcgrl_get_paths_legs / pcgrl_get_paths_bytes / pcgrl_get_paths -- additive in the same way; detected by the symbol
 *     pcgrl_get_paths.
 *     Still 15: + pcgrl_get_changes_bytes / pcgrl_get_changes -- additive in the same way; detected by the symbol pcgrl_get_changes.
 *     Still 15: + pcgrl_tile_graph_desc / pcgrl_tile_graph_bytes / pcgrl_tile_graph -- additive in the same way (one struct, two entry
 *     points); detected by the symbol pcgrl_tile_graph.
 *     Still 15: + pcgrl_tile_local_desc / pcgrl_tile_local_bytes / pcgrl_tile_local -- additive in the same way (one struct, two entry
 *     points); detected by the symbol pcgrl_tile_local.
 *     The developer switches pcgrl_tuning grew at their end (changes_grid, changes_chunk): fill them with pcgrl_tuning_defaults. */
#define PCGRL_ABI_VERSION 15
#define PCGRL_OK 0
#define PCGRL_EINVAL (-1)   /* bad argument / unsupported configuration */
#define PCGRL_EHIP (-2)     /* a HIP runtime call failed (see pcgrl_last_hip_error) */
#define PCGRL_ESTATE (-3)   /* call order violated (e.g. step before bind/reset) */

enum { PCGRL_BINARY = 0, PCGRL_ZELDA = 1, PCGRL_SOKOBAN = 2, PCGRL_MDUNGEON = 3, PCGRL_DDAVE = 4, PCGRL_SMB = 5 };
enum { PCGRL_NARROW = 0, PCGRL_WIDE = 1, PCGRL_TURTLE = 2, PCGRL_NARROW_CAST = 3, PCGRL_NARROW_MULTI = 4, PCGRL_TURTLE_CAST = 5 };

/* Batch-wide parameters (everything the reference keeps as attributes of PcgrlEnv/Problem/Representation). */
typedef struct pcgrl_config {
    int32_t prob, rep;
    int32_t num_envs;
    int32_t width, height;                 /* the maps' width / height: 1..255 each (search problems: (width + 2) * (height + 2) <= 16384;
                                              smb: width up to 250, height 3..32).  Up to 64 x 64 the row-bitboard kernels, beyond
                                              them the general path (csrc/bigmap.h) */
    int32_t prob_width, prob_height;       /* Problem._width/_height when they differ from the maps' -- adjust_param(width, height)
                                              without a reset(): the reference goes on stepping the old maps with the problem's new
                                              size in its formulas (pcgrl_env.py:106-115, zelda_prob.py:99); 0 = same as width / height */
    int32_t max_changes, max_iterations;   /* pcgrl_env.py:33-34 / :108-110, computed by the host */
    int32_t random_start, random_tile, warp, random_probs;
    int32_t auto_reset;                    /* 1: a done env is reset inside step (vector-env semantics) */
    int32_t target_path;                   /* binary 20, zelda 16 */
    int32_t max_enemies, target_enemy_dist;            /* zelda (max_enemies: mdungeon and smb too) */
    int32_t max_crates, target_solution, solver_power; /* sokoban (target_solution, solver_power: mdungeon too) */
    int32_t max_potions, max_treasures;                /* mdungeon */
    int32_t max_diamonds, min_spikes, target_jumps;    /* ddave (+ target_solution, solver_power) */
    int32_t min_empty, min_enemies, min_jumps;         /* smb (+ max_enemies, solver_power) */
    double target_col_enemies;                         /* mdungeon */
    double tile_probs[8];                  /* Problem._prob in tile order (un-normalised) */
    double rewards[12];                    /* Problem._rewards in the problem's own key order */
} pcgrl_config;

/* Byte sizes of the caller-provided device buffers for a configuration (N = num_envs). */
typedef struct pcgrl_layout {
    int32_t group;        /* lanes per map: 16 (height <= 16) or 64 */
    int32_t mask_bytes;   /* bytes per row mask: 4 (width <= 32) or 8 */
    int32_t nplanes;      /* bit planes of the tile id: 1 binary, 3 zelda/sokoban/mdungeon/ddave, 0 smb (statistics from the byte map) */
    int32_t nstats;       /* used slots of a stats row: 2 binary, 7 zelda, 6 sokoban, 8 mdungeon / ddave (packed, see below), 8 smb */
    size_t map;           /* u8  [N,H,W]   observation "map" */
    size_t old_map;       /* u8  [N,H,W]   Representation._old_map */
    size_t heatmap;       /* i16 [N,H,W]   observation "heatmap" (counts; auto_reset: at most max_changes <= 65 535, read as u16);
                                 i32 [N,H,W] without auto_reset (stepping past done: unbounded counts) */
    size_t pos;           /* u8  [N,2]     observation "pos" (x,y); unused for wide */
    size_t planes;        /* mask[N,group,nplanes] row bitboards of the tile-id bits (the planes of a row are adjacent) */
    size_t counters;      /* i32 [N,2]     iteration, changes */
    size_t stats;         /* i32 [N,8]     current _rep_stats.  mdungeon keeps its eleven values in eight slots:
                                            player, exit, potions, treasures, enemies, regions, then slot 6 = sol-length if
                                            the planner won else dist-win, slot 7 = col-potions | col-treasures << 8 |
                                            col-enemies << 16 | won << 24; ddave likewise: player | exit << 8 | key << 16,
                                            dist-floor, diamonds, spikes, regions, num-jumps, then slot 6 = sol-length if the
                                            planner won else dist-win, slot 7 = col-diamonds | won << 24 */
    size_t start_stats;   /* i32 [N,8]     Problem._start_stats */
    size_t info;          /* i32 [N,10]    per-step info: stats[8], iterations, changes */
    size_t reward;        /* f64 [N] */
    size_t done;          /* u8  [N] */
    size_t tile_p;        /* f64 [N,2]     binary: per-env (p_empty, p_solid) */
    size_t rng_rep;       /* u32 [N,624]   representation MT19937 ring */
    size_t rng_prob;      /* u32 [N,624]   problem MT19937 ring (binary only; may be NULL otherwise) */
    size_t rng_cursor;    /* i32 [N,2]     ring cursors (rep, prob) */
    size_t scratch;       /* work lists, counters, sokoban solver arena */
} pcgrl_layout;

typedef struct pcgrl_buffers {
    void *map, *old_map, *heatmap, *pos, *planes, *counters, *stats, *start_stats, *info, *reward,
         *done, *tile_p, *rng_rep, *rng_prob, *rng_cursor, *scratch;
} pcgrl_buffers;

typedef struct pcgrl_env pcgrl_env;

/* Developer switches: which of several equivalent kernels / schedules a handle uses.  Every setting gives the same results (the
 * tests run the alternatives against the same fixtures); they exist for A/B measurements and to force the rarely taken paths in
 * tests.  A negative field = the library's default (pcgrl_tuning_defaults sets them all).  Set with pcgrl_set_tuning between
 * pcgrl_create and pcgrl_bind; the library reads no environment variables and keeps no process-wide state. */
typedef struct pcgrl_tuning {
    int32_t no_fused;        /* 1: binary / zelda steps as k_update + k_stats instead of the one-launch k_step */
    int32_t fused_zelda;     /* 0: zelda steps as two launches (binary unaffected) */
    int32_t step_epb;        /* environments per block of k_step: 64, 128 or 256 (default: from the batch size) */
    int32_t no_inc;          /* 1: no incremental statistics -- every change recomputes */
    int32_t inline_reset;    /* 0: resets through the reset list + k_reset instead of inside the statistics kernel */
    int32_t pair_min;        /* certain resets per launch from which a wavefront of k_stats takes two (default 2048) */
    int32_t no_wide;         /* 1: tall binary maps (17..64 rows) on one wavefront per map instead of k_stats_wide */
    int32_t wide_waves;      /* wavefronts per tall map: 4 or 8 (default 8) */
    int32_t wide_grid;       /* blocks of k_stats_wide (default 2048) */
    int32_t wide_pairs;      /* 0: every full item of a tall map a block of its own */
    int32_t wide_few;        /* region count up to which a tall map's full item takes half a block (default 32) */
    int32_t sok_generic;     /* 1: every Sokoban / MiniDungeons / Dave level takes the generic (not the register-resident) search */
    int32_t sok_hard_cap;    /* levels k_sokoban may publish to idle blocks per launch (default 4096) */
    int32_t sok_spawn;       /* pops after which a Sokoban BFS publishes its level (default 128) */
    int32_t md_only_agent;   /* >= 0: the MiniDungeons planner runs only this agent (timing experiments: results are then wrong) */
    int32_t smb_lds_heap;    /* heap words a k_smb search keeps in LDS (default 2048; tests: the overflow path) */
    int32_t full_per_wave;   /* k_step: maps of full recomputations per wavefront task: 1, 2 or 4 */
    int32_t inc_per_wave;    /* k_step: incremental items per wavefront task: 1, 2 or 4 */
    int32_t wide_spin;       /* k_stats_wide: sleeps a reset's block waits for its partner block before it computes the old map's statistics
                                itself (default 400, ~50 us; tests: 1 forces the take-over path) */
    int32_t step_prio;       /* k_step: s_setprio levels of the wavefronts by what they do, two bits each: bits 0-1 a certain reset, 2-3 a full
                                recomputation, 4-5 an incremental update, 6-7 the update wavefronts; bits 8-11: how many of the leading
                                (dearest) full tasks of a block get the level of bits 2-3 (0 = all of them) */
    int32_t no_touch;        /* 1: k_step recomputes the binary statistics in full when a change is in or next to the champion component
                                (default 0: binary_touch first -- the champion's pieces / its union with the cell and one double sweep) */
    int32_t touch_tight;     /* where a full computation also sweeps the second largest component, for a tight bound on "the others": bit 0 the
                                recomputations of a step, bit 1 the resets (default 1) */
    int32_t step_pair;       /* k_step, zelda: from this many certain resets in a block's step on, a wavefront takes two of them (default 6; 0: never) */
    int32_t async_split;     /* pcgrl_step_async: 1 = the fresh jobs of a tick in a launch of their own with small search regions, several blocks per
                                compute unit (the default for sokoban); 0 = one search launch per tick, the full region for every job */
    int32_t big_team;        /* k_big, binary maps beyond 64 x 64: 1 = a step's few full recomputations are made by all wavefronts of a block
                                together (csrc/bigmap_team.h; the default: four wavefronts a block), 2..8 = that many, 0 = a wavefront
                                per map throughout */
    int32_t obs_at_end;      /* k_step with a bound observation (pcgrl_bind_observation): 1 = every image at the end of the launch (the form up to
                                round 5); default 0 = the images leave while the step runs -- a reset's wavefront writes its new map's, a wide
                                change's lane its piece, "observation tasks" between the statistics tasks the rest (csrc/kernels_step.h) */
    int32_t touch_resume;    /* k_step, binary, maps of at most 16 x 32: 0 = a change to the champion that binary_touch gives up on is computed
                                from scratch; default 1 = the computation resumes from what the touch found (csrc/pcgrl_algos.h rlp_resume).
                                Wider maps (64-bit row masks) and the two-launch pipeline, which has no touch, always compute from scratch */
    int32_t changes_grid;    /* pcgrl_get_changes: blocks of k_get_changes at most (default 8192; tests: 1 = one block walks every item) */
    int32_t changes_chunk;   /* pcgrl_get_changes: cells of a level per work item (default: chosen from count and ncells, csrc/pcgrl_abi.hip
                                changes_chunk) */
} pcgrl_tuning;

int pcgrl_abi_version(void);
const char* pcgrl_error_string(int code);
int pcgrl_last_hip_error(void);

int pcgrl_query_layout(const pcgrl_config* cfg, pcgrl_layout* out);
int pcgrl_create(const pcgrl_config* cfg, pcgrl_env** out);
int pcgrl_destroy(pcgrl_env* env);
void pcgrl_tuning_defaults(pcgrl_tuning* t);
int pcgrl_set_tuning(pcgrl_env* env, const pcgrl_tuning* t);   /* between pcgrl_create and pcgrl_bind (PCGRL_ESTATE afterwards) */
int pcgrl_bind(pcgrl_env* env, const pcgrl_buffers* bufs, void* stream);
/* Change parameters that do not alter buffer sizes (anything but prob/rep/num_envs/width/height).  A host call: nothing is launched
 * and no buffer is touched.  On a handle that has been stepped the next step / rollout / tick runs under the new parameters, like
 * PcgrlEnv.adjust_param between two steps: limits, targets and reward weights apply to the steps that follow (the counters, heat maps,
 * current and start statistics of the running episodes stay), tile probabilities to the resets that follow (binary: after
 * pcgrl_set_tile_probs), and a solver_power that is not larger than the one the handle was bound with to every search that follows.
 * The current statistics are never recomputed here: an unchanged environment keeps the row of its last change, as in the reference.
 * smb: the rows hold play-through results (jumps, jumps-dist, dist-win) that the step kernels carry over a change the play-through
 * cannot see; after a call that changes solver_power every environment's next change is played through again with the new value,
 * whatever it touches, so no row is ever derived from a play-through under another solver_power than the one in force at that change.
 * PCGRL_EINVAL, and nothing changed: a solver_power beyond the bound one, or one that moves the searches to the general kernels --
 * create and bind a new handle.  A caller that steps asynchronously (pcgrl_step_async) calls pcgrl_async_flush first. */
int pcgrl_configure(pcgrl_env* env, const pcgrl_config* cfg);
/* keys: HOST pointer, [count,624] u32 = MT19937 init_by_array state of environment first..first+count-1;
 * seeds both streams identically (pcgrl_env.py:54-57). */
int pcgrl_seed(pcgrl_env* env, const uint32_t* keys, int32_t first, int32_t count, void* stream);
/* The same, with the MT19937 states computed on the device (init_by_array): words HOST u32 [count][3] = (key word 0,
 * key word 1, number of key words 1|2) -- the key gym's seeding.hash_seed derives from the integer seed. */
int pcgrl_seed_words(pcgrl_env* env, const uint32_t* words, int32_t first, int32_t count, void* stream);
/* Broadcast cfg.tile_probs[0..1] into tile_p (binary); call once after the first bind and whenever
 * adjust_param(probs=...) touched them.  tile_p otherwise persists (it carries BinaryProblem._prob). */
int pcgrl_set_tile_probs(pcgrl_env* env, void* stream);
int pcgrl_reset(pcgrl_env* env, void* stream);
/* actions: DEVICE pointer, i32 [N] (narrow, turtle), [N,3] = (x, y, tile) (wide), [N,2] = (type, tile)
 * (narrowcast, turtlecast) or [N,9] (narrowmulti: tile+1 per cell of the 3x3 block, 0 = keep). */
int pcgrl_step(pcgrl_env* env, const int32_t* actions, void* stream);
/* pcgrl_step on `count` handles in one call -- the shards of one batch of environments, one handle per GPU of a node (or several
 * on one GPU), each with its own stream: envs / actions / streams are HOST arrays of `count` entries.  Step k is issued on every
 * handle before the call returns and nothing is waited for; what SubprocVecEnv.step_async does for the reference's worker
 * processes (utils.py:60-71), as one foreign-function call per step of the whole node.  The handles are issued side by side by a
 * small pool of host threads inside the library (one handle each; pcgrl_step_threads(0) beforehand: all on the calling thread);
 * every handle is tried, the first error seen is returned.  One call at a time per process (calls take turns). */
int pcgrl_step_multi(pcgrl_env* const* envs, const int32_t* const* actions, void* const* streams, int32_t count);
/* The issuing threads of pcgrl_step_multi besides the caller's (process-wide; default 7 = a thread per GPU of an eight-GPU node):
 * n >= 0 sets the number -- only until the first multi-handle call has started them --, n < 0 only asks.  Returns the number in
 * effect.  No reference counterpart (its SubprocVecEnv has a process per environment, utils.py:60-71). */
int32_t pcgrl_step_threads(int32_t n);
/* `steps` consecutive pcgrl_step calls on a tape of actions (a random-action rollout as in the reference's README
 * loop `env.step(env.action_space.sample())`, a recorded episode, an evaluation run): actions DEVICE i32
 * [steps, N(, k)] laid out like `steps` action arrays of pcgrl_step one after the other.  Optional DEVICE outputs, one
 * row per step: reward_out f64 [steps, N], done_out u8 [steps, N], info_out i32 [steps, N, 10]; NULL = not wanted.
 * The state buffers end up exactly as after the equivalent sequence of pcgrl_step calls.  Where one kernel does the
 * whole step (binary and zelda maps of at most 16 rows) the rollout is a single launch -- blocks of environments run ahead
 * of each other, there is nothing to wait for between steps; the search problems (sokoban, mdungeon, ddave; up to 131 072
 * environments) run on persistent blocks that own their environments for the whole tape, so that only the block that meets
 * a long search waits for it; everything else is the sequence of steps. */
int pcgrl_rollout(pcgrl_env* env, const int32_t* actions, int32_t steps, double* reward_out, uint8_t* done_out,
                  int32_t* info_out, void* stream);
/* maps: DEVICE pointer u8 [N,H,W]; replaces every map, recomputes stats (start stats unchanged). */
int pcgrl_set_maps(pcgrl_env* env, const uint8_t* maps, void* stream);
/* Observation formatting of the reference's composite wrappers (gym_pcgrl/wrappers.py): Cropped.transform
 * :197-206 + OneHotEncoding.transform :101-104 + ToImage.transform :53-60.  out: DEVICE u8 [N,out_h,out_w,D],
 * D = 1 (tile ids) or number of tiles (one-hot).  centered = 1: window centred on the cursor, cells outside
 * the map = pad_value (CroppedImagePCGRLWrapper :215-231, out_h = out_w = crop_size); centered = 0: the
 * map itself from its origin (ActionMapImagePCGRLWrapper :234-248, out_h = H, out_w = W). */
int pcgrl_observe(pcgrl_env* env, uint8_t* out, int32_t out_h, int32_t out_w, int32_t centered, int32_t pad_value,
                  int32_t onehot, void* stream);
/* The same image kept up to date by the step itself: after this call every pcgrl_reset / pcgrl_step / pcgrl_rollout /
 * pcgrl_set_maps leaves the image of the state it returns in `out` (DEVICE uint8 [N][out_h][out_w][D], 16-byte aligned,
 * caller-owned).  Where the step is one fused kernel (binary, zelda; maps of at most 16 rows) that kernel writes the image from
 * its on-chip copy of the state -- no extra launch, no read of the byte map; elsewhere one extra kernel follows the step.  This
 * is what wrappers.py:215-248 + utils.make_vec_envs :60-71 hand the policy per step.  May be called again at any time with
 * another `out` (a rollout buffer row); out = NULL switches it off.  Only records the target: nothing is written by the call.
 * incremental != 0: the caller will not write into `out`; a step whose target is the buffer the previous step (or reset) left
 * its image in may then update it in place -- for a window that does not follow a cursor (wide representation) that is one
 * 16-byte piece per changed environment and the full image only where an episode ended, instead of every byte.  Binding
 * another buffer, or incremental = 0, always gives full images. */
int pcgrl_bind_observation(pcgrl_env* env, uint8_t* out, int32_t out_h, int32_t out_w, int32_t centered,
                           int32_t pad_value, int32_t onehot, int32_t incremental);
/* The rest of a rollout row written by the step itself (the image goes through pcgrl_bind_observation): what a collector around
 * the reference's VecEnv (utils.py:60-71) and its Monitor (utils.py:13-29) copies out of every step -- actions, reward, done, the
 * episode-start flag of the next row, the finished episodes' return / length -- lands in the caller's columns of row t, and the
 * `actions` argument of the step may be the policy's int64 tensor as it is.  Where the step is one fused kernel (binary, zelda;
 * maps of at most 16 rows, row masks of 32 bits) that kernel writes the columns: no extra launch; elsewhere one small kernel
 * follows the step (the tick).  All pointers DEVICE, caller-owned; any pointer may be NULL = column not wanted. */
typedef struct pcgrl_row {
    int64_t* actions_out;           /* i64 [N(,k)]  the actions handed to the step, widened (all N, also those a pending environment ignores) */
    double*  reward;                /* f64 [N]      the step's reward (asynchronous: 0.0 where not fresh) */
    uint8_t* done;                  /* u8  [N]      0 / 1 (asynchronous: 0 where not fresh) */
    const uint8_t* start_in;        /* u8  [N]      episode-start flags of this row (read by the asynchronous form only) */
    uint8_t* start_out;             /* u8  [N]      episode-start flags of the next row: done (asynchronous: start_in where not fresh) */
    double*  ep_return;             /* f64 [N]      last_return where done, else the quiet NaN 0x7FF8000000000000 */
    int32_t* ep_length;             /* i32 [N]      last_length where done, else 0  (both need pcgrl_bind_episode_stats) */
    uint8_t* took;                  /* u8  [N]      asynchronous: pending[e] == 0 before the tick; lockstep: 1 */
    uint8_t* fresh;                 /* u8  [N]      asynchronous: pending[e] == 0 after the tick; lockstep: 1 */
    int32_t  actions_i64;           /* 1: the `actions` argument of pcgrl_step / pcgrl_step_flat / pcgrl_step_async points to int64 values
                                       whose low 32-bit word is the action (what a conversion to int32 keeps) */
} pcgrl_row;
/* Only records the pointers (nothing is launched or written by the call); may be repeated before every step with other pointers;
 * row = NULL switches it off (the default).  From then on pcgrl_step / pcgrl_step_flat / pcgrl_step_async fill the columns; the
 * handle's own reward / done / info / episode-statistics buffers are written as without a binding.  pcgrl_rollout has its own
 * outputs and ignores the binding (its tape is int32); pcgrl_reset / pcgrl_set_maps write no row.  PCGRL_ESTATE: ep_return /
 * ep_length without bound episode statistics. */
int pcgrl_bind_row(pcgrl_env* env, const pcgrl_row* row);
/* Pictures of levels, drawn on the device: PcgrlEnv.render (pcgrl_env.py:161-175) = Problem.render (problem.py:134-156: a frame of
 * the border tile, then every cell the picture of its tile) + the representation's cursor frame (narrow_rep.py:128-142,
 * turtle_rep.py:142) for `count` chosen environments in one launch.  The reference draws one environment per call on the host.
 * The picture of an environment is u8 [(H + 2 border_y) * ts][(W + 2 border_x) * ts][3], ts = tile_size: the border tile on a frame
 * of border_y rows and border_x columns of cells, the map's tiles inside; cursor = 1 (a representation with `pos` only): the two
 * outermost pixel rows and columns of the cursor's cell are (255, 0, 0).
 * out, grid_rows == grid_cols == 0: the pictures one after the other, u8 [count][Hp * ts][Wp * ts][3]; else ONE picture
 * u8 [grid_rows * Hp * ts][grid_cols * Wp * ts][3] with picture k in cell (k / grid_cols, k % grid_cols).  Every byte of `out` is
 * written (it may be uninitialised): cells beyond `count` are zero, and so is the picture of an index outside [0, N).
 * Asynchronous on the stream; reads the state as it is (pending asynchronous searches are not flushed) and writes nothing but `out`.
 * PCGRL_ESTATE before the first pcgrl_reset.  PCGRL_EINVAL: tiles or out NULL, count < 1, tile_size outside 1..64, border_tile not a
 * tile, a border outside 0..255, a grid with fewer cells than count (or only one of its sides 0), out not 16-byte aligned, cursor = 1
 * on a representation without `pos`.  Where tile_size * 3 is a multiple of 16 (the reference's 16-pixel tiles) the pictures leave as
 * 16-byte stores (csrc/kernels_render.h); any other size is drawn byte by byte. */
typedef struct pcgrl_render_desc {
    const int32_t* indices;         /* DEVICE i32 [count]: the environments, in any order, repeats allowed; NULL = 0 .. count-1 */
    int32_t count;
    const uint8_t* tiles;           /* DEVICE u8 [number of tiles][tile_size][tile_size][3]: the tile pictures */
    int32_t tile_size;
    int32_t border_x, border_y, border_tile, cursor;
    int32_t grid_rows, grid_cols;
    uint8_t* out;                   /* DEVICE, 16-byte aligned */
} pcgrl_render_desc;
int pcgrl_render(pcgrl_env* env, const pcgrl_render_desc* d, void* stream);
/* ---- The problem's pure functions on levels and statistics rows of the caller's: what the reference's users get from calling
 * Problem.get_stats(map), Problem.get_reward(new, old) and Problem.get_episode_over(new, old) on any level -- a generator's output, a
 * level corpus, the candidates of an evolutionary search -- not only on the one an episode edits.  `count` is independent of num_envs;
 * no episode state is read or written (maps, counters, statistics, random streams, work lists, pending asynchronous searches: all
 * untouched, nothing is flushed); pcgrl_bind is needed, pcgrl_reset is not (PCGRL_ESTATE before bind); asynchronous on the stream.
 * The parameters (targets, solver_power, reward weights) are the ones in force on the handle: a pcgrl_configure before the call applies.
 *
 * Problem.get_stats (binary_prob.py:81-92, zelda_prob.py:80-122, sokoban_prob.py:85-145, mdungeon_prob.py, ddave_prob.py)
 *   maps      DEVICE u8 [count,H,W] for the handle's current width / height; read only.
 *   rows_out  DEVICE i32 [count,8] in the packed layout of pcgrl_layout.stats: slots [0,nstats) as in the handle's `stats` rows,
 *             slots [nstats,8) zero (binary: the library's private slots 2 and 3 are zero here).
 *   work      DEVICE, 256-byte aligned, at least pcgrl_get_stats_bytes(cfg, count) bytes; the call's own, free again when the stream
 *             has passed it.
 *   Of the handle only the sticky status word is written: bit 0 for a level outside the search limits, bit 2 for a tile id >= the
 *   number of tiles (the tile is clamped in registers: the caller's map is not modified).
 *   PCGRL_EINVAL: a NULL pointer, count < 1, work not 256-byte aligned, work_bytes below pcgrl_get_stats_bytes, or a configuration
 *   without a fast form.
 * pcgrl_get_stats_bytes: from the configuration alone (num_envs is ignored; no GPU needed).  0 = this configuration has no fast form
 *   (or count < 1); else >= 256.  The fast form: binary, zelda, sokoban, mdungeon and ddave on maps up to 64 x 64 -- the search
 *   problems with levels of at most 256 bordered cells and solver_power <= 5000 (the searches that run in LDS).  smb, larger maps and
 *   the general searches: score them through a scratch handle and pcgrl_set_maps. */
size_t pcgrl_get_stats_bytes(const pcgrl_config* cfg, int32_t count);
int    pcgrl_get_stats(pcgrl_env* env, const uint8_t* maps, int32_t count, int32_t* rows_out,
                       void* work, size_t work_bytes, void* stream);
/* Problem.get_reward + Problem.get_episode_over on statistics rows (binary_prob.py:98-120, zelda_prob.py:124-156,
 * sokoban_prob.py:157-189, mdungeon_prob.py:183-222, ddave_prob.py:187-220, smb_prob.py:169-192): every problem and size, smb included.
 *   rows, ref_rows  DEVICE i32 [count,8]: outputs of pcgrl_get_stats or the handle's own stats / start_stats buffers (the private
 *                   binary slots are not read).  ref_rows is `old_stats` for the reward and the start statistics for `over`.
 *   reward_out      DEVICE f64 [count];  over_out  DEVICE u8 [count] -- either may be NULL, not both.
 *   `over` is the problem's own criterion only: max_changes / max_iterations belong to an episode, not to a level. */
int    pcgrl_get_reward(pcgrl_env* env, const int32_t* rows, const int32_t* ref_rows, int32_t count,
                        double* reward_out, uint8_t* over_out, void* stream);
/* SokobanProblem.get_stats(map)["solution"] (sokoban_prob.py:133-145): the list of moves that _run_game (:85-122) got from the first
 * agent whose returned state wins -- Node.getActions (engine.py:38-44) of that agent's winning node -- of which `sol-length` is only
 * the len().  Same contract as pcgrl_get_stats: a bound handle, no reset needed, no episode state read or written, of the handle only
 * the sticky status word written (bit 0, bit 2: a bad tile id is clamped in the LDS copy, the caller's map stays), asynchronous.
 *   maps        DEVICE u8 [count,H,W], read only.
 *   max_len     columns of a row of moves_out, >= 1.
 *   moves_out   DEVICE i8 [count,max_len]: move i of the solution as the index into engine.py:3 `directions` -- 0..3 = left, right,
 *               up, down -- for i < min(length, max_len); -1 from there to the end of the row.
 *   length_out  DEVICE i32 [count]: the full len(solution), also when it is > max_len (the row then holds the first max_len moves).
 *               0 with an all -1 row: the planner did not run (sokoban_prob.py:143) or no agent won (:122).
 *   agent_out   DEVICE i8 [count] or NULL: -2 = the planner did not run, -1 = no agent won, else the agent of _run_game that won:
 *               0 = BFSAgent (:110), 1..3 = AStarAgent with balance 1, 0.5, 0 (:113-121).
 *   rows_out    DEVICE i32 [count,8] or NULL: exactly what pcgrl_get_stats writes for these maps.
 *   work        DEVICE, 256-byte aligned, at least pcgrl_get_solution_bytes(cfg, count, max_len) bytes; the call's own.
 *   PCGRL_EINVAL: a NULL maps / moves_out / length_out / work, count < 1, max_len < 1, work not 256-byte aligned or too small, or a
 *   configuration for which pcgrl_get_solution_bytes is 0.
 * pcgrl_get_solution_bytes: from the configuration alone.  0 wherever pcgrl_get_stats_bytes is 0, for every problem but sokoban (the
 *   other planners' get_stats keep only the length; binary, zelda and smb have no move list -- binary and zelda have paths:
 *   pcgrl_get_paths) and for max_len < 1; else >= 256. */
size_t pcgrl_get_solution_bytes(const pcgrl_config* cfg, int32_t count, int32_t max_len);
int    pcgrl_get_solution(pcgrl_env* env, const uint8_t* maps, int32_t count, int32_t max_len,
                          int8_t* moves_out, int32_t* length_out, int8_t* agent_out, int32_t* rows_out,
                          void* work, size_t work_bytes, void* stream);
/* The play behind the MiniDungeons and Dangerous Dave statistics.  _run_game (mdungeon_prob.py:100-138, ddave_prob.py:92-127) runs
 * AStarAgent with balance 1, 0.5, 0 and then BFSAgent; each getSolution returns node.getActions() (mdungeon/engine.py:43-49) of the
 * node it ends on, and _run_game keeps only len(sol) and the game status of that node's state.  This entry returns the moves: those of
 * the first agent whose node wins, or -- when no agent wins -- those that lead to the BFS agent's best node, the state the `col-*` /
 * `num-jumps` / `dist-win` columns are taken from.  Same contract as pcgrl_get_solution: a bound handle, no reset needed, no episode
 * state read or written, of the handle only the sticky status word written, asynchronous.
 *   maps        DEVICE u8 [count,H,W], read only.
 *   max_len     columns of a row of moves_out, >= 1.
 *   moves_out   DEVICE i8 [count,max_len]: move i as the index into the engine's `directions` -- mdungeon 0..3 = left, right, up,
 *               down; ddave 0..3 = stay, left, right, jump -- for i < min(length, max_len); -1 from there to the end of the row.
 *   length_out  DEVICE i32 [count]: the depth of the returned node, also when it is > max_len (the row then holds the first max_len
 *               moves).  NOT `sol-length`: when no agent won the row holds the moves to the BFS agent's best node and sol-length is 0.
 *   agent_out   DEVICE i8 [count] or NULL: -2 = the planner did not run (length 0, an all -1 row), -1 = no agent won, else the agent
 *               of _run_game that won: 0..2 = AStarAgent with balance 1, 0.5, 0, 3 = BFSAgent.
 *   rows_out    DEVICE i32 [count,8] or NULL: exactly what pcgrl_get_stats writes for these maps.
 *   work        DEVICE, 256-byte aligned, at least pcgrl_get_playthrough_bytes(cfg, count, max_len) bytes; the call's own.
 *   PCGRL_EINVAL: a NULL maps / moves_out / length_out / work, count < 1, max_len < 1, work not 256-byte aligned or too small, or a
 *   configuration for which pcgrl_get_playthrough_bytes is 0.
 * pcgrl_get_playthrough_bytes: from the configuration alone.  Non-zero exactly for mdungeon and ddave where pcgrl_get_stats_bytes is
 *   non-zero (at most 256 bordered cells, the searches that run in LDS) and max_len >= 1; then >= 256. */
size_t pcgrl_get_playthrough_bytes(const pcgrl_config* cfg, int32_t count, int32_t max_len);
int    pcgrl_get_playthrough(pcgrl_env* env, const uint8_t* maps, int32_t count, int32_t max_len,
                             int8_t* moves_out, int32_t* length_out, int8_t* agent_out, int32_t* rows_out,
                             void* work, size_t work_bytes, void* stream);
/* The play behind smb's `jumps`, `jumps-dist` and `dist-win`.  SMBProblem._run_game (smb_prob.py:90-124) runs AStarAgent with balance 1
 * and, if its node does not win, with balance 0, and takes the statistics from the last node returned; this entry returns that node's
 * moves, node.getActions() (smb/engine.py:43-49): the winner's, or -- when nobody wins -- those that lead to the second agent's best
 * node, the state `dist-win` is measured from.  The contract is pcgrl_get_playthrough's: a bound handle, no reset needed, no episode
 * state read or written, of the handle only the sticky status word written (a tile id >= 7 is clamped on the way), asynchronous.
 *   maps        DEVICE u8 [count,H,W], read only.
 *   max_len     columns of a row of moves_out, >= 1.
 *   moves_out   DEVICE i8 [count,max_len]: move i as the index into the engine's `directions` -- 0 stay, 1 right, 2 jump, 3 right +
 *               jump -- for i < min(length, max_len); -1 from there to the end of the row.
 *   length_out  DEVICE i32 [count]: the depth of the returned node, also when it is > max_len (the row then holds the first max_len
 *               moves).  0 for a level of height 3, where the root already wins.
 *   agent_out   DEVICE i8 [count] or NULL: 0 = AStarAgent with balance 1 won, 1 = with balance 0, -1 = nobody (never -2: smb's planner
 *               always runs).
 *   rows_out    DEVICE i32 [count,8] or NULL: the statistics rows of these maps, as a step or pcgrl_set_maps leaves them in `stats`.
 *   work        DEVICE, 256-byte aligned, at least pcgrl_get_smb_play_bytes(cfg, count, max_len) bytes; the call's own.
 *   PCGRL_EINVAL: a NULL maps / moves_out / length_out / work, count < 1, max_len < 1, work not 256-byte aligned or too small, or a
 *   configuration for which pcgrl_get_smb_play_bytes is 0.
 * pcgrl_get_smb_play_bytes: from the configuration alone.  Non-zero (then >= 256) exactly for the smb configurations pcgrl_create takes,
 *   with count >= 1 and max_len >= 1: every width <= 250, height 3..32 and solver_power <= 16383. */
size_t pcgrl_get_smb_play_bytes(const pcgrl_config* cfg, int32_t count, int32_t max_len);
int    pcgrl_get_smb_play(pcgrl_env* env, const uint8_t* maps, int32_t count, int32_t max_len,
                          int8_t* moves_out, int32_t* length_out, int8_t* agent_out, int32_t* rows_out,
                          void* work, size_t work_bytes, void* stream);
/* The paths behind binary's `path-length` and zelda's `path-length` / `nearest-enemy`.  The reference computes the distance maps these
 * routes follow -- run_dikjstra (helper.py:222-237) inside calc_longest_path (helper.py:250-264) and ZeldaProblem.get_stats
 * (zelda_prob.py:91-110) -- keeps one number of each and throws the maps away.  This entry returns the cells.  A cell is y * W + x.
 *   Walk-back: with D = run_dikjstra(sx, sy, map, passable) and a cell t with D[t] >= 0, the leg from (sx, sy) to t is built backwards
 *   from t: the predecessor of a cell c with D[c] > 0 is the first neighbour n of c in run_dikjstra's order -- (dx, dy) = (-1,0), (1,0),
 *   (0,-1), (0,1): left, right, up, down -- with D[n] == D[c] - 1.  The leg is reported start -> target: length = D[t] steps,
 *   length + 1 cells; D[t] == -1: length -1, no cells.  "First" among cells is row-major (np.argmax, get_tile_locations).
 *   binary, one leg ("longest"): the regions in the order of their first cell; for each, calc_longest_path's first map from that cell,
 *   (mx, my) = its first arg-max, the second map D2 from (mx, my).  The region is the first whose D2.max() equals the returned
 *   path-length (the reference updates on `>` only); the leg is the walk-back over D2 from (mx, my) to the first arg-max of D2.  A
 *   path-length of 0 with an empty tile: that region's single start cell (length 0, one cell).  No empty tile: length -1.  Whenever
 *   length >= 0, length == path-length.
 *   zelda, three legs ("key", "door", "enemy"), conditions and passable sets of zelda_prob.py:91-110.  Legs 0 and 1 exist when player == 1
 *   and regions == 1 and key == 1 and door == 1: leg 0 over run_dikjstra(player; empty, key, player, enemies) to the key, leg 1 over
 *   run_dikjstra(key; the same + door) to the door, length -1 when the door is walled off; length[0] + length[1] == path-length (the
 *   reference adds the -1 too).  Leg 2 exists when player == 1 and regions == 1 and enemies > 0 and some enemy has D > 0 in
 *   run_dikjstra(player; empty, player, enemies) -- the key is not passable there: its target is the first enemy cell with
 *   D == nearest-enemy, its length is nearest-enemy.  A leg whose condition does not hold has length -1.
 * Same contract as pcgrl_get_solution: a bound handle, no reset needed, no episode state read or written, of the handle only the sticky
 * status word written (bit 2: a tile id beyond the last is clamped in the LDS copy, the caller's map stays), asynchronous on the stream.
 *   maps        DEVICE u8 [count,H,W], read only.
 *   max_len     columns of a leg's row of cells_out, >= 1 (H * W holds every leg).
 *   cells_out   DEVICE i16 [count,legs,max_len], legs = pcgrl_get_paths_legs(cfg): cell i of the leg for i < min(length + 1, max_len);
 *               -1 from there to the end of the row.
 *   length_out  DEVICE i32 [count,legs]: the full length in steps, also when length + 1 > max_len (the row then holds the first max_len
 *               cells); -1: the leg does not exist.
 *   rows_out    DEVICE i32 [count,8] or NULL: exactly what pcgrl_get_stats writes for these maps.
 *   work        DEVICE, 256-byte aligned, at least pcgrl_get_paths_bytes(cfg, count, max_len) bytes; the call's own.
 *   PCGRL_EINVAL: a NULL maps / cells_out / length_out / work, count < 1, max_len < 1, work not 256-byte aligned or too small, or a
 *   configuration for which pcgrl_get_paths_bytes is 0.  PCGRL_ESTATE before pcgrl_bind.
 * pcgrl_get_paths_legs: 1 for binary, 3 for zelda, 0 for the other problems (their routes are plays: pcgrl_get_solution,
 *   pcgrl_get_playthrough, pcgrl_get_smb_play) and for a NULL cfg.
 * pcgrl_get_paths_bytes: from the configuration alone.  Non-zero (then >= 256) exactly for binary and zelda where pcgrl_get_stats_bytes is
 *   non-zero (maps up to 64 x 64), with count >= 1 and max_len >= 1. */
int32_t pcgrl_get_paths_legs(const pcgrl_config* cfg);
size_t pcgrl_get_paths_bytes(const pcgrl_config* cfg, int32_t count, int32_t max_len);
int    pcgrl_get_paths(pcgrl_env* env, const uint8_t* maps, int32_t count, int32_t max_len,
                       int16_t* cells_out, int32_t* length_out, int32_t* rows_out,
                       void* work, size_t work_bytes, void* stream);
/* ---- Every one-cell change of a level: what a representation's action (narrow_rep.py:99-114, wide_rep.py:67-70, turtle_rep.py:101-129)
 * or a mutation would do to the statistics, and what the step that makes it would pay.  For each of `count` levels and each of its
 * `ncells` listed cells, entry (m, k, t) is the level m with cell k set to tile t, for every tile t of the problem (T of them):
 *   rows     Problem.get_stats of that level;
 *   reward   Problem.get_reward(new = that row, old = the level's own row);
 *   over     Problem.get_episode_over(new = that row, start), `start` being start_rows[m] or, without, the level's own row.
 * The entry of the tile the cell already holds changes nothing: it is the level's own row with reward 0 and is not computed again.
 *   maps           DEVICE u8 [count,H,W], read only.  A tile id >= T is clamped in the staged copy and reported (status bit 2), as in
 *                  pcgrl_get_stats; the no-op entry of such a cell is the one of tile T - 1.
 *   cells          DEVICE i32 [count,ncells], a cell being y * W + x, or NULL = every cell in row-major order (ncells must then be H * W).
 *                  Cells may repeat.  A cell outside [0, H*W) is clamped into the range and reported like an action outside the action
 *                  space (status bit 1).
 *   start_rows     DEVICE i32 [count,8] or NULL: the start statistics `over` is judged against (NULL: the level's own row).
 *   base_rows_out  DEVICE i32 [count,8] or NULL: exactly what pcgrl_get_stats writes for these maps.
 *   rows_out       DEVICE i32 [count,ncells,T,8] or NULL, each row packed like pcgrl_get_stats' rows.
 *   reward_out     DEVICE f64 [count,ncells,T] or NULL;  over_out  DEVICE u8 [count,ncells,T] or NULL.  At least one of rows_out, reward_out
 *                  and over_out is needed.
 *   work           DEVICE, 256-byte aligned, at least pcgrl_get_changes_bytes(cfg, count, ncells) bytes; the call's own.
 * Same contract as pcgrl_get_stats: a bound handle, no reset needed, no episode state read or written, of the handle only the sticky
 * status word written; asynchronous on the stream, nothing is cleared with a memset and nothing waited for.
 *   PCGRL_EINVAL: a NULL maps or work, no output, count < 1, ncells < 1, NULL cells with ncells != H * W, work not 256-byte aligned or too
 *   small, or a configuration for which pcgrl_get_changes_bytes is 0.  PCGRL_ESTATE before pcgrl_bind.
 * pcgrl_get_changes_bytes: from the configuration alone.  Non-zero (then >= 256) exactly where pcgrl_get_stats_bytes(cfg, count) is, with
 *   count >= 1, ncells >= 1 and count * ncells * T + count <= 2^31 - 1: an entry's index, and the search problems' job list -- the entries,
 *   then the levels -- are 32-bit.  Beyond that bound it is 0: split the call. */
size_t pcgrl_get_changes_bytes(const pcgrl_config* cfg, int32_t count, int32_t ncells);
int    pcgrl_get_changes(pcgrl_env* env, const uint8_t* maps, int32_t count,
                         const int32_t* cells, int32_t ncells, const int32_t* start_rows,
                         int32_t* base_rows_out, int32_t* rows_out, double* reward_out, uint8_t* over_out,
                         void* work, size_t work_bytes, void* stream);
/* ---- helper.py for any tile set (helper.py:170-296): the functions a custom Problem builds its get_stats from -- calc_num_regions
 * (:197-207) with the color_map it throws away, calc_longest_path (:250-264), run_dikjstra's whole map (:222-237) and
 * calc_num_reachable_tile (:288-296) -- for `count` levels of any tiles 0..31, whatever problem the handle has.
 * The set rule.  The reference's helpers take a LIST of passable values and _get_certain_tiles (:150-154) orders cells by list position
 * first, row-major second: calc_longest_path's double sweep starts elsewhere in a component, and the color_map is numbered differently,
 * for [0, 1] than for [1, 0].  Here `passable` is a SET (bit t: tile t), and every result is the reference's result on the level in
 * which every passable tile has been renamed to one single value: a component's first sweep starts at its first cell in row-major
 * order, regions are numbered 1, 2, ... by the row-major order of their first cell.  For a single passable value that is the reference
 * exactly; for several, regions, dist and reach are still exactly the reference's, longest and the label numbering are the merged-tile
 * ones (the reference's own longest depends on the order of its list).
 *   maps          DEVICE u8 [count,H,W], read only.  A byte >= 32 is in no set (impassable) and reported (status bit 2).
 *   passable, source_tiles, reach_tiles   tile sets, bit t = tile t.
 *   sources       DEVICE i32 [count] or NULL: the source cell of each level, y * W + x, -1 = none; a value outside the map that is not
 *                 -1 counts as none and is reported like a cell outside the map in pcgrl_get_changes (status bit 1).  NULL: the first
 *                 cell in row-major order that holds a tile of source_tiles (_get_certain_tiles(locs, [start_value])[0]), none without one.
 *   Outputs, DEVICE, each one optional: NULL = neither computed nor stored; at least one is needed.
 *   regions_out   i32 [count]      calc_num_regions(map, locs, passable).
 *   longest_out   i32 [count]      calc_longest_path(map, locs, passable) under the set rule.
 *   labels_out    i16 [count,H,W]  the color_map: -1 on impassable cells, 1 .. regions elsewhere, numbered by the set rule.
 *   dist_out      i16 [count,H,W]  run_dikjstra(source; passable)'s map: -1 where unreached or impassable; all -1 without a source or
 *                                  with a source cell that is not passable.
 *   reach_out     i32 [count]      calc_num_reachable_tile: the cells of reach_tiles with dist >= 0 (the source itself when in the set).
 *   source_out    i32 [count]      the source cell that was used (passable or not), -1 if none.
 * Every element of every requested output is stored exactly once, nothing else is written.
 * Same contract as pcgrl_get_paths: a bound handle, no reset needed; only the device, the stream, the width, the height and the lane-group
 * form are taken from the handle; no episode state read or written, of the handle only the sticky status word written; asynchronous.
 *   work          DEVICE, 256-byte aligned, at least pcgrl_tile_graph_bytes(cfg, count) bytes; the call's own.
 *   PCGRL_EINVAL: a NULL desc, maps or work, no output, count < 1, work not 256-byte aligned or too small, or a configuration for
 *   which pcgrl_tile_graph_bytes is 0.  PCGRL_ESTATE before pcgrl_bind.
 * pcgrl_tile_graph_bytes: from the configuration alone.  0: no form (maps beyond 64 x 64, smb, count < 1, a NULL or invalid cfg);
 *   else >= 256. */
typedef struct pcgrl_tile_graph_desc {
    const uint8_t* maps;
    int32_t count;
    uint32_t passable, source_tiles, reach_tiles;
    const int32_t* sources;
    int32_t *regions_out, *longest_out;
    int16_t *labels_out, *dist_out;
    int32_t *reach_out, *source_out;
} pcgrl_tile_graph_desc;
size_t pcgrl_tile_graph_bytes(const pcgrl_config* cfg, int32_t count);
int    pcgrl_tile_graph(pcgrl_env* env, const pcgrl_tile_graph_desc* desc, void* work, size_t work_bytes, void* stream);
/* ---- the local half of helper.py for any tile set (helper.py:37-137): get_floor_dist (:56-62), get_type_grouping (:100-108) and
 * get_changes (:120-137) -- the helpers behind smb's dist-floor, disjoint-tubes and noise and ddave's dist-floor -- with the per-cell
 * values the reference computes and throws away, _calc_dist_floor (:37-43) and _calc_group_value (:77-85), and a count of every tile,
 * for `count` levels of any tiles 0..31.  These rules read the tile bytes alone: there is a form for EVERY configuration a handle can
 * be created for -- smb's 114 x 14, maps beyond 64 x 64 -- whatever problem the handle has.  The reference only tests `in types`, so a
 * tile SET is the reference exactly (no set rule as in pcgrl_tile_graph).
 *   maps          DEVICE u8 [count,H,W], read only.  A byte >= 32 is in no set and in no counts column, and reported (status bit 2);
 *                 changes compares it as it is.
 *   from_tiles, floor_tiles   get_floor_dist's fromTypes / floorTypes, bit t = tile t.
 *   group_tiles, group_min, group_max, noffsets, offsets   get_type_grouping's types, min, max and relLocs: (dx, dy) each, the first
 *                 noffsets (0 .. PCGRL_MAX_OFFSETS) count; an offset listed twice counts twice, (0, 0) counts the cell itself.
 *   Outputs, DEVICE, each one optional: NULL = neither computed nor stored; at least one is needed.
 *   counts_out      i32 [count,32]   the cells that hold tile t.
 *   floor_dist_out  i32 [count]      get_floor_dist(map, from, floor): the sum of floor_map over the cells of from_tiles; can be negative.
 *   floor_map_out   i16 [count,H,W]  _calc_dist_floor(map, x, y, floor) of EVERY cell: the smallest dy >= 0 with y + dy < H and
 *                                    map[y+dy][x] in floor_tiles gives dy - 1 (a floor cell itself: -1); without one H - 1, whatever y.
 *   grouping_out    i32 [count]      get_type_grouping: the cells of group_tiles with group_min <= group_map <= group_max (min > max: 0).
 *   group_map_out   i8  [count,H,W]  _calc_group_value of EVERY cell: the offsets whose cell is inside the map and holds a group tile.
 *   changes_out     i32 [count,2]    get_changes(map, False), get_changes(map, True): unequal horizontally / vertically adjacent pairs
 *                                    of raw bytes.
 * Every element of every requested output is stored exactly once, nothing else is written.
 * Same contract as pcgrl_tile_graph: a bound handle, no reset needed; only the device, the stream, the width and the height are taken
 * from the handle; no episode state read or written, of the handle only the sticky status word written; asynchronous.
 *   work          DEVICE, 256-byte aligned, at least pcgrl_tile_local_bytes(cfg, count) bytes; the call's own.
 *   PCGRL_EINVAL: a NULL desc, maps or work, no output, count < 1, noffsets outside 0 .. PCGRL_MAX_OFFSETS when grouping_out or
 *   group_map_out is asked for, work not 256-byte aligned or too small, or a configuration for which pcgrl_tile_local_bytes is 0.
 *   PCGRL_ESTATE before pcgrl_bind.  A refused call writes nothing.
 * pcgrl_tile_local_bytes: from the configuration alone.  >= 256 for every configuration a handle can be created for (with
 *   num_envs = 1), smb and maps beyond 64 x 64 included; 0 for count < 1, a NULL cfg and an invalid one: here a problem or a
 *   representation the library does not know, or a side outside 1 .. 4096 -- the rules read the tile bytes alone, the problem's own
 *   limits do not matter to them. */
#define PCGRL_MAX_OFFSETS 16
typedef struct pcgrl_tile_local_desc {
    const uint8_t* maps;
    int32_t count;
    uint32_t from_tiles, floor_tiles;
    uint32_t group_tiles;
    int32_t group_min, group_max, noffsets;
    int8_t offsets[PCGRL_MAX_OFFSETS][2];
    int32_t* counts_out;
    int32_t* floor_dist_out;
    int16_t* floor_map_out;
    int32_t* grouping_out;
    int8_t* group_map_out;
    int32_t* changes_out;
} pcgrl_tile_local_desc;
size_t pcgrl_tile_local_bytes(const pcgrl_config* cfg, int32_t count);
int    pcgrl_tile_local(pcgrl_env* env, const pcgrl_tile_local_desc* desc, void* work, size_t work_bytes, void* stream);
/* ActionMap.step for the wide representation (wrappers.py:139-154): flat DEVICE i32 [N] index into
 * (H, W, tiles) -> xyv DEVICE i32 [N,3] = (x, y, tile), the action pcgrl_step takes. */
int pcgrl_action_map(pcgrl_env* env, const int32_t* flat, int32_t* xyv, void* stream);
/* ActionMap.step followed by PcgrlEnv.step (wrappers.py:139-154 + pcgrl_env.py:129-150) for the wide representation in one call:
 * flat DEVICE i32 [N]; xyv DEVICE i32 [N,3] scratch of the caller (filled where the decode is a kernel of its own; the fused step
 * kernel decodes inside and leaves it alone).  PCGRL_EINVAL for another representation. */
int pcgrl_step_flat(pcgrl_env* env, const int32_t* flat, int32_t* xyv, void* stream);
/* ---- Asynchronous stepping of the search problems (sokoban, mdungeon, ddave; csrc/kernels_search_async.h).  No reference
 * counterpart as such: it is what the reference gets from running every environment in a process of its own behind
 * SubprocVecEnv (utils.py:60-71) -- no environment waits for another environment's solver (sokoban_prob.py:85-122,
 * mdungeon_prob.py:110-126, ddave_prob.py) -- on one GPU and one stream.
 * pcgrl_step_async is one *tick*: every environment whose previous step is complete takes its action from `actions` (laid out
 * as for pcgrl_step) and steps; every search gets at most `pop_budget` pops; an environment whose search is not finished by then
 * is marked pending (its search is suspended and goes on in the following ticks) and takes no further action -- the entries of
 * `actions` for pending environments are ignored -- until a tick completes its step.  After a tick, pending[e] == 0 means: the
 * observation / reward / done / info of environment e are those of its last taken action, and it takes the next one.  Per
 * environment, the sequence of (taken action -> outputs) is bitwise what pcgrl_step gives for the same actions.
 *   pcgrl_async_bytes      DEVICE bytes the caller provides for `nslots` suspended searches (0: the configuration has no
 *                          asynchronous form -- another problem, levels or solver_power beyond the compact searches).
 *   pcgrl_bind_async       after pcgrl_bind; arena DEVICE, 256-byte aligned, zeroed by the call.  Its head is the caller's to
 *                          read: pending u8 [N] at offset 0 (0: complete; 1: a search is suspended; 2: the search ended the episode,
 *                          the next tick resets the environment), then (256-byte aligned) eight u64 counters: -, searches suspended,
 *                          jobs finished from a slot, slot overflows (no free slot: that search ran to its end inside its tick), pops
 *                          of the resumable searches; then sixteen u64 words 64 bytes apart whose sum is the number of actions taken.
 *   pcgrl_async_flush      finishes every pending step (unbounded budget) -- pcgrl_step, pcgrl_rollout, pcgrl_set_maps and
 *                          pcgrl_reset do it themselves (pcgrl_reset drops the pending steps instead).
 * pop_budget < 1: PCGRL_EINVAL. */
size_t pcgrl_async_bytes(const pcgrl_config* cfg, int32_t nslots);
int pcgrl_bind_async(pcgrl_env* env, void* arena, size_t bytes, int32_t nslots, void* stream);
int pcgrl_step_async(pcgrl_env* env, const int32_t* actions, int32_t pop_budget, void* stream);
int pcgrl_async_flush(pcgrl_env* env, void* stream);
/* Episode statistics kept by the step kernels -- what stable-baselines' Monitor keeps around the reference env in
 * utils.make_env / make_vec_envs (utils.py:13-29, 60-71).  ep_return f64 [N], ep_length i32 [N]: reward sum (in step
 * order) and step count of the running episode; last_return / last_length: the same, latched when an episode ends
 * (read them where done == 1).  DEVICE pointers, zeroed by the call; pass four NULLs to switch the feature off (the
 * default).  Call after pcgrl_bind. */
int pcgrl_bind_episode_stats(pcgrl_env* env, double* ep_return, int32_t* ep_length, double* last_return,
                             int32_t* last_length, void* stream);
/* Test hook, no reference counterpart: runs the heap primitives of the two-wavefront searches (the CPython heapq of
 * sokoban/engine.py:96-119, mdungeon/engine.py, ddave/engine.py: heappush / heappop on entries compared by priority only)
 * over a tape of operations on the current device.  ops DEVICE u32 [n_ops]: a packed word (priority << 16 | payload) to push, or
 * 0xFFFFFFFF = pop.  pops DEVICE u32 [number of pops]: the popped words in order (0xFFFFFFFF: the heap was empty); heap_out DEVICE
 * u32 [16384] and n_out DEVICE i32 [1]: the heap array afterwards.  At most 16 384 entries are kept (further pushes are dropped).
 * tests/test_gpu_parity.py holds the result against Python's heapq slot for slot. */
int pcgrl_selftest_heap(const uint32_t* ops, int32_t n_ops, uint32_t* pops, uint32_t* heap_out, int32_t* n_out, void* stream);
/* Test hook, no reference counterpart, no GPU needed: the issuing threads of pcgrl_step_multi driven with `count` (2..64) stand-in
 * handles for `calls` calls; hits HOST i32 [count] is incremented once per stand-in and call, stand-in `fail_at` (-1: none) reports an
 * error.  Returns the number of calls that returned an error, -1 when the pool is switched off (pcgrl_step_threads(0)). */
int pcgrl_selftest_step_pool(int32_t count, int32_t calls, int32_t fail_at, int32_t* hits);
/* Test hook for get_range_reward (helper.py:366-376), which every reward term of every problem goes through: the integer form the
 * step kernels evaluate (bounds are integers or +-inf, statistics are small integers; INT32_MAX / INT32_MIN stand for +-inf), run
 * on the current device over a table.  rows DEVICE i32 [n][4] = (new value, old value, low, high); out DEVICE i32 [n].
 * tests/test_gpu_parity.py holds it against the reference's exhaustive table (tests/golden/range_reward.npz). */
int pcgrl_selftest_range_reward(const int32_t* rows, int32_t n, int32_t* out, void* stream);
/* Sticky device status word, 0 = fine.  Bit 0 (1): a level was outside a search kernel's limits -- a Sokoban level with more crates
 * than the search takes (32 in the compact searches, 256 in the general ones of csrc/search_big.h), or more than 255 tiles / collected
 * things of one kind in a packed statistics row: Dave's player, exit and key tiles and collected diamonds, MiniDungeons' collected potions,
 * treasures and enemies, on a map of any size and on every route that computes statistics (reset, step, rollout, asynchronous ticks,
 * pcgrl_set_maps, pcgrl_get_stats).  Such a count is stored saturated at 255 -- a level with 257 players never reads as a level with
 * one -- so the statistics of that level, and the rewards computed from them, are not exact; the columns that own a whole slot are.
 * Bit 1 (2): an action outside the action space was clamped into it (the reference raises IndexError or writes the
 * bad value: narrow_rep.py:101-103, wide_rep.py:68-69, turtle_rep.py:101-129, wrappers.py:139-154).  Bit 2 (4):
 * pcgrl_set_maps was handed a tile id >= the number of tiles (clamped).  Synchronises the stream. */
int pcgrl_status(pcgrl_env* env, void* stream, int32_t* status);
/* Zero the status word (asynchronous on the stream): a caller that turns bit 1 into the reference's IndexError at the offending
 * call clears it afterwards, so that the next call reports only its own actions. */
int pcgrl_clear_status(pcgrl_env* env, void* stream);


/* Per-phase GPU timing of pcgrl_step with HIP events recorded on the caller's stream (bench.py's
 * roofline leg).  Phases: 0 update, 1 stats(step), 2 solver(step), 3 mapgen, 4 stats(start), 5 solver(start). */
#define PCGRL_NPHASE 6
int pcgrl_profile(pcgrl_env* env, int enable);
int pcgrl_profile_read(pcgrl_env* env, double* phase_ms /*[PCGRL_NPHASE]*/, int32_t* steps);

#ifdef __cplusplus
}
#endif
#endif
