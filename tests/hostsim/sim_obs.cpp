// gym_pcgrl_amd/csrc/kernels_obs.h on the CPU: the device functions of the wrapped observation compiled by g++ and called thread by
// thread.  TEST ONLY.
//
// The header's routines -- obs_pieces_any, obs_write_block, obs_write_env_lean, obs_write_envs_rows, obs_write_delta_piece,
// obs_write_block_lean, obs_lean_mode -- take their thread index as an argument and have no barrier, so a block is the loop
// tid = 0 .. nthreads-1 over them.  The two kernels around them (k_obs, k_obs_huge) and obs_view are left out of this compile
// (PCGRL_OBS_HOST_SIM); what k_obs does before it calls obs_write_block -- the planes of the block's environments behind one another,
// then their cursors -- is done here by hand.
//
// Host stand-ins: __umulhi, __umul24, uint2 / uint4 with their make_ functions, the qualifiers as empty macros, and readfirstlane as
// the identity.  What that identity cannot show: readfirstlane hands every lane the value of the FIRST active lane, so device code
// that feeds it a value that differs between the lanes of a wavefront silently computes with lane 0's -- here each "lane" keeps its own
// and the result looks right.  The call sites feed it the environment of a wavefront (tid >> 6) and that environment's cursor; that
// they are wave-uniform is read from the code (and checked by the device tests), not by this simulator.
//
// Built as a shared library for tests/test_obs_host.py and, with -DSIM_OBS_MAIN -fsanitize=address,undefined, as a stand-alone program
// that runs a built-in table of shapes with every target carved out of a heap buffer of exactly the images' size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
#define __builtin_amdgcn_readfirstlane(x) (x)
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
// worklist.h (tests/test_obs_host.py holds this copy against it)
struct ObsView { uint8_t* out; int oh, ow, depth, centered, pad, W, H; };
#define PCGRL_OBS_HOST_SIM 1
#include "../../gym_pcgrl_amd/csrc/kernels_obs.h"

enum { FORM_BLOCK = 0, FORM_BLOCK_LEAN = 1, FORM_ENV_LEAN = 2 };

// row bit planes [env][G rows][NPL planes] from the byte maps
template <class T, int NPL>
static std::vector<T> planes_of(const uint8_t* map, int n, int H, int W, int G) {
    std::vector<T> p((size_t)n * G * NPL, 0);
    for (int e = 0; e < n; e++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const int t = map[((size_t)e * H + y) * W + x];
                for (int k = 0; k < NPL; k++) p[((size_t)e * G + y) * NPL + k] |= (T)((t >> k) & 1) << x;
            }
    return p;
}

// one block: environments [e0, e0 + ne) of the batch, by `nthreads` threads
template <class Src>
static int run_block(const Src& src, const ObsView& V, const uint8_t* pos, int ne, int form, int nthreads, const int32_t* act, const uint8_t* changed,
                     const uint8_t* fresh) {
    if (form == FORM_BLOCK) {
        for (int tid = 0; tid < nthreads; tid++) obs_write_block(src, V, pos, ne, tid, nthreads);
        return 0;
    }
    if (obs_mode<Src>(V) == 0) return -2;                // the fused kernel carries the lean routines only
    if (form == FORM_BLOCK_LEAN) {
        for (int tid = 0; tid < nthreads; tid++) obs_write_block_lean(src, V, pos, ne, act != nullptr, act, changed, fresh, tid, nthreads);
        return 0;
    }
    for (int e = 0; e < ne; e++)                          // an observation task: a wavefront an environment
        for (int lane = 0; lane < 64; lane++) obs_write_env_lean(src, V, pos, e, lane);
    return 0;
}

template <class T, int NPL>
static int run_planes(const uint8_t* map, const uint8_t* pos, int n, int H, int W, int G, ObsView V, int form, int epb, int nthreads, const int32_t* act,
                      const uint8_t* changed, const uint8_t* fresh) {
    if (H > G || W > (int)(8 * sizeof(T))) return -1;
    const std::vector<T> pl = planes_of<T, NPL>(map, n, H, W, G);
    uint8_t* const out = V.out;
    const size_t per_env = (size_t)V.oh * V.ow * V.depth;
    for (int e0 = 0; e0 < n; e0 += epb) {
        const int ne = n - e0 < epb ? n - e0 : epb;
        // exactly what the block holds: the planes and cursors of its environments (an index past them is a sanitizer report)
        const std::vector<T> blk(pl.begin() + (size_t)e0 * G * NPL, pl.begin() + (size_t)(e0 + ne) * G * NPL);
        const std::vector<uint8_t> bpos(pos + 2 * (size_t)e0, pos + 2 * (size_t)(e0 + ne));
        const ObsPlanes<T, NPL> src = {blk.data(), G};
        V.out = out + (size_t)e0 * per_env;
        const int rc = run_block(src, V, bpos.data(), ne, form, nthreads, act ? act + 3 * (size_t)e0 : nullptr, changed ? changed + e0 : nullptr,
                                 fresh ? fresh + e0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

extern "C" {
int sim_obs_lean_mode(int nplanes, int word32, int W, int oh, int ow, int depth, int pad) { return obs_lean_mode(nplanes, word32 != 0, W, oh, ow, depth, pad); }
int sim_obs_epb(void) { return OBS_EPB; }

// obs_lean_mode over W 1..wmax, oh, ow 1..omax, depths[nd], pad 0..pmax: out[W][oh][ow][depth][pad], one byte each
void sim_obs_lean_grid(int nplanes, int word32, int wmax, int omax, const int32_t* depths, int nd, int pmax, uint8_t* out) {
    for (int W = 1; W <= wmax; W++)
        for (int oh = 1; oh <= omax; oh++)
            for (int ow = 1; ow <= omax; ow++)
                for (int k = 0; k < nd; k++)
                    for (int pad = 0; pad <= pmax; pad++) *out++ = (uint8_t)obs_lean_mode(nplanes, word32 != 0, W, oh, ow, depths[k], pad);
}

// The images of n environments: map [n][H][W], pos [n][2] = (x, y), out [n][oh][ow][depth] (16-byte aligned).
// source 0: the byte map; 1: one 32-bit plane; 2: one 64-bit plane; 3: three 32-bit planes (k_obs<source>); G rows a plane set.
// form 0: obs_write_block (k_obs: blocks of `epb` = OBS_EPB environments, 256 threads); 1: obs_write_block_lean (k_step at the end of
// its launch: blocks of `epb` environments, `nthreads` threads; act / changed / fresh given: the in-place update of the wide
// representation, act [n][3] = (x, y, tile)); 2: obs_write_env_lean environment by environment (k_step's observation tasks).
// Returns 0, -1 when the source does not hold the map, -2 for a fused form on a shape without a lean routine.
int sim_obs(const uint8_t* map, const uint8_t* pos, int n, int H, int W, int source, int G, int oh, int ow, int depth, int centered, int pad, int form,
            int epb, int nthreads, const int32_t* act, const uint8_t* changed, const uint8_t* fresh, uint8_t* out) {
    const ObsView V = {out, oh, ow, depth, centered, pad, W, H};
    if (((uintptr_t)out & 15) != 0 || epb < 1 || (epb & 15) != 0 || nthreads < 64 || (nthreads & 63) != 0) return -3;
    if (source == 1) return run_planes<uint32_t, 1>(map, pos, n, H, W, G, V, form, epb, nthreads, act, changed, fresh);
    if (source == 2) return run_planes<uint64_t, 1>(map, pos, n, H, W, G, V, form, epb, nthreads, act, changed, fresh);
    if (source == 3) return run_planes<uint32_t, 3>(map, pos, n, H, W, G, V, form, epb, nthreads, act, changed, fresh);
    if (source != 0 || form != FORM_BLOCK) return -3;
    const size_t per_env = (size_t)oh * ow * depth;
    for (int e0 = 0; e0 < n; e0 += epb) {
        const int ne = n - e0 < epb ? n - e0 : epb;
        const std::vector<uint8_t> blk(map + (size_t)e0 * H * W, map + (size_t)(e0 + ne) * H * W), bpos(pos + 2 * (size_t)e0, pos + 2 * (size_t)(e0 + ne));
        const ObsBytes src = {blk.data(), W, H};
        ObsView Vb = V;
        Vb.out = out + (size_t)e0 * per_env;
        run_block(src, Vb, bpos.data(), ne, form, nthreads, nullptr, nullptr, nullptr);
    }
    return 0;
}

// obs_write_delta_piece alone (k_step's update lane): for every environment the piece of its image that holds map cell xy[e] = (x, y)
int sim_obs_delta(const uint8_t* map, int n, int H, int W, int G, int oh, int ow, int pad, const int32_t* xy, uint8_t* out) {
    if (H > G || W > 32 || ((uintptr_t)out & 15) != 0) return -1;
    const ObsView V = {out, oh, ow, 8, 0, pad, W, H};
    if (obs_lean_mode(3, true, W, oh, ow, 8, pad) != 2) return -2;
    const std::vector<uint32_t> pl = planes_of<uint32_t, 3>(map, n, H, W, G);
    const ObsPlanes<uint32_t, 3> src = {pl.data(), G};
    for (int e = 0; e < n; e++) obs_write_delta_piece(src, V, e, xy[2 * e], xy[2 * e + 1]);
    return 0;
}
}

#ifdef SIM_OBS_MAIN
// the rule, cell by cell
static uint8_t want_byte(const uint8_t* map, const uint8_t* pos, int e, int H, int W, int oh, int ow, int depth, int centered, int pad, size_t rem) {
    const int d = (int)(rem % depth), i = (int)(rem / depth), r = i / ow, c = i % ow;
    const int y = r + (centered ? pos[2 * e + 1] - oh / 2 : 0), x = c + (centered ? pos[2 * e] - ow / 2 : 0);
    const int t = (y >= 0 && y < H && x >= 0 && x < W) ? map[((size_t)e * H + y) * W + x] : pad;
    return depth == 1 ? (uint8_t)t : (uint8_t)(d == t);
}

struct Shape { int ntiles, H, W, oh, ow, onehot, pad; };
static const Shape SHAPES[] = {
    // rows: the limits of 16 <= ow <= 32, odd widths, one row, 4096 cells, W = 32 / 64, pad 0 / 1; beside the rule: 15, 33, pad 2
    {2, 3, 5, 1, 16, 0, 0}, {2, 16, 32, 1, 32, 0, 1}, {2, 16, 16, 16, 16, 0, 1}, {2, 3, 31, 16, 17, 0, 0}, {2, 16, 33, 16, 31, 0, 1}, {2, 3, 48, 32, 32, 0, 0},
    {2, 16, 63, 128, 32, 0, 1}, {2, 3, 64, 16, 17, 0, 1}, {2, 17, 64, 1, 32, 0, 1}, {2, 64, 64, 16, 31, 0, 0}, {2, 64, 32, 16, 16, 0, 1}, {2, 16, 32, 16, 15, 0, 1},
    {2, 16, 33, 16, 33, 0, 1}, {2, 16, 16, 16, 16, 0, 2},
    // one-hot over eight tiles: ow 1, 2, 63.., 4096 cells, W = 32, a pad tile in the second word of the pair; 77 cells: general
    {8, 4, 3, 2, 1, 1, 4}, {8, 7, 11, 1, 2, 1, 7}, {8, 7, 11, 8, 12, 1, 1}, {8, 16, 32, 6, 8, 1, 3}, {8, 7, 11, 8, 9, 1, 0}, {8, 16, 32, 63, 64, 1, 4},
    {8, 5, 32, 64, 64, 1, 7}, {8, 7, 11, 7, 11, 1, 1},
    // the general routine: one column, tiny windows, five and seven tiles, byte counts that are no multiple of 16
    {2, 3, 5, 1, 1, 0, 1}, {2, 3, 5, 3, 1, 0, 1}, {8, 7, 11, 5, 1, 1, 3}, {5, 5, 5, 3, 1, 1, 3}, {5, 5, 5, 1, 3, 0, 3}, {7, 6, 12, 3, 5, 1, 3}, {7, 6, 12, 5, 1, 0, 3},
};

int main() {
    long images = 0, bytes = 0;
    unsigned rng = 7u;
    setvbuf(stdout, nullptr, _IONBF, 0);              // (a failure leaves with its target allocated: the leak report ends the process unflushed)
    for (const Shape& s : SHAPES) {
        const int depth = s.onehot ? s.ntiles : 1, G = s.H <= 16 ? 16 : 64;
        const int n = s.H * s.W < 200 ? s.H * s.W : 200;              // a cursor per cell (a sample on the large maps), some blocks partial
        std::vector<uint8_t> map((size_t)n * s.H * s.W), pos((size_t)2 * n);
        for (auto& v : map) { rng = rng * 1664525u + 1013904223u; v = (uint8_t)((rng >> 16) % (unsigned)s.ntiles); }
        for (int e = 0; e < n; e++) {
            const int cell = s.H * s.W <= 200 ? e : (int)((long)e * (s.H * s.W - 1) / (n - 1));
            pos[2 * e] = (uint8_t)(cell % s.W); pos[2 * e + 1] = (uint8_t)(cell / s.W);
        }
        const size_t per_env = (size_t)s.oh * s.ow * depth, total = (size_t)n * per_env;
        const int plane_src = s.ntiles == 2 ? (depth == 1 ? (s.W <= 32 ? 1 : 2) : -1) : ((s.ntiles == 8 && depth == 8 && s.W <= 32) ? 3 : -1);
        for (int centered = 0; centered < 2; centered++)
            for (int source = 0; source < 2; source++) {
                const int src = source ? plane_src : 0;
                if (src < 0) continue;
                for (int form = 0; form < 3; form++) {
                    // exactly `total` bytes, 16-byte aligned: a store past either end is a report
                    void* mem = nullptr;
                    if (posix_memalign(&mem, 16, total) != 0) return 20;
                    uint8_t* tgt = (uint8_t*)mem;
                    memset(tgt, 0xA5, total);
                    const int rc = sim_obs(map.data(), pos.data(), n, s.H, s.W, src, G, s.oh, s.ow, depth, centered, s.pad, form, form == 0 ? OBS_EPB : 64,
                                           256, nullptr, nullptr, nullptr, tgt);
                    if (rc == -2 || (rc == -3 && src == 0 && form != 0)) { free(tgt); continue; }       // no lean routine / byte maps: k_obs only
                    if (rc != 0) { printf("shape %dx%d window %dx%dx%d source %d form %d: status %d\n", s.H, s.W, s.oh, s.ow, depth, src, form, rc); return 21; }
                    for (size_t o = 0; o < total; o++)
                        if (tgt[o] != want_byte(map.data(), pos.data(), (int)(o / per_env), s.H, s.W, s.oh, s.ow, depth, centered, s.pad, o % per_env)) {
                            printf("shape %dx%d window %dx%dx%d centred %d pad %d source %d form %d: byte %zu is %d\n", s.H, s.W, s.oh, s.ow, depth, centered,
                                   s.pad, src, form, o, tgt[o]);
                            return 22;
                        }
                    images += n; bytes += (long)total;
                    free(tgt);
                }
            }
    }
    // the in-place update: every cell of a map changed to every tile; the window the map itself, larger, smaller, and of odd width
    // (the 7 x 11 map itself is 77 cells, 616 bytes: no multiple of 16, so never updated in place)
    const int wins[4][4] = {{16, 11, 16, 11}, {7, 11, 8, 12}, {7, 11, 6, 8}, {7, 11, 8, 9}};
    for (int wi = 0; wi < 4; wi++) {
        const int H = wins[wi][0], W = wins[wi][1], oh = wins[wi][2], ow = wins[wi][3], n = H * W * 8, pad = 1;
        std::vector<uint8_t> a((size_t)H * W), maps((size_t)n * H * W), pos((size_t)2 * n, 0);
        for (auto& v : a) { rng = rng * 1664525u + 1013904223u; v = (uint8_t)((rng >> 16) & 7); }
        std::vector<int32_t> xy((size_t)2 * n);
        const size_t per_env = (size_t)oh * ow * 8, total = (size_t)n * per_env;
        void* mem = nullptr;
        if (posix_memalign(&mem, 16, total) != 0) return 20;
        uint8_t* tgt = (uint8_t*)mem;
        std::vector<uint8_t> olds((size_t)n * H * W);
        for (int e = 0; e < n; e++) {
            memcpy(&olds[(size_t)e * H * W], a.data(), a.size());
            memcpy(&maps[(size_t)e * H * W], a.data(), a.size());
            const int cell = e >> 3;
            maps[(size_t)e * H * W + cell] = (uint8_t)(e & 7);
            xy[2 * e] = cell % W; xy[2 * e + 1] = cell / W;
        }
        if (sim_obs(olds.data(), pos.data(), n, H, W, 3, 16, oh, ow, 8, 0, pad, 0, OBS_EPB, 256, nullptr, nullptr, nullptr, tgt) != 0) return 30;
        if (sim_obs_delta(maps.data(), n, H, W, 16, oh, ow, pad, xy.data(), tgt) != 0) return 31;
        for (size_t o = 0; o < total; o++)
            if (tgt[o] != want_byte(maps.data(), pos.data(), (int)(o / per_env), H, W, oh, ow, 8, 0, pad, o % per_env)) return 32;
        images += n; bytes += (long)total;
        free(tgt);
    }
    if (images < 5000) return 40;
    printf("images %ld bytes %ld\nok\n", images, bytes);
    return 0;
}
#endif
