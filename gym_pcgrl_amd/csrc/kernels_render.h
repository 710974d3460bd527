// Level pictures on the device (pcgrl_render): PcgrlEnv.render (pcgrl_env.py:161-175) = Problem.render (problem.py:134-156: a frame of
// the border tile around the map, every cell the picture of its tile) + the representation's cursor frame (narrow_rep.py:128-142,
// turtle_rep.py:142: the two outermost pixel rows and columns of the cursor's cell in (255, 0, 0)) -- for `count` chosen environments
// in one launch, stacked or laid out on a grid.  Part of the core part of pcgrl_abi.hip.
//
// A pure function of the byte map, the cursor and a small palette, and a store stream like k_obs (kernels_obs.h): 14 x 14 cells at
// 16-pixel tiles are 196 608 bytes an image.  The output is cut into cells (one image each; the stacked form is a grid one image
// wide) and a cell into bands of whole tile rows: a work unit is one band, a block takes units in a grid-stride loop.  The block
// keeps in LDS the palette (staged once) and the tile ids of its band, frame included (staged per unit); every output byte is then
// a function of two LDS reads.
//   fast path   (tile_size * 3) % 16 == 0 -- the reference's 16-pixel tiles: a 16-byte piece of a pixel row lies inside one tile, so a
//               thread's work item is one piece: tile id -> one ds_read_b128 of the palette row -> one dwordx4 store; consecutive
//               lanes take consecutive pieces (a wavefront writes 1 KB contiguous).  Row stride, band and image offsets are multiples
//               of 16 by construction, `out` is checked by the host.  The pieces of the cursor's cell are patched in registers.
//   general     any tile size 1..64: a work item is one byte, the palette is read from memory (cached).  For correctness only.
// Every byte of `out` is written: cells beyond `count` and images of an index outside [0, N) are zero.  All output offsets are
// 64-bit (540 images of a 100 x 100 map pass 4 GB).  No atomics, no scratch.
#pragma once

struct RenderArgs {
    const uint8_t* map;          // u8 [N][H][W]
    const uint8_t* pos;          // u8 [N][2] (x, y); NULL: no cursor frame
    const int32_t* indices;      // i32 [count]; NULL: 0 .. count-1
    const uint8_t* tiles;        // u8 [ntiles][ts][ts][3]
    uint8_t* out;
    long long cells;             // cells of the output (stacked: count)
    int32_t N, W, H, ntiles, ts, bx, by, border_tile;
    int32_t count;
    int32_t gcols;               // images side by side (stacked: 1)
    int32_t band, nbands;        // tile rows a work unit draws, units per cell
    int32_t pal_bytes;           // fast path: ntiles * ts * ts * 3 (a multiple of 16), staged in LDS in front of the ids
};
#define RENDER_IDS_MAX 8192      /* tile ids of a band (band * (W + 2 bx) bytes of LDS) */
#define RENDER_BAND_BYTES (192 * 1024)   /* what a unit writes, where the image is that large: 48 pieces a thread */

// the two-pixel frame inside a cell of ts x ts pixels, clipped like the host's slices [:2], [-2:] (ts <= 4: the whole cell)
__device__ __forceinline__ bool render_on_frame(int py, int px, int ts) { return py < 2 || py >= ts - 2 || px < 2 || px >= ts - 2; }

// FAST 1: 16-byte pieces, palette in LDS.  FAST 0: bytes, palette from memory.
template <int FAST>
__global__ __launch_bounds__(256) void k_render(RenderArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t render_lds[];
    uint8_t* ids = render_lds + (FAST ? A.pal_bytes : 0);
    const int tid = (int)threadIdx.x;
    const int ts = A.ts, Wp = A.W + 2 * A.bx, Hp = A.H + 2 * A.by;
    const int tile_row = ts * 3;                             // bytes of one pixel row of a tile
    const size_t row_bytes = (size_t)Wp * tile_row;          // ... of an image
    const size_t out_stride = row_bytes * (size_t)A.gcols;   // ... of the output
    if (FAST) {
        if ((reinterpret_cast<uintptr_t>(A.tiles) & 15) == 0)
            for (int i = tid; i < A.pal_bytes >> 4; i += 256) reinterpret_cast<uint4*>(render_lds)[i] = reinterpret_cast<const uint4*>(A.tiles)[i];
        else
            for (int i = tid; i < A.pal_bytes; i += 256) render_lds[i] = A.tiles[i];
    }
    const long long units = A.cells * A.nbands;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long cell = u / A.nbands;
        const int ty0 = (int)(u - cell * A.nbands) * A.band;
        const int nrows = (Hp - ty0) < A.band ? (Hp - ty0) : A.band;         // tile rows of this unit
        // which environment (block-uniform); none: a black image
        long long e = -1;
        if (cell < A.count) e = A.indices ? (long long)A.indices[cell] : cell;
        const bool black = e < 0 || e >= A.N;
        int cx = -1, cy = -1;                                 // the cursor's cell in frame coordinates, (-1, -1): none in this band
        __syncthreads();                                      // (the previous unit's ids are read no more; the palette is there)
        if (!black) {
            const uint8_t* m = A.map + (size_t)e * A.H * A.W;
            for (int i = tid; i < nrows * Wp; i += 256) {
                const int r = i / Wp, tx = i - r * Wp;
                const int y = ty0 + r - A.by, x = tx - A.bx;
                int t = A.border_tile;
                if ((unsigned)y < (unsigned)A.H && (unsigned)x < (unsigned)A.W) {
                    t = (int)m[(size_t)y * A.W + x];
                    t = t < A.ntiles ? t : A.ntiles - 1;      // (the map holds tile ids; never read past the palette)
                }
                ids[i] = (uint8_t)t;
            }
            if (A.pos) {
                const int px = (int)A.pos[2 * e] + A.bx, py = (int)A.pos[2 * e + 1] + A.by - ty0;
                if (py >= 0 && py < nrows) { cx = px; cy = py; }
            }
        }
        __syncthreads();
        const size_t cell_r = (size_t)(cell / A.gcols), cell_c = (size_t)(cell - (long long)cell_r * A.gcols);
        uint8_t* o = A.out + (cell_r * Hp + ty0) * ts * out_stride + cell_c * row_bytes;     // first byte of the band
        if (FAST) {
            const int ppt = tile_row >> 4, ppr = Wp * ppt;    // pieces per tile row / per image row
            const int total = nrows * ts * ppr;               // < 2^24 (RENDER_BAND_BYTES, or one tile row of at most 4606 x 64 x 12 pieces)
            const int dr = 256 / ppr, dp = 256 - dr * ppr;
            const uint32_t mg_ppt = 0xFFFFFFFFu / (uint32_t)ppt + 1u, mg_ts = 0xFFFFFFFFu / (uint32_t)ts + 1u;   // exact floors: kernels_obs.h obs_magic
            int r = tid / ppr, p = tid - r * ppr;             // pixel row of the band, piece of the row: carried along, not divided out
            for (int i = tid; i < total; i += 256) {
                uint4 w = make_uint4(0u, 0u, 0u, 0u);
                if (!black) {
                    const int tx = (int)__umulhi((uint32_t)p, mg_ppt), sub = p - tx * ppt;
                    const int ty = (int)__umulhi((uint32_t)r, mg_ts), py = r - ty * ts;
                    const int t = (int)ids[ty * Wp + tx];
                    w = *reinterpret_cast<const uint4*>(render_lds + (t * ts + py) * tile_row + (sub << 4));
                    if (tx == cx && ty == cy) {               // the cursor's cell: at most ts * ppt pieces of the image
                        uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                        for (int k = 0; k < 16; k++) {
                            const int b = (sub << 4) + k, px = (int)__umulhi((uint32_t)b, 0x55555556u), ch = b - 3 * px;
                            if (render_on_frame(py, px, ts)) v[k >> 2] = (v[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | ((ch == 0 ? 0xFFu : 0u) << (8 * (k & 3)));
                        }
                        w = make_uint4(v[0], v[1], v[2], v[3]);
                    }
                }
                *reinterpret_cast<uint4*>(o + (size_t)r * out_stride + ((size_t)p << 4)) = w;
                r += dr; p += dp;
                if (p >= ppr) { p -= ppr; ++r; }
            }
        } else {
            const int rb = (int)row_bytes;                    // at most 4606 x 64 x 3
            const long long total = (long long)nrows * ts * rb;
            for (long long i = tid; i < total; i += 256) {
                const int r = (int)(i / rb), b = (int)(i - (long long)r * rb);
                uint8_t v = 0;
                if (!black) {
                    const int px_row = b / 3, ch = b - 3 * px_row;
                    const int tx = px_row / ts, px = px_row - tx * ts, ty = r / ts, py = r - ty * ts;
                    const int t = (int)ids[ty * Wp + tx];
                    v = A.tiles[((size_t)(t * ts + py) * ts + px) * 3 + ch];
                    if (tx == cx && ty == cy && render_on_frame(py, px, ts)) v = ch == 0 ? 255 : 0;
                }
                o[(size_t)r * out_stride + b] = v;
            }
        }
    }
}
