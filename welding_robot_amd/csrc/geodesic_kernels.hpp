// geodesic_kernels.hpp -- device side of wa_grid_geodesic_fields / _matrix / _paths: exact hop counts on the 6-neighbour lattice of free
// voxels by a bit-parallel, level-synchronous breadth-first search, many sources per launch.
// Bitmaps: one bit per voxel, 64 voxels of a row in x per 64-bit word (bit b of word wx = voxel x = 64 wx + b), rows padded to whole
// words: W = ceil(nx / 64) words per row, word index = (z * ny + y) * W + wx, nw = W * ny * nz words per bitmap.  The padding bits of
// the free bitmap are 0, so no level ever sets one.  Every kernel of one search runs on one stream: a level reads what the launch before
// it wrote, nothing inside a launch reads what the same launch writes.
#pragma once
#include "wa_device.h"

struct WaGeoDims {
    int32_t nx, ny, nz;
    int32_t W;        // words per row
    int64_t nw;       // words per bitmap
    int64_t n;        // voxels
};

// ---- what the kernels of this file and of weighted_kernels.hpp share
// voxel id -> its word within a bitmap; *bit = its bit in that word
__device__ __forceinline__ int64_t geo_word_of(long long v, const WaGeoDims &g, int32_t *bit)
{
    const long long row = v / g.nx;
    const int32_t x = (int32_t)(v - row * g.nx);
    *bit = x & 63;
    return row * g.W + (x >> 6);
}

// level 0 of every source of a chunk for the searches that keep a ring of R bitmaps per source (weighted_kernels.hpp and
// chamfer_kernels.hpp): its bit in `seen` and in ring slot 0 (both zeroed before, the whole ring), 0 in its field when one is given (the
// start is not paid for), last[s] = 0, stop[s] = 0.  The weighted search gives none: its field gets the 0 from the launch of level 0.
__global__ __launch_bounds__(256) void k_geo_ring_seed(const long long *__restrict__ src, int32_t n_src, WaGeoDims g, int32_t R,
                                                       unsigned long long *__restrict__ seen, unsigned long long *__restrict__ ring,
                                                       int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop)
{
    const int32_t s = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (s >= n_src) return;
    const long long v = src[s];
    int32_t bit;
    const int64_t w = geo_word_of(v, g, &bit);
    const unsigned long long b = 1ull << bit;
    seen[(int64_t)s * g.nw + w] = b;
    ring[(int64_t)s * R * g.nw + w] = b;
    if (field) field[(int64_t)s * g.n + v] = 0;
    last[s] = 0;
    stop[s] = 0;
}

// The matrix's targets, by all 256 threads of the first block of a source: `value` goes to row_out[t] for every target t in the frontier
// cur (which the launch before completed); once no entry of the row is missing, stop[s] = 1.
__device__ __forceinline__ void geo_lookup_targets(const unsigned long long *__restrict__ cur, const WaGeoDims &g, const long long *__restrict__ tgt,
                                                   int32_t n_tgt, int32_t *__restrict__ row_out, int32_t value, int32_t *__restrict__ stop_s)
{
    int missing = 0;
    for (int32_t t = (int32_t)threadIdx.x; t < n_tgt; t += 256) {
        int32_t bit;
        const int64_t w = geo_word_of(tgt[t], g, &bit);
        if ((cur[w] >> bit) & 1ull) row_out[t] = value;
        else if (row_out[t] < 0) missing = 1;
    }
    if (!__syncthreads_or(missing) && threadIdx.x == 0) *stop_s = 1;
}

// the six neighbours of the voxels of cur, at word w = row * W + wx of one bitmap: the word shifted both ways with the carries of the
// words beside it in the row, ORed with the words at +-1 row and +-1 slab (none across the grid's faces).  *own = cur[w].
__device__ __forceinline__ unsigned long long geo_neighbours(const unsigned long long *__restrict__ cur, const WaGeoDims &g, int64_t w, int64_t row,
                                                             int32_t wx, unsigned long long *own)
{
    const int32_t z = (int32_t)(row / g.ny), y = (int32_t)(row - (int64_t)z * g.ny);
    const int64_t slab = (int64_t)g.W * g.ny;
    const unsigned long long c = cur[w];
    const unsigned long long l = wx > 0 ? cur[w - 1] : 0ull, r = wx < g.W - 1 ? cur[w + 1] : 0ull;
    const unsigned long long ym = y > 0 ? cur[w - g.W] : 0ull, yp = y < g.ny - 1 ? cur[w + g.W] : 0ull;
    const unsigned long long zm = z > 0 ? cur[w - slab] : 0ull, zp = z < g.nz - 1 ? cur[w + slab] : 0ull;
    *own = c;
    return ((c << 1) | (l >> 63)) | ((c >> 1) | (r << 63)) | ym | yp | zm | zp;
}

// f[b] = level for every set bit b of m (m != 0; f: the field at the word's first voxel)
__device__ __forceinline__ void geo_store_level(int32_t *__restrict__ f, unsigned long long m, int32_t level)
{
    do {
        f[__builtin_ctzll(m)] = level;
        m &= m - 1;
    } while (m);
}

// the walk-backs' predecessor of v: the first neighbour in the order -x, +x, -y, +y, -z, +z that is inside the grid and holds `want` in
// the field f; -1 when there is none
__device__ __forceinline__ long long geo_predecessor(const int32_t *__restrict__ f, const WaGeoDims &g, int64_t nxy, long long v, int32_t want)
{
    const int32_t x = (int32_t)(v % g.nx), y = (int32_t)((v / g.nx) % g.ny), z = (int32_t)(v / nxy);
    if (x > 0 && f[v - 1] == want) return v - 1;
    if (x < g.nx - 1 && f[v + 1] == want) return v + 1;
    if (y > 0 && f[v - g.nx] == want) return v - g.nx;
    if (y < g.ny - 1 && f[v + g.nx] == want) return v + g.nx;
    if (z > 0 && f[v - nxy] == want) return v - nxy;
    if (z < g.nz - 1 && f[v + nxy] == want) return v + nxy;
    return -1;
}

// free bytes (1 = free) to the bit-packed copy: one wavefront per word, lane b reads voxel 64 wx + b of the row, the ballot is the word
__global__ __launch_bounds__(256) void k_geo_pack(const uint8_t *__restrict__ free_, WaGeoDims g, unsigned long long *__restrict__ bits)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= g.nw) return;   // (whole waves)
    const int64_t row = w / g.W;
    const int32_t x = (int32_t)(w - row * g.W) * 64 + lane;
    const unsigned long long m = __ballot(x < g.nx && free_[row * g.nx + x] != 0);
    if (lane == 0) bits[w] = m;
}

// out[i] = free byte of voxel ids[i] (the host checks sources and end points with it; ids are inside the grid)
__global__ __launch_bounds__(256) void k_geo_gather_free(const uint8_t *__restrict__ free_, const long long *__restrict__ ids, int64_t n,
                                                         uint8_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = free_[ids[i]];
}

// level 0 of every source of a chunk: its bit in `visited` and in the first frontier (both zeroed before), hop count 0 in its field,
// last[s] = 0 (the last level that produced a new voxel), stop[s] = 0
__global__ __launch_bounds__(256) void k_geo_seed(const long long *__restrict__ src, int32_t n_src, WaGeoDims g,
                                                  unsigned long long *__restrict__ visited, unsigned long long *__restrict__ frontier,
                                                  int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop)
{
    const int32_t s = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (s >= n_src) return;
    const long long v = src[s];
    int32_t bit;
    const int64_t w = (int64_t)s * g.nw + geo_word_of(v, g, &bit);
    const unsigned long long b = 1ull << bit;
    visited[w] = b;
    frontier[w] = b;
    if (field) field[(int64_t)s * g.n + v] = 0;
    last[s] = 0;
    stop[s] = 0;
}

// One level for every source of a chunk: blockIdx.y = source, one lane per word, lanes along x then y then z.
//   next = (cur << 1 | carry from the word before in the row) | (cur >> 1 | carry from the word behind) | words at +-1 row | words at
//          +-1 slab, then & free & ~visited
// cur is the frontier level - 1 produced, nxt receives this level's (every word is written: the buffer holds the frontier of two levels
// ago).  A word with new bits ORs them into visited (this lane is the only one that touches the word), stores `level` at each new voxel
// of the field (when one is kept: every voxel is written at most once per source) and stores last[s] = level: every writer of a launch
// stores the same value.  A source whose last productive level is below level - 1 has an empty frontier and returns at once, and so does
// one whose targets are all reached (stop[s], matrix only).
// Matrix (tgt != NULL): the first block of each source looks up the n_tgt target voxels in cur, which the launch before completed, and
// stores level - 1 in the source's matrix row for those in it; the level after the last productive one sees the last frontier, so every
// non-empty frontier is looked at once.  When the whole row is filled it sets stop[s]; blocks of the same launch may or may not see
// that, which only changes bitmaps nobody reads again.
__global__ __launch_bounds__(256) void k_geo_level(const unsigned long long *__restrict__ freeb, WaGeoDims g, int32_t level,
                                                   unsigned long long *__restrict__ visited, const unsigned long long *__restrict__ cur,
                                                   unsigned long long *__restrict__ nxt, int32_t *__restrict__ field,
                                                   int32_t *__restrict__ last, int32_t *__restrict__ stop,
                                                   const long long *__restrict__ tgt, int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    if (last[s] < level - 1 || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int64_t sb = (int64_t)s * g.nw;
    cur += sb;
    if (tgt && blockIdx.x == 0) geo_lookup_targets(cur, g, tgt, n_tgt, mat + (int64_t)s * n_tgt, level - 1, stop + s);
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= g.nw) return;
    const int64_t row = w / g.W;
    const int32_t wx = (int32_t)(w - row * g.W);
    unsigned long long c;
    unsigned long long m = geo_neighbours(cur, g, w, row, wx, &c);
    const unsigned long long vis = visited[sb + w];
    m &= freeb[w] & ~vis;
    nxt[sb + w] = m;
    if (m) {
        visited[sb + w] = vis | m;
        last[s] = level;
        if (field) geo_store_level(field + (int64_t)s * g.n + row * g.nx + (int64_t)wx * 64, m, level);
    }
}

// hops[p] = field of the pair's start (slot[p] within the chunk) at its end voxel
__global__ __launch_bounds__(256) void k_geo_pair_hops(const int32_t *__restrict__ field, int64_t n, const int32_t *__restrict__ slot,
                                                       const long long *__restrict__ end, int32_t n_pairs, int32_t *__restrict__ hops)
{
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p < n_pairs) hops[p] = field[(int64_t)slot[p] * n + end[p]];
}

// Walk back, one lane per pair: from the end (hop count k) to the start (0); at a node with k > 0 the predecessor is the first
// neighbour in the order -x, +x, -y, +y, -z, +z that is inside the grid and has hop count k - 1 (a voxel with a hop count is free).  The
// node with hop count k is written at out[dst[p] + k], so the path reads start -> end.  dst[p] < 0: nothing to write (unreachable, or
// the caller's range is too small).  The field is exact, so a predecessor always exists; the loop still ends after k steps if not.
__global__ __launch_bounds__(256) void k_geo_walkback(const int32_t *__restrict__ field, WaGeoDims g, const int32_t *__restrict__ slot,
                                                      const long long *__restrict__ end, const long long *__restrict__ dst,
                                                      int32_t n_pairs, long long *__restrict__ out)
{
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_pairs || dst[p] < 0) return;
    const int32_t *f = field + (int64_t)slot[p] * g.n;
    const int64_t nxy = (int64_t)g.nx * g.ny;
    long long v = end[p];
    long long *o = out + dst[p];
    for (int32_t k = f[v]; k >= 0; k--) {
        o[k] = v;
        if (k == 0) break;
        v = geo_predecessor(f, g, nxy, v, k - 1);
        if (v < 0) break;
    }
}
