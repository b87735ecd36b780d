// weighted_kernels.hpp -- device side of wa_grid_clearance_costs and wa_grid_weighted_fields / _matrix / _paths: exact shortest paths on
// the 6-neighbour lattice of free voxels where entering voxel v costs cost[v] in 1 .. WA_COST_MAX, by a level-synchronous search on the
// bitmaps of geodesic_kernels.hpp (64 voxels of a row per word, one lane per word, blockIdx.y = source).
// The cost is paid on entry, so a voxel's distance is known the first time a neighbour settles: the neighbour with the smallest distance
// settles first, at level L, and the voxel settles at L + cost.  A source keeps a `touched` bitmap and a ring of R = W + 1 frontier
// bitmaps (W = the largest cost present on a free voxel); slot L mod R holds the voxels whose distance is L.  No atomics anywhere: every
// word a lane writes is its own, and the only words it reads from other lanes are in the slot nobody writes in that launch.
// The costs travel as three bit planes of cost - 1 (plane j, bit b of word w = bit j of cost - 1 of that voxel; 0 on occupied voxels and
// padding), shared by all sources of a call; a lane reads them only when its word has newly touched voxels.
#pragma once
#include "geodesic_kernels.hpp"

#define WA_COST_MAX_DEV 8

struct WaThr2 { int32_t n; int32_t v[WA_COST_MAX_DEV - 1]; };

// cost[v] = 0 on occupied voxels, else 1 + #{k : d2[v] <= thr2[k]}; four voxels per lane (both arrays come from the device allocator and
// i is a multiple of 4: aligned), the last lane takes the tail one by one
__global__ __launch_bounds__(256) void k_wgt_clearance_costs(const uint8_t *__restrict__ free_, const int32_t *__restrict__ d2, int64_t n,
                                                             WaThr2 t, uint8_t *__restrict__ cost)
{
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        const int4 d = *reinterpret_cast<const int4 *>(d2 + i);
        const uchar4 f = *reinterpret_cast<const uchar4 *>(free_ + i);
        int32_t c0 = 1, c1 = 1, c2 = 1, c3 = 1;
        for (int32_t k = 0; k < t.n; k++) {
            c0 += d.x <= t.v[k]; c1 += d.y <= t.v[k]; c2 += d.z <= t.v[k]; c3 += d.w <= t.v[k];
        }
        uchar4 o;
        o.x = f.x ? (uint8_t)c0 : 0; o.y = f.y ? (uint8_t)c1 : 0; o.z = f.z ? (uint8_t)c2 : 0; o.w = f.w ? (uint8_t)c3 : 0;
        *reinterpret_cast<uchar4 *>(cost + i) = o;
    } else {
        for (int64_t j = i; j < n; j++) {
            int32_t c = 1;
            for (int32_t k = 0; k < t.n; k++) c += d2[j] <= t.v[k];
            cost[j] = free_[j] ? (uint8_t)c : 0;
        }
    }
}

// cost bytes to the three bit planes of cost - 1, like k_geo_pack: one wavefront per word, the ballots are the words.  The same pass
// validates: info[0] = 1 when a free voxel holds 0 or more than WA_COST_MAX, info[c] = 1 when cost c is present on a free voxel (info is
// zeroed before; every writer of a word stores the same value).  Bytes of occupied voxels are ignored.
__global__ __launch_bounds__(256) void k_wgt_planes(const uint8_t *__restrict__ free_, const uint8_t *__restrict__ cost, WaGeoDims g,
                                                    unsigned long long *__restrict__ planes, int32_t *__restrict__ info)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= g.nw) return;   // (whole waves)
    const int64_t row = w / g.W;
    const int32_t x = (int32_t)(w - row * g.W) * 64 + lane;
    const bool fr = x < g.nx && free_[row * g.nx + x] != 0;
    const int32_t c = fr ? (int32_t)cost[row * g.nx + x] : 1;
    const bool bad = c < 1 || c > WA_COST_MAX_DEV;
    const int32_t m = bad ? 0 : c - 1;
    const unsigned long long p0 = __ballot(m & 1), p1 = __ballot(m & 2), p2 = __ballot(m & 4);
    if (lane == 0) {
        planes[w] = p0;
        planes[g.nw + w] = p1;
        planes[2 * g.nw + w] = p2;
    }
    if (bad) info[0] = 1;
    else if (fr) info[c] = 1;
}

// Level 0 is k_geo_ring_seed without a field: the source's bit in `touched` and in ring slot 0, last[s] = 0 (the last launch that saw a
// frontier or touched a voxel).
// The launch of level L for every source of a chunk (ring of R = W + 1 slots per source, slot = L mod R):
//   1. F = ring[slot] at the lane's word and its six neighbour words (nobody writes that slot in this launch); the voxels of the own word
//      get L in the field, when one is kept (a voxel is in exactly one frontier, so every field entry is written at most once);
//   2. T = neighbours(F) & free & ~touched[w]; touched[w] |= T;
//   3. for k = 1 .. W - 1: T & class_k (cost == k, from the planes) is ORed into slot (L + k) mod R where it is not empty;
//   4. T & class_W is STORED into slot (L + W) mod R = (L - 1) mod R: that slot held the frontier of level L - 1, which nothing reads
//      again, and no earlier level can have scheduled anything for L + W, so the store also clears the ring.  Every lane of a live
//      source does it on every level.
// last[s] = L wherever F or T is not empty.  Once R launches in a row have left it alone the whole ring is empty (every slot has been
// the frontier once and nothing was scheduled since): the source returns at once, and so does one whose targets are all reached
// (stop[s], matrix only).  Blocks of one launch may disagree on stop[s]; that only changes bitmaps nobody reads again.
// Matrix (tgt != NULL): the first block of each source looks its n_tgt targets up in F and stores L in the source's row for those in it.
__global__ __launch_bounds__(256) void k_wgt_level(const unsigned long long *__restrict__ freeb, const unsigned long long *__restrict__ planes,
                                                   WaGeoDims g, int32_t level, int32_t slot, int32_t W,
                                                   unsigned long long *__restrict__ touched, unsigned long long *__restrict__ ring,
                                                   int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop,
                                                   const long long *__restrict__ tgt, int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    const int32_t R = W + 1;
    if (last[s] < level - R || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    unsigned long long *rs = ring + (int64_t)s * R * g.nw;
    const unsigned long long *cur = rs + (int64_t)slot * g.nw;
    if (tgt && blockIdx.x == 0) geo_lookup_targets(cur, g, tgt, n_tgt, mat + (int64_t)s * n_tgt, level, stop + s);
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= g.nw) return;
    const int64_t row = w / g.W;
    const int32_t wx = (int32_t)(w - row * g.W);
    unsigned long long c;
    unsigned long long T = geo_neighbours(cur, g, w, row, wx, &c);
    const int64_t sw = (int64_t)s * g.nw + w;
    const unsigned long long tch = touched[sw];
    T &= freeb[w] & ~tch;
    const int32_t top = slot == 0 ? W : slot - 1;   // (L + W) mod R
    if (c) {
        last[s] = level;
        if (field) geo_store_level(field + (int64_t)s * g.n + row * g.nx + (int64_t)wx * 64, c, level);
    }
    if (!T) {
        rs[(int64_t)top * g.nw + w] = 0ull;
        return;
    }
    touched[sw] = tch | T;
    last[s] = level;
    const unsigned long long p0 = planes[w], p1 = planes[g.nw + w], p2 = planes[2 * g.nw + w];
    int32_t sl = slot;
    for (int32_t k = 1; k < W; k++) {
        sl = sl == W ? 0 : sl + 1;   // (L + k) mod R
        const int32_t b = k - 1;
        const unsigned long long m = T & ((b & 1) ? p0 : ~p0) & ((b & 2) ? p1 : ~p1) & ((b & 4) ? p2 : ~p2);
        if (m) rs[(int64_t)sl * g.nw + w] |= m;
    }
    const int32_t b = W - 1;
    rs[(int64_t)top * g.nw + w] = T & ((b & 1) ? p0 : ~p0) & ((b & 2) ? p1 : ~p1) & ((b & 4) ? p2 : ~p2);
}

// Walk back, one lane per pair, from the end to the start of the pair's field (slot[p] within the chunk): at a node p with distance
// D > 0 the predecessor is the first neighbour in the order -x, +x, -y, +y, -z, +z that is inside the grid and has distance D - cost[p]
// (a voxel with a distance is free; D - cost[p] >= 0 never matches WA_DIST_NONE).
// Counting pass (out == NULL): dist[p] = the field at the end, len[p] = the nodes of the path (0 when unreachable).
// Writing pass: the i-th node from the end goes to out[dst[p] + len[p] - 1 - i], so the path reads start -> end; dst[p] < 0: nothing to
// write (unreachable, or the caller's range is too small).  The field is exact, so a predecessor always exists; the loop still ends if not.
__global__ __launch_bounds__(256) void k_wgt_walkback(const int32_t *__restrict__ field, const uint8_t *__restrict__ cost, WaGeoDims g,
                                                      const int32_t *__restrict__ slot, const long long *__restrict__ end,
                                                      const long long *__restrict__ dst, int32_t n_pairs, int32_t *__restrict__ dist,
                                                      int32_t *__restrict__ len, long long *__restrict__ out)
{
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_pairs) return;
    if (out && dst[p] < 0) return;
    const int32_t *f = field + (int64_t)slot[p] * g.n;
    const int64_t nxy = (int64_t)g.nx * g.ny;
    long long v = end[p];
    int32_t D = f[v];
    if (!out) dist[p] = D;
    int32_t cnt = 0;
    const int32_t total = out ? len[p] : 0;
    long long *o = out ? out + dst[p] : nullptr;
    while (D >= 0) {
        if (out) {
            if (cnt >= total) break;
            o[total - 1 - cnt] = v;
        }
        cnt++;
        if (D == 0) break;
        const int32_t want = D - (int32_t)cost[v];
        if (want < 0) break;
        v = geo_predecessor(f, g, nxy, v, want);
        if (v < 0) break;
        D = want;
    }
    if (!out) len[p] = cnt;
}
