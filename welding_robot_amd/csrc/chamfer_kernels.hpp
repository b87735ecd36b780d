// chamfer_kernels.hpp -- device side of wa_grid_chamfer_fields / _matrix / _paths: exact shortest paths on the 26-neighbour lattice of free
// voxels with integer step weights step[0], step[1], step[2] for face, edge and corner moves, by a level-synchronous search on the bitmaps
// of geodesic_kernels.hpp (64 voxels of a row per word, one lane per word, blockIdx.y = source).
// A move u -> v exists iff every voxel of the box the two span is free.  A voxel first reached by an expensive move can later be reached
// more cheaply, so nothing is scheduled ahead (weighted_kernels.hpp's push form): level L PULLS.  A source keeps a `done` bitmap and a
// ring of R = max(step) + 1 bitmaps, slot L mod R = S_L, the voxels whose distance is exactly L; the launch of level L computes S_L from
// S_{L - step[0]}, S_{L - step[1]}, S_{L - step[2]}, which earlier launches completed, and stores it whole into its own slot.  No atomics:
// every word a lane writes is its own.
// The move-allowed masks are built in the launch from the free words of the lane's row and its eight neighbour rows, which all sources of
// a call share (DESIGN 4q says why they are not precomputed).
#pragma once
#include "geodesic_kernels.hpp"

#define WA_STEP_MAX_DEV 16

struct WaChmStep { int32_t s[3]; int32_t M; };   // M = the largest of the three

// a bitmap row seen from word w: m / c / p hold, at bit b, the row's bit at x - 1 / x / x + 1 (x = 64 wx + b); nothing beyond the row's ends
struct ChmRow { unsigned long long m, c, p; };

__device__ __forceinline__ ChmRow chm_row(const unsigned long long *__restrict__ B, int64_t w, bool has_l, bool has_r)
{
    const unsigned long long c = B[w], l = has_l ? B[w - 1] : 0ull, r = has_r ? B[w + 1] : 0ull;
    ChmRow o;
    o.m = (c << 1) | (l >> 63);
    o.c = c;
    o.p = (c >> 1) | (r << 63);
    return o;
}

// level 0 of every source of a chunk: its bit in `done` and in ring slot 0 (both zeroed before, the whole ring), 0 in its field, last[s] = 0
// (the last level that settled a voxel), stop[s] = 0
__global__ __launch_bounds__(256) void k_chm_seed(const long long *__restrict__ src, int32_t n_src, WaGeoDims g, int32_t R,
                                                  unsigned long long *__restrict__ done, unsigned long long *__restrict__ ring,
                                                  int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop)
{
    const int32_t s = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (s >= n_src) return;
    const long long v = src[s];
    int32_t bit;
    const int64_t w = geo_word_of(v, g, &bit);
    const unsigned long long b = 1ull << bit;
    done[(int64_t)s * g.nw + w] = b;
    ring[(int64_t)s * R * g.nw + w] = b;
    if (field) field[(int64_t)s * g.n + v] = 0;
    last[s] = 0;
    stop[s] = 0;
}

// The launch of level L >= 1 for every source of a chunk (ring of R = M + 1 slots per source, slot = L mod R).  The lane of word w, whose
// voxels p are the TARGETS of the moves:
//   cand = for every offset o of class a with L >= step[a - 1]: (S_{L - step[a - 1]} seen at p + o) & (every other voxel of the box of p and
//          p + o is free); a row outside the grid has no voxels, and a source voxel in S is free by construction:
//     face   -+x: S1 at x -+ 1;  +-y, +-z: S1 of that row
//     edge   (sx, sy, 0): S2 of row y + sy at x + sx  &  free(x + sx, y)  &  free(x, y + sy); likewise (sx, 0, sz);
//            (0, sy, sz): S2 of row (y + sy, z + sz)  &  free(x, y + sy)  &  free(x, z + sz)
//     corner (sx, sy, sz): S3 of row (y + sy, z + sz) at x + sx  &  the six free bits of the box's other voxels
//   S = cand & free[w] & ~done[w] is STORED into slot L mod R on every level: that slot held S_{L - R}, which nothing reads any more.
//   Where S is not empty: done[w] |= S, L goes to the field at S's voxels (when one is kept), last[s] = L.
// A word with nothing left to settle (free & ~done empty) stores 0 without reading its neighbourhood.
// A source whose last M levels settled nothing has nothing left in reach of a pull and returns at once, and so does one whose targets are
// all reached (stop[s], matrix only).  Blocks of one launch may disagree on stop[s]; that only changes bitmaps nobody reads again.
// Matrix (tgt != NULL): the first block of each source looks its n_tgt targets up in S_{L - 1}, which the launch before completed (the seed
// for L = 1), and stores L - 1 in the source's row for those in it; the launch after the last productive level sees that level's set.
__global__ __launch_bounds__(256) void k_chm_level(const unsigned long long *__restrict__ freeb, WaGeoDims g, int32_t level, int32_t slot,
                                                   WaChmStep st, unsigned long long *__restrict__ done, unsigned long long *__restrict__ ring,
                                                   int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop,
                                                   const long long *__restrict__ tgt, int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    if (last[s] < level - st.M || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t R = st.M + 1;
    unsigned long long *rs = ring + (int64_t)s * R * g.nw;
    if (tgt && blockIdx.x == 0)
        geo_lookup_targets(rs + (int64_t)(slot == 0 ? st.M : slot - 1) * g.nw, g, tgt, n_tgt, mat + (int64_t)s * n_tgt, level - 1, stop + s);
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= g.nw) return;
    const int64_t sw = (int64_t)s * g.nw + w;
    const unsigned long long dn = done[sw];
    const unsigned long long open = freeb[w] & ~dn;
    unsigned long long *mine = rs + (int64_t)slot * g.nw + w;
    if (!open) {
        *mine = 0ull;
        return;
    }
    const int64_t row = w / g.W;
    const int32_t wx = (int32_t)(w - row * g.W);
    const int32_t z = (int32_t)(row / g.ny), y = (int32_t)(row - (int64_t)z * g.ny);
    const bool hl = wx > 0, hr = wx < g.W - 1;
    const bool vy[2] = {y > 0, y < g.ny - 1}, vz[2] = {z > 0, z < g.nz - 1};
    const int64_t oy[2] = {-(int64_t)g.W, (int64_t)g.W}, oz[2] = {-(int64_t)g.W * g.ny, (int64_t)g.W * g.ny};
    const ChmRow none = {0ull, 0ull, 0ull};
    const ChmRow f0 = chm_row(freeb, w, hl, hr);
    ChmRow fy[2], fz[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        fy[i] = vy[i] ? chm_row(freeb, w + oy[i], hl, hr) : none;
        fz[i] = vz[i] ? chm_row(freeb, w + oz[i], hl, hr) : none;
    }
    unsigned long long cand = 0ull;
    if (level >= st.s[0]) {
        const int32_t sl = slot - st.s[0];
        const unsigned long long *S = rs + (int64_t)(sl < 0 ? sl + R : sl) * g.nw;
        const ChmRow r = chm_row(S, w, hl, hr);
        cand = r.m | r.p;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (vy[i]) cand |= S[w + oy[i]];
            if (vz[i]) cand |= S[w + oz[i]];
        }
    }
    if (level >= st.s[1]) {
        const int32_t sl = slot - st.s[1];
        const unsigned long long *S = rs + (int64_t)(sl < 0 ? sl + R : sl) * g.nw;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (vy[i]) {
                const ChmRow r = chm_row(S, w + oy[i], hl, hr);
                cand |= fy[i].c & ((r.m & f0.m) | (r.p & f0.p));
            }
            if (vz[i]) {
                const ChmRow r = chm_row(S, w + oz[i], hl, hr);
                cand |= fz[i].c & ((r.m & f0.m) | (r.p & f0.p));
            }
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (vy[i] && vz[j]) cand |= S[w + oy[i] + oz[j]] & fy[i].c & fz[j].c;
        }
    }
    if (level >= st.s[2]) {
        const int32_t sl = slot - st.s[2];
        const unsigned long long *S = rs + (int64_t)(sl < 0 ? sl + R : sl) * g.nw;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (vy[i] && vz[j]) {
                    const int64_t wc = w + oy[i] + oz[j];
                    const ChmRow r = chm_row(S, wc, hl, hr);
                    cand |= fy[i].c & fz[j].c & freeb[wc] &((r.m & f0.m & fy[i].m & fz[j].m) | (r.p & f0.p & fy[i].p & fz[j].p));
                }
    }
    const unsigned long long S = cand & open;
    *mine = S;
    if (S) {
        done[sw] = dn | S;
        last[s] = level;
        if (field) geo_store_level(field + (int64_t)s * g.n + row * g.nx + (int64_t)wx * 64, S, level);
    }
}

// the walk-backs' predecessor of v = (x, y, z) with distance D in the field f: the first offset o, in the order -x, +x, -y, +y, -z, +z,
// then the 12 edge offsets, then the 8 corner offsets (both sorted by (dz, dy, dx) ascending), for which q = v + o is inside the grid,
// f[q] = D - step[class(o)] >= 0 and every voxel of the box of v and q is free; -1 when there is none.  *paid = the step's cost.
__device__ __forceinline__ long long chm_predecessor(const int32_t *__restrict__ f, const uint8_t *__restrict__ free_, const WaGeoDims &g,
                                                     const WaChmStep &st, long long v, int32_t D, int32_t *paid)
{
    const int64_t nxy = (int64_t)g.nx * g.ny;
    const int32_t x = (int32_t)(v % g.nx), y = (int32_t)((v / g.nx) % g.ny), z = (int32_t)(v / nxy);
    for (int32_t cls = 1; cls <= 3; cls++) {
        const int32_t want = D - st.s[cls - 1];
        if (want < 0) continue;
        for (int32_t k = 0; k < 27; k++) {
            int32_t dx, dy, dz;
            if (cls == 1) {
                if (k >= 6) break;
                const int32_t sgn = (k & 1) ? 1 : -1;
                dx = k < 2 ? sgn : 0; dy = (k >> 1) == 1 ? sgn : 0; dz = k >= 4 ? sgn : 0;
            } else {
                dx = k % 3 - 1; dy = (k / 3) % 3 - 1; dz = k / 9 - 1;   // (dz, dy, dx) ascending
                if ((dx != 0) + (dy != 0) + (dz != 0) != cls) continue;
            }
            const int32_t qx = x + dx, qy = y + dy, qz = z + dz;
            if (qx < 0 || qx >= g.nx || qy < 0 || qy >= g.ny || qz < 0 || qz >= g.nz) continue;
            const long long q = v + dx + (long long)dy * g.nx + (long long)dz * nxy;
            if (f[q] != want) continue;
            // v and q are free (both hold a distance); the other voxels of the box
            bool ok = true;
            if (cls >= 2) {
                for (int32_t c = 1; c < 7 && ok; c++) {
                    const int32_t ax = (c & 1) ? dx : 0, ay = (c & 2) ? dy : 0, az = (c & 4) ? dz : 0;
                    if (((c & 1) && !dx) || ((c & 2) && !dy) || ((c & 4) && !dz)) continue;   // (a corner already looked at)
                    ok = free_[v + ax + (long long)ay * g.nx + (long long)az * nxy] != 0;
                }
            }
            if (ok) { *paid = st.s[cls - 1]; return q; }
        }
    }
    return -1;
}

// Walk back, one lane per pair, from the end to the start of the pair's field (slot[p] within the chunk) by chm_predecessor.
// Counting pass (out == NULL): dist[p] = the field at the end, len[p] = the nodes of the path (0 when unreachable).
// Writing pass: the i-th node from the end goes to out[dst[p] + len[p] - 1 - i], so the path reads start -> end; dst[p] < 0: nothing to
// write (unreachable, or the caller's range is too small).  The field is exact, so a predecessor always exists; the loop still ends if not.
__global__ __launch_bounds__(256) void k_chm_walkback(const int32_t *__restrict__ field, const uint8_t *__restrict__ free_, WaGeoDims g,
                                                      WaChmStep st, const int32_t *__restrict__ slot, const long long *__restrict__ end,
                                                      const long long *__restrict__ dst, int32_t n_pairs, int32_t *__restrict__ dist,
                                                      int32_t *__restrict__ len, long long *__restrict__ out)
{
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_pairs) return;
    if (out && dst[p] < 0) return;
    const int32_t *f = field + (int64_t)slot[p] * g.n;
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
        int32_t paid = 0;
        v = chm_predecessor(f, free_, g, st, v, D, &paid);
        if (v < 0) break;
        D -= paid;
    }
    if (!out) len[p] = cnt;
}
