// chamfer_weighted_kernels.hpp -- device side of wa_grid_chamfer_weighted_fields / _matrix / _paths: exact shortest paths on the
// 26-neighbour lattice of free voxels (chamfer_kernels.hpp's graph, box rule and step weights) where the move u -> v costs
// step[class - 1] + pen[v], pen a per-voxel penalty in 0 .. WA_PEN_MAX paid once per voxel entered.
// The two searches this combines compose: the step belongs to the move, so a level PULLS from the settled sets of earlier levels
// (chamfer_kernels.hpp); the penalty is paid on entry, so the first pull that reaches a voxel fixes its distance (weighted_kernels.hpp's
// push, into the lane's own word).  A source keeps an `arrived` bitmap and a ring of R = M + P + 1 bitmaps (M = max(step), P = the
// largest penalty present on a free voxel), slot L mod R = S_L, the voxels whose distance is exactly L.  Levels ascend and a pull reads
// only S_{L - step}, complete since the launch of level L - 1, so the first level A at which a pull reaches a voxel is the least
// dist(u) + step over its moves, and the voxel's distance is A + pen: it goes into slot A + pen at once and gets A + pen in the field.
// One 26-offset gather per level, whatever the penalties.  No atomics: every word a lane writes is its own, and the slots it reads
// from other words (L - step <= L - 1) are written by no lane of the launch (a launch writes slots L .. L + P).
// The penalties travel as five bit planes (plane j, bit b of word w = bit j of pen of that voxel; 0 on occupied voxels and padding),
// shared by all sources of a call; a lane reads them only when voxels of its word arrive.
#pragma once
#include "chamfer_kernels.hpp"

#define WA_PEN_MAX_DEV 31
#define WA_PEN_PLANES 5

struct WaCwStep { int32_t s[3]; int32_t M, P; };   // M = the largest step, P = the largest penalty present on a free voxel

// penalty bytes to the five bit planes, like k_wgt_planes: one wavefront per word, the ballots are the words.  The same pass validates:
// info[0] = 1 when a free voxel holds more than WA_PEN_MAX, info[1 + q] = 1 when penalty q is present on a free voxel (info is zeroed
// before; every writer of a word stores the same value).  Bytes of occupied voxels are ignored.
__global__ __launch_bounds__(256) void k_cw_planes(const uint8_t *__restrict__ free_, const uint8_t *__restrict__ pen, WaGeoDims g,
                                                   unsigned long long *__restrict__ planes, int32_t *__restrict__ info)
{
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= g.nw) return;   // (whole waves)
    const int64_t row = w / g.W;
    const int32_t x = (int32_t)(w - row * g.W) * 64 + lane;
    const bool fr = x < g.nx && free_[row * g.nx + x] != 0;
    const int32_t q = fr ? (int32_t)pen[row * g.nx + x] : 0;
    const bool bad = q > WA_PEN_MAX_DEV;
    const int32_t m = bad ? 0 : q;
    unsigned long long p[WA_PEN_PLANES];
#pragma unroll
    for (int j = 0; j < WA_PEN_PLANES; j++) p[j] = __ballot((m >> j) & 1);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < WA_PEN_PLANES; j++) planes[(int64_t)j * g.nw + w] = p[j];
    }
    if (bad) info[0] = 1;
    else if (fr) info[1 + q] = 1;
}

// level 0 of every source of a chunk: its bit in `arrived` and in ring slot 0 (both zeroed before, the whole ring), 0 in its field (the
// start is not paid for), last[s] = 0 (the last level at which a voxel arrived), stop[s] = 0
__global__ __launch_bounds__(256) void k_cw_seed(const long long *__restrict__ src, int32_t n_src, WaGeoDims g, int32_t R,
                                                 unsigned long long *__restrict__ arrived, unsigned long long *__restrict__ ring,
                                                 int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop)
{
    const int32_t s = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (s >= n_src) return;
    const long long v = src[s];
    int32_t bit;
    const int64_t w = geo_word_of(v, g, &bit);
    const unsigned long long b = 1ull << bit;
    arrived[(int64_t)s * g.nw + w] = b;
    ring[(int64_t)s * R * g.nw + w] = b;
    if (field) field[(int64_t)s * g.n + v] = 0;
    last[s] = 0;
    stop[s] = 0;
}

// k_chm_level's gather, restated for a ring of R slots: the voxels of word w that a move of cost step[a - 1] reaches from S_{L - step[a - 1]}
// (see k_chm_level for the masks).  rs = the source's ring, slot = L mod R, R > M.
__device__ __forceinline__ unsigned long long cw_gather(const unsigned long long *__restrict__ freeb, const unsigned long long *__restrict__ rs,
                                                        const WaGeoDims &g, const WaCwStep &st, int32_t R, int32_t level, int32_t slot, int64_t w)
{
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
                    cand |= fy[i].c & fz[j].c & freeb[wc] & ((r.m & f0.m & fy[i].m & fz[j].m) | (r.p & f0.p & fy[i].p & fz[j].p));
                }
    }
    return cand;
}

// The launch of level L >= 1 for every source of a chunk (ring of R = M + P + 1 slots per source, slot = L mod R).  The lane of word w:
//   A = cw_gather & free[w] & ~arrived[w]: the voxels a pull reaches for the first time; arrived[w] |= A, last[s] = L where A is not empty.
//   A's voxels of penalty P are STORED into slot (L + P) mod R on every level and in every word, the early-returning ones included: that
//   slot held S_{L - M - 1}, which no launch reads again (level L reads L - step >= L - M), and no earlier level can have put anything
//   there (L' + q = L + P with q <= P needs L' >= L).  The store is also the clearing of the ring.
//   A's voxels of penalty q < P are ORed into slot (L + q) mod R where there are any; the field (when one is kept) gets L + q at once, so
//   no word is visited again when its voxels settle.  With P = 0 this is k_chm_level's store.
// A word with nothing left to arrive (free & ~arrived empty) stores its 0 without reading its neighbourhood or the planes.
// An arrival at level L settles by L + P and is pulled from by L + P + M, so a source whose last M + P levels had no arrival is
// finished and returns at once, and so does one whose targets are all reached (stop[s], matrix only).  Blocks of one launch may
// disagree on stop[s]; that only changes bitmaps nobody reads again.
// Matrix (tgt != NULL): the first block of each source looks its n_tgt targets up in S_{L - 1}, complete since the launch before (only
// levels <= L - 1 write it), and stores L - 1 in the source's row for those in it.
__global__ __launch_bounds__(256) void k_cw_level(const unsigned long long *__restrict__ freeb, const unsigned long long *__restrict__ planes,
                                                  WaGeoDims g, int32_t level, int32_t slot, WaCwStep st,
                                                  unsigned long long *__restrict__ arrived, unsigned long long *__restrict__ ring,
                                                  int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop,
                                                  const long long *__restrict__ tgt, int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    if (last[s] < level - (st.M + st.P) || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t R = st.M + st.P + 1;
    unsigned long long *rs = ring + (int64_t)s * R * g.nw;
    if (tgt && blockIdx.x == 0)
        geo_lookup_targets(rs + (int64_t)(slot == 0 ? R - 1 : slot - 1) * g.nw, g, tgt, n_tgt, mat + (int64_t)s * n_tgt, level - 1, stop + s);
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= g.nw) return;
    const int64_t sw = (int64_t)s * g.nw + w;
    const unsigned long long arr = arrived[sw];
    const unsigned long long open = freeb[w] & ~arr;
    const int32_t tp = slot + st.P;
    unsigned long long *top = rs + (int64_t)(tp >= R ? tp - R : tp) * g.nw + w;   // (L + P) mod R
    if (!open) {
        *top = 0ull;
        return;
    }
    unsigned long long A = cw_gather(freeb, rs, g, st, R, level, slot, w) & open;
    if (!A) {
        *top = 0ull;
        return;
    }
    arrived[sw] = arr | A;
    last[s] = level;
    unsigned long long p[WA_PEN_PLANES];
#pragma unroll
    for (int j = 0; j < WA_PEN_PLANES; j++) p[j] = planes[(int64_t)j * g.nw + w];
    int32_t *f = nullptr;
    if (field) {
        const int64_t row = w / g.W;
        f = field + (int64_t)s * g.n + row * g.nx + (w - row * g.W) * 64;
    }
    // one trip per penalty value present among A's voxels: q of A's lowest voxel, then every voxel of A with that q
    unsigned long long of_top = 0ull;
    do {
        const int b = __builtin_ctzll(A);
        int32_t q = 0;
        unsigned long long m = A;
#pragma unroll
        for (int j = 0; j < WA_PEN_PLANES; j++) {
            const bool on = (p[j] >> b) & 1ull;
            q |= on ? (1 << j) : 0;
            m &= on ? p[j] : ~p[j];
        }
        A &= ~m;
        if (f) geo_store_level(f, m, level + q);
        if (q == st.P) of_top = m;
        else {
            const int32_t sl = slot + q;
            rs[(int64_t)(sl >= R ? sl - R : sl) * g.nw + w] |= m;
        }
    } while (A);
    *top = of_top;
}

// Walk back, one lane per pair, from the end to the start of the pair's field (slot[p] within the chunk): at a node v with distance
// D > 0 the predecessor is chm_predecessor's for D - pen[v], that is the first offset o in chamfer_kernels.hpp's order for which the move
// exists and the voxel holds D - pen[v] - step[class(o) - 1] >= 0, which is then the distance to go on with.
// Counting pass (out == NULL): dist[p] = the field at the end, len[p] = the nodes of the path (0 when unreachable).
// Writing pass: the i-th node from the end goes to out[dst[p] + len[p] - 1 - i], so the path reads start -> end; dst[p] < 0: nothing to
// write (unreachable, or the caller's range is too small).  The field is exact, so a predecessor always exists; the loop still ends if not.
__global__ __launch_bounds__(256) void k_cw_walkback(const int32_t *__restrict__ field, const uint8_t *__restrict__ free_, const uint8_t *__restrict__ pen,
                                                     WaGeoDims g, WaChmStep st, const int32_t *__restrict__ slot, const long long *__restrict__ end,
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
        const int32_t moved = D - (int32_t)pen[v];
        int32_t paid = 0;
        v = chm_predecessor(f, free_, g, st, v, moved, &paid);
        if (v < 0) break;
        D = moved - paid;
    }
    if (!out) len[p] = cnt;
}
