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
// wa_grid_chamfer_weighted_fields / _matrix / _paths run on the same kernels: the move u -> v costs step[class - 1] + pen[v], pen a
// per-voxel penalty in 0 .. WA_PEN_MAX paid once per voxel entered.  The step belongs to the move, so a level still pulls from the
// settled sets of earlier levels; the penalty is paid on entry, so the first pull that reaches a voxel fixes its distance
// (weighted_kernels.hpp's push, into the lane's own word).  `done` becomes `arrived`, the ring has R = M + P + 1 slots (P = the largest
// penalty present on a free voxel).  Levels ascend and a pull reads only S_{L - step}, complete since the launch of level L - 1, so the
// first level A at which a pull reaches a voxel is the least dist(u) + step over its moves, and the voxel's distance is A + pen: it goes
// into slot A + pen at once and gets A + pen in the field.  One 26-offset gather per level, whatever the penalties.
// The penalties travel as five bit planes (plane j, bit b of word w = bit j of pen of that voxel; 0 on occupied voxels and padding),
// shared by all sources of a call; a lane reads them only when voxels of its word arrive.
#pragma once
#include "geodesic_kernels.hpp"

#define WA_STEP_MAX_DEV 16
#define WA_PEN_MAX_DEV 31
#define WA_PEN_PLANES 5

struct WaChmStep { int32_t s[3]; int32_t M, P; };   // M = the largest step, P = the largest penalty present on a free voxel (0 without penalties)

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

// The 26-offset gather of level L for the lane of word w, whose voxels p are the TARGETS of the moves: for every offset o of class a with
// L >= step[a - 1], (S_{L - step[a - 1]} seen at p + o) & (every other voxel of the box of p and p + o is free); a row outside the grid
// has no voxels, and a source voxel in S is free by construction:
//     face   -+x: S1 at x -+ 1;  +-y, +-z: S1 of that row
//     edge   (sx, sy, 0): S2 of row y + sy at x + sx  &  free(x + sx, y)  &  free(x, y + sy); likewise (sx, 0, sz);
//            (0, sy, sz): S2 of row (y + sy, z + sz)  &  free(x, y + sy)  &  free(x, z + sz)
//     corner (sx, sy, sz): S3 of row (y + sy, z + sz) at x + sx  &  the six free bits of the box's other voxels
// rs = the source's ring of R > M slots, slot = L mod R.  Not yet masked by the word's own free and settled bits.
__device__ __forceinline__ unsigned long long chm_gather(const unsigned long long *__restrict__ freeb, const unsigned long long *__restrict__ rs,
                                                         const WaGeoDims &g, const WaChmStep &st, int32_t R, int32_t level, int32_t slot, int64_t w)
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

// source s's field at the first voxel of word w (the word's x index as 32 bits: what k_chm_ring_level<false>'s registers were measured with)
__device__ __forceinline__ int32_t *chm_field_word(int32_t *__restrict__ field, int32_t s, const WaGeoDims &g, int64_t w)
{
    const int64_t row = w / g.W;
    const int32_t wx = (int32_t)(w - row * g.W);
    return field + (int64_t)s * g.n + row * g.nx + (int64_t)wx * 64;
}

// The launch of level L >= 1 for every source of a chunk (ring of R = M + P + 1 slots per source, slot = L mod R).  The lane of word w:
//   A = chm_gather & free[w] & ~arrived[w]: the voxels a pull reaches for the first time; arrived[w] |= A, last[s] = L where A is not empty.
//   A's voxels of penalty P are STORED into slot (L + P) mod R on every level and in every word, the early-returning ones included.
//   A's voxels of penalty q < P are ORed into slot (L + q) mod R where there are any; the field (when one is kept) gets L + q at once, so
//   no word is visited again when its voxels settle.
// Which slots a launch touches, and why no lane reads what another lane of the launch writes: level L reads, from other words, only
// slots L - step with 1 <= step <= M, and writes, in its own word only, slots L .. L + P.  R = M + P + 1 keeps the two sets apart.  The
// top slot (L + P) mod R held S_{L - M - 1}, which no launch reads again (level L reads L - step >= L - M), and no earlier level can
// have put anything there (L' + q = L + P with q <= P needs L' >= L): so a plain store is right, and since every word of a live source
// stores there on every level, that store is also the clearing of the ring.
// A word with nothing left to arrive (free & ~arrived empty) stores its 0 without reading its neighbourhood or the planes.
// An arrival at level L settles by L + P and is pulled from by L + P + M, so a source whose last M + P levels had no arrival is
// finished and returns at once, and so does one whose targets are all reached (stop[s], matrix only).  Blocks of one launch may
// disagree on stop[s]; that only changes bitmaps nobody reads again.
// Matrix (tgt != NULL): the first block of each source looks its n_tgt targets up in S_{L - 1}, complete since the launch before (only
// levels <= L - 1 write it; the seed for L = 1), and stores L - 1 in the source's row for those in it; the launch after the last
// productive level sees that level's set.
// PEN == false is the search without penalties: P is the constant 0 whatever st.P holds, `planes` is not read and there is no penalty
// loop.  The top slot is then the lane's own slot L mod R, R = M + 1, arrived = done = settled, and A is S_L, stored whole.
template <bool PEN>
__global__ __launch_bounds__(256) void k_chm_ring_level(const unsigned long long *__restrict__ freeb, const unsigned long long *__restrict__ planes,
                                                        WaGeoDims g, int32_t level, int32_t slot, WaChmStep st,
                                                        unsigned long long *__restrict__ arrived, unsigned long long *__restrict__ ring,
                                                        int32_t *__restrict__ field, int32_t *__restrict__ last, int32_t *__restrict__ stop,
                                                        const long long *__restrict__ tgt, int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    const int32_t P = PEN ? st.P : 0;
    if (last[s] < level - (st.M + P) || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t R = st.M + P + 1;
    unsigned long long *rs = ring + (int64_t)s * R * g.nw;
    if (tgt && blockIdx.x == 0)
        geo_lookup_targets(rs + (int64_t)(slot == 0 ? R - 1 : slot - 1) * g.nw, g, tgt, n_tgt, mat + (int64_t)s * n_tgt, level - 1, stop + s);
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= g.nw) return;
    const int64_t sw = (int64_t)s * g.nw + w;
    const unsigned long long arr = arrived[sw];
    const unsigned long long open = freeb[w] & ~arr;
    const int32_t tp = slot + P;
    unsigned long long *top = rs + (int64_t)(PEN && tp >= R ? tp - R : tp) * g.nw + w;   // (L + P) mod R
    if (!open) {
        *top = 0ull;
        return;
    }
    unsigned long long A = chm_gather(freeb, rs, g, st, R, level, slot, w) & open;
    if (!PEN || !A) *top = A;   // (without penalties A is S_L; with them an empty A still clears the top slot)
    if (!A) return;
    arrived[sw] = arr | A;
    last[s] = level;
    if (!PEN) {
        if (field) geo_store_level(chm_field_word(field, s, g, w), A, level);
        return;
    }
    unsigned long long p[WA_PEN_PLANES];
#pragma unroll
    for (int j = 0; j < WA_PEN_PLANES; j++) p[j] = planes[(int64_t)j * g.nw + w];
    int32_t *f = field ? chm_field_word(field, s, g, w) : nullptr;
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
        if (q == P) of_top = m;
        else {
            const int32_t sl = slot + q;
            rs[(int64_t)(sl >= R ? sl - R : sl) * g.nw + w] |= m;
        }
    } while (A);
    *top = of_top;
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

// Walk back, one lane per pair, from the end to the start of the pair's field (slot[p] within the chunk) by chm_predecessor.  With
// penalties (PEN; `pen` is not read otherwise) the predecessor of a node v with distance D > 0 is chm_predecessor's for D - pen[v],
// that is the first offset o in its order for which the move exists and the voxel holds D - pen[v] - step[class(o) - 1] >= 0, which is
// then the distance to go on with.
// Counting pass (out == NULL): dist[p] = the field at the end, len[p] = the nodes of the path (0 when unreachable).
// Writing pass: the i-th node from the end goes to out[dst[p] + len[p] - 1 - i], so the path reads start -> end; dst[p] < 0: nothing to
// write (unreachable, or the caller's range is too small).  The field is exact, so a predecessor always exists; the loop still ends if not.
template <bool PEN>
__global__ __launch_bounds__(256) void k_chm_walkback(const int32_t *__restrict__ field, const uint8_t *__restrict__ free_, const uint8_t *__restrict__ pen,
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
        const int32_t moved = PEN ? D - (int32_t)pen[v] : D;
        int32_t paid = 0;
        v = chm_predecessor(f, free_, g, st, v, moved, &paid);
        if (v < 0) break;
        D = moved - paid;
    }
    if (!out) len[p] = cnt;
}
