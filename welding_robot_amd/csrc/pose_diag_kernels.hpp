// pose_diag_kernels.hpp -- device side of wa_grid_pose_diag_fields / _matrix / _paths (include/weldacs.h, rules 43 - 47 of the torch
// section): pose_weighted_kernels.hpp's search over the states (voxel, direction) with the 20 diagonal moves of
// chamfer_kernels.hpp added.  A face move is rule 18's step and costs step[0] + turn_cost[class(k, k')] + pen[v']; an edge or corner
// move keeps the direction, exists iff k is open in all 2^c voxels of the box the two voxels span, and costs step[c - 1] + pen[v'].
// The layout, the ring of R settled sets per source, `seen`, the fields, last / stop and the targets are k_posew_level's; R =
// max(step[0] + max turn_cost, step[1], step[2]) + P + 1.  Integers throughout, no atomics: every output is bit-exact and independent
// of scheduling, and every word a lane writes is its own.
//   k_posed_level      one level for every source of a chunk (pull form): k_posew_level plus the diagonal part
//   k_posed_walkback   the path of a pair, one wavefront each, counting pass and writing pass
// k_posew_adj (with the face weights), k_posew_pen_info, k_posew_seed and k_pose_pair_hops are used as they are.
#pragma once
#include "pose_weighted_kernels.hpp"

// the face part is a WaPosewCosts with weight[j] = step[0] + a turn cost and R the ring of this search; s2, s3 = step[1], step[2]
struct WaPosedCosts {
    WaPosewCosts f;
    int32_t s2, s3;
};

// The diagonal pulls of one plane of one lane: the OR over the 12 edge and the 8 corner offsets o of
//   cand & S_c[v + o] & AND(open over the box of v and v + o)
// S_c = the settled set of level - step[c - 1] - pen[v] (s2, s3 point at the lane's word of it in this plane), op = the lane's word of
// `open` in this plane.  v's own open bit is in cand and v + o's in S_c, so an edge move asks two face neighbours and a corner move
// three face and three edge neighbours.
// Addresses: ox[i] is the lane's stride to its -x / +x neighbour, oy[j] and oz[l] the wavefront's strides in y and z, each 0 where that
// neighbour lies outside the grid, and the caller's pointers belong to a voxel inside the grid for every lane: every load is in bounds
// without a branch and all loads of a group are in flight together.  Masks: c2x[i] / c3x[i] = cand where the lane pulls from that class
// and its x neighbour i is inside the grid, c2 = cand where it pulls from class 2, else 0; oy[j] != 0 and oz[l] != 0 are uniform.  A
// frontier word is therefore 0 unless its whole box is inside the grid, and the open words need no mask of their own.  (nx * ny < 2^31.)
// The open words are loaded only when the frontier words of a class are not all zero over the wavefront (called in uniform control
// flow: the ballots see every lane).
struct WaPosedLane {
    unsigned long long c2x[2], c3x[2], c2;
    int32_t ox[2], oy[2], oz[2];
};
__device__ __forceinline__ unsigned long long posed_diag_plane(const unsigned long long *__restrict__ op, const unsigned long long *__restrict__ s2,
                                                               const unsigned long long *__restrict__ s3, const WaPosedLane &a)
{
    unsigned long long fxy[2][2], fxz[2][2], fyz[2][2], f3[2][2][2], any2 = 0, any3 = 0;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            fxy[i][j] = a.oy[j] ? s2[a.ox[i] + a.oy[j]] & a.c2x[i] : 0ull;
            fxz[i][j] = a.oz[j] ? s2[a.ox[i] + a.oz[j]] & a.c2x[i] : 0ull;
            fyz[i][j] = a.oy[i] && a.oz[j] ? s2[a.oy[i] + a.oz[j]] & a.c2 : 0ull;
            any2 |= fxy[i][j] | fxz[i][j] | fyz[i][j];
        }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int l = 0; l < 2; l++) {
                f3[i][j][l] = a.oy[j] && a.oz[l] ? s3[a.ox[i] + a.oy[j] + a.oz[l]] & a.c3x[i] : 0ull;
                any3 |= f3[i][j][l];
            }
    const bool b2 = __ballot(any2 != 0) != 0, b3 = __ballot(any3 != 0) != 0;
    if (!b2 && !b3) return 0ull;
    unsigned long long fx[2], fy[2], fz[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        fx[i] = op[a.ox[i]];
        fy[i] = op[a.oy[i]];
        fz[i] = op[a.oz[i]];
    }
    unsigned long long r = 0;
    if (b2) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) r |= (fxy[i][j] & fx[i] & fy[j]) | (fxz[i][j] & fx[i] & fz[j]) | (fyz[i][j] & fy[i] & fz[j]);
    }
    if (b3) {
        unsigned long long exy[2][2], exz[2][2], eyz[2][2];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                exy[i][j] = op[a.ox[i] + a.oy[j]];
                exz[i][j] = op[a.ox[i] + a.oz[j]];
                eyz[i][j] = op[a.oy[i] + a.oz[j]];
            }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int l = 0; l < 2; l++) r |= f3[i][j][l] & fx[i] & fy[j] & fz[l] & exy[i][j] & exz[i][l] & eyz[j][l];
    }
    return r;
}

// One level for every source of a chunk: k_posew_level (its layout, its WMAX templates, cand = open & ~seen, the early return of a
// wavefront without a candidate, the face part -- one six-neighbour gather per distinct turn weight from slot level - weight - pen[v],
// then the uniform loop over k on scalar-loaded adjacency rows --, seen, the cost field, the state field, last, stop and the targets),
// plus, ahead of the face part, posed_diag_plane for every plane: the lane pulls from class c while step[c - 1] + pen[v] <= level.
// The slots read are (level - back) mod R with 1 <= back <= R - 1, complete since earlier launches; the launch writes slot level mod R.
template <int WMAX>   // planes the registers hold: 1, 2 or 4 >= W
__global__ __launch_bounds__(256) void k_posed_level(const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ adjw,
                                                     const uint8_t *__restrict__ pen, WaDims d, int32_t K, WaPosedCosts cd, int32_t all_one,
                                                     int32_t level, int32_t slot, unsigned long long *__restrict__ seen,
                                                     unsigned long long *__restrict__ ring, int32_t *__restrict__ field, int32_t keep_states,
                                                     int32_t *__restrict__ last, int32_t *__restrict__ stop, const long long *__restrict__ tgt,
                                                     int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    const WaPosewCosts &c = cd.f;
    const int32_t R = c.R;
    if (last[s] < level - (R - 1) || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    const int64_t words = (int64_t)W * n, ints = n + (keep_states ? (int64_t)K * n : 0);   // one set, one source's field (posew_kind's)
    const int32_t nchunk = (d.nx + 63) >> 6;
    ring += (int64_t)s * R * words;
    seen += (int64_t)s * words;
    if (tgt && blockIdx.x == 0)
        pose_lookup_targets(ring + (int64_t)(slot ? slot - 1 : R - 1) * words, n, W, tgt, n_tgt, mat + (int64_t)s * n_tgt, level - 1, stop + s);
    const int lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)d.ny * d.nz;
    const int64_t row = (int64_t)(blockIdx.x / (unsigned)nchunk) * 4 + (threadIdx.x >> 6);
    const int32_t x = (int32_t)(blockIdx.x % (unsigned)nchunk) * 64 + lane;
    if (row >= rows) return;   // (whole wavefronts)
    const bool valid = x < d.nx;
    const int32_t y = (int32_t)(row % d.ny), z = (int32_t)(row / d.ny);   // uniform over the wavefront
    const int64_t v = row * d.nx + x;
    int32_t *cost = field ? field + (int64_t)s * ints : nullptr;
    int32_t *state = field && keep_states ? field + (int64_t)s * ints + n : nullptr;

    unsigned long long sn[WMAX], cand[WMAX], nf[WMAX], m[WMAX];
    unsigned long long any_c = 0, any_s = 0, any_n = 0;
#pragma unroll
    for (int32_t w = 0; w < WMAX; w++) {
        sn[w] = cand[w] = nf[w] = 0;
        if (w < W && valid) {
            sn[w] = seen[(int64_t)w * n + v];
            cand[w] = open[(int64_t)w * n + v] & ~sn[w];
        }
        any_c |= cand[w];
        any_s |= sn[w];
    }
    if (__ballot(any_c != 0) != 0) {
        const int32_t pv = pen && any_c ? (int32_t)pen[v] : 0;   // (any_c: the lane is valid)
        // the diagonal part: the direction is kept, so a plane pulls from the same plane of its 20 diagonal neighbours
        {
            const int32_t back2 = cd.s2 + pv, back3 = cd.s3 + pv;   // 1 .. R - 1 (P covers every free voxel)
            const bool pull2 = any_c && back2 <= level, pull3 = any_c && back3 <= level;
            const int32_t sl2 = slot - back2 < 0 ? slot - back2 + R : slot - back2, sl3 = slot - back3 < 0 ? slot - back3 + R : slot - back3;   // 0 .. R - 1
            const int32_t xa = min(x, d.nx - 1);   // a lane behind the row's end reads the row's last voxel and masks it out
            const int64_t va = row * d.nx + xa;
            WaPosedLane a;
            a.ox[0] = xa > 0 ? -1 : 0; a.ox[1] = xa < d.nx - 1 ? 1 : 0;
            a.oy[0] = y > 0 ? -d.nx : 0; a.oy[1] = y < d.ny - 1 ? d.nx : 0;
            a.oz[0] = z > 0 ? -(int32_t)d.nxy : 0; a.oz[1] = z < d.nz - 1 ? (int32_t)d.nxy : 0;
            const unsigned long long *b2 = ring + (int64_t)sl2 * words + va, *b3 = ring + (int64_t)sl3 * words + va;
#pragma unroll
            for (int32_t w = 0; w < WMAX; w++)
                if (w < W) {
                    a.c2 = pull2 ? cand[w] : 0ull;
                    const unsigned long long c3 = pull3 ? cand[w] : 0ull;
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        a.c2x[i] = a.ox[i] ? a.c2 : 0ull;
                        a.c3x[i] = a.ox[i] ? c3 : 0ull;
                    }
                    nf[w] |= posed_diag_plane(open + (int64_t)w * n + va, b2 + (int64_t)w * n, b3 + (int64_t)w * n, a);
                }
        }
        // the face part: one weight at a time, its gather, then its rows
        for (int32_t j = 0; j < c.n_w; j++) {
            const int32_t back = c.weight[j] + pv;   // 1 .. R - 1
            unsigned long long any_m = 0;
#pragma unroll
            for (int32_t w = 0; w < WMAX; w++) m[w] = 0;
            if (any_c && back <= level && back < R) {   // (back < R always: P covers every free voxel)
                const int32_t sl = slot - back < 0 ? slot - back + R : slot - back;
                const unsigned long long *set = ring + (int64_t)sl * words + v;
#pragma unroll
                for (int32_t w = 0; w < WMAX; w++)
                    if (w < W) {
                        const unsigned long long *e = set + (int64_t)w * n;
                        // six loads in flight: a neighbour outside the grid reads the lane's own word instead and is masked out
                        const unsigned long long xm = e[x > 0 ? -1 : 0], xp = e[x < d.nx - 1 ? 1 : 0];
                        const unsigned long long ym = e[y > 0 ? -(int64_t)d.nx : 0], yp = e[y < d.ny - 1 ? d.nx : 0];
                        const unsigned long long zm = e[z > 0 ? -(int64_t)d.nxy : 0], zp = e[z < d.nz - 1 ? d.nxy : 0];
                        const unsigned long long g = (x > 0 ? xm : 0ull) | (x < d.nx - 1 ? xp : 0ull) | (y > 0 ? ym : 0ull) |
                                                     (y < d.ny - 1 ? yp : 0ull) | (z > 0 ? zm : 0ull) | (z < d.nz - 1 ? zp : 0ull);
                        m[w] = g;
                        any_m |= g;
                    }
            }
            if (__ballot(any_m != 0) == 0) continue;
            if (all_one) {
#pragma unroll
                for (int32_t w = 0; w < WMAX; w++) nf[w] |= any_m ? cand[w] : 0ull;
                continue;
            }
            const unsigned long long *rows = adjw + (int64_t)j * K * W;
#pragma unroll
            for (int32_t w = 0; w < WMAX; w++)
                if (w < W) {
                    const int32_t kend = min(64, K - w * 64);
                    unsigned long long acc = 0;
                    for (int32_t kk = 0; kk < kend; kk++) {
                        const unsigned long long *r = rows + (int64_t)(w * 64 + kk) * W;
                        unsigned long long hit = 0;
#pragma unroll
                        for (int32_t u = 0; u < WMAX; u++)
                            if (u < W) hit |= m[u] & r[u];
                        acc |= hit ? 1ull << kk : 0ull;
                    }
                    nf[w] |= acc & cand[w];
                }
        }
#pragma unroll
        for (int32_t w = 0; w < WMAX; w++) any_n |= nf[w];
        if (state && __ballot(any_n != 0) != 0) {
#pragma unroll
            for (int32_t w = 0; w < WMAX; w++)
                if (w < W) {
                    const int32_t kend = min(64, K - w * 64);
                    for (int32_t kk = 0; kk < kend; kk++)   // (uniform; the stores of one k are coalesced along x)
                        if ((nf[w] >> kk) & 1ull) state[(int64_t)(w * 64 + kk) * n + v] = level;
                }
        }
    }
    if (!valid) return;
    unsigned long long *out = ring + (int64_t)slot * words + v;
#pragma unroll
    for (int32_t w = 0; w < WMAX; w++)
        if (w < W) {
            out[(int64_t)w * n] = nf[w];
            if (nf[w]) seen[(int64_t)w * n + v] = sn[w] | nf[w];
        }
    if (any_n) {
        if (cost && !any_s) cost[v] = level;
        last[s] = level;
    }
}

// Walk back, one wavefront per pair, as k_posew_walkback: at (v, k) with distance L > 0 first the six faces in the order -x, +x, -y,
// +y, -z, +z, the lowest k' with adj(k', k) and dist(k') + weight(class(k', k)) + pen[v] == L (lanes over k'); then the 12 edge offsets,
// then the 8 corner offsets, each group sorted by (dz, dy, dx), the direction kept: the first offset whose voxel holds
// L - step[c - 1] - pen[v] for k and whose box has k open throughout (lanes over the offsets; a lane asks the state field first, the
// masks only when it matches).  Passes, outputs and keys are k_posew_walkback's.
__global__ __launch_bounds__(64) void k_posed_walkback(const int32_t *__restrict__ field, int64_t ints, WaDims d, int32_t K,
                                                       const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ adjw,
                                                       WaPosedCosts cd, const uint8_t *__restrict__ pen, const int32_t *__restrict__ slot,
                                                       const long long *__restrict__ end, const long long *__restrict__ dst,
                                                       const int32_t *__restrict__ dist, const int32_t *__restrict__ kend, int32_t n_pairs,
                                                       int32_t *__restrict__ len, long long *__restrict__ out)
{
    const int32_t p = (int32_t)blockIdx.x;
    if (p >= n_pairs || (out && dst[p] < 0)) return;
    const int lane = threadIdx.x;
    const WaPosewCosts &c = cd.f;
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    const int32_t *state = field + (int64_t)slot[p] * ints + n;
    int32_t v = (int32_t)pose_key_id(end[p]);   // (n <= 2^29: ids and strides fit 32 bits, which keeps the divisions and the scalars small)
    int32_t k = kend[p], L = dist[p], cnt = 0;
    const int32_t total = out ? len[p] : 0;
    long long *o = out ? out + dst[p] : nullptr;
    // lane r < 20 takes the r-th diagonal offset of the walk-back's order: the 12 edges, then the 8 corners, each sorted by (dz, dy, dx);
    // oy, oz = its strides in y and z, stepc = its step (the other lanes: one no distance can pay)
    int32_t dx = 0, dy = 0, dz = 0, stepc = 1 << 30;
    {
        int32_t r2 = 0, r3 = 12;
#pragma unroll
        for (int32_t t = 0; t < 27; t++) {
            const int32_t ax = t % 3 - 1, ay = (t / 3) % 3 - 1, az = t / 9 - 1, cl = (ax != 0) + (ay != 0) + (az != 0);
            if (cl < 2) continue;
            const int32_t r = cl == 2 ? r2++ : r3++;
            if (lane == r) {
                dx = ax; dy = ay; dz = az;
                stepc = cl == 2 ? cd.s2 : cd.s3;
            }
        }
    }
    const int32_t oy = dy * d.nx, oz = dz * d.nxy;
    while (L >= 0) {
        if (out) {
            if (cnt >= total) break;
            if (lane == 0) o[total - 1 - cnt] = (long long)v | ((long long)k << WA_POSE_KEY_SHIFT);
        }
        cnt++;
        if (L == 0) break;
        const int32_t x = v % d.nx, y = (v / d.nx) % d.ny, z = v / d.nxy;
        const int32_t paid = L - (pen ? (int32_t)pen[v] : 0);
        bool found = false;
#pragma unroll 1
        for (int32_t i = 0; i < 6 && !found; i++) {   // -x, +x, -y, +y, -z, +z
            const int32_t ax = i >> 1;
            const int32_t co = ax == 0 ? x : ax == 1 ? y : z, dim = ax == 0 ? d.nx : ax == 1 ? d.ny : d.nz;
            if ((i & 1) ? co >= dim - 1 : co <= 0) continue;
            const int32_t stp = ax == 0 ? 1 : ax == 1 ? d.nx : d.nxy;
            const int32_t nbv = (i & 1) ? v + stp : v - stp;
            for (int32_t w = 0; w < W && !found; w++) {
                const int32_t k2 = w * 64 + lane;
                int32_t wt = -1;
#pragma unroll
                for (int32_t j = 0; j < WA_POSEW_MAX_WEIGHTS; j++)
                    if (j < c.n_w && ((adjw[((int64_t)j * K + k) * W + w] >> lane) & 1ull)) wt = c.weight[j];
                const int32_t need = paid - wt;
                const bool ok = k2 < K && wt >= 0 && need >= 0 && state[(int64_t)k2 * n + nbv] == need;
                const unsigned long long b = __ballot(ok);
                if (b) {
                    const int first = __builtin_ctzll(b);
                    k = w * 64 + first;
                    v = nbv;
                    L = __shfl(need, first);
                    found = true;
                }
            }
        }
        if (found) continue;
        // the diagonals: lane r < 20 holds the r-th offset of the order; the lowest lane that holds is the predecessor
        {
            const int32_t need = paid - stepc;
            const int32_t q = v + dx + oy + oz;
            bool ok = need >= 0 && (uint32_t)(x + dx) < (uint32_t)d.nx && (uint32_t)(y + dy) < (uint32_t)d.ny && (uint32_t)(z + dz) < (uint32_t)d.nz;
            ok = ok && state[(int64_t)k * n + q] == need;
            if (ok) {
                // v and q have k open (both hold a distance for it); the other voxels of the box (a coordinate that does not change
                // repeats a voxel, which changes nothing)
                const unsigned long long *ow = open + (int64_t)(k >> 6) * n + v;
#pragma unroll
                for (int32_t b = 1; b < 7; b++) ok = ok && ((ow[((b & 1) ? dx : 0) + ((b & 2) ? oy : 0) + ((b & 4) ? oz : 0)] >> (k & 63)) & 1ull) != 0;
            }
            const unsigned long long b = __ballot(ok);
            if (b) {
                const int first = __builtin_ctzll(b);
                v = __shfl(q, first);
                L = __shfl(need, first);
                found = true;
            }
        }
        if (!found) break;
    }
    if (!out && lane == 0) len[p] = cnt;
}
