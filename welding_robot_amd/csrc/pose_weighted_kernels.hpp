// pose_weighted_kernels.hpp -- device side of wa_grid_pose_weighted_fields / _matrix / _paths (include/weldacs.h, rules 30 - 36 of the
// torch section): exact cheapest paths over the states (voxel, direction) of pose_kernels.hpp where the step
// (v, k) -> (v', k') costs hop_cost + turn_cost[class(k, k')] + pen[v'].  Level-synchronous like k_pose_level, with the level now the
// distance: a source keeps `seen` (every settled state) and a ring of R = hop_cost + max turn_cost + P + 1 settled sets in pose_kernels.hpp's
// bitmap layout (W * n words each, slot L mod R = the states whose distance is exactly L), contiguous per source.  Every step costs at
// least 1, so a pull at level L reads only sets that earlier launches completed, and levels ascend, so the first level at which a pull
// reaches a state is its distance.  Integers throughout, no atomics: every output is bit-exact and independent of scheduling.
//   k_posew_adj        one K x W bit matrix per distinct step weight hop_cost + turn_cost[c]
//   k_posew_pen_info   which penalties are present on free voxels (the argument check and P)
//   k_posew_seed       level 0 of every source of a chunk
//   k_posew_level      one level for every source of a chunk (pull form)
//   k_posew_walkback   the path of a pair, one wavefront each, counting pass and writing pass
// k_pose_pair_hops (pose_kernels.hpp) gives a pair's distance and end direction: rule 21's end state is rule 33's.
#pragma once
#include "pose_kernels.hpp"

#define WA_POSEW_MAX_BANDS 4
#define WA_POSEW_MAX_WEIGHTS 5   // WA_POSEW_MAX_BANDS + 1 turn classes, merged where their costs are equal
#define WA_POSEW_PEN_MAX 15

// a cost description as the kernels see it: the bands, the turn classes dealt over the n_w distinct step weights (ascending), the ring
struct WaPosewCosts {
    int32_t n_bands, band[WA_POSEW_MAX_BANDS];
    int32_t group[WA_POSEW_MAX_WEIGHTS];    // turn class -> its matrix
    int32_t n_w, weight[WA_POSEW_MAX_WEIGHTS];
    int32_t R;
};

// adjw[(j * K + k) * W + w]: bit b holds iff adj(k, 64 w + b) and the turn class of the two directions has step weight j
__global__ __launch_bounds__(256) void k_posew_adj(const short4 *__restrict__ q, int32_t K, int32_t max_turn, WaPosewCosts c,
                                                   unsigned long long *__restrict__ adjw)
{
    const int32_t W = (K + 63) >> 6;
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= c.n_w * K * W) return;
    const int32_t j = i / (K * W), kw = i - j * K * W;
    const int32_t k = kw / W, w = kw - k * W;
    const short4 a = q[k];
    unsigned long long bits = 0;
    for (int32_t b = 0; b < 64 && w * 64 + b < K; b++) {
        const short4 e = q[w * 64 + b];
        const int64_t dx = a.x - e.x, dy = a.y - e.y, dz = a.z - e.z;
        const int64_t U = (dx * dx + dy * dy + dz * dz) >> 10;
        if (max_turn >= 0 && U > max_turn) continue;
        int32_t cls = 0;
#pragma unroll
        for (int32_t t = 0; t < WA_POSEW_MAX_BANDS; t++) cls += (t < c.n_bands && U > c.band[t]) ? 1 : 0;
        int32_t gr = 0;
#pragma unroll
        for (int32_t t = 0; t < WA_POSEW_MAX_WEIGHTS; t++) gr = cls == t ? c.group[t] : gr;
        if (gr == j) bits |= 1ull << b;
    }
    adjw[i] = bits;
}

// info[min(pen, WA_POSEW_PEN_MAX + 1)] = 1 for every free voxel (info is zeroed before; every writer of a word stores the same value)
__global__ __launch_bounds__(256) void k_posew_pen_info(const uint8_t *__restrict__ free_, const uint8_t *__restrict__ pen, int64_t n,
                                                        int32_t *__restrict__ info)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n || !free_[v]) return;
    info[min((int32_t)pen[v], WA_POSEW_PEN_MAX + 1)] = 1;
}

// level 0 of every source of a chunk: k_pose_seed for a ring -- the seed goes into `seen` and into slot 0 of the source's ring (both
// zeroed before, the whole ring), 0 into its cost field and its state field, last[s] = 0, stop[s] = 0
__global__ __launch_bounds__(256) void k_posew_seed(const long long *__restrict__ src, int32_t n_src, const unsigned long long *__restrict__ open,
                                                    int64_t n, int32_t K, int32_t R, int64_t words, int64_t ints, unsigned long long *__restrict__ seen,
                                                    unsigned long long *__restrict__ ring, int32_t *__restrict__ field, int32_t keep_states,
                                                    int32_t *__restrict__ last, int32_t *__restrict__ stop)
{
    const int32_t s = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (s >= n_src) return;
    const long long v = pose_key_id(src[s]);
    const int32_t pin = pose_key_pin(src[s]);
    const int32_t W = (K + 63) >> 6;
    bool any = false;
    for (int32_t w = 0; w < W; w++) {
        unsigned long long b = open[(int64_t)w * n + v];
        if (pin >= 0) b = (pin >> 6) == w ? b & (1ull << (pin & 63)) : 0ull;
        if (!b) continue;
        any = true;
        seen[(int64_t)s * words + (int64_t)w * n + v] = b;
        ring[(int64_t)s * R * words + (int64_t)w * n + v] = b;
        if (field && keep_states)
            for (unsigned long long r = b; r; r &= r - 1) field[(int64_t)s * ints + n + (int64_t)(w * 64 + __builtin_ctzll(r)) * n + v] = 0;
    }
    if (any && field) field[(int64_t)s * ints + v] = 0;
    last[s] = 0;
    stop[s] = 0;
}

// One level for every source of a chunk, in k_pose_level's layout: blockIdx.y = source, a wavefront takes 64 consecutive x of one row, a
// workgroup four rows.  Per lane and plane w, cand[w] = open[w] & ~seen[w].  For each distinct step weight j in turn the lane gathers
//   m_j[w] = the OR over the six neighbours of ring set (level - weight[j] - pen[v]) mod R      (nothing below level 0)
// pen[v] is the lane's own byte, paid on entry, so the slot varies over the lanes while the six neighbour offsets do not.  State (v, k)
// is settled at this level iff cand has bit k and for some j, m_j & row_j[k] is not empty: the rows have wavefront-uniform addresses and
// stay in scalar registers, the loop over k is uniform, and a weight whose m is empty for the whole wavefront has no loop.  Only one
// weight's m is alive at a time (the registers of k_pose_level, not five times its m).  A lane without a candidate gathers nothing; a
// wavefront without one writes its zero words and is done.  all_one (max_turn < 0 and one weight): every m reaches every cand, no loop.
// Kept states are stored after the weights, one uniform loop over k, each new state once.
// The level's set is written whole into slot level mod R: it held level - R, which no later level reads (the largest step is R - 1).
// seen, the cost field, the state field, last[s], stop[s] and the matrix's targets follow k_pose_level: a target is found in the set
// that the launch before completed, level - 1 is its cost.  A source is alive while one of the last R - 1 levels settled a state.
template <int WMAX>   // planes the registers hold: 1, 2 or 4 >= W (K <= 64 keeps k_pose_level's occupancy)
__global__ __launch_bounds__(256) void k_posew_level(const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ adjw,
                                                     const uint8_t *__restrict__ pen, WaDims d, int32_t K, WaPosewCosts c, int32_t all_one,
                                                     int32_t nchunk, int32_t level, int32_t slot, int64_t words, int64_t ints,
                                                     unsigned long long *__restrict__ seen, unsigned long long *__restrict__ ring,
                                                     int32_t *__restrict__ field, int32_t keep_states, int32_t *__restrict__ last,
                                                     int32_t *__restrict__ stop, const long long *__restrict__ tgt, int32_t n_tgt,
                                                     int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    const int32_t R = c.R;
    if (last[s] < level - (R - 1) || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
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
        // one weight at a time: its gather, then its rows; only one weight's m is alive, and a weight whose sets are empty around
        // this wavefront costs the gather only
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

// Walk back, one wavefront per pair, lanes over the directions k' = lane + 64 w, from the end state (dist[p], kend[p]: k_pose_pair_hops)
// to the seed.  At (v, k) with distance L > 0 the predecessor voxel is the first neighbour in the order -x, +x, -y, +y, -z, +z that is
// inside the grid and has some k' with adj(k', k) and dist(k') + weight(class(k', k)) + pen[v] == L, the predecessor direction the lowest
// such k': the first plane with a non-empty ballot, its lowest lane.  (A direction is in the row of at most one weight.)
// Counting pass (out == NULL): len[p] = the nodes of the path, 0 when dist[p] < 0.  Writing pass: the i-th node from the end goes to
// out[dst[p] + len[p] - 1 - i] as a key (direction above the id), so the path reads start -> end; dst[p] < 0: nothing to write.  The
// field is exact, so a predecessor always exists; the loop still ends if not (L falls with every step).
__global__ __launch_bounds__(64) void k_posew_walkback(const int32_t *__restrict__ field, int64_t ints, WaDims d, int32_t K,
                                                       const unsigned long long *__restrict__ adjw, WaPosewCosts c, const uint8_t *__restrict__ pen,
                                                       const int32_t *__restrict__ slot, const long long *__restrict__ end,
                                                       const long long *__restrict__ dst, const int32_t *__restrict__ dist,
                                                       const int32_t *__restrict__ kend, int32_t n_pairs, int32_t *__restrict__ len,
                                                       long long *__restrict__ out)
{
    const int32_t p = (int32_t)blockIdx.x;
    if (p >= n_pairs || (out && dst[p] < 0)) return;
    const int lane = threadIdx.x;
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    const int32_t *state = field + (int64_t)slot[p] * ints + n;
    long long v = pose_key_id(end[p]);
    int32_t k = kend[p], L = dist[p], cnt = 0;
    const int32_t total = out ? len[p] : 0;
    long long *o = out ? out + dst[p] : nullptr;
    while (L >= 0) {
        if (out) {
            if (cnt >= total) break;
            if (lane == 0) o[total - 1 - cnt] = v | ((long long)k << WA_POSE_KEY_SHIFT);
        }
        cnt++;
        if (L == 0) break;
        const int32_t x = (int32_t)(v % d.nx), y = (int32_t)((v / d.nx) % d.ny), z = (int32_t)(v / d.nxy);
        const bool in[6] = {x > 0, x < d.nx - 1, y > 0, y < d.ny - 1, z > 0, z < d.nz - 1};
        const long long nb[6] = {v - 1, v + 1, v - d.nx, v + d.nx, v - d.nxy, v + d.nxy};
        const int32_t paid = L - (pen ? (int32_t)pen[v] : 0);
        bool found = false;
#pragma unroll
        for (int32_t i = 0; i < 6; i++) {
            if (found || !in[i]) continue;
            for (int32_t w = 0; w < W && !found; w++) {
                const int32_t k2 = w * 64 + lane;
                int32_t wt = -1;
#pragma unroll
                for (int32_t j = 0; j < WA_POSEW_MAX_WEIGHTS; j++)
                    if (j < c.n_w && ((adjw[((int64_t)j * K + k) * W + w] >> lane) & 1ull)) wt = c.weight[j];
                const int32_t need = paid - wt;
                const bool ok = k2 < K && wt >= 0 && need >= 0 && state[(int64_t)k2 * n + nb[i]] == need;
                const unsigned long long b = __ballot(ok);
                if (b) {
                    const int first = __builtin_ctzll(b);
                    k = w * 64 + first;
                    v = nb[i];
                    L = __shfl(need, first);
                    found = true;
                }
            }
        }
        if (!found) break;
    }
    if (!out && lane == 0) len[p] = cnt;
}
