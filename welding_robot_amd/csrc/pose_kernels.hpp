// pose_kernels.hpp -- device side of wa_grid_pose_fields / _matrix / _paths (include/weldacs.h, rules 17 - 23 of the torch section; DESIGN
// 4t): an exact breadth-first search over the states (voxel, direction) with open(v, k), level-synchronous and bit-parallel over the
// directions.  Integers throughout: every output is bit-exact and independent of scheduling.
// A state bitmap holds one 64-bit word per voxel and plane of 64 directions, word-plane-major like the masks of k_reach: bit (k & 63)
// of word [(k >> 6) * n + v] is state (v, k); W = ceil(K / 64) planes, W * n words.  There is no padding: a voxel outside the grid has
// no word.  Every kernel of one search runs on one stream: a level reads what the launch before it wrote, nothing inside a launch reads
// what the same launch writes.
//   k_pose_adj        the K x W adjacency bit matrix from q and max_turn
//   k_pose_level      one level for every source of a chunk (pull form)
//   k_pose_pair_hops  hop count and end direction per pair
//   k_pose_walkback   the path of a pair, one wavefront each
// Level 0 is k_posew_seed's (pose_weighted_kernels.hpp) with a ring of one set: the first frontier.
#pragma once
#include "reach_kernels.hpp"

#define WA_POSE_MAX_W 4   // WA_TORCH_MAX_DIRS / 64

// A source, point, start or end travels through the search driver as one key: the voxel id in the low 48 bits, pin + 1 above them
// (0: no pin).  Two starts with different pins are different keys, which is what groups the pairs of a _paths call.  The walk-back
// returns its nodes in the same form, the direction index above the id.
#define WA_POSE_KEY_SHIFT 48
__host__ __device__ __forceinline__ long long pose_key(long long id, int32_t pin) { return id | ((long long)(pin + 1) << WA_POSE_KEY_SHIFT); }
__host__ __device__ __forceinline__ long long pose_key_id(long long key) { return key & ((1ll << WA_POSE_KEY_SHIFT) - 1); }
__host__ __device__ __forceinline__ int32_t pose_key_pin(long long key) { return (int32_t)(key >> WA_POSE_KEY_SHIFT) - 1; }

// adj[k * W + w]: bit b is adj(k, 64 w + b) = max_turn < 0 or U(q_k, q_(64 w + b)) <= max_turn; bits of directions >= K are 0
__global__ __launch_bounds__(256) void k_pose_adj(const short4 *__restrict__ q, int32_t K, int32_t max_turn, unsigned long long *__restrict__ adj)
{
    const int32_t W = (K + 63) >> 6;
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= K * W) return;
    const int32_t k = i / W, w = i - k * W;
    const short4 a = q[k];
    unsigned long long bits = 0;
    for (int32_t b = 0; b < 64 && w * 64 + b < K; b++) {
        const short4 c = q[w * 64 + b];
        const int64_t dx = a.x - c.x, dy = a.y - c.y, dz = a.z - c.z;
        const int64_t U = (dx * dx + dy * dy + dz * dz) >> 10;   // (up to 3 * 2^30 before the shift)
        if (max_turn < 0 || U <= max_turn) bits |= 1ull << b;
    }
    adj[i] = bits;
}

// The matrix's targets, by all 256 threads of the first block of a source: `value` goes to row_out[t] for every target t that has no
// entry yet and has a state in the frontier cur (which the launch before completed) -- any state, or the pinned one; once no entry of
// the row is missing, stop[s] = 1.  (A voxel is in the frontiers of several levels, one per direction that arrives: the first counts.)
__device__ __forceinline__ void pose_lookup_targets(const unsigned long long *__restrict__ cur, int64_t n, int32_t W, const long long *__restrict__ tgt,
                                                    int32_t n_tgt, int32_t *__restrict__ row_out, int32_t value, int32_t *__restrict__ stop_s)
{
    int missing = 0;
    for (int32_t t = (int32_t)threadIdx.x; t < n_tgt; t += 256) {
        if (row_out[t] >= 0) continue;
        const long long v = pose_key_id(tgt[t]);
        const int32_t pin = pose_key_pin(tgt[t]);
        unsigned long long in = 0;
        if (pin >= 0) in = (cur[(int64_t)(pin >> 6) * n + v] >> (pin & 63)) & 1ull;
        else
            for (int32_t w = 0; w < W; w++) in |= cur[(int64_t)w * n + v];
        if (in) row_out[t] = value;
        else missing = 1;
    }
    if (!__syncthreads_or(missing) && threadIdx.x == 0) *stop_s = 1;
}

// One level for every source of a chunk: blockIdx.y = source; a wavefront takes 64 consecutive x of one (y, z) row and a workgroup four
// neighbouring rows, as in k_reach (nchunk = ceil(nx / 64) chunks per row).  Per lane and plane w:
//   cand[w] = open[w] & ~seen[w]                                    the states this voxel can still gain
//   m[w]    = the OR of the previous frontier at the six neighbours   (the +-x neighbours are loads of the lines the lanes beside read)
// State (v, k) joins the level iff cand has bit k and some k' of m has adj(k', k): row k of the adjacency matrix has a wavefront-uniform
// address, so the compiler keeps it in scalar registers, and the loop over k is uniform.  A wavefront without a lane that has both an m
// and a cand writes its zero frontier words and is done; one without any cand does not even gather.  all_adj (max_turn < 0): every
// m reaches every cand, no loop unless states are kept.
// nxt receives this level's frontier whole (it holds the frontier of two levels ago).  A voxel with new states ORs them into seen (this
// lane is the only one that touches the voxel's words), stores `level` in hops the first time it gains any state, in state[k * n + v] for
// every new state (kept states only; coalesced along x for one k), and stores last[s] = level: every writer of a launch stores the same
// value.  Termination, stop[s] and the matrix's targets work as in k_geo_level.  Tail lanes (x >= nx) and the missing rows of the last
// workgroup read and write nothing.
__global__ __launch_bounds__(256) void k_pose_level(const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ adj, WaDims d,
                                                    int32_t K, int32_t all_adj, int32_t nchunk, int32_t level, int64_t words, int64_t ints,
                                                    unsigned long long *__restrict__ seen, const unsigned long long *__restrict__ cur,
                                                    unsigned long long *__restrict__ nxt, int32_t *__restrict__ field, int32_t keep_states,
                                                    int32_t *__restrict__ last, int32_t *__restrict__ stop, const long long *__restrict__ tgt,
                                                    int32_t n_tgt, int32_t *__restrict__ mat)
{
    const int32_t s = (int32_t)blockIdx.y;
    if (last[s] < level - 1 || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    cur += (int64_t)s * words;
    nxt += (int64_t)s * words;
    seen += (int64_t)s * words;
    if (tgt && blockIdx.x == 0) pose_lookup_targets(cur, n, W, tgt, n_tgt, mat + (int64_t)s * n_tgt, level - 1, stop + s);
    const int lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)d.ny * d.nz;
    const int64_t row = (int64_t)(blockIdx.x / (unsigned)nchunk) * 4 + (threadIdx.x >> 6);
    const int32_t x = (int32_t)(blockIdx.x % (unsigned)nchunk) * 64 + lane;
    if (row >= rows) return;   // (whole wavefronts)
    const bool valid = x < d.nx;
    const int32_t y = (int32_t)(row % d.ny), z = (int32_t)(row / d.ny);   // uniform over the wavefront
    const int64_t v = row * d.nx + x;
    int32_t *hops = field ? field + (int64_t)s * ints : nullptr;
    int32_t *state = field && keep_states ? field + (int64_t)s * ints + n : nullptr;

    unsigned long long sn[WA_POSE_MAX_W], cand[WA_POSE_MAX_W], m[WA_POSE_MAX_W], nf[WA_POSE_MAX_W];
    unsigned long long any_c = 0, any_s = 0, any_m = 0;
#pragma unroll
    for (int32_t w = 0; w < WA_POSE_MAX_W; w++) {
        sn[w] = cand[w] = m[w] = nf[w] = 0;
        if (w < W && valid) {
            sn[w] = seen[(int64_t)w * n + v];
            cand[w] = open[(int64_t)w * n + v] & ~sn[w];
        }
        any_c |= cand[w];
        any_s |= sn[w];
    }
    if (__ballot(any_c != 0) != 0) {
#pragma unroll
        for (int32_t w = 0; w < WA_POSE_MAX_W; w++)
            if (w < W && valid) {
                const unsigned long long *c = cur + (int64_t)w * n + v;
                // six loads in flight: a neighbour outside the grid reads the lane's own word instead and is masked out
                const unsigned long long xm = c[x > 0 ? -1 : 0], xp = c[x < d.nx - 1 ? 1 : 0];
                const unsigned long long ym = c[y > 0 ? -(int64_t)d.nx : 0], yp = c[y < d.ny - 1 ? d.nx : 0];
                const unsigned long long zm = c[z > 0 ? -(int64_t)d.nxy : 0], zp = c[z < d.nz - 1 ? d.nxy : 0];
                const unsigned long long g = (x > 0 ? xm : 0ull) | (x < d.nx - 1 ? xp : 0ull) | (y > 0 ? ym : 0ull) | (y < d.ny - 1 ? yp : 0ull) |
                                             (z > 0 ? zm : 0ull) | (z < d.nz - 1 ? zp : 0ull);
                m[w] = g;
                any_m |= g;
            }
    }
    if (__ballot(any_c != 0 && any_m != 0) != 0) {
        if (all_adj && !state) {
#pragma unroll
            for (int32_t w = 0; w < WA_POSE_MAX_W; w++) nf[w] = any_m ? cand[w] : 0ull;
        } else {
#pragma unroll
            for (int32_t w = 0; w < WA_POSE_MAX_W; w++)
                if (w < W) {
                    const int32_t kend = min(64, K - w * 64);
                    unsigned long long acc = 0;
                    for (int32_t kk = 0; kk < kend; kk++) {
                        const int32_t k = w * 64 + kk;
                        const unsigned long long *r = adj + (int64_t)k * W;
                        unsigned long long hit = 0;
#pragma unroll
                        for (int32_t u = 0; u < WA_POSE_MAX_W; u++)
                            if (u < W) hit |= m[u] & r[u];
                        if (hit && ((cand[w] >> kk) & 1ull)) {
                            acc |= 1ull << kk;
                            if (state) state[(int64_t)k * n + v] = level;
                        }
                    }
                    nf[w] = acc;
                }
        }
    }
    if (!valid) return;
    unsigned long long any_n = 0;
#pragma unroll
    for (int32_t w = 0; w < WA_POSE_MAX_W; w++)
        if (w < W) {
            nxt[(int64_t)w * n + v] = nf[w];
            if (nf[w]) seen[(int64_t)w * n + v] = sn[w] | nf[w];
            any_n |= nf[w];
        }
    if (any_n) {
        if (hops && !any_s) hops[v] = level;
        last[s] = level;
    }
}

// per pair: D = hops(start; end, end pin) in the field of the pair's start (slot[p] within the chunk) and the end state's direction, the
// lowest k the end pin allows with level D (-1 with D = WA_HOPS_NONE)
__global__ __launch_bounds__(256) void k_pose_pair_hops(const int32_t *__restrict__ field, int64_t ints, int64_t n, int32_t K,
                                                        const int32_t *__restrict__ slot, const long long *__restrict__ end, int32_t n_pairs,
                                                        int32_t *__restrict__ hops, int32_t *__restrict__ kend)
{
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_pairs) return;
    const int32_t *f = field + (int64_t)slot[p] * ints;
    const long long v = pose_key_id(end[p]);
    const int32_t pin = pose_key_pin(end[p]);
    int32_t D, k = -1;
    if (pin >= 0) {
        D = f[n + (int64_t)pin * n + v];
        if (D >= 0) k = pin;
    } else {
        D = f[v];
        if (D >= 0)
            for (k = 0; k < K - 1 && f[n + (int64_t)k * n + v] != D; k++) {}
    }
    hops[p] = D;
    kend[p] = k;
}

// Walk back, one wavefront per pair, lanes over the directions k' = lane + 64 w: from the end state (level D) to the start (0).  At
// (v, k) with level L > 0 the predecessor voxel is the first neighbour in the order -x, +x, -y, +y, -z, +z that is inside the grid and
// has some k' with level L - 1 and adj(k', k), the predecessor direction the lowest such k': the first plane with a non-empty ballot,
// its lowest lane.  The node with level L goes to out[dst[p] + L] as a key (direction above the id), so the path reads start -> end.
// dst[p] < 0: nothing to write.  The field is exact, so a predecessor always exists; the loop still ends after D steps if not.
__global__ __launch_bounds__(64) void k_pose_walkback(const int32_t *__restrict__ field, int64_t ints, WaDims d, int32_t K,
                                                      const unsigned long long *__restrict__ adj, const int32_t *__restrict__ slot,
                                                      const long long *__restrict__ end, const long long *__restrict__ dst,
                                                      const int32_t *__restrict__ hops, const int32_t *__restrict__ kend, int32_t n_pairs,
                                                      long long *__restrict__ out)
{
    const int32_t p = (int32_t)blockIdx.x;
    if (p >= n_pairs || dst[p] < 0) return;
    const int lane = threadIdx.x;
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    const int32_t *state = field + (int64_t)slot[p] * ints + n;
    long long v = pose_key_id(end[p]);
    int32_t k = kend[p];
    long long *o = out + dst[p];
    for (int32_t L = hops[p]; L >= 0; L--) {
        if (lane == 0) o[L] = v | ((long long)k << WA_POSE_KEY_SHIFT);
        if (L == 0) break;
        const int32_t x = (int32_t)(v % d.nx), y = (int32_t)((v / d.nx) % d.ny), z = (int32_t)(v / d.nxy);
        const bool in[6] = {x > 0, x < d.nx - 1, y > 0, y < d.ny - 1, z > 0, z < d.nz - 1};
        const long long nb[6] = {v - 1, v + 1, v - d.nx, v + d.nx, v - d.nxy, v + d.nxy};
        bool found = false;
#pragma unroll
        for (int32_t i = 0; i < 6; i++) {
            if (found || !in[i]) continue;
            for (int32_t w = 0; w < W && !found; w++) {
                const int32_t k2 = w * 64 + lane;
                const bool ok = k2 < K && state[(int64_t)k2 * n + nb[i]] == L - 1 && ((adj[(int64_t)k * W + w] >> lane) & 1ull);
                const unsigned long long b = __ballot(ok);
                if (b) {
                    k = w * 64 + __builtin_ctzll(b);
                    v = nb[i];
                    found = true;
                }
            }
        }
        if (!found) break;
    }
}
