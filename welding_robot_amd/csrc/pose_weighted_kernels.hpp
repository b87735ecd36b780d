// pose_weighted_kernels.hpp -- the ring search over the states (voxel, direction) of pose_kernels.hpp: device side of
// wa_grid_pose_weighted_fields / _matrix / _paths (include/weldacs.h, rules 30 - 36 of the torch section) and of
// wa_grid_pose_diag_fields / _matrix / _paths (rules 43 - 47), and the seed of wa_grid_pose_fields / _matrix / _paths.
// A face move is rule 18's step (v, k) -> (v', k') and costs hop + turn_cost[class(k, k')] + pen[v'] (hop = hop_cost, or step[0] on the
// 26-neighbour lattice).  On that lattice (DIAG) there are also the 20 diagonal moves of chamfer_kernels.hpp: an edge or corner move
// keeps the direction, exists iff k is open in all 2^c voxels of the box the two voxels span, and costs step[c - 1] + pen[v'].
// Level-synchronous like k_pose_level, with the level now the distance: a source keeps `seen` (every settled state) and a ring of
// R = (the largest step) + P + 1 settled sets in pose_kernels.hpp's bitmap layout (W * n words each, slot L mod R = the states whose
// distance is exactly L), contiguous per source.  Every step costs at least 1, so a pull at level L reads only sets that earlier
// launches completed, and levels ascend, so the first level at which a pull reaches a state is its distance.  Integers throughout, no
// atomics: every output is bit-exact and independent of scheduling, and every word a lane writes is its own.
//   k_posew_adj        one K x W bit matrix per distinct face weight hop + turn_cost[c]
//   k_posew_pen_info   which penalties are present on free voxels (the argument check and P)
//   k_posew_seed       level 0 of every source of a chunk (R = 1: the breadth-first search of pose_kernels.hpp)
//   k_pose_ring_level  one level for every source of a chunk (pull form), <WMAX, DIAG>; k_posew_level<WMAX>[DIAG] names its instantiations
//   k_posew_walkback   the path of a pair, one wavefront each, counting pass and writing pass, <DIAG>
// k_pose_pair_hops (pose_kernels.hpp) gives a pair's distance and end direction: rule 21's end state is rule 33's.
#pragma once
#include "pose_kernels.hpp"

#define WA_POSEW_MAX_BANDS 4
#define WA_POSEW_MAX_WEIGHTS 5   // WA_POSEW_MAX_BANDS + 1 turn classes, merged where their costs are equal
#define WA_POSEW_PEN_MAX 15

// a cost description as the kernels see it: the bands, the turn classes dealt over the n_w distinct face weights (ascending), the ring,
// and the edge and corner steps step[1], step[2] of the 26-neighbour lattice (0 on the face lattice, where no kernel reads them)
struct WaPosewCosts {
    int32_t n_bands, band[WA_POSEW_MAX_BANDS];
    int32_t group[WA_POSEW_MAX_WEIGHTS];    // turn class -> its matrix
    int32_t n_w, weight[WA_POSEW_MAX_WEIGHTS];
    int32_t R;
    int32_t s2, s3;
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

// level 0 of every source of a chunk: the open directions of its voxel (all of them, or the pinned one) go into `seen` and into slot 0
// of the source's ring (both zeroed before, the whole ring), 0 into its cost field and its state field, last[s] = 0, stop[s] = 0.  An
// empty seed writes nothing: the first level finds no settled set and the search ends there.  With R = 1 the ring is the first of the
// two frontiers of k_pose_level (source s's begins at fronts + s * words): the breadth-first search seeds with this kernel too.
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

// One level for every source of a chunk, in k_pose_level's layout: blockIdx.y = source, a wavefront takes 64 consecutive x of one row, a
// workgroup four rows (nchunk_h = ceil(nx / 64) chunks per row; one set has words_h = W * n words, one source's field ints_h = n, or
// n + K * n where states are kept).  Per lane and plane w, cand[w] = open[w] & ~seen[w].
// The diagonal part (DIAG only) comes first: posed_diag_plane for every plane; the lane pulls from class c while
// step[c - 1] + pen[v] <= level.
// The face part: for each distinct face weight j in turn the lane gathers
//   m_j[w] = the OR over the six neighbours of ring set (level - weight[j] - pen[v]) mod R      (nothing below level 0)
// pen[v] is the lane's own byte, paid on entry, so the slot varies over the lanes while the six neighbour offsets do not.  State (v, k)
// is settled at this level iff cand has bit k and for some j, m_j & row_j[k] is not empty: the rows have wavefront-uniform addresses and
// stay in scalar registers, the loop over k is uniform, and a weight whose m is empty for the whole wavefront has no loop.  Only one
// weight's m is alive at a time (the registers of k_pose_level, not five times its m).  A lane without a candidate gathers nothing; a
// wavefront without one writes its zero words and is done.  all_one (max_turn < 0 and one weight): every m reaches every cand, no loop.
// Kept states are stored after the weights, one uniform loop over k, each new state once.
// The slots read are (level - back) mod R with 1 <= back <= R - 1, complete since earlier launches.  The level's set is written whole
// into slot level mod R: it held level - R, which no later level reads (the largest step is R - 1).
// seen, the cost field, the state field, last[s], stop[s] and the matrix's targets follow k_pose_level: a target is found in the set
// that the launch before completed, level - 1 is its cost.  A source is alive while one of the last R - 1 levels settled a state.
template <int WMAX, bool DIAG>   // planes the registers hold: 1, 2 or 4 >= W (K <= 64 keeps k_pose_level's occupancy); the 26-neighbour lattice
__global__ __launch_bounds__(256) void k_pose_ring_level(const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ adjw,
                                                     const uint8_t *__restrict__ pen, WaDims d, int32_t K, WaPosewCosts c, int32_t all_one,
                                                     int32_t level, int32_t slot, unsigned long long *__restrict__ seen,
                                                     unsigned long long *__restrict__ ring, int32_t *__restrict__ field, int32_t keep_states,
                                                     int32_t *__restrict__ last, int32_t *__restrict__ stop, const long long *__restrict__ tgt,
                                                     int32_t n_tgt, int32_t *__restrict__ mat, int32_t nchunk_h, int64_t words_h, int64_t ints_h)
{
    const int32_t s = (int32_t)blockIdx.y;
    const int32_t R = c.R;
    if (last[s] < level - (R - 1) || stop[s]) return;   // (blocks of this launch may already have stored `level`: never !=)
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    // nchunk, words and ints are posew_kind's.  The face instantiations take the host's, the last three arguments; the 26-neighbour
    // ones work them out and leave those arguments unread.  Each keeps the code it was measured with: the 18 scalar instructions of
    // working them out, in every wavefront's prelude, cost the face lattice 1 % of a matrix call at 256^3 (profiles/pose_family/README.md).
    const int64_t words = DIAG ? (int64_t)W * n : words_h, ints = DIAG ? n + (keep_states ? (int64_t)K * n : 0) : ints_h;
    const int32_t nchunk = DIAG ? (d.nx + 63) >> 6 : nchunk_h;
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
        if constexpr (DIAG) {
            const int32_t back2 = c.s2 + pv, back3 = c.s3 + pv;   // 1 .. R - 1 (P covers every free voxel)
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

// The level kernels whose registers hold WMAX planes: [0] the face lattice, [1] the 26-neighbour lattice.  The host picks WMAX from K
// once for both and indexes with the lattice.
typedef decltype(&k_pose_ring_level<1, false>) WaPosewLevelFn;
template <int WMAX>
constexpr WaPosewLevelFn k_posew_level[2] = {k_pose_ring_level<WMAX, false>, k_pose_ring_level<WMAX, true>};

// Walk back, one wavefront per pair, from the end state (dist[p], kend[p]: k_pose_pair_hops) to the seed.  At (v, k) with distance L > 0
// first the six faces in the order -x, +x, -y, +y, -z, +z (lanes over the directions k' = lane + 64 w): the predecessor voxel is the
// first neighbour inside the grid that has some k' with adj(k', k) and dist(k') + weight(class(k', k)) + pen[v] == L, the predecessor
// direction the lowest such k': the first plane with a non-empty ballot, its lowest lane.  (A direction is in the row of at most one
// weight.)  Then (DIAG only) the 12 edge offsets, then the 8 corner offsets, each group sorted by (dz, dy, dx), the direction kept:
// the first offset whose voxel holds L - step[c - 1] - pen[v] for k and whose box has k open throughout (lanes over the offsets; a lane
// asks the state field first, the masks only when it matches).
// Counting pass (out == NULL): len[p] = the nodes of the path, 0 when dist[p] < 0.  Writing pass: the i-th node from the end goes to
// out[dst[p] + len[p] - 1 - i] as a key (direction above the id), so the path reads start -> end; dst[p] < 0: nothing to write.  The
// field is exact, so a predecessor always exists; the loop still ends if not (L falls with every step).
template <bool DIAG>   // the 26-neighbour lattice (`open` is read only there)
__global__ __launch_bounds__(64) void k_posew_walkback(const int32_t *__restrict__ field, int64_t ints, WaDims d, int32_t K,
                                                       const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ adjw,
                                                       WaPosewCosts c, const uint8_t *__restrict__ pen, const int32_t *__restrict__ slot,
                                                       const long long *__restrict__ end, const long long *__restrict__ dst,
                                                       const int32_t *__restrict__ dist, const int32_t *__restrict__ kend, int32_t n_pairs,
                                                       int32_t *__restrict__ len, long long *__restrict__ out)
{
    const int32_t p = (int32_t)blockIdx.x;
    if (p >= n_pairs || (out && dst[p] < 0)) return;
    const int lane = threadIdx.x;
    const int32_t W = (K + 63) >> 6;
    const int64_t n = d.n;
    const int32_t *state = field + (int64_t)slot[p] * ints + n;
    int32_t v = (int32_t)pose_key_id(end[p]);   // (n <= 2^29: ids and strides fit 32 bits, which keeps the divisions and the scalars small)
    int32_t k = kend[p], L = dist[p], cnt = 0;
    const int32_t total = out ? len[p] : 0;
    long long *o = out ? out + dst[p] : nullptr;
    // DIAG: lane r < 20 takes the r-th diagonal offset of the walk-back's order: the 12 edges, then the 8 corners, each sorted by
    // (dz, dy, dx); oy, oz = its strides in y and z, stepc = its step (the other lanes: one no distance can pay)
    int32_t dx = 0, dy = 0, dz = 0, stepc = 1 << 30;
    if constexpr (DIAG) {
        int32_t r2 = 0, r3 = 12;
#pragma unroll
        for (int32_t t = 0; t < 27; t++) {
            const int32_t ax = t % 3 - 1, ay = (t / 3) % 3 - 1, az = t / 9 - 1, cl = (ax != 0) + (ay != 0) + (az != 0);
            if (cl < 2) continue;
            const int32_t r = cl == 2 ? r2++ : r3++;
            if (lane == r) {
                dx = ax; dy = ay; dz = az;
                stepc = cl == 2 ? c.s2 : c.s3;
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
        if constexpr (DIAG) {
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