// pose_shortcut_kernels.hpp -- device side of wa_grid_pose_shortcut (include/weldacs.h, rules 27 - 29 of the torch section):
// the greedy shortcut of shortcut_kernels.hpp over (voxel, direction) paths.  A candidate is good when the two directions are adjacent
// and one of them is open in every voxel of the supercover; the masks are those of k_reach (reach_kernels.hpp), word-plane-major.
// Integers throughout except the float64 length, which is sc_chain_path's: every output is bit-exact and independent of scheduling.
//   k_psc_reach   step and hold per anchor, one wavefront each
//   k_psc_chain   waypoints, holds, lengths and the summary's counters, one lane per path
#pragma once
#include "shortcut_kernels.hpp"
#include "pose_kernels.hpp"

// Under which of the two directions ka (bit 0 of the result) and km (bit 1) is EVERY voxel of the supercover between a and b open?  One
// walk (clr_cover_visit) for both: per voxel the word of plane ka >> 6, and a second word only when km lies in another plane; the walk
// ends when both flags are down.  The occupancy is not read: an occupied voxel has no open direction (rule 10).
__device__ __forceinline__ uint32_t psc_cover_open(long long a, long long b, WaDims d, const unsigned long long *__restrict__ mask, int32_t ka,
                                                   int32_t km)
{
    const unsigned long long *pa = mask + (int64_t)(ka >> 6) * d.n, *pm = mask + (int64_t)(km >> 6) * d.n;
    const bool one_plane = (ka >> 6) == (km >> 6);
    const unsigned long long ba = 1ull << (ka & 63), bm = 1ull << (km & 63);
    bool fa = true, fm = true;
    clr_cover_visit(a, b, d, [&](int64_t v) {
        const unsigned long long wa = pa[v];
        const unsigned long long wm = one_plane ? wa : pm[v];
        fa = fa && (wa & ba) != 0;
        fm = fm && (wm & bm) != 0;
        return !fa && !fm;
    });
    return (fa ? 1u : 0u) | (fm ? 2u : 0u);
}

// rule 17's adj from the two quantised triples
__device__ __forceinline__ bool psc_adj(short4 a, short4 c, int32_t max_turn)
{
    const int64_t dx = a.x - c.x, dy = a.y - c.y, dz = a.z - c.z;
    return max_turn < 0 || ((dx * dx + dy * dy + dz * dz) >> 10) <= max_turn;
}

// Reach pass, as k_sc_reach: one wavefront per node i of the batch (the anchor), lane l tests candidate m = i + 1 + l of a chunk of 64,
// the first candidate without ok(i, m) is the lowest set bit of the chunk's ballot, and the next chunk is tested only behind a chunk
// that was good throughout.  A lane's flags are psc_cover_open's when the directions are adjacent, 0 otherwise: ok(i, m) = flags != 0.
// Writes step[i] = next(i) - i (>= 1) and hold[i], the direction held from i to next(i): k_i if bit 0 of that candidate's flags is set,
// else k_next if bit 1 is, else -1 (the fallback hop, whose candidate failed).  The flags of the chosen candidate come from its lane:
// the lane before the first failure, or the last lane of the chunk before.  The last node of a path is not written.
__global__ __launch_bounds__(256) void k_psc_reach(const long long *__restrict__ ids, const int32_t *__restrict__ ks,
                                                   const long long *__restrict__ off, int32_t n_paths, int64_t n_nodes, int32_t max_span,
                                                   WaDims d, const unsigned long long *__restrict__ mask, const short4 *__restrict__ q,
                                                   int32_t max_turn, int32_t *__restrict__ step, int32_t *__restrict__ hold)
{
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_nodes) return;   // (whole waves)
    const int64_t last = sc_last_node(off, n_paths, i);
    if (i >= last) return;
    const int64_t top = min(i + (int64_t)max_span, last);
    const long long va = ids[i];
    const int32_t ka = ks[i];
    const short4 qa = q[ka];
    int64_t j = top;            // the farthest candidate such that every candidate up to it is good
    uint32_t fj = 0, fprev = 0; // the flags of candidate j; of the last candidate of the chunk before
    for (int64_t c0 = i + 1; c0 <= top; c0 += 64) {
        const int64_t m = c0 + lane;
        uint32_t f = 0;
        if (m <= top) {
            const int32_t km = ks[m];
            if (psc_adj(qa, q[km], max_turn)) f = psc_cover_open(va, ids[m], d, mask, ka, km);
        }
        const unsigned long long bad = __ballot(m <= top && f == 0);
        if (bad) {
            const int t = __builtin_ctzll(bad);
            j = c0 + t - 1;
            fj = t > 0 ? (uint32_t)__shfl((int)f, t - 1, 64) : fprev;
            break;
        }
        fprev = (uint32_t)__shfl((int)f, 63, 64);
        fj = (uint32_t)__shfl((int)f, (int)(min(top, c0 + 63) - c0), 64);
    }
    if (lane == 0) {
        if (j <= i) { j = i + 1; fj = 0; }   // nothing good: the neighbour, unheld
        step[i] = (int32_t)(j - i);
        hold[i] = (fj & 1u) ? ka : ((fj & 2u) ? ks[j] : -1);
    }
}

// the summary's counters, reduced over a wavefront and added with one integer atomic per wavefront and counter
enum { WA_PSC_WAYPOINTS = 0, WA_PSC_HELD_START, WA_PSC_HELD_END, WA_PSC_UNHELD, WA_PSC_MAX_TURN, WA_PSC_ACC };

// Chain pass: k_sc_chain's, one lane per path (sc_chain_path).  Besides the waypoints, the count and the length it copies hold[a] of
// every waypoint's node a to hold_wp (the last waypoint's entry is -1), counts the segments by their hold (held with the anchor's
// direction, with the arrival's, unheld) and takes the largest U between the holds of two consecutive segments that are both held.
__global__ __launch_bounds__(256) void k_psc_chain(const long long *__restrict__ ids, const int32_t *__restrict__ ks,
                                                   const long long *__restrict__ off, int32_t n_paths, const int32_t *__restrict__ step,
                                                   const int32_t *__restrict__ hold, WaDims d, const float *__restrict__ cx,
                                                   const float *__restrict__ cy, const float *__restrict__ cz, const short4 *__restrict__ q,
                                                   long long *__restrict__ wp, int32_t *__restrict__ hold_wp, int32_t *__restrict__ count,
                                                   double *__restrict__ length, unsigned long long *__restrict__ acc /* WA_PSC_ACC */)
{
    const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    unsigned long long n_wp = 0, n_start = 0, n_end = 0, n_unheld = 0, turn = 0;
    if (p < n_paths) {
        const int64_t b = off[p], L = off[p + 1] - b;
        int32_t cnt = 0;
        double total = 0.0;
        if (L > 0) {
            int32_t before = -1;   // the hold of the segment before
            cnt = sc_chain_path(ids, b, L, step, d, cx, cy, cz, wp, &total, [&](int32_t t, int64_t a) {
                const int32_t h = hold[b + a];
                hold_wp[b + t] = h;
                n_unheld += h < 0;
                n_start += h >= 0 && h == ks[b + a];
                n_end += h >= 0 && h != ks[b + a];
                if (h >= 0 && before >= 0) {
                    const short4 u = q[before], w = q[h];
                    const int64_t dx = u.x - w.x, dy = u.y - w.y, dz = u.z - w.z;
                    const unsigned long long U = (unsigned long long)((dx * dx + dy * dy + dz * dz) >> 10);
                    turn = U > turn ? U : turn;
                }
                before = h;
            });
            hold_wp[b + cnt - 1] = -1;
        }
        count[p] = cnt;
        length[p] = total;
        n_wp = (unsigned long long)cnt;
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_wp += __shfl_down(n_wp, o, 64);
        n_start += __shfl_down(n_start, o, 64);
        n_end += __shfl_down(n_end, o, 64);
        n_unheld += __shfl_down(n_unheld, o, 64);
        const unsigned long long t2 = __shfl_down(turn, o, 64);
        turn = t2 > turn ? t2 : turn;
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_wp) atomicAdd(&acc[WA_PSC_WAYPOINTS], n_wp);
        if (n_start) atomicAdd(&acc[WA_PSC_HELD_START], n_start);
        if (n_end) atomicAdd(&acc[WA_PSC_HELD_END], n_end);
        if (n_unheld) atomicAdd(&acc[WA_PSC_UNHELD], n_unheld);
        if (turn) atomicMax(&acc[WA_PSC_MAX_TURN], turn);
    }
}
