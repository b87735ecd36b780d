// pose_fit_kernels.hpp -- device side of wa_grid_pose_fit_trajectory (include/weldacs.h, rules 37 - 39 of the torch section):
// the round of fit_kernels.hpp with "a planned direction is open along this piece of curve" in place of "this piece of curve is free".
// Everything else of the round is the fit's own: pieces, scan, emit, knots, ends, evaluation, sample lookup, blame (on the blocked bytes)
// and bump.  The masks are those of k_reach (reach_kernels.hpp), word-plane-major.  Integers throughout: every output is bit-exact and
// independent of scheduling.
//   k_pfit_segments   the segment test of one round, one lane per segment, in the place of k_clr_segments
//   k_pfit_dir_stats  behind the last round: changes of direction between consecutive segments, and the largest turn among them
#pragma once
#include "fit_kernels.hpp"
#include "pose_shortcut_kernels.hpp"

#define WA_PFIT_SLOTS 8   // 2 samples x (D + 1) control points, D <= 3

// Which of the candidates in cand[0 .. WA_PFIT_SLOTS) with a bit in `live` are open in EVERY voxel of the supercover between a and b?
// One walk (clr_cover_visit) for all of them; per voxel one load of the mask word of each distinct plane c >> 6 among the candidates
// still live; the walk ends when no bit is left.  The slots are indexed by constants only (the loops unroll): the list stays in
// registers.  The occupancy is not read: an occupied voxel has no open direction (rule 10).
__device__ __forceinline__ uint32_t pfit_cover_open(long long a, long long b, WaDims d, const unsigned long long *__restrict__ mask,
                                                    const int32_t (&cand)[WA_PFIT_SLOTS], uint32_t live)
{
    clr_cover_visit(a, b, d, [&](int64_t v) {
        uint32_t done = 0;
#pragma unroll
        for (int j = 0; j < WA_PFIT_SLOTS; j++) {
            if (!((live & ~done) >> j & 1u)) continue;
            const int32_t plane = cand[j] >> 6;
            const unsigned long long w = mask[(int64_t)plane * d.n + v];
#pragma unroll
            for (int t = j; t < WA_PFIT_SLOTS; t++) {
                if (!((live & ~done) >> t & 1u) || (cand[t] >> 6) != plane) continue;
                done |= 1u << t;
                if (!((w >> (cand[t] & 63)) & 1ull)) live &= ~(1u << t);
            }
        }
        return live == 0;
    });
    return live;
}

// Segment i = samples i, i + 1 at u = (float)i * dt.  Slot e * (DEG + 1) + q holds the hold of the leg that owns control point
// span_e - DEG + q, span_e the knot span of sample i + e as k_fit_blame finds it (a sample k_fit_blame skips leaves its slots empty);
// a slot is live when its hold is >= 0 and no earlier slot holds the same value: the live slots in ascending order are rule 37's
// candidates.  With a candidate the segment's direction is the first one open on the whole cover, and the segment is blocked when
// there is none; without one the lane runs the occupancy visitor of k_clr_segments and the direction is -1.
// acc[1] takes the first blocked segment (atomicMin), acc[2] their number, *n_none the lanes without a candidate: wave reductions, one
// integer atomic per wavefront and counter.
template <int DEG>
__global__ __launch_bounds__(256) void k_pfit_segments(const long long *__restrict__ ids, int64_t n, WaDims d, const uint8_t *__restrict__ free_,
                                                       const unsigned long long *__restrict__ mask, WaSpline S, float dt,
                                                       const int32_t *__restrict__ owner, const int32_t *__restrict__ leg_hold,
                                                       uint8_t *__restrict__ blocked_out, int32_t *__restrict__ dir_out,
                                                       unsigned long long *__restrict__ acc /* [1] first, [2] n_blocked */,
                                                       unsigned long long *__restrict__ n_none)
{
    static_assert(2 * (DEG + 1) <= WA_PFIT_SLOTS, "two samples' control points fill the slots");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool blocked = false, none = false;
    if (i + 1 < n) {
        const float *K = S.knots;
        const float lastk = K[S.n_knots - 1];
        int32_t cand[WA_PFIT_SLOTS];
#pragma unroll
        for (int j = 0; j < WA_PFIT_SLOTS; j++) cand[j] = -1;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            float u = 0.0f + (float)(i + e) * dt;
            if (u < K[0]) u = K[0];
            else if (u > lastk) u = lastk;
            long long span = 0;
            if (!wa_bs_find_span(K, S.n_knots, u, &span) || span - DEG < 0 || span >= S.n_cps) continue;
#pragma unroll
            for (int q = 0; q <= DEG; q++) cand[e * (DEG + 1) + q] = leg_hold[owner[span - DEG + q]];
        }
        uint32_t live = 0;
#pragma unroll
        for (int j = 0; j < WA_PFIT_SLOTS; j++) {
            bool fresh = cand[j] >= 0;
#pragma unroll
            for (int t = 0; t < j; t++) fresh = fresh && cand[t] != cand[j];
            live |= fresh ? 1u << j : 0u;
        }
        int32_t dir = -1;
        if (live == 0) {
            none = true;
            blocked = clr_cover_hits(ids[i], ids[i + 1], d, free_);
        } else {
            live = pfit_cover_open(ids[i], ids[i + 1], d, mask, cand, live);
            blocked = live == 0;
#pragma unroll
            for (int j = WA_PFIT_SLOTS - 1; j >= 0; j--)
                if ((live >> j) & 1u) dir = cand[j];
        }
        blocked_out[i] = blocked ? 1 : 0;
        dir_out[i] = dir;
    }
    unsigned long long first = blocked ? (unsigned long long)i : ~0ull, cnt = blocked ? 1 : 0, nn = none ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long f2 = __shfl_down(first, o, 64);
        first = f2 < first ? f2 : first;
        cnt += __shfl_down(cnt, o, 64);
        nn += __shfl_down(nn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (cnt) {
            atomicMin(&acc[1], first);
            atomicAdd(&acc[2], cnt);
        }
        if (nn) atomicAdd(n_none, nn);
    }
}

// One lane per pair of consecutive segments (i, i + 1), behind the last round: both directions >= 0 and different is a change; its turn
// is U(q_a, q_b) of rule 2.  out[0] += changes, out[1] = max turn.  A pair reads its neighbour's direction, which the segment kernel's
// own launch cannot see across lanes and blocks, and only the last round's figures leave the call: hence a launch of its own.
__global__ __launch_bounds__(256) void k_pfit_dir_stats(const int32_t *__restrict__ dir, int64_t n_seg, const short4 *__restrict__ q,
                                                        unsigned long long *__restrict__ out /* [0] n_dir_changes, [1] max_dir_turn */)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long chg = 0, turn = 0;
    if (i + 1 < n_seg) {
        const int32_t a = dir[i], b = dir[i + 1];
        if (a >= 0 && b >= 0 && a != b) {
            const short4 u = q[a], w = q[b];
            const int64_t dx = u.x - w.x, dy = u.y - w.y, dz = u.z - w.z;
            chg = 1;
            turn = (unsigned long long)((dx * dx + dy * dy + dz * dz) >> 10);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        chg += __shfl_down(chg, o, 64);
        const unsigned long long t2 = __shfl_down(turn, o, 64);
        turn = t2 > turn ? t2 : turn;
    }
    if ((threadIdx.x & 63) == 0 && chg) {
        atomicAdd(&out[0], chg);
        atomicMax(&out[1], turn);
    }
}
