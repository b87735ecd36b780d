// jerk_axes_kernels.hpp -- device side of the torch axes at jerk-limited ticks (wa_traj_retime_jerk_axes; include/weldacs.h rules 56 - 60
// hold the definition, DESIGN 4ac the reasoning, tests/jerk_axes_ref.py restates it in numpy).  The filtered arc length S stays on
// the device: the stage below runs behind k_jk_ticks inside the one call and reads the prefix sums that kernel read.
//   k_jk_ticks_first  the FIRST == true instantiation of jk_ticks (jerk_kernels.hpp): the lowest rest tick of every stop, beside its count
//   k_jk_axes         one lane per output tick: S by jk_s, the segment or the stop by the search of k_jk_ticks, the axis of rule 57 or
//                     58, rule 2 at the tick's voxel, stores staged through LDS, counters through the slots of WaAxRec
//   k_jx_groups       one lane per segment: the groups of stops whose run of coincident samples begins and ends with different axes
// Integers and single correctly rounded fp64 operations throughout; what is accumulated across lanes is an integer.
#pragma once
#include "jerk_kernels.hpp"
#include "ticks_kernels.hpp"

__global__ __launch_bounds__(256) void k_jk_ticks_first(WaJkTicks T, unsigned long long *__restrict__ first)
{
    jk_ticks<true>(T, first);
}

struct WaJxRec {
    unsigned long long max_rest_turn, n_turning, min_turn_ticks /* ~0: no turning group */;
};

struct WaJkAxes {
    const short4 *q;                    // n
    const unsigned long long *first;    // per stop segment: its lowest rest tick (with next)
    int32_t check;                      // a grid and a tool are given
    float *axes;                        // n_ticks x 3 or nullptr
    uint8_t *blocked;                   // n_ticks or nullptr
    WaJxRec *rec;
};

// rule 26's expression between two axes, quantised by rule 1; a where they cancel
__device__ __forceinline__ short4 jx_axis(short4 a, short4 b, double lam)
{
    const double vx = (double)a.x + ((double)b.x - (double)a.x) * lam, vy = (double)a.y + ((double)b.y - (double)a.y) * lam,
                 vz = (double)a.z + ((double)b.z - (double)a.z) * lam;
    if (vx == 0.0 && vy == 0.0 && vz == 0.0) {
        a.w = 0;
        return a;
    }
    return ax_quantise(vx, vy, vz);
}

struct JxTick {
    RtTick r;        // the position, as k_jk_ticks forms it
    long long below; // the last sample with GL < S (-1: none): the bracket of the ticks behind
    short4 qt;
    bool rest;
};

// Rules 54, 57 and 58 for tick k at arc length S.  base = the last sample with GL < S_base brackets the search from below where
// S >= S_base; a tick in front of it searches the samples in front.
__device__ __forceinline__ JxTick jx_tick(const WaJkTicks &T, const WaJkAxes &A, long long k, long long S, long long base, long long S_base)
{
    const long long *__restrict__ GL = T.GL;
    JxTick t;
    long long a;
    if (S >= S_base) {
        long long step = 1;
        a = base;
        while (a + step <= T.n - 2 && GL[a + step] < S) {
            a += step;
            step <<= 1;
        }
        a = jk_last_below(GL, a + 1, a + step - 1 < T.n - 2 ? a + step - 1 : T.n - 2, S);
    } else {
        a = jk_last_below(GL, 0, base, S);
    }
    t.below = a;
    const long long lo = a + 1;   // the first sample with GL >= S, at most n - 1
    const long long f = T.next ? T.next[lo] : T.n;
    t.rest = f < T.n - 1 && GL[f] == S;
    t.r.lam = 0.0;
    t.r.exact = 0;
    if (t.rest) {   // rule 58: the run lo .. e of samples at S turns as one
        long long b = f, step = 1;
        while (b + step <= T.n - 1 && GL[b + step] <= S) {
            b += step;
            step <<= 1;
        }
        const long long e = jk_last_at_most(GL, b + 1, b + step - 1 < T.n - 1 ? b + step - 1 : T.n - 1, S);
        const double lam = __ddiv_rn((double)(k - (long long)A.first[f]), (double)T.rest_cnt[f]);
        t.r.i = f;
        t.r.exact = 2;
        t.qt = jx_axis(A.q[lo], A.q[e], lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam));
        return t;
    }
    long long i;
    if (GL[lo] > S) {
        i = lo - 1;   // (GL_0 = 0 <= S: lo >= 1)
    } else if (lo >= T.n - 2) {
        i = T.n - 2;
    } else {   // the last sample of the run with GL = S, up to n - 2
        long long b = lo, step = 1;
        while (b + step <= T.n - 2 && GL[b + step] <= S) {
            b += step;
            step <<= 1;
        }
        i = jk_last_at_most(GL, b + 1, b + step - 1 < T.n - 2 ? b + step - 1 : T.n - 2, S);
    }
    const long long g0 = GL[i], g1 = GL[i + 1];
    t.r.i = i;
    if (S >= g1) t.r.exact = 1;
    else if (g1 == g0) t.r.exact = 2;
    else t.r.lam = __ddiv_rn((double)(S - g0), (double)(g1 - g0));
    t.qt = jx_axis(A.q[i], A.q[i + 1], t.r.exact == 1 ? 1.0 : t.r.lam);
    return t;
}

// One lane per output tick, 256 per workgroup.  Every lane of a wave locates the tick in front of the wave's first one (the same
// search in every lane: one address per step); that tick's last sample below S brackets every lane's own search, and its axis is what
// lane 0 needs for the turn -- nothing is read that another workgroup writes.  The tool sits in LDS, the block's 256 axes go through
// LDS so that consecutive lanes store consecutive floats, its counters are added up in LDS and leave as one atomic each.
// FR (wa_traj_retime_jerk_frames, rules 61 - 67): the same body, which also forms the lateral, the weave's offset and the woven
// position of the tick it has just located; what that adds is compiled in only where FR::on (frames_kernels.hpp holds that
// instantiation and FR's members), so k_jk_axes keeps its registers, its LDS and its occupancy.
struct JxNoFrames {
    static constexpr bool on = false;
    struct State {};
};

template <class FR>
__device__ __forceinline__ void jx_axes(const WaJkTicks &T, const WaJkAxes &A, const WaField &F, const WaTorchTool *__restrict__ tool,
                                        WaAxRec *__restrict__ rec, const FR &fr)
{
    __shared__ float stage[256 * 3];
    __shared__ int32_t tl[192];
    __shared__ unsigned int cnt[3], blk_turn, blk_rest_turn;   // the workgroup's ticks outside / blocked / near, its largest turns
    __shared__ unsigned long long blk_first;                   // its first blocked tick
    if (A.check) ax_stage_tool(tool, tl);
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        blk_turn = blk_rest_turn = 0;
        blk_first = ~0ull;
    }
    typename FR::State fs;
    if constexpr (FR::on) fr.begin(fs);
    __syncthreads();
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long k_first = k - lane;   // (wave-uniform)
    const bool live = k < T.n_ticks;
    bool outside = false, blocked = false, near = false, rest = false;
    unsigned long long turn = 0;
    long long mine = 0;
    if (k_first < T.n_ticks) {
        const long long k_front = k_first > 0 ? k_first - 1 : 0, S_front = jk_s(T, k_front);
        const JxTick front = jx_tick(T, A, k_front, S_front, jk_last_below(T.GL, 0, T.n - 2, S_front), S_front);
        if (live) {
            const long long S = jk_s(T, k);
            const JxTick t = jx_tick(T, A, k, S, front.below, S_front);
            rest = t.rest;
            mine = tk_pack(t.qt);
            for (int c = 0; c < 3; c++) stage[3 * threadIdx.x + c] = (float)((double)(c == 0 ? t.qt.x : (c == 1 ? t.qt.y : t.qt.z)) / 16384.0);
            float px = rt_tick_pos(T.xyz, t.r, 0), py = rt_tick_pos(T.xyz, t.r, 1), pz = rt_tick_pos(T.xyz, t.r, 2);
            if constexpr (FR::on) fr.tick(fs, T, t, S, &px, &py, &pz);   // rule 66: the check below runs at the woven position
            if (A.check) {
                int64_t id;
                const int3 v = field_voxel(F, px, py, pz, &id, &outside);
                const int32_t res = ax_beads(F, v, t.qt, tl, tool->n_beads);
                blocked = res & 1;
                near = !blocked && (res >> 8) > 0;
            }
            if (A.blocked) A.blocked[k] = blocked ? 1 : 0;
        }
        long long before = __shfl_up(mine, 1, 64);
        if (lane == 0) before = tk_pack(front.qt);
        if (live && k > 0) turn = ax_chord2(tk_unpack(before), tk_unpack(mine)) >> 10;
        if constexpr (FR::on) fr.steps(fs, T, front, S_front, live, k, blocked);
    }
    const unsigned long long mo = __ballot(outside), mb = __ballot(blocked), mn = __ballot(near);
    unsigned long long rturn = rest ? turn : 0;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t2 = __shfl_down(turn, o, 64), r2 = __shfl_down(rturn, o, 64);
        turn = t2 > turn ? t2 : turn;
        rturn = r2 > rturn ? r2 : rturn;
    }
    if (lane == 0) {   // (LDS atomics)
        if (mo) atomicAdd(&cnt[0], (unsigned int)__popcll(mo));
        if (mb) {
            atomicAdd(&cnt[1], (unsigned int)__popcll(mb));
            atomicMin(&blk_first, (unsigned long long)(k + __builtin_ctzll(mb)));
        }
        if (mn) atomicAdd(&cnt[2], (unsigned int)__popcll(mn));
        if (turn) atomicMax(&blk_turn, (unsigned int)turn);
        if (rturn) atomicMax(&blk_rest_turn, (unsigned int)rturn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        WaAxSlot *s = &rec->slot[blockIdx.x & (WA_AX_SLOTS - 1)];
        if (cnt[0]) atomicAdd(&s->n_outside, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&s->n_blocked, (unsigned long long)cnt[1]);
        if (cnt[2]) atomicAdd(&s->n_near, (unsigned long long)cnt[2]);
        // first_blocked only falls and the turns only rise: a value that cannot win against what is there already is not sent
        if (blk_first < __hip_atomic_load(&rec->first_blocked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&rec->first_blocked, blk_first);
        if (blk_turn > __hip_atomic_load(&rec->max_tick_turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&rec->max_tick_turn, (unsigned long long)blk_turn);
        if (blk_rest_turn > __hip_atomic_load(&A.rec->max_rest_turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&A.rec->max_rest_turn, (unsigned long long)blk_rest_turn);
    }
    if (A.axes) {
        const long long first = (long long)blockIdx.x * blockDim.x * 3, end = T.n_ticks * 3;
        for (int e = threadIdx.x; e < 256 * 3; e += 256)
            if (first + e < end) A.axes[first + e] = stage[e];
    }
    if constexpr (FR::on) fr.end(T);
}

__global__ __launch_bounds__(256) void k_jk_axes(WaJkTicks T, WaJkAxes A, WaField F, const WaTorchTool *__restrict__ tool,
                                                 WaAxRec *__restrict__ rec)
{
    jx_axes(T, A, F, tool, rec, JxNoFrames());
}

// Rule 60: a group of stops is every stop with one GL; its head (k_jk_groups) holds the group's rest ticks.  The run of samples at that
// GL begins at a and ends at e; the group turns where their axes differ.
__global__ __launch_bounds__(256) void k_jx_groups(const long long *__restrict__ GL, long long n, const long long *__restrict__ dq,
                                                   const long long *__restrict__ next, const short4 *__restrict__ q,
                                                   const unsigned long long *__restrict__ rest_cnt, WaJxRec *__restrict__ rec)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool turning = false;
    unsigned long long r = ~0ull;
    if (j < n - 1 && dq[j] >= 0) {
        const long long a = jk_last_below(GL, 0, j, GL[j]) + 1;
        if (next[a] == j) {
            const long long e = jk_last_at_most(GL, j + 1, n - 1, GL[j]);   // (L_j = 0: at least j + 1)
            turning = ax_chord2(q[a], q[e]) != 0;
            if (turning) r = rest_cnt[j];
        }
    }
    const unsigned long long mt = __ballot(turning);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long r2 = __shfl_down(r, o, 64);
        r = r2 < r ? r2 : r;
    }
    if ((threadIdx.x & 63) == 0 && mt) {
        atomicAdd(&rec->n_turning, (unsigned long long)__popcll(mt));
        atomicMin(&rec->min_turn_ticks, r);
    }
}
