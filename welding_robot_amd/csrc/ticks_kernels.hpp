// ticks_kernels.hpp -- device side of the tool poses at controller ticks (wa_traj_axes_smooth, wa_traj_axes_limits, wa_traj_tick_axes;
// include/weldacs.h rules 24 - 26 hold the definition, DESIGN 4u the reasoning, tests/ticks_ref.py restates it in numpy).
//   k_ax_lengths   one lane per sample: L of retime rule 1 for the segment behind it, the sum of L, non-finite coordinates
//   k_scan         (scan_kernels.hpp) over Ax3Samples: inclusive prefix sums of the three axis components (int64 each) under plain
//                  addition
//   k_ax_level0    rule 24, one lane per sample: its leg, level 0; the few samples whose level-0 candidate is blocked are compacted
//   k_ax_climb     rule 24, one lane per compacted sample: levels 1 .. max_level until one is clear
//   k_ax_summary   rule 24's counters over the finished arrays
//   k_ax_limits    rule 25, one lane per sample
//   k_tk_axes      rule 26, one lane per tick: where the tick lies (rt_tick_locate, rule 6), the interpolated axis, rule 2 at the tick's
//                  voxel, stores staged through LDS
//                  (the STOPS == false instantiation of tk_axes; stops_kernels.hpp holds the other)
// Integers and single correctly rounded fp64 operations throughout (the translation unit is built without contraction): every output
// is bit-exact and independent of scheduling; what is accumulated across lanes is an integer.
#pragma once
#include "retime_kernels.hpp"
#include "torch_kernels.hpp"

#define WA_AX_MAX_LEVEL 8

// The tick kernel's counters: 84 M ticks are 1.3 M wavefronts, and one atomic per wavefront and counter on ONE address is what the
// kernel then waits for.  A workgroup adds up in LDS and sends one atomic per counter to one of WA_AX_SLOTS lines, chosen by its index;
// the host adds the lines.  Integers: the sums do not depend on the order or on the line.
#define WA_AX_SLOTS 32
struct WaAxSlot {
    unsigned long long n_outside, n_blocked, n_near, pad[5];   // one 64-byte line
};

struct WaAxRec {
    WaAxSlot slot[WA_AX_SLOTS];
    unsigned long long sumL[2];
    unsigned long long n_outside, n_level[WA_AX_MAX_LEVEL + 1], n_blocked, first_blocked /* ~0: none */, n_zero_sum, max_turn_in, max_turn_out;
    unsigned long long n_turning, n_jump, n_floored, n_limited;
    unsigned long long max_tick_turn;
    unsigned int min_limit_bits;   // the bits of a positive float order like the float
    unsigned int n_climb;          // samples compacted by k_ax_level0
    unsigned int bad;              // bit 0: a coordinate is not finite; bit 2: a v_limit_in entry is not finite or <= 0
    unsigned int pad;
};

// Rule 1 of the tool section on a double triple that is not all zero: rint((c / len) * 16384) per component
__device__ __forceinline__ short4 ax_quantise(double x, double y, double z)
{
    const double len = rt_norm(x, y, z);
    short4 q;
    q.x = (short)(int32_t)rint(__ddiv_rn(x, len) * 16384.0);
    q.y = (short)(int32_t)rint(__ddiv_rn(y, len) * 16384.0);
    q.z = (short)(int32_t)rint(__ddiv_rn(z, len) * 16384.0);
    q.w = 0;
    return q;
}

// the turn measure U without its shift: the exact squared chord in units of 2^-14, at most 3 * 2^30
__device__ __forceinline__ uint32_t ax_chord2(short4 a, short4 b)
{
    const int32_t dx = (int32_t)a.x - b.x, dy = (int32_t)a.y - b.y, dz = (int32_t)a.z - b.z;
    return (uint32_t)(dx * dx) + (uint32_t)(dy * dy) + (uint32_t)(dz * dz);
}

// Rule 2 for one axis at one voxel, the tool in LDS (tl: dist16, r2, rn, 64 words each): bit 0 blocked, bits 8.. the near beads.
// torch_bead's rule without its branch: a bead outside the grid loads entry 0 and is masked, so that the loads of several beads are
// in flight together (the beads are independent; one gather's latency is what a bead costs otherwise).
__device__ __forceinline__ int32_t ax_beads(const WaField &F, int3 v, short4 q, const int32_t *tl, int32_t nb)
{
    int32_t n_near = 0, blocked = 0;
#pragma unroll 8
    for (int32_t j = 0; j < nb; j++) {
        const short4 o = torch_offset(q, tl[j]);
        const int32_t bx = v.x + o.x, by = v.y + o.y, bz = v.z + o.z;
        const bool in = (uint32_t)bx < (uint32_t)F.d.nx && (uint32_t)by < (uint32_t)F.d.ny && (uint32_t)bz < (uint32_t)F.d.nz;
        const int64_t id = in ? (int64_t)bz * F.d.nxy + (int64_t)by * F.d.nx + bx : 0;
        const uint32_t d = (uint32_t)F.d2[id];
        const bool blk = in && d <= (uint32_t)tl[64 + j];
        n_near += in && !blk && d <= (uint32_t)tl[128 + j];
        blocked |= blk;
    }
    return blocked | (n_near << 8);
}
__device__ __forceinline__ void ax_stage_tool(const WaTorchTool *__restrict__ tool, int32_t *tl)
{
    if (threadIdx.x < 64) {
        tl[threadIdx.x] = tool->dist16[threadIdx.x];
        tl[64 + threadIdx.x] = (int32_t)tool->r2[threadIdx.x];
        tl[128 + threadIdx.x] = (int32_t)tool->rn[threadIdx.x];
    }
}

__global__ __launch_bounds__(256) void k_ax_lengths(const float *__restrict__ xyz, long long n, long long *__restrict__ L, WaAxRec *__restrict__ rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long l = 0;
    if (i < n) {
        bool finite = true;
        for (int c = 0; c < 3; c++) finite = finite && isfinite(xyz[3 * i + c]);
        if (!finite) atomicOr(&rec->bad, 1u);
        if (i < n - 1) l = rt_quanta(rt_seg_len(xyz, i));
        L[i] = l;
    }
    const unsigned long long sl = rt_wave_sat_sum((unsigned long long)l);
    if ((threadIdx.x & 63) == 0) rt_acc_split(rec->sumL, sl);
}

// ---- the three-component prefix sum: the operator of its scan (scan_kernels.hpp)
struct Ax3 { long long x, y, z; };
struct Ax3Sum {
    typedef Ax3 T;
    static __device__ __forceinline__ Ax3 id() { return Ax3{0, 0, 0}; }
    static __device__ __forceinline__ Ax3 comb(Ax3 a, Ax3 b) { return Ax3{a.x + b.x, a.y + b.y, a.z + b.z}; }
    static __device__ __forceinline__ Ax3 up(Ax3 a, int o) { return Ax3{__shfl_up(a.x, o, 64), __shfl_up(a.y, o, 64), __shfl_up(a.z, o, 64)}; }
};
// Samples: the element is q[e], the result the INCLUSIVE prefix.
struct Ax3Samples {
    typedef Ax3Sum Op;
    const short4 *q;
    Ax3 *out;
    long long n;
    __device__ __forceinline__ Ax3 load(long long e) const
    {
        const short4 v = q[e];
        Ax3 r = {v.x, v.y, v.z};
        return r;
    }
    __device__ __forceinline__ void store(long long e, Ax3 excl, Ax3 v) const { out[e] = Ax3Sum::comb(excl, v); }
};

// ---- rule 24
struct WaAxSmooth {
    const float *xyz;
    const short4 *q;
    const long long *GL;     // n
    const Ax3 *P;            // n, inclusive prefix sums of q
    const long long *off;    // n_legs + 1
    long long n, h_q;
    int32_t n_legs, max_level, check;   // check: a grid and a tool are given
    short4 *q_out;
    uint8_t *level, *blocked;
    unsigned int *list;      // n: the samples that go on beyond level 0
};

// the leg of sample i: the largest l with off[l] <= i (off[l + 1] > i then: empty legs are passed over)
__device__ __forceinline__ void ax_leg(const long long *__restrict__ off, int32_t n_legs, long long i, long long *s, long long *e)
{
    int32_t lo = 0, hi = n_legs - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    *s = off[lo];
    *e = off[lo + 1];
}

// the candidate of sample i at a level below max_level: the window [GL_i - w, GL_i + w] inside the leg s .. e-1, its sum, rule 1
__device__ __forceinline__ short4 ax_candidate(const WaAxSmooth &A, long long i, long long s, long long e, long long w, bool *zero_sum)
{
    const long long gi = A.GL[i], glo = gi - w, ghi = gi + w;
    long long a = s, b = i;          // the first j in [s, i] with GL_j >= glo
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if (A.GL[m] >= glo) b = m; else a = m + 1;
    }
    const long long jlo = a;
    a = i; b = e - 1;                // the last j in [i, e - 1] with GL_j <= ghi
    while (a < b) {
        const long long m = a + ((b - a + 1) >> 1);
        if (A.GL[m] <= ghi) a = m; else b = m - 1;
    }
    Ax3 S = A.P[a];
    if (jlo > 0) {
        const Ax3 p = A.P[jlo - 1];
        S.x -= p.x; S.y -= p.y; S.z -= p.z;
    }
    *zero_sum = S.x == 0 && S.y == 0 && S.z == 0;
    if (*zero_sum) return A.q[i];
    return ax_quantise((double)S.x, (double)S.y, (double)S.z);
}

__global__ __launch_bounds__(256) void k_ax_level0(WaAxSmooth A, WaField F, const WaTorchTool *__restrict__ tool, WaAxRec *__restrict__ rec)
{
    __shared__ int32_t tl[192];
    if (A.check) ax_stage_tool(tool, tl);
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool outside = false, go_on = false, zs = false;
    if (i < A.n) {
        short4 c = A.q[i];
        c.w = 0;
        if (A.max_level > 0) {
            long long s, e;
            ax_leg(A.off, A.n_legs, i, &s, &e);
            c = ax_candidate(A, i, s, e, A.h_q, &zs);
        }
        bool blk = false;
        if (A.check) {
            bool bad = false;
            const int3 v = torch_sample_voxel(A.xyz, i, F, &outside, &bad);
            blk = ax_beads(F, v, c, tl, tool->n_beads) & 1;
        }
        go_on = blk && A.max_level > 0;
        if (!go_on) {
            A.q_out[i] = c;
            A.level[i] = 0;
            A.blocked[i] = blk ? 1 : 0;
        } else {
            zs = false;
        }
    }
    const unsigned long long mo = __ballot(outside), mg = __ballot(go_on), mz = __ballot(zs);
    const int lane = threadIdx.x & 63;
    unsigned int base = 0;
    if (lane == 0) {
        if (mo) atomicAdd(&rec->n_outside, (unsigned long long)__popcll(mo));
        if (mz) atomicAdd(&rec->n_zero_sum, (unsigned long long)__popcll(mz));
        if (mg) base = atomicAdd(&rec->n_climb, (unsigned int)__popcll(mg));
    }
    base = __shfl(base, 0, 64);
    if (go_on) A.list[base + __popcll(mg & ((1ull << lane) - 1))] = (unsigned int)i;   // (n <= 2^31: an index fits)
}

// The order of the list differs from run to run; a sample's result does not depend on it.
__global__ __launch_bounds__(256) void k_ax_climb(WaAxSmooth A, WaField F, const WaTorchTool *__restrict__ tool, WaAxRec *__restrict__ rec)
{
    __shared__ int32_t tl[192];
    ax_stage_tool(tool, tl);
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool zs = false;
    if (e0 < (long long)__hip_atomic_load(&rec->n_climb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const long long i = A.list[e0];
        long long s, e;
        ax_leg(A.off, A.n_legs, i, &s, &e);
        bool outside = false, bad = false;
        const int3 v = torch_sample_voxel(A.xyz, i, F, &outside, &bad);
        const int32_t nb = tool->n_beads;
        short4 c = A.q[i];
        c.w = 0;
        int32_t lev = 1;
        bool blk = true;
        for (; lev <= A.max_level; lev++) {
            zs = false;
            if (lev < A.max_level) {
                c = ax_candidate(A, i, s, e, A.h_q >> lev, &zs);
            } else {
                c = A.q[i];
                c.w = 0;
            }
            blk = ax_beads(F, v, c, tl, nb) & 1;
            if (!blk) break;
        }
        if (lev > A.max_level) lev = A.max_level;   // every level is blocked: the last candidate, q_i, stays
        A.q_out[i] = c;
        A.level[i] = (uint8_t)lev;
        A.blocked[i] = blk ? 1 : 0;
    }
    const unsigned long long mz = __ballot(zs);
    if ((threadIdx.x & 63) == 0 && mz) atomicAdd(&rec->n_zero_sum, (unsigned long long)__popcll(mz));
}

__global__ __launch_bounds__(256) void k_ax_summary(WaAxSmooth A, WaAxRec *__restrict__ rec)
{
    __shared__ unsigned int cnt[WA_AX_MAX_LEVEL + 1];
    if (threadIdx.x <= WA_AX_MAX_LEVEL) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool blk = false;
    unsigned long long t_in = 0, t_out = 0;
    if (i < A.n) {
        atomicAdd(&cnt[A.level[i]], 1u);   // (LDS)
        blk = A.blocked[i] != 0;
        long long s, e;
        ax_leg(A.off, A.n_legs, i, &s, &e);
        if (i + 1 < e) {
            t_in = ax_chord2(A.q[i], A.q[i + 1]) >> 10;
            t_out = ax_chord2(A.q_out[i], A.q_out[i + 1]) >> 10;
        }
    }
    const unsigned long long mb = __ballot(blk);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_down(t_in, o, 64), b = __shfl_down(t_out, o, 64);
        t_in = a > t_in ? a : t_in;
        t_out = b > t_out ? b : t_out;
    }
    if ((threadIdx.x & 63) == 0) {
        if (mb) {
            atomicAdd(&rec->n_blocked, (unsigned long long)__popcll(mb));
            atomicMin(&rec->first_blocked, (unsigned long long)(i + __builtin_ctzll(mb)));
        }
        if (t_in) atomicMax(&rec->max_turn_in, t_in);
        if (t_out) atomicMax(&rec->max_turn_out, t_out);
    }
    __syncthreads();
    if (threadIdx.x <= WA_AX_MAX_LEVEL && cnt[threadIdx.x]) atomicAdd(&rec->n_level[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// ---- rule 25
// m of segment i, +inf where the segment sets no limit; *turning: D > 0; *jump: D > 0 on a segment without length
__device__ __forceinline__ double ax_seg_limit(const float *__restrict__ xyz, const short4 *__restrict__ q, long long i, double omega,
                                               bool *turning, bool *jump)
{
    const uint32_t D = ax_chord2(q[i], q[i + 1]);
    *turning = D > 0;
    *jump = false;
    if (!D) return INFINITY;
    const double ds = rt_seg_len(xyz, i);
    if (rt_quanta(ds) == 0) {
        *jump = true;
        return INFINITY;
    }
    const double psi = __dsqrt_rn((double)D) / 16384.0;
    return __ddiv_rn(ds * omega, psi);
}

__global__ __launch_bounds__(256) void k_ax_limits(const float *__restrict__ xyz, const short4 *__restrict__ q, long long n, double omega,
                                                   double v_cap, double v_floor, float floor_f, const float *__restrict__ v_in,
                                                   float *__restrict__ v_out, WaAxRec *__restrict__ rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool turning = false, jump = false, floored = false, limited = false;
    unsigned int fb = 0xffffffffu;
    if (i < n) {
        bool finite = true;
        for (int c = 0; c < 3; c++) finite = finite && isfinite(xyz[3 * i + c]);
        if (!finite) atomicOr(&rec->bad, 1u);
        double lim = v_cap;
        if (i > 0) {
            bool t2, j2;
            const double m = ax_seg_limit(xyz, q, i - 1, omega, &t2, &j2);
            lim = m < lim ? m : lim;
        }
        if (i < n - 1) {   // the counters of segment i belong to sample i
            const double m = ax_seg_limit(xyz, q, i, omega, &turning, &jump);
            lim = m < lim ? m : lim;
        }
        if (v_in) {
            const double vl = (double)v_in[i];
            if (!(vl > 0.0) || !isfinite(vl)) atomicOr(&rec->bad, 4u);
            lim = vl < lim ? vl : lim;
        }
        float f = (float)lim;
        if ((double)f > lim) f = __uint_as_float(__float_as_uint(f) - 1u);   // (f > lim >= 0: a positive float or +inf, one step down)
        if ((double)f < v_floor) {
            f = floor_f;
            floored = true;
        }
        limited = (double)f < v_cap;
        v_out[i] = f;
        fb = __float_as_uint(f);
    }
    const unsigned long long mt = __ballot(turning), mj = __ballot(jump), mf = __ballot(floored), ml = __ballot(limited);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int b = __shfl_down(fb, o, 64);
        fb = b < fb ? b : fb;
    }
    if ((threadIdx.x & 63) == 0) {
        if (mt) atomicAdd(&rec->n_turning, (unsigned long long)__popcll(mt));
        if (mj) atomicAdd(&rec->n_jump, (unsigned long long)__popcll(mj));
        if (mf) atomicAdd(&rec->n_floored, (unsigned long long)__popcll(mf));
        if (ml) atomicAdd(&rec->n_limited, (unsigned long long)__popcll(ml));
        atomicMin(&rec->min_limit_bits, fb);
    }
}

// ---- rule 26
struct WaTkArgs {
    const float *xyz;
    const short4 *q;
    const long long *B, *time_q;   // w_q and time_q of wa_traj_retime, n each
    long long n, tick_q, n_full, n_ticks;
    double acc, dec;
    int32_t check;                 // a grid and a tool are given
    float *axes;                   // n_ticks x 3 or nullptr
    uint8_t *blocked;              // n_ticks or nullptr
};

__device__ __forceinline__ long long tk_pack(short4 q)
{
    return (long long)(((unsigned long long)(unsigned short)q.x) | ((unsigned long long)(unsigned short)q.y << 16) |
                       ((unsigned long long)(unsigned short)q.z << 32));
}
__device__ __forceinline__ short4 tk_unpack(long long p)
{
    short4 q;
    q.x = (short)(p & 0xffff);
    q.y = (short)((p >> 16) & 0xffff);
    q.z = (short)((p >> 32) & 0xffff);
    q.w = 0;
    return q;
}

// the axis at a located tick: the two samples' axes interpolated in double, quantised by rule 1; q_i where they cancel
__device__ __forceinline__ short4 tk_axis(const short4 *__restrict__ q, const RtTick &r)
{
    const short4 a = q[r.i], b = q[r.i + 1];
    const double lam = r.exact == 1 ? 1.0 : r.lam;
    const double vx = (double)a.x + ((double)b.x - (double)a.x) * lam, vy = (double)a.y + ((double)b.y - (double)a.y) * lam,
                 vz = (double)a.z + ((double)b.z - (double)a.z) * lam;
    if (vx == 0.0 && vy == 0.0 && vz == 0.0) {
        short4 c = a;
        c.w = 0;
        return c;
    }
    return ax_quantise(vx, vy, vz);
}

// One lane per tick, 256 ticks per workgroup.  The ticks of a wave are consecutive in time, so the segment of the tick in front of the
// wave's first one (found once, the same search in every lane: one address per step) is a lower end for every lane's own search,
// which gallops up from there: ticks that share a segment or sit a few segments on take a step or two where the full search takes
// log2(n).  The tool sits in LDS; a bead's thresholds are LDS broadcasts.  The wave's first lane works out the axis of the tick in front
// of it a second time for max_tick_turn (the other lanes get their neighbour's by a shuffle): nothing is read that another
// workgroup writes.  The block's 256 axes go through LDS so that consecutive lanes store consecutive floats; its counters are added
// up in LDS and leave as one atomic each (WaAxSlot).
// STOPS (wa_traj_tick_axes_stops, rule 41): the same kernel with a dwell's turn in place, a tag per tick and three more counters; what it
// adds is compiled in only there.
struct WaTkStopsSlot {
    unsigned long long n_dwell, n_tagged, pad[6];   // one 64-byte line, as WaAxSlot
};
struct WaTkStopsRec {
    WaTkStopsSlot slot[WA_AX_SLOTS];
    unsigned long long max_dwell_turn;
};
struct WaTkStops {
    const uint8_t *seg_tag;   // n - 1 or nullptr
    uint8_t *tag;             // n_ticks or nullptr
    WaTkStopsRec *rec;
};

// Rule 6 for one tau, and in a dwell (a located segment without length whose time goes on, tau before its end) the lambda of rule 41 for
// the AXIS: the position of such a tick stays p_i (exact == 2 keeps rt_tick_pos off lam).
template <bool STOPS>
__device__ __forceinline__ RtTick tk_locate(const WaTkArgs &T, long long tau, long long lo, long long hi, bool *dwell)
{
    RtTick r = rt_tick_locate(T.xyz, T.acc, T.dec, T.B, T.time_q, tau, lo, hi);
    *dwell = false;
    if (STOPS && r.exact == 2) {
        const long long t0 = T.time_q[r.i], t1 = T.time_q[r.i + 1];
        if (t1 > t0) {
            *dwell = true;
            const double lam = __ddiv_rn((double)(tau - t0), (double)(t1 - t0));
            r.lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
        }
    }
    return r;
}

template <bool STOPS>
__device__ __forceinline__ void tk_axes(const WaTkArgs &T, const WaField &F, const WaTorchTool *__restrict__ tool, WaAxRec *__restrict__ rec,
                                        const WaTkStops &S)
{
    __shared__ float stage[256 * 3];
    __shared__ int32_t tl[192];
    __shared__ unsigned int cnt[3], blk_turn;   // the workgroup's ticks outside / blocked / near, its largest turn
    __shared__ unsigned long long blk_first;    // its first blocked tick
    __shared__ unsigned int st_cnt[2], st_turn; // STOPS: its ticks in a dwell / with a tag, its largest turn at a dwell tick
    __shared__ uint32_t st_tag[64];             // STOPS: its 256 tags, so that a lane stores four of them as one word
    if (T.check) ax_stage_tool(tool, tl);
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        blk_turn = 0;
        blk_first = ~0ull;
        if (STOPS) st_cnt[0] = st_cnt[1] = st_turn = 0;
    }
    __syncthreads();
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long k_first = k - lane;   // (wave-uniform)
    bool outside = false, blocked = false, near = false, dwell = false, front_dwell;
    unsigned long long turn = 0;
    long long mine = 0;
    uint8_t tag = 0;
    bool live = k < T.n_ticks;
    if (k_first < T.n_ticks) {
        const long long total = T.time_q[T.n - 1];
        // the segment of tick k_first - 1 (always a full tick), or of tick 0
        const long long tau_front = k_first > 0 ? (k_first - 1) * T.tick_q : 0;
        const RtTick front = tk_locate<STOPS>(T, tau_front, 0, T.n - 2, &front_dwell);
        if (live) {
            const long long tau = k < T.n_full ? k * T.tick_q : total;
            long long lo = front.i, hi = T.n - 2, step = 1;
            while (lo + step <= hi && T.time_q[lo + step] <= tau) {
                lo += step;
                step <<= 1;
            }
            hi = lo + step - 1 < hi ? lo + step - 1 : hi;
            const RtTick r = tk_locate<STOPS>(T, tau, lo, hi, &dwell);
            const short4 qt = tk_axis(T.q, r);
            mine = tk_pack(qt);
            if (STOPS && S.seg_tag) tag = S.seg_tag[r.i];
            for (int c = 0; c < 3; c++) stage[3 * threadIdx.x + c] = (float)((double)(c == 0 ? qt.x : (c == 1 ? qt.y : qt.z)) / 16384.0);
            if (T.check) {
                int64_t id;
                const int3 v = field_voxel(F, rt_tick_pos(T.xyz, r, 0), rt_tick_pos(T.xyz, r, 1), rt_tick_pos(T.xyz, r, 2), &id, &outside);
                const int32_t res = ax_beads(F, v, qt, tl, tool->n_beads);
                blocked = res & 1;
                near = !blocked && (res >> 8) > 0;
            }
            if (T.blocked) T.blocked[k] = blocked ? 1 : 0;
        }
        long long before = __shfl_up(mine, 1, 64);
        if (lane == 0 && k > 0) before = tk_pack(tk_axis(T.q, front));
        if (live && k > 0) turn = ax_chord2(tk_unpack(before), tk_unpack(mine)) >> 10;
    }
    const unsigned long long mo = __ballot(outside), mb = __ballot(blocked), mn = __ballot(near);
    if (STOPS) {
        ((uint8_t *)st_tag)[threadIdx.x] = tag;   // (0 past the last tick)
        const unsigned long long md = __ballot(dwell), mg = __ballot(tag != 0);
        unsigned long long dturn = dwell ? turn : 0;
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t2 = __shfl_down(dturn, o, 64);
            dturn = t2 > dturn ? t2 : dturn;
        }
        if (lane == 0) {   // (LDS atomics)
            if (md) atomicAdd(&st_cnt[0], (unsigned int)__popcll(md));
            if (mg) atomicAdd(&st_cnt[1], (unsigned int)__popcll(mg));
            if (dturn) atomicMax(&st_turn, (unsigned int)dturn);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t2 = __shfl_down(turn, o, 64);
        turn = t2 > turn ? t2 : turn;
    }
    if (lane == 0) {   // (LDS atomics)
        if (mo) atomicAdd(&cnt[0], (unsigned int)__popcll(mo));
        if (mb) {
            atomicAdd(&cnt[1], (unsigned int)__popcll(mb));
            atomicMin(&blk_first, (unsigned long long)(k + __builtin_ctzll(mb)));
        }
        if (mn) atomicAdd(&cnt[2], (unsigned int)__popcll(mn));
        if (turn) atomicMax(&blk_turn, (unsigned int)turn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        WaAxSlot *s = &rec->slot[blockIdx.x & (WA_AX_SLOTS - 1)];
        if (cnt[0]) atomicAdd(&s->n_outside, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&s->n_blocked, (unsigned long long)cnt[1]);
        if (cnt[2]) atomicAdd(&s->n_near, (unsigned long long)cnt[2]);
        // first_blocked only falls and max_tick_turn only rises: a value that cannot win against what is there already is not sent
        if (blk_first < __hip_atomic_load(&rec->first_blocked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&rec->first_blocked, blk_first);
        if (blk_turn > __hip_atomic_load(&rec->max_tick_turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&rec->max_tick_turn, (unsigned long long)blk_turn);
        if (STOPS) {
            WaTkStopsSlot *s2 = &S.rec->slot[blockIdx.x & (WA_AX_SLOTS - 1)];
            if (st_cnt[0]) atomicAdd(&s2->n_dwell, (unsigned long long)st_cnt[0]);
            if (st_cnt[1]) atomicAdd(&s2->n_tagged, (unsigned long long)st_cnt[1]);
            if (st_turn > __hip_atomic_load(&S.rec->max_dwell_turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&S.rec->max_dwell_turn, (unsigned long long)st_turn);
        }
    }
    if (T.axes) {
        const long long first = (long long)blockIdx.x * blockDim.x * 3, end = T.n_ticks * 3;
        for (int e = threadIdx.x; e < 256 * 3; e += 256)
            if (first + e < end) T.axes[first + e] = stage[e];
    }
    if (STOPS && S.tag && threadIdx.x < 64) {   // (the block's first tick is a multiple of 256: the words are aligned)
        const long long first = (long long)blockIdx.x * blockDim.x + 4 * threadIdx.x;
        if (first + 4 <= T.n_ticks) {
            *(uint32_t *)(S.tag + first) = st_tag[threadIdx.x];
        } else {
            for (int b = 0; b < 4; b++)
                if (first + b < T.n_ticks) S.tag[first + b] = ((const uint8_t *)st_tag)[4 * threadIdx.x + b];
        }
    }
}

__global__ __launch_bounds__(256) void k_tk_axes(WaTkArgs T, WaField F, const WaTorchTool *__restrict__ tool, WaAxRec *__restrict__ rec)
{
    tk_axes<false>(T, F, tool, rec, WaTkStops{});
}
