// jerk_kernels.hpp -- device side of the jerk-limited controller ticks (wa_traj_retime_jerk; include/weldacs.h rules 48 - 55 hold the
// definition, DESIGN 4ab the reasoning, tests/jerk_ref.py restates it in numpy).  The W last ticks are averaged in the ARC LENGTH, so
// the filtered tick stays on the polyline; the caps are lowered over the distance a window can span before the profile is computed,
// and the dwells arrive already extended (the host adds (W - 1) * tick_q).  The profile itself is the stops path of retime_run as it
// stands: k_rt_segments, k_st_caps or the lowering below, the scans, k_st_times.
//   k_jk_caps     rt_caps<false, true>: kinds 1 - 3 for every sample as one key C * 4 + kind
//   k_scan        (scan_kernels.hpp) over JkLengths (GL, the minimum ignored), JkNext (the next stop at or after a sample, a suffix
//                 minimum) and, through RtSamples, over the arc lengths of the unfiltered ticks modulo 2^64, in place
//   k_jk_window   one lane per sample: two binary searches in GL give the index range of rule 49; the widest range goes to the record
//   k_jk_level    one level of the sparse table of power-of-two minima of the keys
//   k_jk_lower    one lane per sample: the range minimum by two overlapping loads, C', its kind, the kind-0 caps, the lowered flag
//   k_jk_groups   one lane per sample: bit 6 of bound; per stop the dwell the caller asked for, added to the head of its group
//   k_jk_arcs     one lane per unfiltered tick: rt_tick_locate, unchanged, and the arc length U of the tick
//   k_jk_ticks    one lane per output tick: S from two prefix entries and one division, the segment by binary search in GL bracketed
//                 per wavefront, the position through LDS, the tag, s_q, the maxima and counters of the summary
//   k_jk_rests    one lane per segment: groups of stops with fewer rest ticks than their dwells hold
// Integers and single correctly rounded fp64 operations throughout; what is accumulated across lanes is an integer, one atomic per
// wavefront; no workgroup waits for another.
#pragma once
#include "stops_kernels.hpp"

#define WA_JK_MAX_W (1 << 20)

struct WaJkRec {
    unsigned long long max_width;   // the widest window of rule 49, in samples (read before the table is sized)
    unsigned long long n_lowered;
    unsigned long long max_d1, max_d2, max_d3, in_max_d2;
    unsigned long long n_rest, n_short, n_back;
};

__global__ __launch_bounds__(256) void k_jk_caps(const float *__restrict__ xyz, long long n, WaRtLimits lim, const float *__restrict__ v_limit,
                                                 WaField F, long long *__restrict__ key, WaRtRec *__restrict__ rec)
{
    rt_caps<false, true>(xyz, n, lim, v_limit, F, key, nullptr, rec, nullptr);
}

// GL: element e is sample e, its weight L_e (0 behind the last sample); the result is the exclusive sum.
struct JkLengths {
    typedef RtMinSum Op;
    const float *xyz;
    long long *out;
    long long n;
    __device__ __forceinline__ RtPair load(long long e) const
    {
        RtPair v;
        v.s = e < n - 1 ? rt_quanta(rt_seg_len(xyz, e)) : 0;
        v.m = WA_RT_INF;
        return v;
    }
    __device__ __forceinline__ void store(long long e, RtPair excl, RtPair) const { out[e] = excl.s; }
};
// The lowest stop segment at or after sample j (n where there is none): element e is sample n - 1 - e, all weights 0, so the pair's
// minimum is the plain minimum of what came before -- a suffix minimum of (j if segment j is a stop, else n).
struct JkNext {
    typedef RtMinSum Op;
    const long long *dq;
    long long *out;
    long long n;
    __device__ __forceinline__ RtPair load(long long e) const
    {
        const long long j = n - 1 - e;
        RtPair v;
        v.s = 0;
        v.m = j < n - 1 && dq[j] >= 0 ? j : n;
        return v;
    }
    __device__ __forceinline__ void store(long long e, RtPair excl, RtPair v) const { out[n - 1 - e] = rt_comb(excl, v).m; }
};

// the largest m in [lo, hi] with GL[m] < x, lo - 1 where there is none
__device__ __forceinline__ long long jk_last_below(const long long *__restrict__ GL, long long lo, long long hi, long long x)
{
    long long a = lo - 1;
    while (a < hi) {
        const long long mid = a + ((hi - a + 1) >> 1);
        if (GL[mid] < x) a = mid; else hi = mid - 1;
    }
    return a;
}
// the largest m in [lo, hi] with GL[m] <= x, lo - 1 where there is none
__device__ __forceinline__ long long jk_last_at_most(const long long *__restrict__ GL, long long lo, long long hi, long long x)
{
    long long a = lo - 1;
    while (a < hi) {
        const long long mid = a + ((hi - a + 1) >> 1);
        if (GL[mid] <= x) a = mid; else hi = mid - 1;
    }
    return a;
}

// Rule 49, the range.  The window of sample j holds j - 1, j and j + 1 whatever R_q: the searches run outside them.
__global__ __launch_bounds__(256) void k_jk_window(const long long *__restrict__ GL, long long n, long long R_q, uint2 *__restrict__ win,
                                                   WaJkRec *__restrict__ rec)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long width = 0;
    if (j < n) {
        const long long jl = j > 0 ? j - 1 : 0, jr = j < n - 1 ? j + 1 : n - 1;
        const long long lo = jk_last_below(GL, 0, jl, GL[jl] - R_q) + 1;
        long long hi = jk_last_at_most(GL, jr, n - 1, GL[jr] + R_q);
        hi = hi < jr ? jr : hi;
        win[j] = make_uint2((unsigned int)(lo > jl ? jl : lo), (unsigned int)hi);
        width = (unsigned long long)(hi - (lo > jl ? jl : lo) + 1);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w2 = __shfl_down(width, o, 64);
        width = w2 > width ? w2 : width;
    }
    if ((threadIdx.x & 63) == 0 && width) atomicMax(&rec->max_width, width);
}

// next[m] = min(prev[m .. m + 2 * h - 1]) from prev[m] = min(prev0[m .. m + h - 1]), indices clamped to n - 1
__global__ __launch_bounds__(256) void k_jk_level(const unsigned long long *__restrict__ prev, unsigned long long *__restrict__ next,
                                                  long long n, long long h)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const unsigned long long a = prev[m], b = prev[m + h < n ? m + h : n - 1];
    next[m] = a < b ? a : b;
}

// Rule 49, the minimum, and retime rule 2's kind 0 behind it.  table holds the levels 1 .. P of the keys' sparse table, n entries each.
__global__ __launch_bounds__(256) void k_jk_lower(const unsigned long long *__restrict__ key, const unsigned long long *__restrict__ table,
                                                  long long n, const uint2 *__restrict__ win, const long long *__restrict__ dq,
                                                  long long *__restrict__ C, uint8_t *__restrict__ kind, uint8_t *__restrict__ low,
                                                  WaJkRec *__restrict__ rec)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool lowered = false;
    if (j < n) {
        const uint2 w = win[j];
        const long long lo = w.x, hi = w.y, width = hi - lo + 1;
        const int p = 63 - __clzll((unsigned long long)width);
        const unsigned long long *src = p ? table + (long long)(p - 1) * n : key;
        const unsigned long long a = src[lo], b = src[hi - (1ll << p) + 1], m = a < b ? a : b;
        long long c = (long long)(m >> 2);
        int k = (int)(m & 3);
        lowered = c < (long long)(key[j] >> 2);
        if (j == 0 || j == n - 1 || dq[j > 0 ? j - 1 : 0] >= 0 || dq[j < n - 1 ? j : n - 2] >= 0) { c = 0; k = 0; }
        C[j] = c;
        kind[j] = (uint8_t)k;
        low[j] = lowered ? 1 : 0;
    }
    const unsigned long long ml = __ballot(lowered);
    if ((threadIdx.x & 63) == 0 && ml) atomicAdd(&rec->n_lowered, (unsigned long long)__popcll(ml));
}

// Behind k_st_times.  Bit 6 of bound (low == nullptr: nothing was lowered).  A stop's group is every stop with its GL; the lowest one
// is its head (next[] of the first sample with that GL) and collects the dwells the caller asked for (dq holds them extended by ext).
__global__ __launch_bounds__(256) void k_jk_groups(const long long *__restrict__ GL, long long n, const uint8_t *__restrict__ low,
                                                   const long long *__restrict__ dq, const long long *__restrict__ next, long long ext,
                                                   uint8_t *__restrict__ bound, unsigned long long *__restrict__ need)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (low && low[j]) bound[j] |= 0x40;
    if (next && j < n - 1 && dq[j] >= 0) {
        const long long first = jk_last_below(GL, 0, j, GL[j]) + 1;
        atomicAdd(&need[next[first]], (unsigned long long)(dq[j] - ext));
    }
}

// Rule 52.  The ticks of a wave are consecutive in time: the segment of the wave's first tick (the same search in every lane) is a
// lower end for every lane's own search, which gallops up from there, as in tk_axes.  U goes where the scan turns it into prefix sums.
__global__ __launch_bounds__(256) void k_jk_arcs(const float *__restrict__ xyz, long long n, double acc, double dec,
                                                 const long long *__restrict__ B, const long long *__restrict__ time_q,
                                                 const long long *__restrict__ GL, long long tick_q, long long n_full, long long n_u,
                                                 long long *__restrict__ U)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long k_first = k - (threadIdx.x & 63);
    if (k >= n_u) return;
    const RtTick front = rt_tick_locate(xyz, acc, dec, B, time_q, k_first * tick_q, 0, n - 2);   // (tick k_first < n_u is a full tick or the last)
    const long long tau = k < n_full ? k * tick_q : time_q[n - 1];
    long long lo = k_first < n_full ? front.i : 0, hi = n - 2, step = 1;
    while (lo + step <= hi && time_q[lo + step] <= tau) {
        lo += step;
        step <<= 1;
    }
    hi = lo + step - 1 < hi ? lo + step - 1 : hi;
    const RtTick r = rt_tick_locate(xyz, acc, dec, B, time_q, tau, lo, hi);
    const long long g = GL[r.i], len = GL[r.i + 1] - g;
    U[k] = g + (r.exact == 1 ? len : (r.exact == 2 ? 0 : (long long)rint(r.lam * (double)len)));
}

struct WaJkTicks {
    const float *xyz;
    long long n;
    const long long *GL, *next;   // next: nullptr without a stop
    const long long *P;           // n_u + 1 prefix sums of U modulo 2^64
    long long n_u, n_ticks, length_q;
    unsigned long long W;
    const uint8_t *seg_tag;       // n - 1 or nullptr
    float *out;                   // 3 * n_ticks or nullptr
    long long *s_q;               // n_ticks or nullptr
    uint8_t *tag;                 // n_ticks or nullptr
    unsigned long long *rest_cnt; // per stop segment (with next)
    WaJkRec *rec;
};

__device__ __forceinline__ long long jk_u(const WaJkTicks &T, long long k)   // rule 52 with its padding
{
    if (k < 0) return 0;
    if (k >= T.n_u) return T.length_q;
    return (long long)((unsigned long long)T.P[k + 1] - (unsigned long long)T.P[k]);
}
__device__ __forceinline__ long long jk_s(const WaJkTicks &T, long long k)   // rule 53, k in 0 .. n_ticks - 1
{
    const long long hi = (k < T.n_u - 1 ? k : T.n_u - 1) + 1, lo = k - (long long)T.W + 1 > 0 ? k - (long long)T.W + 1 : 0;
    const long long behind = k - T.n_u + 1 > 0 ? k - T.n_u + 1 : 0;
    const unsigned long long sum = (unsigned long long)T.P[hi] - (unsigned long long)T.P[lo] + (unsigned long long)behind * (unsigned long long)T.length_q;
    return (long long)(sum / T.W);
}
__device__ __forceinline__ unsigned long long jk_abs(long long v) { return v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v; }
__device__ __forceinline__ unsigned long long jk_wave_max(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v2 = __shfl_down(v, o, 64);
        v = v2 > v ? v2 : v;
    }
    return v;
}

// Rules 53 - 55.  S of the three ticks in front of a wave is worked out a second time by its first three lanes: nothing is read that
// another workgroup writes.  S rises along a wave (n_back counts where it does not), so the first sample at or behind the wave's first S
// brackets every lane's search from below; a lane whose S lies in front of it searches the samples in front.  A run of samples
// that share one GL is crossed by galloping, never sample by sample; the stop that takes a rest tick comes from next[].
// FIRST (wa_traj_retime_jerk_axes, rule 58): the same kernel, which also leaves the lowest rest tick of every stop in first[]; what it
// adds is compiled in only there (jerk_axes_kernels.hpp holds that instantiation).
template <bool FIRST>
__device__ __forceinline__ void jk_ticks(const WaJkTicks &T, unsigned long long *__restrict__ first)
{
    __shared__ float stage[256 * 3];
    __shared__ uint32_t st_tag[64];
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long k_first = k - lane;   // (wave-uniform)
    const bool live = k < T.n_ticks;
    unsigned long long d1 = 0, d2 = 0, d3 = 0, u2 = 0;
    bool back = false, rest = false;
    long long seg = -1;
    uint8_t tag = 0;
    if (k_first < T.n_ticks) {
        const long long S = live ? jk_s(T, k) : T.length_q;
        const long long kh = k_first - 1 - lane;
        const long long halo = lane < 3 && kh >= 0 ? jk_s(T, kh) : 0;
        const long long h1 = __shfl(halo, 0, 64), h2 = __shfl(halo, 1, 64), h3 = __shfl(halo, 2, 64);
        long long s1 = __shfl_up(S, 1, 64), s2 = __shfl_up(S, 2, 64), s3 = __shfl_up(S, 3, 64);
        if (lane < 1) s1 = h1;
        if (lane < 2) s2 = lane == 1 ? h1 : h2;
        if (lane < 3) s3 = lane == 2 ? h1 : (lane == 1 ? h2 : h3);
        const long long S0 = __shfl(S, 0, 64);
        const long long base = jk_last_below(T.GL, 0, T.n - 2, S0);   // (GL_(n-1) = length_q >= every S)
        if (live) {
            if (k >= 1) {
                d1 = jk_abs(S - s1);
                back = S < s1;
            }
            if (k >= 2) d2 = jk_abs((S - s1) - (s1 - s2));
            if (k >= 3) d3 = jk_abs(((S - s1) - (s1 - s2)) - ((s1 - s2) - (s2 - s3)));
            const long long uk = jk_u(T, k), um = jk_u(T, k - 1);
            u2 = jk_abs((jk_u(T, k + 1) - uk) - (uk - um));
            if (k == 0 && (unsigned long long)uk > u2) u2 = (unsigned long long)uk;   // (the difference centred on tick -1 is U_0)
            // a = the last sample with GL < S
            long long a;
            if (S >= S0) {
                long long step = 1;
                a = base;
                while (a + step <= T.n - 2 && T.GL[a + step] < S) {
                    a += step;
                    step <<= 1;
                }
                a = jk_last_below(T.GL, a + 1, a + step - 1 < T.n - 2 ? a + step - 1 : T.n - 2, S);
            } else {
                a = jk_last_below(T.GL, 0, base, S);
            }
            const long long lo = a + 1;   // the first sample with GL >= S, at most n - 1
            long long i;
            const long long f = T.next ? T.next[lo] : T.n;
            if (f < T.n - 1 && T.GL[f] == S) {   // rule 54 (a)
                rest = true;
                i = f;
            } else if (T.GL[lo] > S) {
                i = lo - 1;   // (GL_0 = 0 <= S: lo >= 1)
            } else if (lo >= T.n - 2) {
                i = T.n - 2;
            } else {   // the last sample of the run with GL = S, up to n - 2
                long long b = lo, step = 1;
                while (b + step <= T.n - 2 && T.GL[b + step] <= S) {
                    b += step;
                    step <<= 1;
                }
                i = jk_last_at_most(T.GL, b + 1, b + step - 1 < T.n - 2 ? b + step - 1 : T.n - 2, S);
            }
            seg = i;
            RtTick r;
            r.i = i;
            r.lam = 0.0;
            r.exact = 0;
            const long long g0 = T.GL[i], g1 = T.GL[i + 1];
            if (rest) r.exact = 2;
            else if (S >= g1) r.exact = 1;
            else if (g1 == g0) r.exact = 2;
            else r.lam = __ddiv_rn((double)(S - g0), (double)(g1 - g0));
            if (T.out)
                for (int c = 0; c < 3; c++) stage[3 * threadIdx.x + c] = rt_tick_pos(T.xyz, r, c);
            if (T.seg_tag) tag = T.seg_tag[i];
            if (T.s_q) T.s_q[k] = S;
        }
        // rest ticks per stop: one atomic per wave and stop (a wave rarely holds more than one)
        unsigned long long todo = __ballot(rest);
        while (todo) {
            const long long who = __shfl(seg, __builtin_ctzll(todo), 64);
            const unsigned long long same = __ballot(rest && seg == who);
            if (lane == 0) {
                atomicAdd(&T.rest_cnt[who], (unsigned long long)__popcll(same));
                if (FIRST) atomicMin(&first[who], (unsigned long long)(k_first + __builtin_ctzll(same)));
            }
            todo &= ~same;
        }
        const unsigned long long mr = __ballot(rest), mb = __ballot(back);
        d1 = jk_wave_max(d1);
        d2 = jk_wave_max(d2);
        d3 = jk_wave_max(d3);
        u2 = jk_wave_max(u2);
        if (lane == 0) {   // (a maximum only rises: a value that cannot win against what is there already is not sent)
            if (d1 > __hip_atomic_load(&T.rec->max_d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&T.rec->max_d1, d1);
            if (d2 > __hip_atomic_load(&T.rec->max_d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&T.rec->max_d2, d2);
            if (d3 > __hip_atomic_load(&T.rec->max_d3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&T.rec->max_d3, d3);
            if (u2 > __hip_atomic_load(&T.rec->in_max_d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&T.rec->in_max_d2, u2);
            if (mr) atomicAdd(&T.rec->n_rest, (unsigned long long)__popcll(mr));
            if (mb) atomicAdd(&T.rec->n_back, (unsigned long long)__popcll(mb));
        }
    }
    ((uint8_t *)st_tag)[threadIdx.x] = tag;   // (0 past the last tick)
    __syncthreads();
    if (T.out) {
        const long long first = (long long)blockIdx.x * blockDim.x * 3, end = T.n_ticks * 3;
        for (int e = threadIdx.x; e < 256 * 3; e += 256)
            if (first + e < end) T.out[first + e] = stage[e];
    }
    if (T.tag && threadIdx.x < 64) {   // (the block's first tick is a multiple of 256: the words are aligned)
        const long long first = (long long)blockIdx.x * blockDim.x + 4 * threadIdx.x;
        if (first + 4 <= T.n_ticks) {
            *(uint32_t *)(T.tag + first) = st_tag[threadIdx.x];
        } else {
            for (int b = 0; b < 4; b++)
                if (first + b < T.n_ticks) T.tag[first + b] = ((const uint8_t *)st_tag)[4 * threadIdx.x + b];
        }
    }
}

__global__ __launch_bounds__(256) void k_jk_ticks(WaJkTicks T)
{
    jk_ticks<false>(T, nullptr);
}

// Rule 55, n_short_rests: the head of a group holds the group's rest ticks and the dwells its stops were given.
__global__ __launch_bounds__(256) void k_jk_rests(const long long *__restrict__ GL, long long n, const long long *__restrict__ dq,
                                                  const long long *__restrict__ next, const unsigned long long *__restrict__ need,
                                                  const unsigned long long *__restrict__ rest_cnt, unsigned long long tick_q,
                                                  WaJkRec *__restrict__ rec)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool shrt = false;
    if (j < n - 1 && dq[j] >= 0 && next[jk_last_below(GL, 0, j, GL[j]) + 1] == j) shrt = rest_cnt[j] < need[j] / tick_q;
    const unsigned long long ms = __ballot(shrt);
    if ((threadIdx.x & 63) == 0 && ms) atomicAdd(&rec->n_short, (unsigned long long)__popcll(ms));
}
