// retime_kernels.hpp -- device side of wa_traj_retime: speed caps, acceleration / deceleration ramps and controller ticks along a sampled
// trajectory (include/weldacs.h states the definition; tests/retime_ref.py restates it in numpy).
//   k_rt_segments  one lane per segment: its float64 length, L, A, D in quanta of 2^-30; the sums of L, A, D; non-finite coordinates
//   k_rt_caps      one lane per sample: the smallest of the speed caps (end point, v_max / v_limit, curvature, clearance), its kind
//   k_scan         (scan_kernels.hpp) over pairs (weight, cap) under  (s1, m1) + (s2, m2) = (s1 + s2, min(m1, m2 - s1)):  after
//                  sample i the pair holds GA_{i+1} and min_{j <= i} (C_j - GA_j), so F_i = m + GA_i comes out of ONE pass -- the add-scan
//                  and the min-scan of a direction share every launch.  The backward pass is the same scan on reversed indices, the
//                  time scan the same scan with the minimum ignored.
//   k_rt_times     one lane per sample: bound bits, the segment's time T, the summary's counters
//   k_rt_ticks     one lane per tick: binary search in time_q, the position on its segment, stores staged through LDS
// k_rt_caps and k_rt_times are the STOPS == false instantiations of rt_caps / rt_times; stops_kernels.hpp holds the others.
// Integers and single correctly rounded fp64 operations throughout (the translation unit is built without contraction): every output
// is bit-exact and independent of scheduling; what is accumulated across lanes is an integer.
#pragma once
#include "clearance_kernels.hpp"
#include "scan_kernels.hpp"

#define WA_RT_Q 1073741824.0                // 2^30 quanta per unit
#define WA_RT_CAP (1ll << 61)               // "no cap"; also the bound every sum must stay below
#define WA_RT_INF (1ll << 62)               // the scan's neutral minimum
#define WA_RT_MAX_N (1ll << 31)

// what the host reads once, behind k_rt_times.  Sums that may not reach 2^61 are kept as two words, low 32 bits and the rest, each
// added with integer atomics (one per wave, the wave's share saturated at 2^61): exact whatever the order, no overflow below 2^31 samples.
struct WaRtRec {
    unsigned long long sumL[2], sumA[2], sumD[2], sumT[2];
    unsigned long long n_bound[4], n_on_cap, n_on_ramp, n_triangle, n_outside;
    long long peak;
    int32_t bad;     // bit 0: a coordinate is not finite; bit 1: a segment time does not fit; bit 2: a v_limit entry is not finite or <= 0;
                     // bit 3: a stop on a segment that has a length
    int32_t pad;
};

struct RtPair { long long s, m; };

__device__ __forceinline__ RtPair rt_comb(RtPair x, RtPair y)
{
    RtPair r;
    r.s = (long long)((unsigned long long)x.s + (unsigned long long)y.s);
    const long long ym = (long long)((unsigned long long)y.m - (unsigned long long)x.s);
    r.m = x.m < ym ? x.m : ym;
    return r;
}
// the scan's operator (scan_kernels.hpp)
struct RtMinSum {
    typedef RtPair T;
    static __device__ __forceinline__ RtPair id() { return RtPair{0, WA_RT_INF}; }
    static __device__ __forceinline__ RtPair comb(RtPair x, RtPair y) { return rt_comb(x, y); }
    static __device__ __forceinline__ RtPair up(RtPair v, int o) { return RtPair{__shfl_up(v.s, o, 64), __shfl_up(v.m, o, 64)}; }
};

__device__ __forceinline__ unsigned long long rt_sat_add(unsigned long long a, unsigned long long b)   // a, b <= 2^61
{
    const unsigned long long s = a + b;
    return s > (unsigned long long)WA_RT_CAP ? (unsigned long long)WA_RT_CAP : s;
}
__device__ __forceinline__ unsigned long long rt_wave_sat_sum(unsigned long long v)   // lane 0 holds the wave's sum, saturated
{
    for (int o = 32; o > 0; o >>= 1) v = rt_sat_add(v, __shfl_down(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long rt_wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ void rt_acc_split(unsigned long long *acc2, unsigned long long v)
{
    if (!v) return;
    atomicAdd(&acc2[0], v & 0xffffffffull);
    atomicAdd(&acc2[1], v >> 32);
}

// rint(x * 2^30) as an integer, 2^61 where that is 2^61 or more
__device__ __forceinline__ long long rt_quanta(double x)
{
    const double q = rint(x * WA_RT_Q);
    return !(q < (double)WA_RT_CAP) ? WA_RT_CAP : (long long)q;
}

__device__ __forceinline__ double rt_norm(double x, double y, double z)
{
    return __dsqrt_rn((x * x + y * y) + z * z);
}
// the length of segment i as wa_grid_path_shortcut defines one
__device__ __forceinline__ double rt_seg_len(const float *__restrict__ xyz, long long i)
{
    const float *a = xyz + 3 * i, *b = a + 3;
    return rt_norm((double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]);
}

// Rule 1.  A and D get n entries: entry n - 1 (no segment behind the last sample) is 0, which is what the scans want there.
__global__ __launch_bounds__(256) void k_rt_segments(const float *__restrict__ xyz, long long n, double acc, double dec,
                                                     long long *__restrict__ A, long long *__restrict__ D, WaRtRec *__restrict__ rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long l = 0, a = 0, d = 0;
    if (i < n) {
        bool finite = true;
        for (int c = 0; c < 3; c++) finite = finite && isfinite(xyz[3 * i + c]);
        if (!finite) atomicOr(&rec->bad, 1);
        if (i < n - 1) {
            const double ds = rt_seg_len(xyz, i);
            l = rt_quanta(ds);
            if (l > 0) {
                a = rt_quanta((2.0 * acc) * ds);
                d = rt_quanta((2.0 * dec) * ds);
                a = a < 1 ? 1 : a;
                d = d < 1 ? 1 : d;
            }
        }
        A[i] = a;
        D[i] = d;
    }
    const unsigned long long sl = rt_wave_sat_sum((unsigned long long)l), sa = rt_wave_sat_sum((unsigned long long)a),
                             sd = rt_wave_sat_sum((unsigned long long)d);
    if ((threadIdx.x & 63) == 0) {
        rt_acc_split(rec->sumL, sl);
        rt_acc_split(rec->sumA, sa);
        rt_acc_split(rec->sumD, sd);
    }
}

struct WaRtLimits {
    double v_max, acc, dec, a_lat, v_near;
    int32_t near_d2;      // < 0: no clearance cap
    int32_t curv;         // a_lat is finite and not 0
};

// Rule 2.  The voxel of a sample is found by field_voxel, the lookup k_clr_samples runs; a call without a grid passes a zeroed view.
// STOPS (wa_traj_retime_stops, stops_kernels.hpp): dq holds the dwell of every segment in quanta, -1 where the segment is no stop; both
// samples of a stop get the kind-0 cap of the end points.
// KEYS (wa_traj_retime_jerk, jerk_kernels.hpp): kinds 1 - 3 only, for every sample, and C takes the pair as ONE unsigned 64-bit key
// C * 4 + kind (kind is not written): the smallest key of a range is its smallest cap with the lowest-numbered kind attaining it.
template <bool STOPS, bool KEYS = false>
__device__ __forceinline__ void rt_caps(const float *__restrict__ xyz, long long n, const WaRtLimits &lim, const float *__restrict__ v_limit,
                                        const WaField &F, long long *__restrict__ C, uint8_t *__restrict__ kind, WaRtRec *__restrict__ rec,
                                        const long long *__restrict__ dq)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long outs = 0;
    if (i < n) {
        const float *p = xyz + 3 * i;
        double vm = lim.v_max;
        if (v_limit) {
            const double vl = (double)v_limit[i];
            if (!(vl > 0.0) || !isfinite(vl)) atomicOr(&rec->bad, 4);
            vm = vl < vm ? vl : vm;
        }
        double cap = vm * vm;
        int k = 1;
        if (lim.curv && i > 0 && i < n - 1) {
            const double ux = (double)p[0] - (double)p[-3], uy = (double)p[1] - (double)p[-2], uz = (double)p[2] - (double)p[-1];
            const double vx = (double)p[3] - (double)p[0], vy = (double)p[4] - (double)p[1], vz = (double)p[5] - (double)p[2];
            const double wx = (double)p[3] - (double)p[-3], wy = (double)p[4] - (double)p[-2], wz = (double)p[5] - (double)p[-1];
            const double c = rt_norm(uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx);
            const double den = (rt_norm(ux, uy, uz) * rt_norm(vx, vy, vz)) * rt_norm(wx, wy, wz);
            if (c > 0.0 && den > 0.0) {
                const double k2 = __ddiv_rn(lim.a_lat, __ddiv_rn(2.0 * c, den));
                if (k2 < cap) { cap = k2; k = 2; }
            }
        }
        if (F.d2) {
            bool out = false;
            int64_t id;
            field_voxel(F, p[0], p[1], p[2], &id, &out);
            outs = out ? 1 : 0;
            if (lim.near_d2 >= 0 && F.d2[id] <= lim.near_d2) {
                const double k3 = lim.v_near * lim.v_near;
                if (k3 < cap) { cap = k3; k = 3; }
            }
        }
        if (!KEYS && (i == 0 || i == n - 1)) { cap = 0.0; k = 0; }
        if (STOPS && ((i > 0 && dq[i - 1] >= 0) || (i < n - 1 && dq[i] >= 0))) { cap = 0.0; k = 0; }
        const double q = cap * WA_RT_Q;
        const long long cq = !(q < (double)WA_RT_CAP) ? WA_RT_CAP : (long long)floor(q);
        if (KEYS) {
            C[i] = (long long)((unsigned long long)cq * 4ull + (unsigned long long)k);
        } else {
            C[i] = cq;
            kind[i] = (uint8_t)k;
        }
    }
    outs = rt_wave_sum(outs);
    if ((threadIdx.x & 63) == 0 && outs) atomicAdd(&rec->n_outside, outs);
}
__global__ __launch_bounds__(256) void k_rt_caps(const float *__restrict__ xyz, long long n, WaRtLimits lim, const float *__restrict__ v_limit,
                                                 WaField F, long long *__restrict__ C, uint8_t *__restrict__ kind,
                                                 WaRtRec *__restrict__ rec)
{
    rt_caps<false>(xyz, n, lim, v_limit, F, C, kind, rec, nullptr);
}

// ---- the scan's sources (k_scan, scan_kernels.hpp: a source hands out element e = 0 .. n - 1 and takes its result).
// Samples: element e is sample e (rev: sample n - 1 - e); its weight is that of the segment towards element e + 1 (0 behind the last
// one), its cap c[sample].  With c == nullptr the minimum is not used and the result is the exclusive sum; otherwise it is
// min_{j <= e} (c_j - S_j) + S_e with S the exclusive sums: F of rule 3 going forward, B going backward on F.
struct RtSamples {
    typedef RtMinSum Op;
    const long long *w, *c;
    long long *out;
    long long n;
    int32_t rev;
    __device__ __forceinline__ RtPair load(long long e) const
    {
        RtPair v;
        v.s = e < n - 1 ? w[rev ? n - 2 - e : e] : 0;
        v.m = c ? c[rev ? n - 1 - e : e] : WA_RT_INF;
        return v;
    }
    __device__ __forceinline__ void store(long long e, RtPair excl, RtPair v) const
    {
        out[rev ? n - 1 - e : e] = c ? rt_comb(excl, v).m + excl.s : excl.s;
    }
};

__device__ __forceinline__ double rt_speed(long long b) { return __dsqrt_rn((double)b / WA_RT_Q); }

// Rules 4 and 5 and the summary.  T gets n entries, entry n - 1 is 0.  STOPS: a stop segment takes its dwell dq_i as T_i; one that has
// a length is reported in rec->bad.
template <bool STOPS>
__device__ __forceinline__ void rt_times(const float *__restrict__ xyz, long long n, double acc, double dec,
                                         const long long *__restrict__ A, const long long *__restrict__ D,
                                         const long long *__restrict__ C, const long long *__restrict__ B,
                                         const uint8_t *__restrict__ kind, uint8_t *__restrict__ bound, long long *__restrict__ T,
                                         WaRtRec *__restrict__ rec, const long long *__restrict__ dq)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long t = 0, b = 0;
    int k = -1;
    bool on_cap = false, on_ramp = false, tri = false;
    if (i < n) {
        b = B[i];
        k = kind[i];
        on_cap = b == C[i];
        const bool up = i > 0 && b - B[i - 1] == A[i - 1];
        long long bn = 0;
        bool down = false;
        if (i < n - 1) {
            bn = B[i + 1];
            down = b - bn == D[i];
        }
        on_ramp = up || down;
        bound[i] = (uint8_t)((on_cap ? 1 : 0) | (up ? 2 : 0) | (down ? 4 : 0) | (k << 4));
        if (i < n - 1) {
            const double ds = rt_seg_len(xyz, i);
            if (rt_quanta(ds) > 0) {
                const double vs = rt_speed(b) + rt_speed(bn);
                double dt;
                if (vs == 0.0) {
                    tri = true;
                    const double wp = __ddiv_rn(((2.0 * ds) * acc) * dec, acc + dec), r = __dsqrt_rn(wp);
                    dt = __ddiv_rn(r, acc) + __ddiv_rn(r, dec);
                } else {
                    dt = __ddiv_rn(2.0 * ds, vs);
                }
                t = rt_quanta(dt);
                if (t >= WA_RT_CAP) atomicOr(&rec->bad, 2);
                if (STOPS && dq[i] >= 0) atomicOr(&rec->bad, 8);
            } else if (STOPS && dq[i] >= 0) {
                t = dq[i];
            }
        }
        T[i] = t;
    }
    const unsigned long long st = rt_wave_sat_sum((unsigned long long)t);
    const unsigned long long m0 = __ballot(k == 0), m1 = __ballot(k == 1), m2 = __ballot(k == 2), m3 = __ballot(k == 3);
    const unsigned long long mc = __ballot(on_cap), mr = __ballot(on_ramp), mt = __ballot(tri);
    long long pk = b;
    for (int o = 32; o > 0; o >>= 1) {
        const long long p2 = __shfl_down(pk, o, 64);
        pk = p2 > pk ? p2 : pk;
    }
    if ((threadIdx.x & 63) == 0) {
        rt_acc_split(rec->sumT, st);
        if (m0) atomicAdd(&rec->n_bound[0], (unsigned long long)__popcll(m0));
        if (m1) atomicAdd(&rec->n_bound[1], (unsigned long long)__popcll(m1));
        if (m2) atomicAdd(&rec->n_bound[2], (unsigned long long)__popcll(m2));
        if (m3) atomicAdd(&rec->n_bound[3], (unsigned long long)__popcll(m3));
        if (mc) atomicAdd(&rec->n_on_cap, (unsigned long long)__popcll(mc));
        if (mr) atomicAdd(&rec->n_on_ramp, (unsigned long long)__popcll(mr));
        if (mt) atomicAdd(&rec->n_triangle, (unsigned long long)__popcll(mt));
        if (pk > 0) atomicMax(&rec->peak, pk);
    }
}
__global__ __launch_bounds__(256) void k_rt_times(const float *__restrict__ xyz, long long n, double acc, double dec,
                                                  const long long *__restrict__ A, const long long *__restrict__ D,
                                                  const long long *__restrict__ C, const long long *__restrict__ B,
                                                  const uint8_t *__restrict__ kind, uint8_t *__restrict__ bound, long long *__restrict__ T,
                                                  WaRtRec *__restrict__ rec)
{
    rt_times<false>(xyz, n, acc, dec, A, D, C, B, kind, bound, T, rec, nullptr);
}

// Rule 6 for one tau: the segment i (the largest index in [lo, hi] with time_q[i] <= tau; the caller brackets it, [0, n - 2] always
// does), lambda on it, and the two cases in which the output is a sample as it stands.  Shared by k_rt_ticks and the tick-axis
// kernel (ticks_kernels.hpp): one definition of where a tick lies.
struct RtTick {
    long long i;
    double lam;      // 0 in the exact cases
    int32_t exact;   // 0: interpolate with lam; 1: the tick is p_(i+1) (lambda = 1); 2: it is p_i (lambda = 0)
};
__device__ __forceinline__ RtTick rt_tick_locate(const float *__restrict__ xyz, double acc, double dec, const long long *__restrict__ B,
                                                 const long long *__restrict__ time_q, long long tau, long long lo, long long hi)
{
    while (lo < hi) {
        const long long mid = lo + ((hi - lo + 1) >> 1);
        if (time_q[mid] <= tau) lo = mid; else hi = mid - 1;
    }
    RtTick r;
    r.i = lo;
    r.lam = 0.0;
    r.exact = 0;
    const long long i = lo;
    const double ds = rt_seg_len(xyz, i);
    if (tau >= time_q[i + 1]) {
        r.exact = 1;
    } else if (rt_quanta(ds) == 0) {
        r.exact = 2;
    } else {
        const double e = (double)(tau - time_q[i]) / WA_RT_Q;
        const long long bi = B[i], bn = B[i + 1];
        const double vi = rt_speed(bi), vs = vi + rt_speed(bn);
        double s;
        if (vs == 0.0) {
            const double wp = __ddiv_rn(((2.0 * ds) * acc) * dec, acc + dec), rr = __dsqrt_rn(wp);
            const double t_up = __ddiv_rn(rr, acc), dt = t_up + __ddiv_rn(rr, dec);
            if (e <= t_up) {
                s = ((0.5 * acc) * e) * e;
            } else {
                const double rem = dt - e;
                s = ds - ((0.5 * dec) * rem) * rem;
            }
        } else {
            const double al = __ddiv_rn((double)(bn - bi) / WA_RT_Q, 2.0 * ds);
            s = (vi * e) + ((0.5 * al) * e) * e;
        }
        double lam = __ddiv_rn(s, ds);
        r.lam = lam < 0.0 ? 0.0 : (lam > 1.0 ? 1.0 : lam);
    }
    return r;
}
// the position of a located tick, component c
__device__ __forceinline__ float rt_tick_pos(const float *__restrict__ xyz, const RtTick &r, int c)
{
    const float *a = xyz + 3 * r.i, *b = a + 3;
    if (r.exact) return r.exact == 1 ? b[c] : a[c];
    const double pa = (double)a[c], pb = (double)b[c];
    return (float)(pa + (pb - pa) * r.lam);
}

// Rule 6.  Tick k < n_full sits at k * tick_q, tick n_full (when the duration is no multiple of tick_q) at the duration.  The block's
// 256 positions go through LDS so that consecutive lanes store consecutive floats.
__global__ __launch_bounds__(256) void k_rt_ticks(const float *__restrict__ xyz, long long n, double acc, double dec,
                                                  const long long *__restrict__ B, const long long *__restrict__ time_q, long long tick_q,
                                                  long long n_full, long long n_ticks, float *__restrict__ out)
{
    __shared__ float stage[256 * 3];
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_ticks) {
        const long long tau = k < n_full ? k * tick_q : time_q[n - 1];
        const RtTick r = rt_tick_locate(xyz, acc, dec, B, time_q, tau, 0, n - 2);
        for (int c = 0; c < 3; c++) stage[3 * threadIdx.x + c] = rt_tick_pos(xyz, r, c);
    }
    __syncthreads();
    const long long first = (long long)blockIdx.x * blockDim.x * 3, end = n_ticks * 3;
    for (int q = threadIdx.x; q < 256 * 3; q += 256)
        if (first + q < end) out[first + q] = stage[q];
}
