// fit_kernels.hpp -- device side of wa_grid_fit_trajectory: a B-spline whose control points lie ON a collision-free polyline, refined
// leg by leg until its samples clear the grid (include/weldacs.h states the definition; tests/fit_ref.py restates it in numpy).
//   k_fit_pieces     one lane per leg: its float64 length, its piece count m_k at the leg's level, the block's share of the scan
//   k_fit_scan_sums  the block sums scanned by one workgroup; the total goes into the round's record
//   k_fit_scan_add   block offsets added: off[k] = m_0 + ... + m_{k-1}, off[n_legs] = the total
//   k_fit_emit       one lane per point of the control polygon, written straight into the spline's control array, with its owner leg
//   k_fit_knots      the knot vector of a chain whose step is exactly 1.0f: knot i is the integer i - D, clamped at both ends
//   k_fit_ends       one lane: the end rows (positions, zero derivatives), the constrained control points, the record's reset
//   k_fit_blame      one lane per hit segment: the legs that own a control point with a non-zero basis at either sample
//   k_fit_bump       one lane per leg: blamed legs below the cap rise by one level; what changed and what stayed at the cap
// Sampling and checking are k_bspline_eval, k_clr_samples and k_clr_segments as every other caller runs them.
// Integers and single correctly rounded fp32 / fp64 operations throughout: every output is bit-exact and independent of scheduling.
#pragma once
#include "clearance_kernels.hpp"
#include "traj_kernels.hpp"

#define WA_FIT_MAX_CPS (1ll << 24)   // knots are integers held in fp32: exact up to 2^24
#define WA_FIT_MAX_LEVEL 8
#define WA_FIT_MAX_ROUNDS 32

// what the host reads once per round
struct WaFitRec {
    unsigned long long acc[4];   // k_clr_samples / k_clr_segments: min key, first hit, n_hit, n_outside
    long long total;             // m_0 + ... + m_{n_legs-1} at the levels behind k_fit_bump: the NEXT fit's pieces
    int32_t changed;             // legs k_fit_bump raised
    int32_t at_cap;              // blamed legs it found at max_level
    int32_t bad;                 // a coordinate of the polyline is not finite
    int32_t pad;
};

__device__ __forceinline__ long long fit_wave_scan(long long v, int lane)   // inclusive, over the 64 lanes
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// len_k: float64 on the fp32 coordinates, (dx*dx + dy*dy) + dz*dz, every operation rounded on its own (wa_grid_path_shortcut's length);
// m_k = max(1, ceil((len_k * 2^s_k) / spacing)), capped at 2^24 + 1 (such a request is refused: the sum exceeds what a fit may hold).
// off[k] = the exclusive scan of m within the block, bsum[block] = the block's sum.
__global__ __launch_bounds__(256) void k_fit_pieces(const float *__restrict__ xyz, long long n_legs, const int32_t *__restrict__ level,
                                                    double spacing, long long *__restrict__ off, long long *__restrict__ bsum,
                                                    WaFitRec *__restrict__ rec)
{
    __shared__ long long wsum[4];
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long m = 0;
    if (k < n_legs) {
        const float *a = xyz + 3 * k, *b = a + 3;
        bool finite = true;
        for (int c = 0; c < 6; c++) finite = finite && isfinite(a[c]);
        if (!finite) rec->bad = 1;   // (every writer stores the same value)
        const double dx = __dsub_rn((double)b[0], (double)a[0]), dy = __dsub_rn((double)b[1], (double)a[1]),
                     dz = __dsub_rn((double)b[2], (double)a[2]);
        const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
        const double q = ceil(__ddiv_rn(__dmul_rn(len, (double)(1 << level[k])), spacing));
        m = !(q >= 1.0) ? 1 : (q > (double)WA_FIT_MAX_CPS ? WA_FIT_MAX_CPS + 1 : (long long)q);
    }
    const long long incl = fit_wave_scan(m, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long long before = 0;
    for (int w = 0; w < wave; w++) before += wsum[w];
    if (k < n_legs) off[k] = before + incl - m;
    if (threadIdx.x == 255) bsum[blockIdx.x] = before + incl;
}

// one workgroup: bsum[] -> its exclusive scan in place, the total into the record
__global__ __launch_bounds__(256) void k_fit_scan_sums(long long *__restrict__ bsum, long long n_blocks, WaFitRec *__restrict__ rec)
{
    __shared__ long long wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long long base = 0; base < n_blocks; base += 256) {
        const long long i = base + threadIdx.x;
        const long long v = i < n_blocks ? bsum[i] : 0;
        const long long incl = fit_wave_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = carry;
        for (int w = 0; w < wave; w++) before += wsum[w];
        if (i < n_blocks) bsum[i] = before + incl - v;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) rec->total = carry;
}

__global__ __launch_bounds__(256) void k_fit_scan_add(long long *__restrict__ off, long long n_legs, const long long *__restrict__ bsum,
                                                      const WaFitRec *__restrict__ rec)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_legs) off[k] += bsum[blockIdx.x];
    if (k == n_legs) off[k] = rec->total;   // (the launch covers n_legs + 1 lanes)
}

// the leg of polygon point c < off[n_legs]: the largest k in [lo, hi] with off[k] <= c (m_k >= 1: off increases strictly)
__device__ __forceinline__ long long fit_leg_of(const long long *__restrict__ off, long long lo, long long hi, long long c)
{
    while (lo < hi) {
        const long long mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Polygon point c: leg k contributes j = 0 .. m_k - 1 at a + (b - a) * ((float)j / (float)m_k) per axis (fp32, each operation rounded on its
// own); the point behind the last leg is the polyline's last point.  Point 0 is the spline's initial position (control point 0), the
// last one its final position (control point n_cps - 1), point c between them is middle point c - 1 = control point D + c - 1.
// The wave's first and last points are looked up by all lanes together (the same addresses: one request each); a lane then searches
// only the legs between those two.
__global__ __launch_bounds__(256) void k_fit_emit(const float *__restrict__ xyz, long long n_legs, const long long *__restrict__ off,
                                                  WaSpline S, int32_t *__restrict__ owner)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = S.n_middle + 1;   // polygon points 0 .. total
    const long long w0 = c - (threadIdx.x & 63), w1 = w0 + 63 < total - 1 ? w0 + 63 : total - 1;
    if (w0 > total) return;                   // (whole waves)
    long long klo = 0, khi = n_legs - 1;
    if (w0 < total) {
        klo = fit_leg_of(off, 0, n_legs - 1, w0);
        khi = fit_leg_of(off, klo, n_legs - 1, w1);
    }
    if (c > total) return;
    float p[3];
    long long k;
    if (c == total) {
        k = n_legs - 1;
        for (int q = 0; q < 3; q++) p[q] = xyz[3 * n_legs + q];
    } else {
        k = fit_leg_of(off, klo, khi, c);
        const float t = __fdiv_rn((float)(c - off[k]), (float)(off[k + 1] - off[k]));
        const float *a = xyz + 3 * k, *b = a + 3;
        for (int q = 0; q < 3; q++) p[q] = __fadd_rn(a[q], __fmul_rn(__fsub_rn(b[q], a[q]), t));
    }
    const long long cp = c == 0 ? 0 : (c == total ? S.n_cps - 1 : S.degree + c - 1);
    for (int q = 0; q < 3; q++) S.cps[3 * cp + q] = p[q];
    owner[cp] = (int32_t)k;
}

// k_bspline_setup's chain K[i] = K[i-1] + step with step == 1.0f exactly adds 1 to an integer below 2^24 every time: no rounding, the
// chain IS i - D.  D + 1 zeros in front, D + 1 times fin_time behind (_CalcKnot, BSplineBasic.h:150-171).
__global__ __launch_bounds__(256) void k_fit_knots(WaSpline S, float fin_time)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n_knots) return;
    const int D = S.degree;
    S.knots[i] = i <= D ? 0.0f : (i >= S.n_knots - D - 1 ? fin_time : (float)(i - D));
}

// one lane, behind k_fit_knots and k_fit_emit: the end rows (position, then zero derivatives) for _CalcConstrainedCPoints, the
// owners of the constrained control points (the first / the last leg), and the record's per-round fields back to their start values
__global__ void k_fit_ends(const float *__restrict__ xyz, long long n_legs, WaSpline S, float *__restrict__ ends, float fin_time,
                           int32_t *__restrict__ owner, WaFitRec *__restrict__ rec)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int D = S.degree;
    float *init = ends, *fin = ends + 3 * D;
    for (int q = 0; q < 3 * D; q++) init[q] = fin[q] = 0.0f;
    for (int q = 0; q < 3; q++) {
        init[q] = xyz[q];
        fin[q] = xyz[3 * n_legs + q];
    }
    __threadfence();
    wa_bs_constrained_cps(S, init, fin, fin_time);
    for (int j = 1; j < D; j++) {
        owner[j] = 0;
        owner[S.n_cps - 1 - j] = (int32_t)(n_legs - 1);
    }
    clr_acc_init(rec->acc);
    rec->changed = 0;
    rec->at_cap = 0;
}

// Segment i = samples i, i + 1 at u = (float)i * dt.  Where it hit: the knot span of each of the two samples as the evaluation found
// it (u clamped into the knot range, _findSpan); the control points with a non-zero basis there are span - D .. span; the leg that
// owns one is marked.  Every writer stores 1.
template <int DEG>
__global__ __launch_bounds__(256) void k_fit_blame(WaSpline S, const uint8_t *__restrict__ hit, long long n_seg, float dt,
                                                   const int32_t *__restrict__ owner, uint8_t *__restrict__ mark)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seg || !hit[i]) return;
    const float *K = S.knots;
    const float lastk = K[S.n_knots - 1];
    for (int e = 0; e < 2; e++) {
        float u = 0.0f + (float)(i + e) * dt;
        if (u < K[0]) u = K[0];
        else if (u > lastk) u = lastk;
        long long span = 0;
        if (!wa_bs_find_span(K, S.n_knots, u, &span) || span - DEG < 0 || span >= S.n_cps) continue;
        for (int q = 0; q <= DEG; q++) mark[owner[span - DEG + q]] = 1;
    }
}

// Marked legs below max_level rise by one (apply == 0, the last round allowed: they stay); marks are cleared for the next round.
// One integer atomic per wave and counter: sums of integers, the same in any order.
__global__ __launch_bounds__(256) void k_fit_bump(int32_t *__restrict__ level, uint8_t *__restrict__ mark, long long n_legs, int32_t max_level,
                                                  int32_t apply, WaFitRec *__restrict__ rec)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool rise = false, cap = false;
    if (k < n_legs && mark[k]) {
        mark[k] = 0;
        const int32_t s = level[k];
        rise = s < max_level;
        cap = !rise;
        if (rise && apply) level[k] = s + 1;
    }
    const unsigned long long mr = __ballot(rise && apply), mc = __ballot(cap);
    if ((threadIdx.x & 63) == 0) {
        if (mr) atomicAdd(&rec->changed, (int32_t)__popcll(mr));
        if (mc) atomicAdd(&rec->at_cap, (int32_t)__popcll(mc));
    }
}
