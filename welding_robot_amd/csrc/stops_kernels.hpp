// stops_kernels.hpp -- device side of the weld passes in a timed trajectory (wa_traj_retime_stops, wa_traj_tick_axes_stops,
// wa_traj_axes_dwells; include/weldacs.h rules 40 - 42 hold the definition, DESIGN 4y the reasoning, tests/stops_ref.py restates it in
// numpy).  A stop is a segment without length that has a duration; the algorithm of the retime section carries it as it stands: a cap
// of 0 inside the trajectory resets the prefix and the suffix minimum of rule 3, so the scans (k_scan, scan_kernels.hpp), k_rt_segments
// and k_rt_ticks are reused.
//   k_st_caps        k_rt_caps with the kind-0 cap on both samples of a stop (rt_caps<true>)
//   k_st_times       k_rt_times with T_i = dq_i on a stop; a stop that has a length goes into the record (rt_times<true>)
//   k_tk_axes_stops  k_tk_axes with the turn in place during a dwell, a tag per tick and the dwell counters (tk_axes<true>)
//   k_ax_dwells      rule 42, one lane per segment: the dwell a change of direction on a segment without length needs
// Integers and single correctly rounded fp64 operations throughout, as in the files this one builds on.
#pragma once
#include "ticks_kernels.hpp"

__global__ __launch_bounds__(256) void k_st_caps(const float *__restrict__ xyz, long long n, WaRtLimits lim, const float *__restrict__ v_limit,
                                                 WaField F, const long long *__restrict__ dq, long long *__restrict__ C,
                                                 uint8_t *__restrict__ kind, WaRtRec *__restrict__ rec)
{
    rt_caps<true>(xyz, n, lim, v_limit, F, C, kind, rec, dq);
}

__global__ __launch_bounds__(256) void k_st_times(const float *__restrict__ xyz, long long n, double acc, double dec,
                                                  const long long *__restrict__ A, const long long *__restrict__ D,
                                                  const long long *__restrict__ C, const long long *__restrict__ B,
                                                  const uint8_t *__restrict__ kind, const long long *__restrict__ dq,
                                                  uint8_t *__restrict__ bound, long long *__restrict__ T, WaRtRec *__restrict__ rec)
{
    rt_times<true>(xyz, n, acc, dec, A, D, C, B, kind, bound, T, rec, dq);
}

__global__ __launch_bounds__(256) void k_tk_axes_stops(WaTkArgs T, WaField F, const WaTorchTool *__restrict__ tool, WaAxRec *__restrict__ rec,
                                                       WaTkStops S)
{
    tk_axes<true>(T, F, tool, rec, S);
}

// ---- rule 42
struct WaDwRec {
    unsigned long long n_jump, n_stops, n_raised;
    unsigned long long max_need_bits;   // the bits of a double >= 0 order like the double
    unsigned int bad;                   // bit 0: a coordinate is not finite; bit 3: a dwell given on a segment that has a length
    unsigned int pad;
};

__global__ __launch_bounds__(256) void k_ax_dwells(const float *__restrict__ xyz, const short4 *__restrict__ q, long long n, double omega,
                                                   const double *__restrict__ dwell_in, double *__restrict__ dwell_out,
                                                   WaDwRec *__restrict__ rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool jump = false, stop = false, raised = false;
    unsigned long long nb = 0;
    if (i < n) {
        bool finite = true;
        for (int c = 0; c < 3; c++) finite = finite && isfinite(xyz[3 * i + c]);
        if (!finite) atomicOr(&rec->bad, 1u);
    }
    if (i < n - 1) {
        const double given = dwell_in ? dwell_in[i] : -1.0;
        const uint32_t D = ax_chord2(q[i], q[i + 1]);
        double out = -1.0;
        if (rt_quanta(rt_seg_len(xyz, i)) > 0) {
            if (given >= 0.0) atomicOr(&rec->bad, 8u);
        } else if (!D) {
            out = given >= 0.0 ? given : -1.0;
        } else {
            jump = true;
            const double need = __ddiv_rn(__dsqrt_rn((double)D) / 16384.0, omega);
            raised = given < need;
            out = raised ? need : given;
            nb = (unsigned long long)__double_as_longlong(need);
        }
        stop = out >= 0.0;
        dwell_out[i] = out;
    }
    const unsigned long long mj = __ballot(jump), ms = __ballot(stop), mr = __ballot(raised);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long b = __shfl_down(nb, o, 64);
        nb = b > nb ? b : nb;
    }
    if ((threadIdx.x & 63) == 0) {
        if (mj) atomicAdd(&rec->n_jump, (unsigned long long)__popcll(mj));
        if (ms) atomicAdd(&rec->n_stops, (unsigned long long)__popcll(ms));
        if (mr) atomicAdd(&rec->n_raised, (unsigned long long)__popcll(mr));
        if (nb) atomicMax(&rec->max_need_bits, nb);
    }
}
