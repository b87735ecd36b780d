// shortcut_kernels.hpp -- device side of wa_grid_path_shortcut: greedy line-of-sight shortening of a batch of planned paths.
// Visibility is clr_cover_hits (clearance_kernels.hpp), the segment test of wa_traj_clearance; lengths are float64 without contraction.
#pragma once
#include "wa_device.h"
#include "clearance_kernels.hpp"

// the last node of the path holding node i: the path is the last p with off[p] <= i (empty paths share their offset with the next
// path, so they are skipped)
__device__ __forceinline__ int64_t sc_last_node(const long long *__restrict__ off, int32_t n_paths, int64_t i)
{
    int32_t lo = 0, hi = n_paths - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return off[lo + 1] - 1;
}

// Reach pass: one wavefront per node i of the batch (global index; the anchor).  Lane l tests candidate k = i + 1 + l of a chunk of
// 64; the first candidate whose supercover from the anchor meets an occupied voxel is the lowest set bit of the chunk's ballot, and
// the next chunk is tested only while the whole chunk was visible and the span cap is not reached.  Writes step[i] = next(i) - i
// (>= 1: an anchor that sees nothing steps to its neighbour); the last node of a path has no step and is not written.
// off: n_paths + 1 non-decreasing offsets, off[n_paths] = n_nodes (checked by the host).
__global__ __launch_bounds__(256) void k_sc_reach(const long long *__restrict__ ids, const long long *__restrict__ off, int32_t n_paths,
                                                  int64_t n_nodes, int32_t max_span, WaDims d, const uint8_t *__restrict__ free_,
                                                  int32_t *__restrict__ step)
{
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_nodes) return;   // (whole waves)
    const int64_t last = sc_last_node(off, n_paths, i);
    if (i >= last) return;
    const int64_t top = min(i + (int64_t)max_span, last);
    const long long va = ids[i];
    int64_t j = top;   // the farthest candidate such that every candidate up to it is visible
    for (int64_t c0 = i + 1; c0 <= top; c0 += 64) {
        const int64_t k = c0 + lane;
        const unsigned long long m = __ballot(k <= top && clr_cover_hits(va, ids[k], d, free_));
        if (m) {
            j = c0 + __builtin_ctzll(m) - 1;
            break;
        }
    }
    if (lane == 0) step[i] = (int32_t)(j > i ? j - i : 1);
}

// The chain of one path (nodes ids[b .. b + L), L >= 1): follows the steps from node 0 to node L-1, writes the waypoints (indices into
// the path) from wp[b] on and sums the straight lengths between consecutive waypoints in float64 on the fp32 axis-table coordinates,
// in waypoint order, every operation rounded on its own (__d*_rn: no contraction whatever the flags).  seg(t, a) is called for the
// segment that leaves waypoint t at node a, in order.  Returns the number of waypoints.  Shared by k_sc_chain and k_psc_chain
// (pose_shortcut_kernels.hpp): one definition of the waypoints and of the length.
template <class Seg>
__device__ __forceinline__ int32_t sc_chain_path(const long long *__restrict__ ids, int64_t b, int64_t L, const int32_t *__restrict__ step,
                                                 WaDims d, const float *__restrict__ cx, const float *__restrict__ cy,
                                                 const float *__restrict__ cz, long long *__restrict__ wp, double *total_out, Seg &&seg)
{
    long long v = ids[b];
    double px = cx[v % d.nx], py = cy[(v / d.nx) % d.ny], pz = cz[v / d.nxy];
    double total = 0.0;
    int64_t a = 0;
    int32_t cnt = 0;
    wp[b + cnt++] = 0;
    while (a < L - 1) {
        seg(cnt - 1, a);
        a += step[b + a];
        v = ids[b + a];
        const double qx = cx[v % d.nx], qy = cy[(v / d.nx) % d.ny], qz = cz[v / d.nxy];
        const double dx = __dsub_rn(qx, px), dy = __dsub_rn(qy, py), dz = __dsub_rn(qz, pz);
        const double s2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        total = __dadd_rn(total, __dsqrt_rn(s2));
        wp[b + cnt++] = a;
        px = qx; py = qy; pz = qz;
    }
    *total_out = total;
    return cnt;
}

// Chain pass: one lane per path (sc_chain_path); an empty path has no waypoint and length 0.
__global__ __launch_bounds__(256) void k_sc_chain(const long long *__restrict__ ids, const long long *__restrict__ off, int32_t n_paths,
                                                  const int32_t *__restrict__ step, WaDims d, const float *__restrict__ cx,
                                                  const float *__restrict__ cy, const float *__restrict__ cz, long long *__restrict__ wp,
                                                  int32_t *__restrict__ count, double *__restrict__ length)
{
    const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n_paths) return;
    const int64_t b = off[p], L = off[p + 1] - b;
    if (L == 0) {
        count[p] = 0;
        length[p] = 0.0;
        return;
    }
    double total;
    count[p] = sc_chain_path(ids, b, L, step, d, cx, cy, cz, wp, &total, [](int32_t, int64_t) {});
    length[p] = total;
}
