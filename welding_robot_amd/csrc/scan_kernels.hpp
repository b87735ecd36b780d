// scan_kernels.hpp -- the one device-wide prefix scan of the trajectory stages (retime, stops, jerk, ticks).
//   k_scan   reduce (tile aggregates) - scan (of the aggregates, recursively) - add (tile prefixes), with kernel boundaries in between: no
//            workgroup waits for another.
// A source hands out element e = 0 .. n - 1 (load) and takes its result (store: the exclusive prefix and the element itself); it names
// its operator as SRC::Op:  T the element,  id() the neutral element,  comb(a, b) with a the lower index,  up(v, o) = __shfl_up of v.
// The operators are associative over integers, so a result does not depend on the tiling.
#pragma once
#include <hip/hip_runtime.h>

#define WA_SCAN_ITEMS 8
#define WA_SCAN_TILE (256 * WA_SCAN_ITEMS)   // elements per workgroup of k_scan

// Tile aggregates of a level below: scanned in place into their exclusive prefixes.
template <class OP>
struct ScanAggs {
    typedef OP Op;
    typename OP::T *p;
    long long n;
    __device__ __forceinline__ typename OP::T load(long long e) const { return p[e]; }
    __device__ __forceinline__ void store(long long e, typename OP::T excl, typename OP::T) const { p[e] = excl; }
};

// One workgroup per tile of 2 048 elements, a lane takes 8 consecutive ones.  WRITE == false: the tile's aggregate into agg[block].
// WRITE == true: every element's result, behind prefix[block] (nullptr: a lone tile).  An operator need not be commutative: the lower
// index is always the left operand.
template <class SRC, bool WRITE>
__global__ __launch_bounds__(256) void k_scan(SRC src, const typename SRC::Op::T *__restrict__ prefix, typename SRC::Op::T *__restrict__ agg)
{
    typedef typename SRC::Op Op;
    typedef typename Op::T T;
    __shared__ T wtot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * WA_SCAN_TILE + (long long)threadIdx.x * WA_SCAN_ITEMS;
    const T id = Op::id();
    T v[WA_SCAN_ITEMS], t = id;
#pragma unroll
    for (int k = 0; k < WA_SCAN_ITEMS; k++) {
        v[k] = base + k < src.n ? src.load(base + k) : id;
        t = Op::comb(t, v[k]);
    }
    T inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = Op::up(inc, o);
        if (lane >= o) inc = Op::comb(u, inc);
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    T before = id;
    for (int w = 0; w < wave; w++) before = Op::comb(before, wtot[w]);
    if (!WRITE) {
        if (threadIdx.x == 255) agg[blockIdx.x] = Op::comb(before, inc);
        return;
    }
    T prev = Op::up(inc, 1);
    if (lane == 0) prev = id;
    T run = Op::comb(before, prev);
    if (prefix) run = Op::comb(prefix[blockIdx.x], run);
#pragma unroll
    for (int k = 0; k < WA_SCAN_ITEMS; k++) {
        if (base + k < src.n) src.store(base + k, run, v[k]);
        run = Op::comb(run, v[k]);
    }
}

// the elements of scratch a scan of n elements needs: the aggregates of every level above the first
static long long wa_scan_scratch(long long n)
{
    long long total = 0;
    for (long long m = (n + WA_SCAN_TILE - 1) / WA_SCAN_TILE; m > 1; m = (m + WA_SCAN_TILE - 1) / WA_SCAN_TILE) total += m;
    return total + 1;
}

// host side: the tiles' aggregates, their exclusive prefixes (by this very function when they exceed one tile), the results
template <class SRC>
static hipError_t wa_scan(hipStream_t st, SRC src, typename SRC::Op::T *scratch)
{
    const long long blocks = (src.n + WA_SCAN_TILE - 1) / WA_SCAN_TILE;
    if (blocks <= 1) {
        k_scan<SRC, true><<<1, 256, 0, st>>>(src, nullptr, nullptr);
        return hipGetLastError();
    }
    k_scan<SRC, false><<<(unsigned)blocks, 256, 0, st>>>(src, nullptr, scratch);
    hipError_t e = hipGetLastError();
    const ScanAggs<typename SRC::Op> up = {scratch, blocks};
    e = e ? e : wa_scan(st, up, scratch + blocks);
    if (e != hipSuccess) return e;
    k_scan<SRC, true><<<(unsigned)blocks, 256, 0, st>>>(src, scratch, nullptr);
    return hipGetLastError();
}
