// reach_kernels.hpp -- device side of the torch-fit planning grids (wa_grid_tool_reach, wa_grid_tool_fit, wa_grid_tool_penalties;
// include/weldacs.h holds the definition, DESIGN 4s the reasoning).  Integers throughout: every output is bit-exact and independent
// of scheduling.
//   k_reach            rule 2 of the torch section for EVERY voxel of a grid: open-direction masks, counts and the summary
//   k_reach_fit        the occupancy of the torch-fit grid from the counts (elementwise)
//   k_reach_keep       its keep bubbles (one workgroup per keep id)
//   k_reach_penalties  the penalty array from the counts (elementwise)
#pragma once
#include "torch_kernels.hpp"

#define WA_REACH_GROUP 4      // beads loaded together before the next exit test
#define WA_REACH_LDS_HEAD 272   // bytes of dynamic LDS in front of the offsets: 64 thresholds, then one flag word per wavefront

struct WaReachTool {
    int32_t n_beads;
    int32_t dist16[64];
    uint32_t r2[64];
};

struct WaReachThr {
    int32_t n;
    int32_t thr[32];
};

// A wavefront takes 64 consecutive x of one (y, z) row, the four wavefronts of a workgroup four neighbouring rows (row = z * ny + y),
// so that the bead rows they gather share cache lines of d2.  The offset of (direction, bead) is the same for every lane: the
// workgroup stages the K x n_beads offsets in LDS once, a wavefront reads one as a broadcast and moves it to scalar registers, the
// y and z bounds tests are scalar, and the load of one bead is one contiguous (unaligned) 256-byte segment of a row of d2.
// A lane is alive for a direction while its voxel is free and no bead has blocked it; beads are loaded WA_REACH_GROUP at a time and
// the bead loop of a direction ends at the first group after which no lane is alive.
// far2: a free voxel with d2 >= far2 has every direction open (DESIGN 4s has the proof) and is never alive; a workgroup without a
// near voxel does not even stage the offsets.  far2 = 2^32 - 1 turns the shortcut off (every free voxel is near).
// Dynamic LDS: WA_REACH_LDS_HEAD bytes, then K * n_beads * 8 bytes of offsets (at most 128 KiB + 272 B); no static LDS, so the
// workgroup's vote below is four ballots through the head rather than the library's reduction, which brings a static block.
__global__ __launch_bounds__(256) void k_reach(const uint8_t *__restrict__ free_, const int32_t *__restrict__ d2, WaDims d,
                                               const short4 *__restrict__ q, int32_t K, const WaReachTool *__restrict__ tool, uint32_t far2,
                                               int32_t nchunk, unsigned long long *__restrict__ mask /* W * n, or NULL */,
                                               uint16_t *__restrict__ count, unsigned long long *__restrict__ rec /* 4 */)
{
    extern __shared__ __align__(16) unsigned char reach_lds[];
    uint32_t *thr = (uint32_t *)reach_lds;
    int32_t *vote = (int32_t *)(reach_lds + 256);
    const int2 *offs = (const int2 *)(reach_lds + WA_REACH_LDS_HEAD);
    const int lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)d.ny * d.nz;
    const int64_t row = (int64_t)(blockIdx.x / (unsigned)nchunk) * 4 + (threadIdx.x >> 6);
    const int32_t x = (int32_t)(blockIdx.x % (unsigned)nchunk) * 64 + lane;
    const bool valid = row < rows && x < d.nx;   // (tail lanes and tail rows stay inactive)
    const int32_t y = (int32_t)(row % d.ny), z = (int32_t)(row / d.ny);   // uniform over the wavefront
    const int64_t v = row * d.nx + x;
    const bool isfree = valid && free_[v] != 0;
    const bool near = isfree && (uint32_t)d2[v] < far2;
    const int32_t nb = tool->n_beads;
    const int32_t W = (K + 63) >> 6;
    int32_t cnt = 0;
    const bool wave_near = __ballot(near) != 0;
    if (lane == 0) vote[threadIdx.x >> 6] = wave_near ? 1 : 0;
    __syncthreads();
    if (!(vote[0] | vote[1] | vote[2] | vote[3])) {
        // every voxel of the workgroup is occupied or far: no gather
        if (valid) {
            if (mask)
                for (int32_t w = 0; w < W; w++) {
                    const int32_t kend = min(64, K - w * 64);
                    mask[(int64_t)w * d.n + v] = isfree ? (kend == 64 ? ~0ull : ((1ull << kend) - 1)) : 0ull;
                }
            cnt = isfree ? K : 0;
        }
    } else {
        {
            short4 *st = (short4 *)(reach_lds + WA_REACH_LDS_HEAD);
            for (int32_t e = threadIdx.x; e < K * nb; e += 256) st[e] = torch_offset(q[e / nb], tool->dist16[e % nb]);   // direction-major
            if (threadIdx.x < 64) thr[threadIdx.x] = tool->r2[threadIdx.x];
        }
        __syncthreads();
        const bool gather = wave_near;   // (a wavefront of occupied and far voxels skips the loops)
        for (int32_t w = 0; w < W; w++) {
            const int32_t kend = min(64, K - w * 64);
            unsigned long long word = isfree ? (kend == 64 ? ~0ull : ((1ull << kend) - 1)) : 0ull;
            if (gather) {
                for (int32_t kk = 0; kk < kend; kk++) {
                    const int2 *ok = offs + (int64_t)(w * 64 + kk) * nb;
                    bool alive = near;
                    for (int32_t j0 = 0; j0 < nb && __ballot(alive) != 0; j0 += WA_REACH_GROUP) {
                        uint32_t val[WA_REACH_GROUP], lim[WA_REACH_GROUP];
#pragma unroll
                        for (int32_t u = 0; u < WA_REACH_GROUP; u++) {
                            const int32_t j = min(j0 + u, nb - 1);   // (the last group repeats its last bead)
                            const int2 o = ok[j];
                            const int32_t lo = __builtin_amdgcn_readfirstlane(o.x), hi = __builtin_amdgcn_readfirstlane(o.y);
                            const int32_t ox = (int32_t)(short)(lo & 0xffff), oy = lo >> 16, oz = (int32_t)(short)(hi & 0xffff);
                            const int32_t by = y + oy, bz = z + oz, bx = x + ox;
                            const bool rowin = (uint32_t)by < (uint32_t)d.ny && (uint32_t)bz < (uint32_t)d.nz;   // scalar
                            lim[u] = thr[j];
                            val[u] = 0xffffffffu;   // a bead outside the grid passes
                            if (rowin && alive && (uint32_t)bx < (uint32_t)d.nx) val[u] = (uint32_t)d2[((int64_t)bz * d.ny + by) * d.nx + bx];
                        }
#pragma unroll
                        for (int32_t u = 0; u < WA_REACH_GROUP; u++) alive = alive && val[u] > lim[u];
                    }
                    if (near && !alive) word &= ~(1ull << kk);
                }
            }
            if (valid) {
                if (mask) mask[(int64_t)w * d.n + v] = word;
                cnt += __popcll(word);
            }
        }
    }
    if (valid) count[v] = (uint16_t)cnt;
    // the summary: reduced over the wavefront, then one integer atomic per wavefront and counter
    const unsigned long long mf = __ballot(isfree), m0 = __ballot(isfree && cnt == 0), ma = __ballot(isfree && cnt == K);
    unsigned int closed = isfree ? (unsigned int)(K - cnt) : 0u;
    for (int o = 32; o > 0; o >>= 1) closed += __shfl_down(closed, o, 64);
    if (lane == 0) {
        if (mf) atomicAdd(&rec[0], (unsigned long long)__popcll(mf));
        if (m0) atomicAdd(&rec[1], (unsigned long long)__popcll(m0));
        if (ma) atomicAdd(&rec[2], (unsigned long long)__popcll(ma));
        if (closed) atomicAdd(&rec[3], (unsigned long long)closed);
    }
}

// wa_grid_tool_fit, part 1: free iff free in the source AND at least min_dirs directions are open
__global__ __launch_bounds__(256) void k_reach_fit(const uint8_t *__restrict__ free_, const uint16_t *__restrict__ count, int64_t n,
                                                   int32_t min_dirs, uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (free_[i] && (int32_t)count[i] >= min_dirs) ? 1 : 0;
}

// Part 2, after k_inflate_keep: one workgroup per keep id; every voxel v with |v - k|^2 <= keep_r2 (index units, integers) takes the
// source's state again.  Every writer copies the same source byte, so the result does not depend on the order of the workgroups.
__global__ __launch_bounds__(256) void k_reach_keep(const uint8_t *__restrict__ free_, WaDims d, const long long *__restrict__ keep, int32_t h,
                                                    int64_t keep_r2, uint8_t *__restrict__ out)
{
    const long long id = keep[blockIdx.x];
    const int32_t kx = (int32_t)(id % d.nx), ky = (int32_t)((id / d.nx) % d.ny), kz = (int32_t)(id / d.nxy);
    const int32_t x0 = max(kx - h, 0), x1 = min(kx + h, d.nx - 1);
    const int32_t y0 = max(ky - h, 0), y1 = min(ky + h, d.ny - 1);
    const int32_t z0 = max(kz - h, 0), z1 = min(kz + h, d.nz - 1);
    const int64_t wx = x1 - x0 + 1, wy = y1 - y0 + 1, box = wx * wy * (int64_t)(z1 - z0 + 1);
    for (int64_t p = threadIdx.x; p < box; p += blockDim.x) {
        const int32_t x = x0 + (int32_t)(p % wx), y = y0 + (int32_t)((p / wx) % wy), z = z0 + (int32_t)(p / (wx * wy));
        const int64_t dx = x - kx, dy = y - ky, dz = z - kz;
        if (dx * dx + dy * dy + dz * dz <= keep_r2) {
            const int64_t v = (int64_t)z * d.nxy + (int64_t)y * d.nx + x;
            out[v] = free_[v];
        }
    }
}

// wa_grid_tool_penalties: 0 on occupied voxels, else the number of thresholds above the count
__global__ __launch_bounds__(256) void k_reach_penalties(const uint8_t *__restrict__ free_, const uint16_t *__restrict__ count, int64_t n,
                                                         WaReachThr T, uint8_t *__restrict__ pen)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = count[i];
        int32_t p = 0;
        for (int32_t t = 0; t < T.n; t++) p += c < T.thr[t];
        pen[i] = free_[i] ? (uint8_t)p : 0;
    }
}
