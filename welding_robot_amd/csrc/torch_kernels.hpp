// torch_kernels.hpp -- device side of the torch-axis planner (wa_traj_tool_axes, wa_traj_tool_check; include/weldacs.h holds the
// definition, DESIGN 4o the reasoning).  Integers throughout: every output is bit-exact and independent of scheduling.
//   k_torch_nodes   feasibility of every (sample, direction): n * K * n_beads gathers of the distance field
//   k_torch_dp      the shortest sequence per leg (one workgroup per leg), its backtrack and the chosen-sequence counters
//   k_torch_check   rule 2 for one given axis per sample
#pragma once
#include "clearance_kernels.hpp"

#define WA_TORCH_TILE 32                       // consecutive samples per workgroup of k_torch_nodes
#define WA_TORCH_BLOCK_COST (1ll << 36)
#define WA_TORCH_INF_DEV (1ll << 62)

// what the device knows of the tool: per bead the distance behind the tip, the blocking threshold and the near threshold
// (r2 + near_add, or r2 itself when near is off: a bead that is not blocked is then never near).  Thresholds are at most 2^31.
struct WaTorchTool {
    int32_t n_beads;
    int32_t dist16[64];
    uint32_t r2[64], rn[64];
};

struct WaTorchRec {
    unsigned long long n_outside, n_blocked_pairs, n_no_dir, n_chosen_blocked, first_chosen_blocked /* ~0: none */, n_chosen_near,
        n_over_turn, max_turn_taken;
    unsigned int bad;   // bit 0: a coordinate of the trajectory is not finite
};

// Rule 2, the offset of a bead: floor((q_c * dist16 + 2^17) / 2^18) per axis (|q_c * dist16| <= 2^30, >> is arithmetic), packed as
// three int16 (|o_c| <= 4096) in one 8-byte word.
__device__ __forceinline__ short4 torch_offset(short4 q, int32_t dist16)
{
    short4 o;
    o.x = (short)(((int32_t)q.x * dist16 + (1 << 17)) >> 18);
    o.y = (short)(((int32_t)q.y * dist16 + (1 << 17)) >> 18);
    o.z = (short)(((int32_t)q.z * dist16 + (1 << 17)) >> 18);
    o.w = 0;
    return o;
}

// Rule 2, one bead: 0 passes, 1 near, 2 blocked.  A voxel outside the grid passes without a load.
__device__ __forceinline__ int torch_bead(const int32_t *__restrict__ d2, WaDims d, int32_t x, int32_t y, int32_t z, short4 o, uint32_t r2,
                                          uint32_t rn)
{
    const int32_t bx = x + o.x, by = y + o.y, bz = z + o.z;
    if ((uint32_t)bx >= (uint32_t)d.nx || (uint32_t)by >= (uint32_t)d.ny || (uint32_t)bz >= (uint32_t)d.nz) return 0;
    const uint32_t v = (uint32_t)d2[(int64_t)bz * d.nxy + (int64_t)by * d.nx + bx];
    return v <= r2 ? 2 : (v <= rn ? 1 : 0);
}

// the feasibility byte as the kernels keep it: the near count (0 .. 64) in bits 0-6, bit 7 = blocked (a blocked direction has at
// most 63 near beads).  The host turns it into the public byte (255 = blocked) when feas_out is asked for.
__device__ __forceinline__ uint8_t torch_feas(int n_near, bool blocked) { return (uint8_t)(blocked ? (0x80 | n_near) : n_near); }

// Rule 1, the turn measure.  Every |d| <= 32768, so the sum is at most 3 * 2^30: formed without a sign, it fits 32 bits.
__device__ __forceinline__ int32_t torch_turn(short4 a, short4 b)
{
    const int32_t dx = (int32_t)a.x - b.x, dy = (int32_t)a.y - b.y, dz = (int32_t)a.z - b.z;
    return (int32_t)(((uint32_t)(dx * dx) + (uint32_t)(dy * dy) + (uint32_t)(dz * dz)) >> 10);
}

// The voxel of sample i by the lookup of wa_traj_clearance; *outside as there; *bad when a coordinate is not finite.
__device__ __forceinline__ int3 torch_sample_voxel(const float *__restrict__ xyz, long long i, const WaField &F, bool *outside, bool *bad)
{
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    *bad = !(isfinite(px) && isfinite(py) && isfinite(pz));
    int64_t id;
    return field_voxel(F, px, py, pz, &id, outside);
}

// One workgroup per tile of WA_TORCH_TILE consecutive samples: neighbouring samples of a trajectory touch the same lines of d2, so
// they share a workgroup (and its CU's cache).  The K x n_beads offsets are staged once in LDS, bead-major (entry j * K + k) so that
// the lanes of a wavefront -- consecutive directions -- read consecutive 8-byte words.  The (sample, direction) pairs of the tile are
// laid out sample-major over the threads, which is also the layout of feas: every store is coalesced.
// Dynamic LDS: K * n_beads * 8 bytes (at most 128 KiB).
__global__ __launch_bounds__(256) void k_torch_nodes(const float *__restrict__ xyz, long long n, WaField F, const short4 *__restrict__ q,
                                                     int32_t K, const WaTorchTool *__restrict__ tool, uint8_t *__restrict__ feas,
                                                     WaTorchRec *__restrict__ rec)
{
    extern __shared__ __align__(16) unsigned char torch_lds[];
    short4 *offs = (short4 *)torch_lds;
    __shared__ int3 vox[WA_TORCH_TILE];
    __shared__ int32_t n_blk[WA_TORCH_TILE];
    __shared__ uint32_t thr[2][64];
    const long long i0 = (long long)blockIdx.x * WA_TORCH_TILE;
    const int32_t ts = (int32_t)min((long long)WA_TORCH_TILE, n - i0);
    const int32_t nb = tool->n_beads;
    for (int32_t e = threadIdx.x; e < K * nb; e += 256) offs[e] = torch_offset(q[e % K], tool->dist16[e / K]);
    if (threadIdx.x < 64) {
        thr[0][threadIdx.x] = tool->r2[threadIdx.x];
        thr[1][threadIdx.x] = tool->rn[threadIdx.x];
    }
    if (threadIdx.x < 64) {   // (wavefront 0 as a whole: WA_TORCH_TILE <= 64)
        bool outside = false, bad = false;
        if ((int32_t)threadIdx.x < ts) {
            vox[threadIdx.x] = torch_sample_voxel(xyz, i0 + threadIdx.x, F, &outside, &bad);
            n_blk[threadIdx.x] = 0;
        }
        const unsigned long long mo = __ballot(outside), mb = __ballot(bad);
        if (threadIdx.x == 0) {
            if (mo) atomicAdd(&rec->n_outside, (unsigned long long)__popcll(mo));
            if (mb) atomicOr(&rec->bad, 1u);
        }
    }
    __syncthreads();
    uint8_t *out = feas + i0 * K;
    unsigned int blocked_here = 0;
    for (int32_t p = threadIdx.x; p < ts * K; p += 256) {
        const int32_t s = p / K, k = p - s * K;
        const int3 v = vox[s];
        int n_near = 0;
        bool blocked = false;
        for (int32_t j = 0; j < nb; j++) {
            const int r = torch_bead(F.d2, F.d, v.x, v.y, v.z, offs[j * K + k], thr[0][j], thr[1][j]);
            n_near += r == 1;
            blocked |= r == 2;
        }
        out[p] = torch_feas(n_near, blocked);
        if (blocked) {
            blocked_here++;
            atomicAdd(&n_blk[s], 1);   // (LDS)
        }
    }
    for (int o = 32; o > 0; o >>= 1) blocked_here += __shfl_down(blocked_here, o, 64);
    if ((threadIdx.x & 63) == 0 && blocked_here) atomicAdd(&rec->n_blocked_pairs, (unsigned long long)blocked_here);
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned long long m = __ballot((int32_t)threadIdx.x < ts && n_blk[threadIdx.x] == K);
        if (threadIdx.x == 0 && m) atomicAdd(&rec->n_no_dir, (unsigned long long)__popcll(m));
    }
}

// Rule 2 for one given axis per sample: one lane per sample, the same offset and bead functions as above.
__global__ __launch_bounds__(256) void k_torch_check(const float *__restrict__ xyz, long long n, WaField F, const short4 *__restrict__ q,
                                                     const WaTorchTool *__restrict__ tool, uint8_t *__restrict__ blocked_out,
                                                     uint8_t *__restrict__ near_out, WaTorchRec *__restrict__ rec)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool outside = false, bad = false, blocked = false;
    int n_near = 0;
    if (i < n) {
        const int3 v = torch_sample_voxel(xyz, i, F, &outside, &bad);
        const short4 qi = q[i];
        for (int32_t j = 0; j < tool->n_beads; j++) {
            const int r = torch_bead(F.d2, F.d, v.x, v.y, v.z, torch_offset(qi, tool->dist16[j]), tool->r2[j], tool->rn[j]);
            n_near += r == 1;
            blocked |= r == 2;
        }
        blocked_out[i] = blocked ? 1 : 0;
        near_out[i] = (uint8_t)n_near;
    }
    const unsigned long long mo = __ballot(outside), mb = __ballot(bad), mk = __ballot(blocked), mn = __ballot(!blocked && n_near > 0);
    if ((threadIdx.x & 63) == 0) {
        if (mo) atomicAdd(&rec->n_outside, (unsigned long long)__popcll(mo));
        if (mb) atomicOr(&rec->bad, 1u);
        if (mk) {
            atomicAdd(&rec->n_chosen_blocked, (unsigned long long)__popcll(mk));
            atomicMin(&rec->first_chosen_blocked, (unsigned long long)(i + __builtin_ctzll(mk)));
        }
        if (mn) atomicAdd(&rec->n_chosen_near, (unsigned long long)__popcll(mn));
    }
}

struct WaTorchDp {
    int32_t K, w_near, w_want, w_turn, max_turn;
};

// Rule 5: one workgroup per leg, blockDim = K rounded up to whole wavefronts, thread k = destination state k.  A step reads the
// previous step's alpha and the directions q as LDS broadcasts (every lane the same address) and forms U on the fly: a K x K table
// of turn costs would be 256 KiB at K = 256.  alpha is double-buffered, so a step has one barrier.  The samples of a leg are a
// dependent chain; the parallelism of this kernel is across legs.  The feasibility byte and the wish of the NEXT sample are loaded
// before the inner loop so that their latency is off the chain.
// At the end wavefront 0 walks back from the last state (lane 0) and then counts over the chosen sequence (all 64 lanes).
__global__ __launch_bounds__(256) void k_torch_dp(const short4 *__restrict__ q, const short4 *__restrict__ wish /* n or NULL; .w = 1: given */,
                                                  const uint8_t *__restrict__ feas, const long long *__restrict__ off,
                                                  const int32_t *__restrict__ pin_first, const int32_t *__restrict__ pin_last, WaTorchDp P,
                                                  uint8_t *__restrict__ back, int32_t *__restrict__ dir, long long *__restrict__ leg_cost,
                                                  WaTorchRec *__restrict__ rec)
{
    __shared__ long long alpha[2][256];
    __shared__ short4 qs[256];
    const int32_t K = P.K, k = threadIdx.x;
    const long long s = off[blockIdx.x], e = off[blockIdx.x + 1];   // samples s .. e-1
    if (s >= e) {
        if (k == 0) leg_cost[blockIdx.x] = 0;
        return;
    }
    const bool live = k < K;
    const short4 qk = live ? q[k] : make_short4(0, 0, 0, 0);
    if (live) qs[k] = qk;
    const int32_t pf = pin_first ? pin_first[blockIdx.x] : -1, pl = pin_last ? pin_last[blockIdx.x] : -1;
    uint8_t f = live ? feas[s * K + k] : 0;
    short4 w = wish ? wish[s] : make_short4(0, 0, 0, 0);
    int cur = 0;
    for (long long i = s; i < e; i++) {
        const uint8_t fi = f;
        const short4 wi = w;
        if (i + 1 < e) {
            f = live ? feas[(i + 1) * K + k] : 0;
            if (wish) w = wish[i + 1];
        }
        long long node = (fi & 0x80 ? WA_TORCH_BLOCK_COST : 0) + (long long)P.w_near * (fi & 0x7f);
        if (wi.w) node += (long long)P.w_want * torch_turn(qk, wi);
        long long a;
        if (i == s) {
            a = (pf < 0 || k == pf) ? node : WA_TORCH_INF_DEV;
        } else {
            const long long *prev = alpha[cur ^ 1];
            long long best = WA_TORCH_INF_DEV + WA_TORCH_INF_DEV / 2;   // above every candidate: the first source always takes it
            int32_t arg = 0;
#pragma unroll 4
            for (int32_t kp = 0; kp < K; kp++) {
                const int32_t u = torch_turn(qs[kp], qk);
                long long c = prev[kp] + (long long)P.w_turn * u + ((P.max_turn >= 0 && u > P.max_turn) ? WA_TORCH_BLOCK_COST : 0);
                c = c < WA_TORCH_INF_DEV ? c : WA_TORCH_INF_DEV;
                if (c < best) { best = c; arg = kp; }
            }
            a = node + best;
            a = a < WA_TORCH_INF_DEV ? a : WA_TORCH_INF_DEV;
            if (live) back[i * K + k] = (uint8_t)arg;
        }
        alpha[cur][k] = a;
        __syncthreads();
        cur ^= 1;
    }
    if (threadIdx.x >= 64) return;   // (no barrier below: wavefront 0 alone)
    const long long *fin = alpha[cur ^ 1];
    if (k == 0) {
        int32_t st = pl;
        if (st < 0) {
            st = 0;
            for (int32_t c = 1; c < K; c++)
                if (fin[c] < fin[st]) st = c;
        }
        leg_cost[blockIdx.x] = fin[st];
        for (long long i = e - 1; i >= s; i--) {
            dir[i] = st;
            if (i > s) st = back[i * K + st];
        }
    }
    // lane 0's dir entries are read below by the other lanes of this SAME wavefront, and by nobody else in this launch.  One wavefront
    // is one instruction stream: the stores above are issued before the loads below, the fence makes the wavefront wait until those
    // stores have left it (and keeps the compiler from moving the loads up), and the loads are atomic at agent scope, so they are served
    // where the stores went, not from a line this CU cached earlier.  No second wavefront is involved: no release/acquire pair is needed.
    __threadfence();
    unsigned long long n_blk = 0, first = ~0ull, n_near = 0, n_over = 0, u_max = 0;
    for (long long i = s + k; i < e; i += 64) {
        const int32_t di = __hip_atomic_load(&dir[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint8_t fi = feas[i * K + di];
        if (fi & 0x80) {
            n_blk++;
            first = first < (unsigned long long)i ? first : (unsigned long long)i;
        } else if (fi) {
            n_near++;
        }
        if (i > s) {
            const int32_t u = torch_turn(qs[__hip_atomic_load(&dir[i - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)], qs[di]);
            n_over += P.max_turn >= 0 && u > P.max_turn;
            u_max = u_max > (unsigned long long)u ? u_max : (unsigned long long)u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_blk += __shfl_down(n_blk, o, 64);
        n_near += __shfl_down(n_near, o, 64);
        n_over += __shfl_down(n_over, o, 64);
        const unsigned long long f2 = __shfl_down(first, o, 64), u2 = __shfl_down(u_max, o, 64);
        first = f2 < first ? f2 : first;
        u_max = u2 > u_max ? u2 : u_max;
    }
    if (k == 0) {
        if (n_blk) {
            atomicAdd(&rec->n_chosen_blocked, n_blk);
            atomicMin(&rec->first_chosen_blocked, first);
        }
        if (n_near) atomicAdd(&rec->n_chosen_near, n_near);
        if (n_over) atomicAdd(&rec->n_over_turn, n_over);
        if (u_max) atomicMax(&rec->max_turn_taken, u_max);
    }
}
