// clearance_kernels.hpp -- device side of obstacle clearance: the exact squared Euclidean distance field of a grid's occupancy
// (wa_grid_distance_field), the inflated planning grid (wa_grid_inflate) and the trajectory check (wa_traj_clearance).
// Integer arithmetic throughout: every output is bit-exact and independent of scheduling.
#pragma once
#include "wa_device.h"

#define WA_D2_NONE_DEV 0x7fffffff

// Pass 1 (x, the contiguous axis): one wavefront per row.  For 64 voxels at a time a ballot gives the occupied ones; the nearest
// occupied voxel at or left of a lane is the highest set bit at or below it (else the last one of the chunks before), the nearest at
// or right of it the lowest set bit at or above it (else the first one of the next chunk that has any: looked up ahead once per such
// chunk, so every chunk is read at most twice, the second time from cache).  Writes (x - nearest)^2, WA_D2_NONE for a row without
// an occupied voxel.  free_ = 1 means free (the grid's occupancy convention).
__global__ __launch_bounds__(256) void k_edt_x(const uint8_t *__restrict__ free_, WaDims d, int32_t *__restrict__ d2)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)d.ny * d.nz) return;   // (whole waves)
    const uint8_t *o = free_ + row * d.nx;
    int32_t *out = d2 + row * d.nx;
    const int32_t nchunk = (d.nx + 63) >> 6;
    const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1);   // bits 0..lane
    const unsigned long long ge = ~0ull << lane;                               // bits lane..63
    int64_t lastL = -1;                        // last occupied x before the current chunk (-1: none)
    int32_t nextc = -1;                        // the next chunk after the current one holding an occupied voxel (nchunk: none) ...
    unsigned long long nextm = 0;              // ... and its ballot
    for (int32_t c = 0; c < nchunk; c++) {
        const int32_t x = c * 64 + lane;
        const unsigned long long m = __ballot(x < d.nx && o[x] == 0);
        if (nextc <= c) {
            nextc = c + 1;
            nextm = 0;
            for (; nextc < nchunk; nextc++) {
                const int32_t xn = nextc * 64 + lane;
                nextm = __ballot(xn < d.nx && o[xn] == 0);
                if (nextm) break;
            }
        }
        const unsigned long long lm = m & le, rm = m & ge;
        const int64_t L = lm ? (int64_t)c * 64 + 63 - __builtin_clzll(lm) : lastL;
        const int64_t R = rm ? (int64_t)c * 64 + __builtin_ctzll(rm) : (nextm ? (int64_t)nextc * 64 + __builtin_ctzll(nextm) : -1);
        int64_t best = -1;
        if (L >= 0) best = x - L;
        if (R >= 0 && (best < 0 || R - x < best)) best = R - x;
        if (m) lastL = (int64_t)c * 64 + 63 - __builtin_clzll(m);
        if (x < d.nx) out[x] = best < 0 ? WA_D2_NONE_DEV : (int32_t)(best * best);   // (< 2^31: the host checked the bound)
    }
}

// Passes 2 and 3 (y, z): one lane per column, lanes along x so that every row access is coalesced.  The column's values f(i) (the
// field of the passes before, WA_D2_NONE = no obstacle) become min_i f(i) + (j - i)^2 through the lower envelope of the parabolas
// (Felzenszwalb-Huttenlocher), built without a division: the top parabola t is dropped when the new one q meets it no later than t
// meets the one below it, I(t, q) <= I(t-1, t) with I(a, b) = ((f_b + b^2) - (f_a + a^2)) / (2 (b - a)), compared by cross-multiplying
// (|numerators| < 2^32, denominators < 2^17: int64 is exact).  The query walks the envelope and moves on while the next parabola is
// no worse at j (the envelope's breakpoints increase, so that test is monotone along it).  The envelope (index, value) lives in
// global scratch laid out like the field: entry k of the column at element j = k's address, interleaved across lanes.  The output
// overwrites the input in place: the envelope holds copies of every value it needs.
// Column `col` (0 .. ncols-1) starts at (col / inner) * outer + col % inner and steps by `step`.
__global__ __launch_bounds__(256) void k_edt_cols(int32_t *__restrict__ d2, int2 *__restrict__ env, int64_t ncols, int32_t len,
                                                  int64_t step, int64_t inner, int64_t outer)
{
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    const int64_t base = (col / inner) * outer + col % inner;
    int32_t top = -1;
    int64_t tv = 0, tf = 0;   // the top entry, kept in registers
    for (int32_t j = 0; j < len; j++) {
        const int32_t f = d2[base + (int64_t)j * step];
        if (f == WA_D2_NONE_DEV) continue;
        const int64_t qf = (int64_t)f + (int64_t)j * j;
        while (top >= 1) {
            const int2 b = env[base + (int64_t)(top - 1) * step];
            const int64_t bf = (int64_t)b.y + (int64_t)b.x * b.x, tff = tf + tv * tv;
            // I(t, q) <= I(b, t):  (qf - tff) / (2 (j - tv)) <= (tff - bf) / (2 (tv - b.x))
            if ((qf - tff) * (tv - b.x) <= (tff - bf) * ((int64_t)j - tv)) {
                top--;
                tv = b.x; tf = b.y;
            } else {
                break;
            }
        }
        top++;
        tv = j; tf = f;
        env[base + (int64_t)top * step] = make_int2(j, f);
    }
    if (top < 0) return;   // no obstacle in the column's line: it holds WA_D2_NONE already
    int32_t k = 0;
    int2 cur = env[base];
    int2 nxt = top >= 1 ? env[base + step] : cur;
    for (int32_t j = 0; j < len; j++) {
        int64_t dc = (int64_t)j - cur.x, vc = (int64_t)cur.y + dc * dc;
        while (k < top) {
            const int64_t dn = (int64_t)j - nxt.x, vn = (int64_t)nxt.y + dn * dn;
            if (vn > vc) break;
            k++;
            cur = nxt; vc = vn;
            if (k < top) nxt = env[base + (int64_t)(k + 1) * step];
        }
        d2[base + (int64_t)j * step] = (int32_t)vc;
    }
}

// wa_grid_inflate, part 1: free iff free in the source AND farther than the radius from every obstacle (WA_D2_NONE: no obstacle at
// all, which is farther than any radius).
__global__ __launch_bounds__(256) void k_inflate(const uint8_t *__restrict__ free_, const int32_t *__restrict__ d2, int64_t n, double r2,
                                                 uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = d2[i];
        out[i] = (free_[i] && (v == WA_D2_NONE_DEV || (double)v > r2)) ? 1 : 0;
    }
}

// Part 2: one workgroup per keep id; every voxel v with |v - k|^2 <= (radius + 1)^2 (index units) takes the source's state again.
// Every writer copies the same source byte, so the result does not depend on the order of the workgroups.
__global__ __launch_bounds__(256) void k_inflate_keep(const uint8_t *__restrict__ free_, WaDims d, const long long *__restrict__ keep,
                                                      int32_t h, double rk2, uint8_t *__restrict__ out)
{
    const long long id = keep[blockIdx.x];
    const int32_t kx = (int32_t)(id % d.nx), ky = (int32_t)((id / d.nx) % d.ny), kz = (int32_t)(id / d.nxy);
    const int32_t x0 = max(kx - h, 0), x1 = min(kx + h, d.nx - 1);
    const int32_t y0 = max(ky - h, 0), y1 = min(ky + h, d.ny - 1);
    const int32_t z0 = max(kz - h, 0), z1 = min(kz + h, d.nz - 1);
    const int64_t wx = x1 - x0 + 1, wy = y1 - y0 + 1, box = wx * wy * (int64_t)(z1 - z0 + 1);
    for (int64_t q = threadIdx.x; q < box; q += blockDim.x) {
        const int32_t x = x0 + (int32_t)(q % wx), y = y0 + (int32_t)((q / wx) % wy), z = z0 + (int32_t)(q / (wx * wy));
        const int64_t dx = x - kx, dy = y - ky, dz = z - kz;
        if ((double)(dx * dx + dy * dy + dz * dz) <= rk2) {
            const int64_t v = (int64_t)z * d.nxy + (int64_t)y * d.nx + x;
            out[v] = free_[v];
        }
    }
}

// Nearest node of one axis: the lowest j minimising |p - c[j]| (fp32 subtraction) after p is clamped into [lo, hi], the table's
// smallest and largest values (NaN clamps to lo).  Binary search on a non-decreasing table, a scan otherwise: the same answer.
__device__ inline int32_t clr_axis_node(const float *__restrict__ c, int32_t n, float lo, float hi, int mono, float p, bool *outside)
{
    if (!(p >= lo)) { *outside = true; p = lo; }
    else if (p > hi) { *outside = true; p = hi; }
    if (!mono) {
        int32_t bj = 0;
        float bd = fabsf(p - c[0]);
        for (int32_t j = 1; j < n; j++) {
            const float dj = fabsf(p - c[j]);
            if (dj < bd) { bd = dj; bj = j; }
        }
        return bj;
    }
    int32_t a = 0, b = n - 1;   // first j with c[j] >= p (exists: p <= hi = c[n-1])
    while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        if (c[m] >= p) b = m; else a = m + 1;
    }
    const int32_t j = a;
    if (c[j] == p || j == 0) return j;
    // left of j |p - c[i]| does not increase with i; the lowest i on which it equals its value at j-1 ties with j-1
    const float dl = fabsf(p - c[j - 1]), dr = fabsf(p - c[j]);
    if (!(dl <= dr)) return j;
    a = 0; b = j - 1;
    while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        if (fabsf(p - c[m]) <= dl) b = m; else a = m + 1;
    }
    return a;
}

// per axis: the table's smallest and largest value, and whether the table is non-decreasing
struct WaClrAxes {
    float lo[3], hi[3];
    int32_t mono[3];
};

// The grid as something a sample is looked up in: its dims, axis tables with their ranges, and its distance field.  One kernel
// argument, filled by the host's grid_field(); all zero when a call has no grid (k_rt_caps).
struct WaField {
    WaDims d;
    const float *cx, *cy, *cz;
    WaClrAxes A;
    const int32_t *d2;
};

// The voxel of a point: the nearest node per axis, and its id.  *outside is set when a coordinate lies outside its table's range
// (never cleared).  The one lookup of wa_traj_clearance, the fit, wa_traj_retime and the torch axis.
__device__ inline int3 field_voxel(const WaField &F, float px, float py, float pz, int64_t *id, bool *outside)
{
    int3 v;
    v.x = clr_axis_node(F.cx, F.d.nx, F.A.lo[0], F.A.hi[0], F.A.mono[0], px, outside);
    v.y = clr_axis_node(F.cy, F.d.ny, F.A.lo[1], F.A.hi[1], F.A.mono[1], py, outside);
    v.z = clr_axis_node(F.cz, F.d.nz, F.A.lo[2], F.A.hi[2], F.A.mono[2], pz, outside);
    *id = (int64_t)v.z * F.d.nxy + (int64_t)v.y * F.d.nx + v.x;
    return v;
}

// the start value of the summary's accumulator acc[4] (k_clr_samples, k_clr_segments): min key, first hit, n_hit, n_outside
__host__ __device__ inline void clr_acc_init(unsigned long long acc[4])
{
    acc[0] = ~0ull; acc[1] = ~0ull; acc[2] = 0; acc[3] = 0;
}

// one lane per sample: its voxel, the field there, and the summary's sample terms (min d2 with its lowest index, packed as
// d2 << 33 | index into one atomicMin; samples outside the coordinate range)
__global__ __launch_bounds__(256) void k_clr_samples(const float *__restrict__ xyz, int64_t n, WaField F, long long *__restrict__ ids,
                                                     int32_t *__restrict__ d2s,
                                                     unsigned long long *__restrict__ acc /* [0] min key, [3] n_outside */)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = ~0ull, outs = 0;
    if (i < n) {
        bool out = false;
        int64_t id;
        field_voxel(F, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &id, &out);
        const int32_t v = F.d2[id];
        ids[i] = id;
        d2s[i] = v;
        key = ((unsigned long long)(uint32_t)v << 33) | (unsigned long long)i;
        outs = out ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k2 = __shfl_down(key, o, 64);
        key = k2 < key ? k2 : key;
        outs += __shfl_down(outs, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (key != ~0ull) atomicMin(&acc[0], key);
        if (outs) atomicAdd(&acc[3], outs);
    }
}

// The event walk over the 3-D supercover between voxels a and b.  Axis c with d_c != 0 changes voxel at t = (2m + 1) / (2 |d_c|),
// m = 0 .. |d_c| - 1; at such a t that axis holds both voxels around the boundary.  The walk visits the events in order (compared by
// cross-multiplying), steps the axes tied at an event together and visits every voxel of the product of the axes' sets there (up to 8
// around a shared corner, the one the walk stands on among them); with no event the cover is voxel a.  visit(id) is called with the
// raster id of each voxel, voxel a first, and returns true to end the walk; every id lies in the box spanned by a and b.
// The one definition of the cover: wa_traj_clearance (k_clr_segments), wa_grid_path_shortcut (k_sc_reach) and wa_grid_pose_shortcut
// (k_psc_reach) all walk it.
template <class Visit>
__device__ __forceinline__ void clr_cover_visit(long long a, long long b, WaDims d, Visit &&visit)
{
    int32_t cur[3] = {(int32_t)(a % d.nx), (int32_t)((a / d.nx) % d.ny), (int32_t)(a / d.nxy)};
    const int32_t end[3] = {(int32_t)(b % d.nx), (int32_t)((b / d.nx) % d.ny), (int32_t)(b / d.nxy)};
    int32_t s[3], D[3], m[3];
    for (int c = 0; c < 3; c++) {
        const int32_t dd = end[c] - cur[c];
        s[c] = dd > 0 ? 1 : (dd < 0 ? -1 : 0);
        D[c] = dd > 0 ? dd : -dd;
        m[c] = 0;
    }
    bool stop = visit((int64_t)a);
    while (!stop) {
        // the earliest pending event: t_c = (2 m_c + 1) / (2 D_c)
        int best = -1;
        for (int c = 0; c < 3; c++) {
            if (m[c] >= D[c]) continue;
            if (best < 0 || (int64_t)(2 * m[c] + 1) * D[best] < (int64_t)(2 * m[best] + 1) * D[c]) best = c;
        }
        if (best < 0) break;
        bool tie[3];
        for (int c = 0; c < 3; c++)
            tie[c] = m[c] < D[c] && (int64_t)(2 * m[c] + 1) * D[best] == (int64_t)(2 * m[best] + 1) * D[c];
        for (int q = 0; q < 8 && !stop; q++) {
            if (((q & 1) && !tie[0]) || ((q & 2) && !tie[1]) || ((q & 4) && !tie[2])) continue;
            const int32_t x = cur[0] + ((q & 1) ? s[0] : 0), y = cur[1] + ((q & 2) ? s[1] : 0), z = cur[2] + ((q & 4) ? s[2] : 0);
            stop = visit((int64_t)z * d.nxy + (int64_t)y * d.nx + x);
        }
        for (int c = 0; c < 3; c++)
            if (tie[c]) { cur[c] += s[c]; m[c]++; }
    }
}

// Does the supercover between voxels a and b meet an occupied voxel of free_ (1 = free)?  Returns at the first occupied voxel.
__device__ inline bool clr_cover_hits(long long a, long long b, WaDims d, const uint8_t *__restrict__ free_)
{
    bool hit = false;
    clr_cover_visit(a, b, d, [&](int64_t v) { return hit = !free_[v]; });
    return hit;
}

// one lane per segment i (samples i, i+1): does the 3-D supercover between the two sample voxels meet an occupied voxel?
__global__ __launch_bounds__(256) void k_clr_segments(const long long *__restrict__ ids, int64_t n, WaDims d, const uint8_t *__restrict__ free_,
                                                      uint8_t *__restrict__ hit_out, unsigned long long *__restrict__ acc /* [1] first, [2] n_hit */)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool hit = false;
    if (i + 1 < n) {
        hit = clr_cover_hits(ids[i], ids[i + 1], d, free_);
        if (hit_out) hit_out[i] = hit ? 1 : 0;
    }
    unsigned long long first = hit ? (unsigned long long)i : ~0ull, cnt = hit ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long f2 = __shfl_down(first, o, 64);
        first = f2 < first ? f2 : first;
        cnt += __shfl_down(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicMin(&acc[1], first);
        atomicAdd(&acc[2], cnt);
    }
}
