// frames_kernels.hpp -- device side of the tool frames and the weld weave at jerk-limited ticks (wa_traj_retime_jerk_frames;
// include/weldacs.h rules 61 - 67 hold the definition, DESIGN 4ad the reasoning, tests/frames_ref.py restates it in numpy).  The lateral
// (the direction across the seam) and the weave's offset need the tick's place on the path, which k_jk_axes has just found: the stage
// below is that kernel's body with one more policy, so no tick is located a second time.
//   k_fr_dirs    one lane per sample: the travel direction of rule 62 between the nearest samples at another arc length, found by the
//                searches k_jk_axes uses for a run of coincident samples
//   k_fr_ticks   jx_axes<WaFrames> (jerk_axes_kernels.hpp): per tick the lateral of rule 63, the offset of rule 65, the woven position of
//                rule 66 in front of the bead check of the same lane, the laterals and the positions through LDS, the counters of rule
//                67 through slots as WaAxRec's
// Integers and single correctly rounded fp64 operations throughout; what is accumulated across lanes is an integer.
#pragma once
#include "jerk_axes_kernels.hpp"

#define WA_FR_MAX_P 4096
#define WA_FR_MAX_WL (1ll << 50)

struct WaFrSlot {
    unsigned long long n_no_lateral, n_weave_ticks, n_weave_blocked, pad[5];   // one 64-byte line
};
struct WaFrRec {
    WaFrSlot slot[WA_AX_SLOTS];
    unsigned long long max_offset_q, max_offset_step_q, max_lat_turn;
};

// Rule 62.  tau.w = 1 marks the all-zero direction (tau is then (0, 0, 0)).
__global__ __launch_bounds__(256) void k_fr_dirs(const float *__restrict__ xyz, const long long *__restrict__ GL, long long n,
                                                 short4 *__restrict__ tau)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long g = GL[j];
    const long long lo = jk_last_below(GL, 0, j, g);            // -1: none
    const long long hi = jk_last_at_most(GL, j, n - 1, g) + 1;   // n: none
    const float *a = xyz + 3 * (lo >= 0 ? lo : j), *b = xyz + 3 * (hi < n ? hi : j);
    const double tx = (double)b[0] - (double)a[0], ty = (double)b[1] - (double)a[1], tz = (double)b[2] - (double)a[2];
    short4 q = make_short4(0, 0, 0, 1);
    if (!(tx == 0.0 && ty == 0.0 && tz == 0.0)) q = ax_quantise(tx, ty, tz);
    tau[j] = q;
}

struct FrLds {
    float lat[256 * 3], pos[256 * 3];
    unsigned int cnt[3], lat_turn, moved;   // the workgroup's ticks without a lateral / weaving / weaving and blocked
    unsigned long long max_off, max_step;
};

struct FrOut {
    long long ql;      // tk_pack; -1: undefined
    long long off_q;
    bool weave;
};

struct WaFrames {
    static constexpr bool on = true;
    const short4 *tau;   // n
    const int2 *run;     // n - 1: the samples O_r and E_r are taken at, x < 0 on a segment that does not weave; nullptr without a weave
    const short *pat;    // P
    int32_t P;
    long long amp_q, wl_q, taper_q;
    float *lat;          // n_ticks x 3
    WaFrRec *rec;
    typedef FrOut State;   // what a lane found for its own tick

    __device__ __forceinline__ FrLds &lds() const
    {
        __shared__ FrLds s;
        return s;
    }
    __device__ __forceinline__ void begin(FrOut &mine) const
    {
        FrLds &s = lds();
        if (threadIdx.x < 3) s.cnt[threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            s.lat_turn = s.moved = 0;
            s.max_off = s.max_step = 0;
        }
        mine.ql = -1;
        mine.off_q = 0;
        mine.weave = false;
    }
    // rules 63 - 65 for a located tick; off: rule 65's double
    __device__ __forceinline__ FrOut locate(const WaJkTicks &T, const JxTick &t, long long S, short4 *ql, double *off) const
    {
        FrOut o;
        const long long i = t.r.i;
        short4 tt;
        if (t.rest) {
            tt = tau[t.below + 1];
        } else {
            tt = jx_axis(tau[i], tau[i + 1], t.r.exact == 1 ? 1.0 : t.r.lam);
        }
        const int32_t zx = t.qt.x, zy = t.qt.y, zz = t.qt.z, ux = tt.x, uy = tt.y, uz = tt.z;
        const int32_t yx = zy * uz - zz * uy, yy = zz * ux - zx * uz, yz = zx * uy - zy * ux;   // (exact: every term below 2^29)
        o.ql = -1;
        *ql = make_short4(0, 0, 0, 0);
        if (yx | yy | yz) {
            *ql = ax_quantise((double)yx, (double)yy, (double)yz);
            o.ql = tk_pack(*ql);
        }
        o.off_q = 0;
        o.weave = false;
        *off = 0.0;
        if (run) {
            const int2 r = run[i];
            if (r.x >= 0) {
                o.weave = true;
                const long long d = S - T.GL[r.x], back = T.GL[r.y] - S;
                const long long phi = d % wl_q;
                const double x = __ddiv_rn((double)phi * (double)P, (double)wl_q);
                int32_t j = (int32_t)floor(x);
                j = j > P - 1 ? P - 1 : j;
                const double f = x - (double)j;
                const double pa = (double)pat[j], pb = (double)pat[j + 1 < P ? j + 1 : 0];
                const double w = pa + (pb - pa) * f;
                const long long m = d < back ? d : back;
                const double env = taper_q == 0 || m >= taper_q ? 1.0 : __ddiv_rn((double)m, (double)taper_q);
                *off = ((((double)amp_q / WA_RT_Q) * env) * w) / 16384.0;
                o.off_q = (long long)rint(*off * WA_RT_Q);
            }
        }
        return o;
    }
    __device__ __forceinline__ void tick(FrOut &mine, const WaJkTicks &T, const JxTick &t, long long S, float *px, float *py, float *pz) const
    {
        FrLds &s = lds();
        short4 ql;
        double off;
        mine = locate(T, t, S, &ql, &off);
        if (off != 0.0 && mine.ql != -1) {   // rule 66
            *px = (float)((double)*px + ((double)ql.x / 16384.0) * off);
            *py = (float)((double)*py + ((double)ql.y / 16384.0) * off);
            *pz = (float)((double)*pz + ((double)ql.z / 16384.0) * off);
            s.moved = 1;   // (every writer stores the same value)
        }
        s.lat[3 * threadIdx.x] = (float)((double)ql.x / 16384.0);
        s.lat[3 * threadIdx.x + 1] = (float)((double)ql.y / 16384.0);
        s.lat[3 * threadIdx.x + 2] = (float)((double)ql.z / 16384.0);
        s.pos[3 * threadIdx.x] = *px;
        s.pos[3 * threadIdx.x + 1] = *py;
        s.pos[3 * threadIdx.x + 2] = *pz;
    }
    // Rule 67: what needs the tick in front -- the same values in every lane for the tick in front of the wave's first, a shuffle for
    // the others -- and the workgroup's counters.  Called by every lane of a wave that holds a live tick.
    __device__ __forceinline__ void steps(const FrOut &mine, const WaJkTicks &T, const JxTick &front, long long S_front, bool live, long long k,
                                          bool blocked) const
    {
        FrLds &s = lds();
        const int lane = threadIdx.x & 63;
        short4 fq;
        double foff;
        const FrOut f = locate(T, front, S_front, &fq, &foff);
        long long ql_before = __shfl_up(mine.ql, 1, 64), off_before = __shfl_up(mine.off_q, 1, 64);
        if (lane == 0) {
            ql_before = f.ql;
            off_before = f.off_q;
        }
        unsigned long long lt = 0, step = 0, mag = 0;
        if (live) {
            mag = jk_abs(mine.off_q);
            if (k > 0) {
                step = jk_abs(mine.off_q - off_before);
                if (mine.ql != -1 && ql_before != -1) lt = ax_chord2(tk_unpack(ql_before), tk_unpack(mine.ql)) >> 10;
            }
        }
        const unsigned long long mn = __ballot(live && mine.ql == -1), mw = __ballot(live && mine.weave),
                                 mb = __ballot(live && mine.weave && blocked);
        lt = jk_wave_max(lt);
        step = jk_wave_max(step);
        mag = jk_wave_max(mag);
        if (lane == 0) {   // (LDS atomics)
            if (mn) atomicAdd(&s.cnt[0], (unsigned int)__popcll(mn));
            if (mw) atomicAdd(&s.cnt[1], (unsigned int)__popcll(mw));
            if (mb) atomicAdd(&s.cnt[2], (unsigned int)__popcll(mb));
            if (lt) atomicMax(&s.lat_turn, (unsigned int)lt);
            if (step) atomicMax(&s.max_step, step);
            if (mag) atomicMax(&s.max_off, mag);
        }
    }
    // behind the body's barrier: the counters, the laterals and, where a tick of the workgroup moved, its positions
    __device__ __forceinline__ void end(const WaJkTicks &T) const
    {
        FrLds &s = lds();
        if (threadIdx.x == 0) {
            WaFrSlot *sl = &rec->slot[blockIdx.x & (WA_AX_SLOTS - 1)];
            if (s.cnt[0]) atomicAdd(&sl->n_no_lateral, (unsigned long long)s.cnt[0]);
            if (s.cnt[1]) atomicAdd(&sl->n_weave_ticks, (unsigned long long)s.cnt[1]);
            if (s.cnt[2]) atomicAdd(&sl->n_weave_blocked, (unsigned long long)s.cnt[2]);
            if (s.max_off > __hip_atomic_load(&rec->max_offset_q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->max_offset_q, s.max_off);
            if (s.max_step > __hip_atomic_load(&rec->max_offset_step_q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&rec->max_offset_step_q, s.max_step);
            if (s.lat_turn > __hip_atomic_load(&rec->max_lat_turn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&rec->max_lat_turn, (unsigned long long)s.lat_turn);
        }
        const long long first = (long long)blockIdx.x * blockDim.x * 3, end = T.n_ticks * 3;
        const bool moved = T.out && s.moved;
        for (int e = threadIdx.x; e < 256 * 3; e += 256)
            if (first + e < end) {
                lat[first + e] = s.lat[e];
                if (moved) T.out[first + e] = s.pos[e];
            }
    }
};

__global__ __launch_bounds__(256) void k_fr_ticks(WaJkTicks T, WaJkAxes A, WaField F, const WaTorchTool *__restrict__ tool,
                                                  WaAxRec *__restrict__ rec, WaFrames Fr)
{
    jx_axes(T, A, F, tool, rec, Fr);
}
