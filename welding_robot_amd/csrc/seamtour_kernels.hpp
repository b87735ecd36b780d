// seamtour_kernels.hpp -- order and direction of two-ended weld seams: the multi-start local search over (order, direction)
// and the exact dynamic programme for small jobs.  Everything on the device is integer arithmetic on the quantised costs the host
// prepared (W, symmetric, 2M x 2M); there are no atomics: every descent owns its state and its outputs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WA_ST_BLOCK 256
#define WA_ST_INF ((long long)1 << 62)
#define WA_ST_MAX_EXACT 16

struct WaStArgs {
    const void *W;         // 2M x 2M quantised costs, row-major: uint32 where every entry fits, else int64
    const uint16_t *e0;    // start 0: the in-endpoint of every position (2 * seam + direction), M entries
    int32_t M, or_len, n_starts, max_passes;
    unsigned long long seed;
    long long *cost;       // per start: final cost
    int32_t *passes;       // per start: passes taken
    uint8_t *capped;       // per start: 1 when max_passes ended it
    uint16_t *tours;       // per start: final in-endpoints, M entries
};

__device__ __forceinline__ unsigned long long st_draw(unsigned long long &s)
{
    s += 0x9E3779B97F4A7C15ull;
    unsigned long long z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The lanes that hold one descent meet here: one wavefront (its LDS accesses are served in issue order, so ordering the compiler's
// view and draining the counter is all it takes), or the whole workgroup.
template <int TEAM>
__device__ __forceinline__ void st_team_sync()
{
    if (TEAM == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// One descent per TEAM lanes (64: a wavefront, four descents per workgroup; 256: the workgroup, for M > 64).  The state is E[k] = in(k)
// = 2 P[k] + delta[k] in LDS (out(k) = in(k) ^ 1), double-buffered so that applying a move is one gather.  Per pass the position i of a
// move runs in an outer loop that the whole team shares (what depends on i alone is read once, as a broadcast), and the lanes stride over
// the 7M moves of that i: M reversals (i, j) and 6M block moves (L, g, r).  The (delta, move number) minimum is a butterfly over the
// wavefront and, for a workgroup-wide team, one more step through LDS.
template <typename WT, bool W_LDS, int TEAM>
__global__ __launch_bounds__(WA_ST_BLOCK) void k_seam_descend(WaStArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    constexpr int TEAMS = WA_ST_BLOCK / TEAM;
    const int tid = threadIdx.x, team = tid / TEAM, lane = tid % TEAM;
    const int M = A.M, N2 = 2 * M, Mpad = (M + 7) & ~7;
    const WT *W = (const WT *)A.W;
    size_t off = 0;
    if (W_LDS) {
        WT *Wl = (WT *)st_lds;
        for (int k = tid; k < N2 * N2; k += WA_ST_BLOCK) Wl[k] = W[k];
        W = Wl;
        off = ((size_t)N2 * N2 * sizeof(WT) + 15) & ~(size_t)15;
    }
    uint16_t *E = (uint16_t *)(st_lds + off) + (size_t)team * 2 * Mpad, *E2 = E + Mpad;
    long long *red_d = (long long *)(st_lds + off + (size_t)TEAMS * 2 * Mpad * sizeof(uint16_t));   // (Mpad % 8 == 0: 16-byte aligned)
    int *red_m = (int *)(red_d + WA_ST_BLOCK / 64);
    __syncthreads();

    const int Lmax = min(A.or_len, M - 2), U = M + (Lmax > 0 ? 2 * M * Lmax : 0);
    for (int start = blockIdx.x * TEAMS + team; start < A.n_starts; start += gridDim.x * TEAMS) {   // (uniform over the team)
        if (start == 0) {
            for (int k = lane; k < M; k += TEAM) E[k] = A.e0[k];
        } else {
            for (int k = lane; k < M; k += TEAM) E[k] = (uint16_t)k;
            st_team_sync<TEAM>();
            if (lane == 0) {
                unsigned long long s = A.seed ^ ((unsigned long long)start * 0xD1B54A32D192ED03ull);
                for (int k = M - 1; k >= 1; k--) {
                    const unsigned long long d = st_draw(s);
                    const int j = (int)(((d >> 32) * (unsigned long long)(k + 1)) >> 32);
                    const uint16_t t = E[k];
                    E[k] = E[j];
                    E[j] = t;
                }
                for (int k = 0; k < M; k++) E[k] = (uint16_t)(2 * E[k] + (int)(st_draw(s) >> 63));
            }
        }
        st_team_sync<TEAM>();

        int passes = 0, capped = 0;
        for (;;) {
            if (passes == A.max_passes) { capped = 1; break; }
            passes++;
            long long bd = 0;
            int bm = 0x7fffffff;
            for (int i = 0; i < M; i++) {
                const int a = i ? i - 1 : M - 1;
                const int oa = E[a] ^ 1, ii = E[i];
                const long long w_oa_ii = (long long)W[oa * N2 + ii];
                for (int u = lane; u < U; u += TEAM) {
                    long long d = 0;
                    int mv = 0;
                    bool ok;
                    if (u < M) {   // A: Reverse(i, j)
                        const int j = u;
                        ok = j >= i && j - i <= M - 2;
                        if (ok) {
                            const int jn = j + 1 == M ? 0 : j + 1;
                            const int oj = E[j] ^ 1, in = E[jn];
                            d = (long long)W[oa * N2 + oj] + (long long)W[ii * N2 + in] - w_oa_ii - (long long)W[oj * N2 + in];
                            mv = i * M + j;
                        }
                    } else {       // B: Move(i, L, g, r)
                        int v = u - M;
                        const int L = 1 + (v >= 2 * M) + (v >= 4 * M);
                        v -= (L - 1) * 2 * M;
                        const int g = v >> 1, r = v & 1, l = i + L - 1;
                        ok = l <= M - 1 && (g < i || g > l) && g != a;
                        if (ok) {
                            const int b = l + 1 == M ? 0 : l + 1, h = g + 1 == M ? 0 : g + 1;
                            const int ol = E[l] ^ 1, ib = E[b], og = E[g] ^ 1, ih = E[h];
                            const long long x = r ? (long long)W[og * N2 + ol] + (long long)W[ii * N2 + ih]
                                                  : (long long)W[og * N2 + ii] + (long long)W[ol * N2 + ih];
                            d = (long long)W[oa * N2 + ib] - w_oa_ii - (long long)W[ol * N2 + ib] - (long long)W[og * N2 + ih] + x;
                            mv = M * M + (((i * 3 + L - 1) * M + g) * 2 + r);
                        }
                    }
                    if (ok && (d < bd || (d == bd && mv < bm))) { bd = d; bm = mv; }
                }
            }
            for (int o = 32; o; o >>= 1) {
                const long long od = __shfl_xor(bd, o);
                const int om = __shfl_xor(bm, o);
                if (od < bd || (od == bd && om < bm)) { bd = od; bm = om; }
            }
            if (TEAM > 64) {
                if ((tid & 63) == 0) { red_d[tid >> 6] = bd; red_m[tid >> 6] = bm; }
                __syncthreads();
                bd = red_d[0];
                bm = red_m[0];
                for (int w = 1; w < TEAM / 64; w++) {
                    const long long od = red_d[w];
                    const int om = red_m[w];
                    if (od < bd || (od == bd && om < bm)) { bd = od; bm = om; }
                }
                __syncthreads();
            }
            if (bd >= 0) break;   // a local optimum
            // apply: the new array is gathered from the old one
            if (bm < M * M) {
                const int i = bm / M, j = bm % M;
                for (int p = lane; p < M; p += TEAM) E2[p] = (p >= i && p <= j) ? (uint16_t)(E[i + j - p] ^ 1) : E[p];
            } else {
                int v = bm - M * M;
                const int r = v & 1;
                v >>= 1;
                const int g = v % M;
                v /= M;
                const int L = v % 3 + 1, i = v / 3, l = i + L - 1;
                // the block leaves the array and goes in behind the element that stood at g: first position of the block afterwards
                const int at = g > l ? g - L + 1 : g + 1;
                for (int p = lane; p < M; p += TEAM) {
                    uint16_t e;
                    if (p >= at && p < at + L) {
                        const int q = p - at;
                        e = r ? (uint16_t)(E[l - q] ^ 1) : E[i + q];
                    } else if (g > l && p >= i && p < at) {
                        e = E[p + L];
                    } else if (g < i && p >= at + L && p <= l) {
                        e = E[p - L];
                    } else {
                        e = E[p];
                    }
                    E2[p] = e;
                }
            }
            st_team_sync<TEAM>();
            uint16_t *t = E;
            E = E2;
            E2 = t;
        }

        long long c = 0;
        for (int k = lane; k < M; k += TEAM) {
            const int kn = k + 1 == M ? 0 : k + 1;
            c += (long long)W[(E[k] ^ 1) * N2 + E[kn]];
            A.tours[(size_t)start * M + k] = E[k];
        }
        for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
        if (TEAM > 64) {
            if ((tid & 63) == 0) red_d[tid >> 6] = c;
            __syncthreads();
            c = 0;
            for (int w = 0; w < TEAM / 64; w++) c += red_d[w];
        }
        if (lane == 0) {
            A.cost[start] = c;
            A.passes[start] = passes;
            A.capped[start] = (uint8_t)capped;
        }
        st_team_sync<TEAM>();   // (E and the reduction words are free for the next start)
    }
}

// Exact tour, one launch per popcount level (pull form): f[S][e] for every S with `level` seams and every endpoint e of a seam in S,
// from the level below.  Seams 1 .. M-1 are the bits of S, endpoint e stands for endpoint e + 2; seam 0 is fixed first with delta 0.
__global__ __launch_bounds__(256) void k_seam_dp_level(const long long *W, int M, int level, long long *f)
{
    const int n = M - 1, ne = 2 * n, N2 = 2 * M;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((long long)1 << n) * ne) return;
    const unsigned S = (unsigned)(idx / ne);
    const int e = (int)(idx % ne), t = e >> 1;
    if (__popc(S) != level || !((S >> t) & 1u)) return;
    const unsigned Sp = S ^ (1u << t);
    const int in = (e ^ 1) + 2;
    long long best;
    if (Sp == 0) {
        best = W[1 * N2 + in];
    } else {
        best = WA_ST_INF;
        for (int e2 = 0; e2 < ne; e2++)
            if ((Sp >> (e2 >> 1)) & 1u) {
                const long long v = f[(size_t)Sp * ne + e2] + W[(e2 + 2) * N2 + in];
                best = v < best ? v : best;
            }
    }
    f[idx] = best;
}
