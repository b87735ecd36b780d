// seamrules_kernels.hpp -- seam tours under job rules: precedences between seams and one-way seams.  k_seam_descend_rules is
// k_seam_descend (seamtour_kernels.hpp: same state, same team mapping, same moves and numbers, same integers) with the anchor seam held
// at position 0 and every move tested for admissibility; k_seam_rules_dp_level is k_seam_dp_level with a predecessor mask per seam and
// the permitted-entry test.  No atomics: every descent owns its state and its outputs.
#pragma once
#include "seamtour_kernels.hpp"

#define WA_SR_WORDS 18   // 16-bit LDS words per position and team: E, E2, the eight arrays below and the eight words of lim

struct WaSrArgs {
    WaStArgs st;
    const int32_t *succ_at, *succ;   // the distinct pairs as lists by seam: M + 1 offsets, then the direct successors ...
    const int32_t *pred_at, *pred;   // ... and the direct predecessors
    const uint8_t *fixed;            // M bytes: 0 free, 1 entered at the even endpoint, 2 at the odd one (the dummy: 0)
    int32_t anchor;                  // the seam that holds position 0: 0, or the dummy of an open tour
};

// what a pass needs to know about the state, per team in LDS (int16: positions run to 1025)
struct WaSrLds {
    int16_t *pos;       // by seam: where it stands
    int16_t *blk;       // by position p: a reversal that starts at i <= blk[p] may not reach p (M for a one-way seam, else the last
                        // position of a direct predecessor, -1: none).  Before the first pass: the repair's counters, by seam
    int16_t *nr[3];     // by position p: the last position before p - k of a direct predecessor (-1: none)
    int16_t *fr[3];     // by position p: the first position behind p + k of a direct successor (M: none)
    int16_t *lim;       // by i, eight words (one 16-byte read per i): [L - 1] the block i .. i + L - 1 may go in behind g >= that when it
                        // jumps back, [4 + L - 1] behind g < that when it jumps forward; [3] rmax(i), the last j that Reverse(i, j) may
                        // take (teams wider than a wavefront; a wavefront takes it from a ballot)
};

template <int TEAM>
__device__ __forceinline__ int sr_team_min(int v, int tid, int *red_m)
{
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    if (TEAM > 64) {
        if ((tid & 63) == 0) red_m[tid >> 6] = v;
        __syncthreads();
        v = red_m[0];
        for (int w = 1; w < TEAM / 64; w++) v = min(v, red_m[w]);
        __syncthreads();
    }
    return v;
}

// The limits of one pass from the state E.  A successor that stands inside a block must not stop the block: nr / fr leave out what
// stands within k positions, and the block (i, L) takes, from its seam at offset q, the entry that skips exactly the rest of the block.
template <int TEAM>
__device__ __forceinline__ void sr_limits(const WaSrArgs &A, const uint16_t *E, const WaSrLds &S, int M, int lane)
{
    for (int p = lane; p < M; p += TEAM) S.pos[E[p] >> 1] = (int16_t)p;
    st_team_sync<TEAM>();
    for (int p = lane; p < M; p += TEAM) {
        const int s = E[p] >> 1;
        int n0 = -1, n1 = -1, n2 = -1, f0 = M, f1 = M, f2 = M;
        for (int q = A.pred_at[s]; q < A.pred_at[s + 1]; q++) {
            const int x = S.pos[A.pred[q]];
            if (x < p) n0 = max(n0, x);
            if (x < p - 1) n1 = max(n1, x);
            if (x < p - 2) n2 = max(n2, x);
        }
        for (int q = A.succ_at[s]; q < A.succ_at[s + 1]; q++) {
            const int x = S.pos[A.succ[q]];
            if (x > p) f0 = min(f0, x);
            if (x > p + 1) f1 = min(f1, x);
            if (x > p + 2) f2 = min(f2, x);
        }
        S.nr[0][p] = (int16_t)n0; S.nr[1][p] = (int16_t)n1; S.nr[2][p] = (int16_t)n2;
        S.fr[0][p] = (int16_t)f0; S.fr[1][p] = (int16_t)f1; S.fr[2][p] = (int16_t)f2;
        S.blk[p] = (int16_t)(A.fixed[s] ? M : n0);
    }
    st_team_sync<TEAM>();
    for (int i = lane; i < M; i += TEAM) {
        int b = -1, f = M;
        for (int L = 1; L <= 3; L++) {
            if (i + L - 1 < M) {
                b = -1;
                f = M;
                for (int q = 0; q < L; q++) {
                    b = max(b, (int)S.nr[q][i + q]);
                    f = min(f, (int)S.fr[L - 1 - q][i + q]);
                }
            }
            S.lim[8 * i + L - 1] = (int16_t)b;
            S.lim[8 * i + 4 + L - 1] = (int16_t)f;
        }
    }
    if (TEAM > 64) {
        // rmax(i) + 1 is the first p >= i with blk[p] >= i.  pos is free again: it takes the largest blk of every 32 positions, so that
        // an i looks through the rest of its own 32, skips the groups that cannot hold its p, and ends inside the one that does
        for (int c = lane; c * 32 < M; c += TEAM) {
            int mx = -1;
            for (int p = c * 32; p < min(M, c * 32 + 32); p++) mx = max(mx, (int)S.blk[p]);
            S.pos[c] = (int16_t)mx;
        }
        st_team_sync<TEAM>();
        for (int i = lane; i < M; i += TEAM) {
            const int own = min(M, (i | 31) + 1);
            int j = i;
            while (j < own && S.blk[j] < i) j++;
            if (j == own && j < M) {
                int c = j >> 5;
                while (c * 32 < M && S.pos[c] < i) c++;
                j = min(M, c * 32);
                while (j < M && S.blk[j] < i) j++;
            }
            S.lim[8 * i + 3] = (int16_t)(j - 1);
        }
    }
    st_team_sync<TEAM>();
}

// One descent per TEAM lanes, as in k_seam_descend.  What differs: position 0 holds the anchor and no move takes it away (i >= 1, but
// for Reverse(0, 0)); a start is repaired on the team before it descends; a pass first derives the limits above, and a move counts only
// if it keeps every pair in order and every one-way seam in its direction: Reverse(i, j) iff j <= rmax(i), a reversed block iff
// rmax(i) reaches its end, a block jump iff g stays on this side of the block's nearest predecessor / successor outside the block.
template <typename WT, bool W_LDS, int TEAM>
__global__ __launch_bounds__(WA_ST_BLOCK) void k_seam_descend_rules(WaSrArgs R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    constexpr int TEAMS = WA_ST_BLOCK / TEAM;
    const WaStArgs &A = R.st;
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
    uint16_t *E = (uint16_t *)(st_lds + off) + (size_t)team * WA_SR_WORDS * Mpad, *E2 = E + Mpad;
    WaSrLds S;
    {
        int16_t *p = (int16_t *)(E + 2 * Mpad);
        S.pos = p; S.blk = p + Mpad; S.lim = p + 8 * Mpad;   // (lim: 20 Mpad bytes into the team's words, 16-byte aligned)
        for (int k = 0; k < 3; k++) {
            S.nr[k] = p + (2 + k) * Mpad; S.fr[k] = p + (5 + k) * Mpad;
        }
    }
    long long *red_d = (long long *)(st_lds + off + (size_t)TEAMS * WA_SR_WORDS * Mpad * sizeof(uint16_t));   // (Mpad % 8 == 0: 16-byte aligned)
    int *red_m = (int *)(red_d + WA_ST_BLOCK / 64);
    __syncthreads();

    const int Lmax = min(A.or_len, M - 2), U = M + (Lmax > 0 ? 2 * M * Lmax : 0);
    for (int start = blockIdx.x * TEAMS + team; start < A.n_starts; start += gridDim.x * TEAMS) {   // (uniform over the team)
        if (start == 0) {
            for (int k = lane; k < M; k += TEAM) E[k] = A.e0[k];
        } else {
            for (int k = lane; k < M; k += TEAM) {
                E[k] = (uint16_t)k;
                S.blk[k] = (int16_t)(R.pred_at[k + 1] - R.pred_at[k]);   // the repair's counter: predecessors not yet placed
            }
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
            st_team_sync<TEAM>();
            // the repair: the anchor, then always the seam that stands earliest in the draw among those whose predecessors are placed
            for (int step = 0; step < M; step++) {
                int cand = 0x7fffffff;
                for (int k = lane; k < M; k += TEAM) {
                    const int s = E[k] >> 1;
                    if (step == 0 ? s == R.anchor : S.blk[s] == 0) { cand = k; break; }
                }
                cand = sr_team_min<TEAM>(cand, tid, red_m);
                if (cand >= M) cand = 0;   // (cannot happen on checked rules; stay inside the arrays whatever comes)
                const int e = E[cand], s = e >> 1, fx = R.fixed[s];
                if (lane == 0) {
                    E2[step] = (uint16_t)(2 * s + (fx ? fx - 1 : (e & 1)));
                    S.blk[s] = -1;
                }
                for (int q = R.succ_at[s] + lane; q < R.succ_at[s + 1]; q += TEAM) S.blk[R.succ[q]]--;   // (distinct pairs: distinct words)
                st_team_sync<TEAM>();
            }
            uint16_t *t = E;
            E = E2;
            E2 = t;
        }
        st_team_sync<TEAM>();

        int passes = 0, capped = 0;
        for (;;) {
            if (passes == A.max_passes) { capped = 1; break; }
            passes++;
            sr_limits<TEAM>(R, E, S, M, lane);
            const int my_blk = (TEAM == 64 && lane < M) ? (int)S.blk[lane] : -1;
            long long bd = 0;
            int bm = 0x7fffffff;
            for (int i = 0; i < M; i++) {
                const int4 lim = *(const int4 *)(S.lim + 8 * i);   // (a broadcast: every lane reads the same 16 bytes)
                const int bk1 = (int16_t)lim.x, bk2 = lim.x >> 16, bk3 = (int16_t)lim.y;
                const int fw1 = (int16_t)lim.z, fw2 = lim.z >> 16, fw3 = (int16_t)lim.w;
                int rm;
                if (TEAM == 64) {
                    const unsigned long long bad = __ballot(lane >= i && my_blk >= i);
                    rm = bad ? __ffsll((long long)bad) - 2 : M - 1;
                } else {
                    rm = lim.y >> 16;
                }
                const int a = i ? i - 1 : M - 1;
                const int oa = E[a] ^ 1, ii = E[i];
                const long long w_oa_ii = (long long)W[oa * N2 + ii];
                const int Ui = i ? U : 1;   // position 0 has one move: Reverse(0, 0)
                for (int u = lane; u < Ui; u += TEAM) {
                    long long d = 0;
                    int mv = 0;
                    bool ok;
                    if (u < M) {   // A: Reverse(i, j)
                        const int j = u;
                        ok = j >= i && j - i <= M - 2 && j <= rm;
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
                        const int bk = L == 1 ? bk1 : L == 2 ? bk2 : bk3, fw = L == 1 ? fw1 : L == 2 ? fw2 : fw3;
                        ok = l <= M - 1 && (g < i || g > l) && g != a && (r == 0 || rm >= l) && (g > l ? g < fw : g >= bk);
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
            if (bd >= 0) break;   // a local optimum among the admissible moves
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
        st_team_sync<TEAM>();   // (the state, the limits and the reduction words are free for the next start)
    }
}

// Exact tour under rules, one launch per popcount level (pull form).  W has the anchor as seam 0, entered at endpoint 0; seams 1 .. M-1
// are the bits of S.  f[S][e] (e + 2 the endpoint at which the last seam of S is left) stays WA_ST_INF where a direct predecessor of
// that seam is missing from S or fixed forbids its entry at (e ^ 1) + 2; as every value is built on one of the level below, exactly
// the subsets that are closed under `before` carry a value.
__global__ __launch_bounds__(256) void k_seam_rules_dp_level(const long long *W, int M, int level, const uint32_t *predmask, const uint8_t *fixed,
                                                             long long *f)
{
    const int n = M - 1, ne = 2 * n, N2 = 2 * M;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((long long)1 << n) * ne) return;
    const unsigned S = (unsigned)(idx / ne);
    const int e = (int)(idx % ne), t = e >> 1;
    if (__popc(S) != level || !((S >> t) & 1u)) return;
    const unsigned Sp = S ^ (1u << t);
    const int in = (e ^ 1) + 2, fx = fixed[t];
    long long best = WA_ST_INF;
    if ((Sp & predmask[t]) == predmask[t] && (fx == 0 || (in & 1) == fx - 1)) {
        if (Sp == 0) {
            best = W[1 * N2 + in];
        } else {
            for (int e2 = 0; e2 < ne; e2++)
                if ((Sp >> (e2 >> 1)) & 1u) {
                    const long long p = f[(size_t)Sp * ne + e2];
                    const long long v = p + W[(e2 + 2) * N2 + in];
                    best = (p < WA_ST_INF && v < best) ? v : best;
                }
        }
    }
    f[idx] = best;
}
