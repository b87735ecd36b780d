// acs_converged.hpp -- converged generations in one launch.  Part of acs_kernels.hpp (included from there, last).
//
// Once a colony has converged every ant replays the best path from start to end, and the generation's result is a function of the control block and
// of the six records of each best-path node: every ant has L = bestL, the ranking is by ant index, the deposits land on the path's own edges, the next
// replay table depends on those records alone, and the rest of the field is multiplied by rho.  k_converged_run, enqueued in front of generation g's
// walk launch, advances that small state over a WINDOW of W generations [g, g + W) in LDS, checks every ant's draws against the rows as it goes, and
// COMMITS the j <= W generations in which every ant stayed on the path: the control block of generation g + j, ctl.spec_until = g + j.  The three
// regular launches of a generation below spec_until return at their top; those of the last committed generation g + j - 1 are the FLUSH: the sweep
// blocks of k_evap_rank_mark multiply every value of the field j times (one rounding each: what j sweeps do), and the table blocks of k_apply_table
// put the path nodes' records and the table rows of generation g + j in place (wa_conv_flush_rows).  The walk of generation g + j then finds the
// field, the table, the control block and the masks as the three-launch path would have left them.
//
// grid = (WA_CONV_BLOCKS, slots), ants dealt over the blocks; every block keeps the whole path state and advances it on its own: no grid barrier,
// no waiting on memory anywhere.  A block whose ant leaves the path (or dies) in generation g + t stops and reports t; block 0 runs the whole
// window and writes, per generation, a snapshot of the path state to the slot's scratch block and the trace row.  The block that finishes last
// (a ticket counter behind a fence) commits j = the smallest t reported.
//
// The verdict also goes to the HOST (wa_conv_report): a word of pinned, coherent host memory per slot takes (seq << 8) | j from every launch that is
// given one -- from block 0 where the window does not apply (j = 0), from the committing block behind its writes otherwise.  The host reads it to leave
// out the launches of committed generations (host_acs.inc: conv_verdict); nothing on the device ever waits for the host.  Behind a window that
// committed whole the host enqueues the next window's flush before it has the verdict, marked WA_GEN_SPEC: such a flush does nothing unless the window
// committed exactly up to its generation.
#pragma once

#define WA_CONV_THREADS 1024
#define WA_CONV_BLOCKS 32
#define WA_CONV_MAX_WINDOW 64
#define WA_CONV_NODE_CAP 1024     // longest best path a window covers: 96 bytes of LDS per node (six records, six heuristic values, the prefix-tabu bits, the row)
#define WA_CONV_NODE_LDS 96
#define WA_CONV_SNAP 14           // floats per node of a snapshot: six records + the row

struct WaConvHdr {                // head of a slot's scratch block; the snapshots follow
    uint32_t rem;                 // max over the window's blocks of (W - generations the block's ants stayed on the path); 0 between windows
    uint32_t ticket;              // blocks of the running window that have finished; 0 between windows
    int32_t pending;              // j of the last commit: evaporations the flush applies
    int32_t pad_;
    unsigned long long whole, cut, gens;   // windows committed whole / cut (0 < j < W), generations committed (wa_acs_converged_info)
    unsigned long long pad2_[3];
};
static_assert(sizeof(WaConvHdr) == 64, "the snapshots start 64 bytes into the block");

__device__ __forceinline__ WaConvHdr *wa_conv_hdr(const WaAcsDev &D, int32_t slot) { return reinterpret_cast<WaConvHdr *>(D.conv + (int64_t)slot * D.conv_stride); }
// snapshot t = the path state after t + 1 generations of the window: [node][WA_CONV_SNAP]
__device__ __forceinline__ float *wa_conv_snap(const WaAcsDev &D, int32_t slot, int32_t t)
{
    return reinterpret_cast<float *>(D.conv + (int64_t)slot * D.conv_stride + sizeof(WaConvHdr)) + (int64_t)t * D.conv_nodes * WA_CONV_SNAP;
}
__device__ __forceinline__ int32_t wa_conv_pending(const WaAcsDev &D, int32_t slot) { return wa_conv_hdr(D, slot)->pending; }

// the flush's table blocks: records (into D.pher, the buffer the flush sweep wrote) and rows of the path nodes from the snapshot of the commit
__device__ __forceinline__ void wa_conv_flush_rows(const WaAcsDev &D, int32_t slot, int32_t first, int32_t step)
{
    const int32_t blen = D.ctl[slot].best_len, j = wa_conv_pending(D, slot);
    if (j < 1) return;
    const float *snap = wa_conv_snap(D, slot, j - 1);
    const int32_t *bpath = D.bestpath + (int64_t)slot * D.path_cap;
    float *pher = D.pher + (int64_t)slot * D.pher_stride;
    float *T = D.rtab + (int64_t)slot * D.path_cap * 8;
    for (int32_t x = first; x < blen * WA_CONV_SNAP; x += step) {
        const int32_t i = x / WA_CONV_SNAP, q = x - i * WA_CONV_SNAP;
        const float v = snap[x];
        if (q < 6) pher[(int64_t)(bpath[i] & (int32_t)WA_ID_MASK) * 6 + q] = v;
        else T[(int64_t)i * 8 + (q - 6)] = v;
    }
}

// What block 0 of k_evap_rank_mark publishes behind a generation in which every ant arrived over the whole best path (all L = bestL: ranks by ant
// index, every depositing rank on the replay track).  Called by one whole wavefront; lane 0 writes.
__device__ __forceinline__ void wa_conv_ctl_step(WaSlotCtl &c, const WaRun &R, int32_t gen)
{
    const int32_t lane = threadIdx.x & 63, o = lane + 1;
    const int32_t colony = c.colony[gen & 1];
    const float lambda = c.lambda[gen & 1], Q = c.Q[gen & 1], bestL = c.bestL;
    const bool ok = lane < colony && !(bestL == INFINITY || (float)o > lambda - 1);   // :200 (at most 64 ranks deposit on the fused path)
    const unsigned long long dep = __ballot(ok);
    const int32_t n_dep = dep ? 64 - (int32_t)__clzll((long long)dep) : 0;
    if (lane == 0) {
        c.dep_lambda = lambda;
        c.dep_Q = Q;
        c.dep_bestL = bestL;
        c.n_dep = n_dep;
        c.gen = gen + 1;
        c.rep_mask = n_dep >= 64 ? ~0ULL : (1ULL << n_dep) - 1ULL;
        c.clean[(gen + 1) & 1] = c.clean[gen & 1] * R.rho;
        wa_next_params(c, R, (gen + 1) & 1);
    }
}

// One lane's report of a window's verdict to the host.  j > 0: a system-scope fence and a release store -- everything this thread has seen written (a barrier in
// front makes that the block's writes of ctl, perm and depA) is visible system-wide before the word is.  j == 0: nothing was committed, so there is
// nothing to order the word behind, and the store is a plain system-scope one: no cache is written back for it (a window that commits nothing sits
// between the launches of an exploring search).  verdict: the group's first slot's word, or null (no report)
__device__ __forceinline__ void wa_conv_report(uint32_t *verdict, int32_t slot, uint32_t seq, int32_t j)
{
    if (!verdict) return;
    if (j > 0) {
        __threadfence_system();
        __hip_atomic_store(verdict + slot, (seq << 8) | (uint32_t)j, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else __hip_atomic_store(verdict + slot, seq << 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(WA_CONV_THREADS) void k_converged_run(WaAcsDev D, WaRun R, int32_t gen0, int32_t W, uint32_t *verdict, uint32_t seq)
{
    extern __shared__ float wa_conv_lds[];
    __shared__ WaSlotCtl s_c, s_c0;
    __shared__ int32_t s_bad, s_last, s_j;
    const int32_t slot = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    WaSlotCtl *ctl = &D.ctl[slot];
    WaConvHdr *hdr = wa_conv_hdr(D, slot);
    // ---- does the window apply at all?  Every block reads the same words (nothing writes them before the commit, and the commit waits for every block)
    const float bestL = ctl->bestL;
    const int32_t blen = ctl->best_len;
    bool off = bestL == INFINITY || blen < 2 || blen > D.conv_nodes || blen > WA_CONV_NODE_CAP || W < 1 || W > WA_CONV_MAX_WINDOW;
    if (D.pool_n) {   // stragglers pending in either pool: a resume block has work in generation gen0 (or the walk of gen0 - 1 is not over for the statistics)
        const WaStrag sg = wa_strag_of(D, slot);
        off = off || sg.pool_n[0] != 0 || sg.pool_n[1] != 0;
    }
    if (off) {   // (no ticket is taken on this path: block 0 reports that nothing was committed)
        if (blk == 0 && tid == 0) wa_conv_report(verdict, slot, seq, 0);
        return;
    }
    float *s_rec = wa_conv_lds;                              // [conv_nodes][16]: records 0..5, heuristic 6..11, prefix-tabu bits 12
    float *s_row = wa_conv_lds + (int64_t)D.conv_nodes * 16;  // [conv_nodes][8]: the replay table's rows
    {
        const int32_t *bpath = D.bestpath + (int64_t)slot * D.path_cap;
        const uint8_t *btabu = D.besttabu + (int64_t)slot * D.path_cap;
        const float *pher = D.pher + (int64_t)slot * D.pher_stride;
        const float *heur = D.heur + (int64_t)ctl->heur_slot * D.pher_stride;
        const float *T = D.rtab + (int64_t)slot * D.path_cap * 8;
        for (int32_t x = tid; x < blen * 16; x += WA_CONV_THREADS) {
            const int32_t i = x >> 4, q = x & 15;
            const int64_t v = bpath[i] & (int32_t)WA_ID_MASK;
            s_rec[x] = q < 6 ? pher[v * 6 + q] : q < 12 ? heur[v * 6 + q - 6] : q == 12 ? __uint_as_float((uint32_t)btabu[i]) : 0.f;
        }
        for (int32_t x = tid; x < blen * 8; x += WA_CONV_THREADS) s_row[x] = T[x];
        if (tid == 0) { s_c = *ctl; s_c0 = s_c; s_bad = 0; }
    }
    __syncthreads();
    const int32_t last = blen - 1;                // decisions exist at nodes 0 .. blen-2
    const int32_t chunks = (last + 63) >> 6;
    int32_t my_t = W;                             // the first generation of the window in which an ant of this block left the path
    for (int32_t t = 0; t < W; t++) {
        const int32_t gen = gen0 + t;
        const int32_t colony = s_c.colony[gen & 1];
        const bool col_ok = colony >= 1 && colony <= D.max_colony;
        // ---- this block's ants against the rows: the test of wa_walk_replay, one lane per node, (ant, 64 nodes) items dealt over the wavefronts
        if (col_ok && blk < colony) {
            const uint64_t genkey = wa_ctr_key(R.seed, s_c.stream, (uint32_t)gen);
            const int32_t items = ((colony - blk + nblk - 1) / nblk) * chunks;
            for (int32_t it = wave; it < items; it += WA_CONV_THREADS / 64) {
                const int32_t q = it / chunks, node = (it - q * chunks) * 64 + lane;
                const uint64_t antkey = wa_ctr_antkey(genkey, (uint32_t)(blk + nblk * q));
                const bool valid = node < last;
                const float4 *r4 = reinterpret_cast<const float4 *>(s_row + (valid ? node : 0) * 8);
                const float4 ca = r4[0], cb = r4[1];
                const uint32_t h = wa_replay_hits(ca, cb, (int32_t)wa_ctr_draw(antkey, (uint32_t)node));
                const int pick = h ? 31 - __clz((int)h) : -1;
                if (__ballot(valid && pick != __float_as_int(cb.w)) != 0 && lane == 0) s_bad = 1;
            }
        }
        __syncthreads();
        const bool bad = !col_ok || s_bad != 0;
        if (bad && my_t == W) my_t = t;
        if (!col_ok || (bad && blk != 0)) break;          // (uniform over the block)
        __syncthreads();
        // ---- generation gen is over: what the post-walk launch publishes
        if (wave == 0) {
            wa_conv_ctl_step(s_c, R, gen);
            if (lane == 0) s_bad = 0;
        }
        __syncthreads();
        // ---- the path's own edges: x rho (the sweep), then the ranked deposits of all n_dep ranks (rep_mask: every one on the replay track), one lane per node
        const int32_t n_dep = s_c.n_dep;
        const unsigned long long G = s_c.rep_mask;
        const float lambda = s_c.dep_lambda, Q = s_c.dep_Q;
        const bool okl = lane < colony && lane < n_dep;
        const float dep_lane = okl ? (lambda - (float)(lane + 1)) * Q / bestL : 0.f;   // :211, rank bit l in lane l
        const float bonus_on = wa_uniform(1.f * lambda * Q / bestL);                   // second term of :211: the edge's two ends lie on the best path (:209)
        for (int32_t i = tid; __any(i < last); i += WA_CONV_THREADS) {
            const bool live = i < last;
            const int32_t ii = live ? i : 0;
            const int32_t nk = __float_as_int(s_row[ii * 8 + 7]);
            float p = s_rec[ii * 16 + nk] * R.rho;
            p = wa_add_ranked(p, live ? G : 0ULL, dep_lane, bonus_on, n_dep);
            if (live) s_rec[ii * 16 + nk] = p;
        }
        __syncthreads();
        // ---- every other record x rho, and the rows of the new values (wa_table_rows' arithmetic, 16 lanes per node)
        {
            const int32_t k2 = tid & 15, kk = k2 < 6 ? k2 : 5;
            for (int32_t i = tid >> 4; __any(i < blen); i += WA_CONV_THREADS / 16) {
                const bool live = i < blen;
                const int32_t ii = live ? i : 0;
                const int32_t nk = __float_as_int(s_row[ii * 8 + 7]);
                float p = s_rec[ii * 16 + kk];
                const float h = s_rec[ii * 16 + 6 + kk];
                const uint32_t bt = __float_as_uint(s_rec[ii * 16 + 12]);
                if (kk != nk) p = p * R.rho;
                float thr, tot;
                wa_row_values(R, p, h, k2, bt, thr, tot);
                if (!live) continue;
                if (k2 < 6) { s_rec[i * 16 + k2] = p; s_row[i * 8 + k2] = thr; }
                if (k2 == 5) s_row[i * 8 + 6] = tot;
            }
        }
        __syncthreads();
        if (blk == 0) {   // snapshot t (the state after t + 1 generations) and the trace row of generation gen
            float *snap = wa_conv_snap(D, slot, t);
            for (int32_t x = tid; x < blen * WA_CONV_SNAP; x += WA_CONV_THREADS) {
                const int32_t i = x / WA_CONV_SNAP, q = x - i * WA_CONV_SNAP;
                snap[x] = q < 6 ? s_rec[i * 16 + q] : s_row[i * 8 + (q - 6)];
            }
            if (tid == 0 && gen < D.trace_cap) {
                const int64_t tr = (int64_t)slot * D.trace_cap + gen;
                D.trBest[tr] = bestL;
                D.trIter[tr] = bestL;
                D.trColony[tr] = colony;
                D.trFinite[tr] = colony;
                D.trSteps[tr] = (long long)colony * (long long)(blen - 1);
            }
        }
    }
    // ---- the block that finishes last commits
    if (tid == 0) {
        atomicMax(&hdr->rem, (uint32_t)(W - my_t));
        __threadfence();
        const uint32_t tk = atomicAdd(&hdr->ticket, 1u);
        int32_t is_last = 0, j = 0;
        if (tk == (uint32_t)nblk - 1u) {
            __threadfence();
            is_last = 1;
            j = W - (int32_t)atomicMax(&hdr->rem, 0u);
        }
        s_last = is_last;
        s_j = j;
    }
    __syncthreads();
    if (!s_last) return;
    const int32_t j = s_j;
    if (wave == 0) {
        for (int32_t t = 0; t < j; t++) wa_conv_ctl_step(s_c0, R, gen0 + t);   // (the control block of generation gen0 + j, from the one the window found)
        if (lane == 0) {
            hdr->rem = 0;
            hdr->ticket = 0;
            if (j > 0) {
                s_c0.spec_until = gen0 + j;
                *ctl = s_c0;
                hdr->pending = j;
                hdr->gens += (unsigned long long)j;
                if (j == W) hdr->whole += 1; else hdr->cut += 1;
            }
        }
    }
    __syncthreads();
    if (j > 0) {   // perm / depA as the ranking of generation gen0 + j - 1 leaves them
        const int32_t colony = s_c0.colony[(gen0 + j - 1) & 1];
        const float lambda = s_c0.dep_lambda, Q = s_c0.dep_Q;
        for (int32_t r = tid; r < colony; r += WA_CONV_THREADS) {
            const int32_t o = r + 1;
            const bool ok = !(bestL == INFINITY || (float)o > lambda - 1);
            D.perm[(int64_t)slot * D.max_colony + r] = r;
            D.depA[(int64_t)slot * D.max_colony + r] = ok ? (lambda - (float)o) * Q / bestL : 0.f;
        }
    }
    // ---- the verdict, behind this block's writes of ctl, perm and depA
    __syncthreads();
    if (tid == 0) wa_conv_report(verdict, slot, seq, j);
}
