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
// grid = (B, slots), the path's NODES dealt over the blocks (B: WA_CONVERGED_BLOCKS when the solver is created): block b owns nodes [b m, (b + 1) m),
// m = ceil(best_len / B), keeps their records, heuristic values, prefix-tabu bits and rows in LDS and nobody else's.  A node's state never reads
// another node's, and no generation's state needs the verdict of the check, so per generation a block advances its own nodes and checks EVERY ant of
// the colony at them: nothing is computed twice except the control block's chain, which depends on neither records nor rows and is run for all W
// generations up front, by one wavefront, into a table in LDS (beside it the generations' draw keys).  In the loop the check (lane = ant, the rows read
// uniformly: one 64-bit ant key per ant, generation and block) and the advance (16 lanes per node, straight into the slot's snapshots at the node's own
// offset) run in different wavefronts, the rows double-buffered, behind ONE barrier per generation.  No grid barrier, no waiting on memory anywhere.
// A block at whose nodes an ant leaves the path (or dies) in generation g + t stops and reports t; a block without nodes reports W.  The block that
// finishes last (a ticket counter behind a fence) commits j = the smallest t reported, with the control block and the trace rows out of its table.
//
// The verdict also goes to the HOST (wa_conv_report): a word of pinned, coherent host memory per slot takes (seq << 8) | j from every launch that is
// given one -- from block 0 where the window does not apply (j = 0), from the committing block behind its writes otherwise.  The host reads it to leave
// out the launches of committed generations (host_acs.inc: conv_verdict); nothing on the device ever waits for the host.  Behind a window that
// committed whole the host enqueues the next window's flush before it has the verdict, marked WA_GEN_SPEC: such a flush does nothing unless the window
// committed exactly up to its generation.
//
// OWED evaporations (WA_GEN_OWED, acs_dev.hpp).  The flush of generation g + W - 1 passes over the whole field, and the sweep of the full generation g + W
// directly behind it passes over it again; between the two only the walk of generation g + W could read the field, and only through an ant that leaves
// the path.  A launch that is told to (judge) therefore tests generation g + W as well when its blocks got through all W generations: the same per-ant
// test with that generation's keys and colony (the chain is run one step further than it commits) against the rows of the last snapshot, nothing
// advanced.  If every ant of g + W replays the path the commit records the window as CARRIED in the header and in the verdict (WA_CONV_CARRIED); the
// host then leaves the flush's sweep out and has the sweep of g + W multiply W + 1 times, from the buffer the window found the field in.  The header
// keeps what a later change needs to chain windows without a field pass in between: `pending`, the evaporations owed, and `carried`.
//
// The CARRIED WALK (WA_CONVERGED_CARRIED_WALK).  The rows of a carried window's last snapshot had one reader: the walk of generation g + W, for the test
// this kernel has just made.  The host therefore enqueues nothing at all for a window it has read as carried, and that generation's walk launch, told so
// by WA_GEN_OWED, delivers every ant as a whole replay without the table (k_walk_dev, wa_walk_carried) -- when the header names its generation: `end`,
// written with every commit, so that a header an earlier window left does not qualify.  k_apply_table of g + W rebuilds every row from the records.
#pragma once

#define WA_CONV_CHECK_WAVES 4     // wavefronts of a block that check the ants (lane = ant), ...
#define WA_CONV_ADV_WAVES 4       // ... and that advance the block's nodes (16 lanes per node)
#define WA_CONV_THREADS ((WA_CONV_CHECK_WAVES + WA_CONV_ADV_WAVES) * 64)
#define WA_CONV_BLOCKS 64         // default of WA_CONVERGED_BLOCKS (profiles/converged_nodes/README.md)
#define WA_CONV_BLOCKS_MAX 256
#define WA_CONV_MAX_WINDOW 64
#define WA_CONV_NODE_CAP 1024     // longest best path a window covers (the snapshots' stride is at most this)
#define WA_CONV_NODE_LDS 128      // LDS per node a block owns: six records, six heuristic values, the prefix-tabu bits (16 floats); the row of this generation and of the next
#define WA_CONV_SNAP 14           // floats per node of a snapshot: six records + the row

struct WaConvHdr {                // head of a slot's scratch block; the snapshots follow
    uint32_t rem;                 // max over the window's blocks of 2 (W - generations the block's ants stayed on the path) + (an ant leaves in the generation behind); 0 between windows
    uint32_t ticket;              // blocks of the running window that have finished; 0 between windows
    int32_t pending;              // j of the last commit: evaporations the flush applies (or, owed, the sweep of the generation behind it)
    int32_t carried;              // the last commit was of a whole window, and every ant of the generation behind it replays the path too
    unsigned long long whole, cut, gens;   // windows committed whole / cut (0 < j < W), generations committed (wa_acs_converged_info)
    int32_t end;                  // the generation behind the last commit (gen0 + j): `carried` speaks of this generation's ants and of no other's
    int32_t pad1_;
    unsigned long long walks;     // walk launches that took the carried path (wa_acs_converged_carried_info)
    unsigned long long pad2_;
};
static_assert(WA_CONV_SNAP == 14, "wa_table_rows strides the owed records by 14 floats");
static_assert(sizeof(WaConvHdr) == 64, "the snapshots start 64 bytes into the block");

__device__ __forceinline__ WaConvHdr *wa_conv_hdr(const WaAcsDev &D, int32_t slot) { return reinterpret_cast<WaConvHdr *>(D.conv + (int64_t)slot * D.conv_stride); }
// snapshot t = the path state after t + 1 generations of the window: [node][WA_CONV_SNAP]
__device__ __forceinline__ float *wa_conv_snap(const WaAcsDev &D, int32_t slot, int32_t t)
{
    return reinterpret_cast<float *>(D.conv + (int64_t)slot * D.conv_stride + sizeof(WaConvHdr)) + (int64_t)t * D.conv_nodes * WA_CONV_SNAP;
}
__device__ __forceinline__ int32_t wa_conv_pending(const WaAcsDev &D, int32_t slot) { return wa_conv_hdr(D, slot)->pending; }
__device__ __forceinline__ bool wa_conv_carried(const WaAcsDev &D, int32_t slot) { return wa_conv_hdr(D, slot)->carried != 0; }
// Generation `gen` is the one a carried window judged: the last commit was of a whole window that ends directly in front of it, and every ant of it
// replays the best path (a header left by an earlier window names another generation and does not qualify)
__device__ __forceinline__ bool wa_conv_carried_at(const WaAcsDev &D, int32_t slot, int32_t gen)
{
    if (!D.conv) return false;
    const WaConvHdr *h = wa_conv_hdr(D, slot);
    return h->carried != 0 && h->end == gen && D.ctl[slot].spec_until == gen;
}
__device__ __forceinline__ void wa_conv_count_walk(const WaAcsDev &D, int32_t slot) { wa_conv_hdr(D, slot)->walks += 1; }   // (one lane of one block per launch)
// the path nodes' records of the last commit, [node][WA_CONV_SNAP] (the table blocks of the generation behind a carried window: wa_table_rows)
__device__ __forceinline__ const float *wa_conv_owed_records(const WaAcsDev &D, int32_t slot) { return wa_conv_snap(D, slot, wa_conv_pending(D, slot) - 1); }
#define WA_CONV_CARRIED 0x80u     // in the verdict word beside j (j <= WA_CONV_MAX_WINDOW < 128)

// the flush's table blocks: records (into D.pher, the buffer the flush sweep wrote) and rows of the path nodes from the snapshot of the commit.
// rows_only: the evaporations are owed (no sweep ran, D.pher is not the field): the records stay in the snapshot for the table blocks of the next generation
__device__ __forceinline__ void wa_conv_flush_rows(const WaAcsDev &D, int32_t slot, int32_t first, int32_t step, bool rows_only)
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
        if (q < 6) { if (!rows_only) pher[(int64_t)(bpath[i] & (int32_t)WA_ID_MASK) * 6 + q] = v; }
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
__device__ __forceinline__ void wa_conv_report(uint32_t *verdict, int32_t slot, uint32_t seq, int32_t j, bool carried = false)
{
    if (!verdict) return;
    if (j > 0) {
        __threadfence_system();
        __hip_atomic_store(verdict + slot, (seq << 8) | (carried ? WA_CONV_CARRIED : 0u) | (uint32_t)j, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else __hip_atomic_store(verdict + slot, seq << 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// wa_add_ranked for an edge that carries EVERY depositing rank or none, which is all a converged generation has (rep_mask: ranks 0..n-1 on the path's own
// edge, nothing anywhere else): p += dep[b] + bonus for b = 0..n-1 in ascending order where `on`, p as it is elsewhere -- the same adds on the same
// operands in the same order, so the bits agree with wa_add_ranked(p, on ? (1 << n) - 1 : 0, ...).  What differs is the cost of a rank: the sum
// dep[b] + bonus is formed once in lane b (the same fp32 add as behind wa_add_ranked's readlane), and with no mask to test a rank is one readlane of a
// constant lane and one add, where the general loop spends nine instructions on it (measured: profiles/converged_nodes/README.md).  Ranks are taken in
// blocks of eight; the ones at and above n add -0.0f, which leaves every value as it is, bit for bit (x + -0 == x, zeros of either sign included).
// The whole wavefront calls this together; dep_lane: lane l holds the coefficient of rank bit l.
__device__ __forceinline__ float wa_add_all_ranked(float p, bool on, float dep_lane, float bonus, int32_t n)
{
    n = __builtin_amdgcn_readfirstlane(n);
    const float t_lane = (int32_t)(threadIdx.x & 63) < n ? dep_lane + bonus : -0.f;
    float q = p;
    asm volatile("" : "+v"(q));   // the edge's record has arrived here: no add waits for a load
#pragma unroll
    for (int b0 = 0; b0 < 64; b0 += 8) {
        if (b0 >= n) break;
        float t[8];   // (eight scalars first, then the eight dependent adds: no add waits for its readlane)
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t_lane), b0 + j));
#pragma unroll
        for (int j = 0; j < 8; j++) q = q + t[j];
    }
    return on ? q : p;
}

// nodes of a path of `nodes` nodes that one of `blocks` blocks owns at most (host: the LDS a block asks for; device: where the shares start)
__host__ __device__ inline int32_t wa_conv_share(int32_t nodes, int32_t blocks) { return (nodes + blocks - 1) / blocks; }

// What a block keeps in LDS behind its nodes' state (all of it in the dynamic region, every offset a multiple of 16 bytes)
struct WaConvShared {
    WaSlotCtl tab[WA_CONV_MAX_WINDOW + 1];   // tab[t]: the control block as generation gen0 + t finds it; tab[t + 1]: as it leaves it
    unsigned long long key[WA_CONV_MAX_WINDOW + 1];   // wa_ctr_key of generation gen0 + t (t = W: the generation behind the window, when it is judged)
    int32_t bad[WA_CONV_MAX_WINDOW + 1];     // an ant left the path at one of this block's nodes in generation gen0 + t
    int32_t run;                             // generations of the window whose colony is in range (the chain stops at the first that is not)
    int32_t last, j, carried;
};
__host__ __device__ inline size_t wa_conv_lds_bytes(int32_t conv_nodes, int32_t blocks)
{
    return (size_t)wa_conv_share(conv_nodes, blocks) * WA_CONV_NODE_LDS + sizeof(WaConvShared);
}

// judge: also test generation gen0 + W (see OWED above); 0: the launch is what it was
__global__ __launch_bounds__(WA_CONV_THREADS) void k_converged_run(WaAcsDev D, WaRun R, int32_t gen0, int32_t W, uint32_t *verdict, uint32_t seq, int32_t judge)
{
    extern __shared__ __attribute__((aligned(16))) float wa_conv_lds[];
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
    // ---- this block's share of the path: nodes n0 .. n0 + mine - 1 (none: a grid of more blocks than the path has nodes)
    const int32_t cap = wa_conv_share(D.conv_nodes, nblk);   // (blen <= conv_nodes: a share never exceeds it)
    const int32_t m = wa_conv_share(blen, nblk), n0 = blk * m;
    const int32_t mine = blen - n0 < 0 ? 0 : blen - n0 < m ? blen - n0 : m;
    const int32_t last = blen - 1;                // decisions exist at nodes 0 .. blen-2: the last node has records and a row, and no edge taken
    const int32_t ndec = (n0 + mine < last ? n0 + mine : last) - n0;
    float *s_row = wa_conv_lds;                   // [2][cap][8]: the replay table's rows, generation gen0 + t in half t & 1
    float *s_rec = wa_conv_lds + cap * 16;        // [cap][16]: records 0..5, heuristic 6..11, prefix-tabu bits 12
    WaConvShared &S = *reinterpret_cast<WaConvShared *>(wa_conv_lds + cap * 32);
    {
        const int32_t *bpath = D.bestpath + (int64_t)slot * D.path_cap + n0;
        const uint8_t *btabu = D.besttabu + (int64_t)slot * D.path_cap + n0;
        const float *pher = D.pher + (int64_t)slot * D.pher_stride;
        const float *heur = D.heur + (int64_t)ctl->heur_slot * D.pher_stride;
        const float *T = D.rtab + ((int64_t)slot * D.path_cap + n0) * 8;
        for (int32_t x = tid; x < mine * 16; x += WA_CONV_THREADS) {
            const int32_t i = x >> 4, q = x & 15;
            const int64_t v = bpath[i] & (int32_t)WA_ID_MASK;
            s_rec[x] = q < 6 ? pher[v * 6 + q] : q < 12 ? heur[v * 6 + q - 6] : q == 12 ? __uint_as_float((uint32_t)btabu[i]) : 0.f;
        }
        for (int32_t x = tid; x < mine * 8; x += WA_CONV_THREADS) {
            const float v = T[x];
            s_row[x] = v;
            if ((x & 7) == 7) s_row[cap * 8 + x] = v;   // (the edge taken stays what it is: both halves hold it)
        }
    }
    // ---- the control block's chain, all W steps: it depends on neither records nor rows.  One wavefront (wa_conv_ctl_step: lane 0 writes); another one
    // forms the generations' draw keys meanwhile
    if (wave == 0) {
        if (lane == 0) S.tab[0] = *ctl;
        int32_t run = 0;
        for (; run < W; run++) {
            const int32_t gen = gen0 + run;
            const int32_t colony = S.tab[run].colony[gen & 1];
            if (!(colony >= 1 && colony <= D.max_colony)) break;   // (uniform: every lane reads the same word)
            if (lane == 0) S.tab[run + 1] = S.tab[run];
            wa_conv_ctl_step(S.tab[run + 1], R, gen);
        }
        if (lane == 0) S.run = run;
    } else if (wave == 1) {
        for (int32_t t = lane; t <= W; t += 64) {   // (W <= 64: lane 0 takes a second trip for t = 64)
            S.key[t] = wa_ctr_key(R.seed, ctl->stream, (uint32_t)(gen0 + t));
            S.bad[t] = 0;
        }
    }
    __syncthreads();
    const int32_t run = S.run;
    int32_t my_t = mine > 0 ? run : W;            // the first generation of the window in which an ant left the path at one of this block's nodes
    for (int32_t t = 0; t < run && mine > 0; t++) {
        const int32_t gen = gen0 + t;
        const int32_t colony = S.tab[t].colony[gen & 1];
        const float *row = s_row + (t & 1) * cap * 8;
        if (wave < WA_CONV_CHECK_WAVES) {
            // ---- every ant of the colony against this block's rows: the test of wa_walk_replay, one lane per ant, the row the same for all lanes
            const uint64_t genkey = S.key[t];
            for (int32_t a = tid; a < colony; a += WA_CONV_CHECK_WAVES * 64) {
                const uint64_t antkey = wa_ctr_antkey(genkey, (uint32_t)a);
                bool bad = false;
                for (int32_t n = 0; n < ndec; n++) {
                    const float4 *r4 = reinterpret_cast<const float4 *>(row + n * 8);
                    const float4 ca = r4[0], cb = r4[1];
                    const uint32_t h = wa_replay_hits(ca, cb, (int32_t)wa_ctr_draw(antkey, (uint32_t)(n0 + n)));
                    const int pick = h ? 31 - __clz((int)h) : -1;
                    bad = bad || pick != __float_as_int(cb.w);
                }
                if (bad) S.bad[t] = 1;
            }
        } else {
            // ---- generation gen is over for this block's nodes.  The path's own edge (role k2 == the edge taken): x rho (the sweep), then the ranked
            // deposits of all n_dep ranks (rep_mask: every one on the replay track); every other record x rho; the rows of the new values
            // (wa_table_rows' arithmetic, 16 lanes per node) into the other half, and all of it into snapshot t (the state after t + 1 generations)
            const WaSlotCtl &c = S.tab[t + 1];    // what the post-walk launch of generation gen publishes
            const int32_t n_dep = c.n_dep;
            const float lambda = c.dep_lambda, Q = c.dep_Q;
            const bool okl = lane < colony && lane < n_dep;
            const float dep_lane = okl ? (lambda - (float)(lane + 1)) * Q / bestL : 0.f;   // :211, rank bit l in lane l
            const float bonus_on = wa_uniform(1.f * lambda * Q / bestL);                   // second term of :211: the edge's two ends lie on the best path (:209)
            float *nrow = s_row + ((t + 1) & 1) * cap * 8;
            float *snap = wa_conv_snap(D, slot, t) + (int64_t)n0 * WA_CONV_SNAP;
            const int32_t k2 = lane & 15, kk = k2 < 6 ? k2 : 5;
            // (the trips are the wavefront's: a row past the share's end goes along on its first node and writes nothing, so that wa_add_all_ranked finds every lane there)
            for (int32_t i = (wave - WA_CONV_CHECK_WAVES) * 4 + (lane >> 4); __any(i < mine); i += WA_CONV_ADV_WAVES * 4) {
                const bool live = i < mine;
                const int32_t ii = live ? i : 0;
                const int32_t nk = __float_as_int(row[ii * 8 + 7]);   // (-1 at the path's last node: nothing is deposited there)
                float p = s_rec[ii * 16 + kk] * R.rho;
                const float h = s_rec[ii * 16 + 6 + kk];
                const uint32_t bt = __float_as_uint(s_rec[ii * 16 + 12]);
                p = wa_add_all_ranked(p, live && k2 == nk, dep_lane, bonus_on, n_dep);
                float thr, tot;
                wa_row_values(R, p, h, k2, bt, thr, tot);
                if (!live) continue;
                float *sn = snap + i * WA_CONV_SNAP;
                if (k2 < 6) {
                    s_rec[i * 16 + k2] = p;
                    nrow[i * 8 + k2] = thr;
                    sn[k2] = p;
                    sn[6 + k2] = thr;
                }
                if (k2 == 5) { nrow[i * 8 + 6] = tot; sn[12] = tot; }
                if (k2 == 0) sn[13] = __int_as_float(nk);
            }
        }
        __syncthreads();
        if (S.bad[t] != 0) { my_t = t; break; }   // (uniform over the block; bad[t] is written in front of this barrier only)
    }
    // ---- the generation behind the window, judged where the window is whole for this block: every ant of generation gen0 + W against the rows of the
    // last snapshot (in half W & 1, complete behind the loop's last barrier), with the colony the chain's last step set.  Nothing is advanced.
    int32_t leaves = 1;                           // an ant leaves the path in generation gen0 + W at one of this block's nodes, or that generation is not judged
    if (judge && run == W && my_t == W) {         // (uniform over the block)
        const int32_t gen = gen0 + W;
        const int32_t colony = S.tab[W].colony[gen & 1];
        leaves = !(colony >= 1 && colony <= D.max_colony);
        if (!leaves && mine > 0) {
            if (wave < WA_CONV_CHECK_WAVES) {
                const float *row = s_row + (W & 1) * cap * 8;
                const uint64_t genkey = S.key[W];
                for (int32_t a = tid; a < colony; a += WA_CONV_CHECK_WAVES * 64) {
                    const uint64_t antkey = wa_ctr_antkey(genkey, (uint32_t)a);
                    bool bad = false;
                    for (int32_t n = 0; n < ndec; n++) {
                        const float4 *r4 = reinterpret_cast<const float4 *>(row + n * 8);
                        const float4 ca = r4[0], cb = r4[1];
                        const uint32_t h = wa_replay_hits(ca, cb, (int32_t)wa_ctr_draw(antkey, (uint32_t)(n0 + n)));
                        const int pick = h ? 31 - __clz((int)h) : -1;
                        bad = bad || pick != __float_as_int(cb.w);
                    }
                    if (bad) S.bad[W] = 1;
                }
            }
            __syncthreads();
            leaves = S.bad[W] != 0;
        }
    }
    // ---- the block that finishes last commits
    if (tid == 0) {
        atomicMax(&hdr->rem, ((uint32_t)(W - my_t) << 1) | (uint32_t)leaves);
        __threadfence();
        const uint32_t tk = atomicAdd(&hdr->ticket, 1u);
        int32_t is_last = 0, j = 0, carried = 0;
        if (tk == (uint32_t)nblk - 1u) {
            __threadfence();
            is_last = 1;
            const uint32_t rem = atomicMax(&hdr->rem, 0u);
            j = W - (int32_t)(rem >> 1);
            carried = rem == 0u;                  // whole, and no block saw an ant leave in the generation behind
        }
        S.last = is_last;
        S.j = j;
        S.carried = carried;
    }
    __syncthreads();
    if (!S.last) return;
    const int32_t j = S.j;                        // (<= run: the block of node 0 reports no more)
    const bool carried = S.carried != 0;
    if (tid == 0) {
        hdr->rem = 0;
        hdr->ticket = 0;
        if (j > 0) {
            WaSlotCtl c = S.tab[j];               // the control block of generation gen0 + j
            c.spec_until = gen0 + j;
            *ctl = c;
            hdr->pending = j;
            hdr->carried = carried ? 1 : 0;
            hdr->end = gen0 + j;
            hdr->gens += (unsigned long long)j;
            if (j == W) hdr->whole += 1; else hdr->cut += 1;
        }
    }
    if (j > 0) {   // perm / depA as the ranking of generation gen0 + j - 1 leaves them, and the trace rows of the committed generations
        const int32_t colony = S.tab[j].colony[(gen0 + j - 1) & 1];
        const float lambda = S.tab[j].dep_lambda, Q = S.tab[j].dep_Q;
        for (int32_t r = tid; r < colony; r += WA_CONV_THREADS) {
            const int32_t o = r + 1;
            const bool ok = !(bestL == INFINITY || (float)o > lambda - 1);
            D.perm[(int64_t)slot * D.max_colony + r] = r;
            D.depA[(int64_t)slot * D.max_colony + r] = ok ? (lambda - (float)o) * Q / bestL : 0.f;
        }
        for (int32_t t = tid; t < j; t += WA_CONV_THREADS) {
            const int32_t gen = gen0 + t;
            if (gen >= D.trace_cap) continue;
            const int32_t col = S.tab[t].colony[gen & 1];
            const int64_t tr = (int64_t)slot * D.trace_cap + gen;
            D.trBest[tr] = bestL;
            D.trIter[tr] = bestL;
            D.trColony[tr] = col;
            D.trFinite[tr] = col;
            D.trSteps[tr] = (long long)col * (long long)(blen - 1);
        }
    }
    // ---- the verdict, behind this block's writes of ctl, perm, depA and the trace rows
    __syncthreads();
    if (tid == 0) wa_conv_report(verdict, slot, seq, j, carried);
}
