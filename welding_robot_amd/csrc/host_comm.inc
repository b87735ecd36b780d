// host_comm.inc -- C ABI: the multi-GPU exchange of north_star (included by weldacs.hip inside extern "C").
// Problems are sharded one set per GPU (one process or host thread per device); there is no data-path collective.  The exchanges
// of SURVEY 8(e), all RCCL over xGMI on the communicator's own stream: (1) per generation the global-best path cost WITH its owner
// (ACSRank_3D.hpp:263-264 is the per-generation best each rank would publish) -- an all-reduce (ncclMin) of one packed 64-bit key,
// overlapped with the next generations; (2) at the end of a sharded pair-planning run the per-pair costs to every rank
// (size-prefixed all-gather) and (3) the paths to the rank that stitches (size-prefixed send / receive).
// No torch, no MPI: the caller ships the 128-byte id from rank 0 to the others.
struct wa_comm {
    wa_ctx *ctx;
    ncclComm_t nccl;
    int32_t rank, world;
    hipStream_t stream;     // side stream of the exchanges
    hipEvent_t ready;       // "the generations enqueued so far are done" (recorded on the solver's stream)
    unsigned long long *gkey;   // device: global best per generation as a packed key (cost bits << 32 | owner), see wa_comm_pack_best_key
    int32_t gcap;
    std::vector<uint8_t> exchanged;   // host: generation g has been through wa_acs_allreduce_best
    double *d_tmp;          // device staging of wa_comm_allreduce_f64
    int32_t tmp_cap;
    // the paths rank `root` received in the last wa_comm_gather_paths (host copies, read by wa_comm_gathered_paths_read)
    std::vector<int32_t> gp_index, gp_ids;
    std::vector<int64_t> gp_len;
    void *scratch;          // device staging of the blocking exchanges below: one block that only grows
    size_t scratch_bytes;
    long long *hdr;         // device: the header rows of every exchange, 8 x (world + 1) words, allocated with the communicator -- joining a
                            // header exchange never needs memory (a rank that cannot allocate must still be able to say so)
    bool aborted;           // wa_comm_abort, or a wait that gave up: the RCCL communicator is gone, every later call fails at once
    double timeout_s;       // WA_COMM_TIMEOUT_S (read by wa_comm_create; 600; 0 = wait for ever): bound of every wait on the exchange stream
    int64_t n_allreduce, n_other;   // collectives issued (wa_comm_stats)
    int32_t fail_scratch_in;        // (-DWA_TEST_KNOBS: the n-th comm_scratch call from now on fails; 0 = off)
};

static int comm_fail(wa_ctx *ctx, const char *what, ncclResult_t r)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, ncclGetErrorString(r));
    return fail(ctx, WA_ERR_DEVICE, "%s", buf);
}
#define NCCLC(ctx, call)                                                     \
    do {                                                                     \
        ncclResult_t r_ = (call);                                            \
        if (r_ != ncclSuccess) return comm_fail((ctx), #call, r_);           \
    } while (0)

// Every wait on the exchange stream is bounded and watches the communicator: a peer that died (RCCL reports it asynchronously) or never
// arrives (timeout) makes this rank give the communicator up -- ncclCommAbort ends the collective kernels that are still waiting -- and
// return WA_ERR_DEVICE instead of blocking for ever (SURVEY 8(b): never hang, status codes).  The communicator is unusable afterwards
// (every call returns WA_ERR_STATE); the caller decides whether the process goes on without its peers or exits non-zero.
static void comm_give_up(wa_comm *c)
{
    if (c->nccl) { ncclCommAbort(c->nccl); c->nccl = nullptr; }
    c->aborted = true;
    if (c->stream) hipStreamSynchronize(c->stream);   // (the aborted kernels leave at once)
}
static int comm_wait(wa_comm *c, const char *what)
{
    wa_ctx *ctx = c->ctx;
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    for (;;) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); comm_give_up(c); return fail(ctx, WA_ERR_DEVICE, "%s: the exchange stream failed", what); }
        (void)hipGetLastError();
        if ((++spins & 63) == 0) {
            ncclResult_t ae = ncclSuccess;
            if (c->nccl && (ncclCommGetAsyncError(c->nccl, &ae) != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress))) {
                comm_give_up(c);
                return comm_fail(ctx, what, ae == ncclSuccess ? ncclSystemError : ae);
            }
            const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (c->timeout_s > 0 && t > c->timeout_s) {
                comm_give_up(c);
                return fail(ctx, WA_ERR_DEVICE, "%s: no answer from the other ranks within WA_COMM_TIMEOUT_S; communicator aborted", what);
            }
        }
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));   // (the first ~2000 polls spin: the usual exchange is over within them)
    }
    ncclResult_t ae = ncclSuccess;
    if (c->nccl && ncclCommGetAsyncError(c->nccl, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) { comm_give_up(c); return comm_fail(ctx, what, ae); }
    return WA_OK;
}
#define COMM_LIVE(c) do { if ((c)->aborted || !(c)->nccl) return fail((c)->ctx, WA_ERR_STATE, "wa_comm: the communicator was aborted"); } while (0)

// The global best as ONE orderable word (SURVEY 8(e)): a path cost is a non-negative float or +inf, whose bit patterns order like
// unsigned integers; the low word names the owner -- rank << 16 | slot -- so that a MIN over ranks yields the best cost AND who holds
// the path that achieved it (ties: the lowest rank, then the lowest slot).
#define WA_OWNER_SLOT_BITS 16
__host__ __device__ inline unsigned long long wa_best_key(float cost, int32_t rank, int32_t slot)
{
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(cost);
#else
    memcpy(&b, &cost, 4);
#endif
    return ((unsigned long long)b << 32) | (unsigned long long)(((uint32_t)rank << WA_OWNER_SLOT_BITS) | ((uint32_t)slot & ((1u << WA_OWNER_SLOT_BITS) - 1u)));
}

// out[g] = MIN over the active slots of key(best_L[gen0 + g], rank, slot)   (one thread per generation; slots are few)
__global__ void k_min_key_over_slots(const float *__restrict__ trBest, int32_t trace_cap, int32_t n_active, int32_t gen0, int32_t count,
                                     int32_t rank, unsigned long long *__restrict__ out)
{
    const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    unsigned long long m = ~0ULL;
    for (int32_t q = 0; q < n_active; q++) {
        const unsigned long long k = wa_best_key(trBest[(int64_t)q * trace_cap + gen0 + g], rank, q);
        m = k < m ? k : m;
    }
    out[gen0 + g] = m;
}

int wa_comm_pack_best_key(float cost, int32_t rank, int32_t slot, uint64_t *key)
{
    if (!key || !(cost >= 0) || rank < 0 || rank >= (1 << (31 - WA_OWNER_SLOT_BITS)) || slot < 0 || slot >= (1 << WA_OWNER_SLOT_BITS)) return WA_ERR_ARG;
    *key = (uint64_t)wa_best_key(cost, rank, slot);
    return WA_OK;
}
int wa_comm_unpack_best_key(uint64_t key, float *cost, int32_t *rank, int32_t *slot)
{
    const uint32_t b = (uint32_t)(key >> 32), o = (uint32_t)key;
    if (cost) memcpy(cost, &b, 4);
    if (rank) *rank = (int32_t)(o >> WA_OWNER_SLOT_BITS);
    if (slot) *slot = (int32_t)(o & ((1u << WA_OWNER_SLOT_BITS) - 1u));
    return WA_OK;
}

int wa_comm_unique_id(uint8_t id_out[WA_COMM_ID_BYTES])
{
    static_assert(WA_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    if (!id_out) return WA_ERR_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return WA_ERR_DEVICE;
    memcpy(id_out, id.internal, WA_COMM_ID_BYTES);
    return WA_OK;
}

int wa_comm_create(wa_ctx *ctx, int32_t rank, int32_t world, const uint8_t id_in[WA_COMM_ID_BYTES], wa_comm **out)
{
    if (!ctx || !out || !id_in || world < 1 || rank < 0 || rank >= world) return fail(ctx, WA_ERR_ARG, "wa_comm_create: bad argument");
    *out = nullptr;
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    wa_comm *c = new wa_comm();
    c->ctx = ctx; c->nccl = nullptr; c->rank = rank; c->world = world; c->stream = nullptr; c->ready = nullptr;
    c->gkey = nullptr; c->gcap = 0; c->d_tmp = nullptr; c->tmp_cap = 0; c->scratch = nullptr; c->scratch_bytes = 0;
    c->hdr = nullptr; c->aborted = false; c->n_allreduce = c->n_other = 0; c->fail_scratch_in = 0;
    { const char *v = getenv("WA_COMM_TIMEOUT_S"); c->timeout_s = v && *v ? atof(v) : 600.0; }
    if (rank >= (1 << (31 - WA_OWNER_SLOT_BITS))) { delete c; return fail(ctx, WA_ERR_ARG, "wa_comm_create: rank does not fit the owner word"); }
    ncclUniqueId id;
    memcpy(id.internal, id_in, WA_COMM_ID_BYTES);
    ncclResult_t r = ncclCommInitRank(&c->nccl, world, id, rank);   // collective over all ranks
    if (r != ncclSuccess) { delete c; return comm_fail(ctx, "ncclCommInitRank", r); }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    e = e ? e : dev_malloc((void **)&c->hdr, sizeof(long long) * 8 * (size_t)(world + 1));
    e = e ? e : hipEventCreateWithFlags(&c->ready, hipEventDisableTiming);
    if (e != hipSuccess) { wa_comm_destroy(c); return fail(ctx, WA_ERR_DEVICE, "wa_comm_create: %s", hipGetErrorString(e)); }
    *out = c;
    return WA_OK;
}

void wa_comm_destroy(wa_comm *c)
{
    if (!c) return;
    WaDevGuard dev_guard_(c->ctx);
    if (c->stream && !c->aborted) hipStreamSynchronize(c->stream);
    if (c->nccl) ncclCommDestroy(c->nccl);
    if (c->ready) hipEventDestroy(c->ready);
    if (c->stream) hipStreamDestroy(c->stream);
    dev_free(c->gkey);
    dev_free(c->d_tmp);
    dev_free(c->scratch);
    dev_free(c->hdr);
    delete c;
}

// Give the communicator up NOW (ncclCommAbort): collectives in flight end, every later call on it returns WA_ERR_STATE.  For a host that
// has learnt by other means that a peer is gone.  wa_comm_destroy still has to be called.
int wa_comm_abort(wa_comm *c)
{
    if (!c) return WA_ERR_ARG;
    WaDevGuard dev_guard_(c->ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    comm_give_up(c);
    return WA_OK;
}

// [0] ranks as RCCL itself counts them (ncclCommCount: what the library was told is in wa_comm_info), [1] RCCL's version code
// (ncclGetVersion), [2] all-reduce calls issued on this communicator, [3] other collectives / sends / receives issued, [4] 1 once aborted
int wa_comm_stats(wa_comm *c, int64_t out[5])
{
    if (!c || !out) return WA_ERR_ARG;
    int n = 0, v = 0;
    if (c->nccl && ncclCommCount(c->nccl, &n) != ncclSuccess) n = -1;
    if (ncclGetVersion(&v) != ncclSuccess) v = -1;
    out[0] = n; out[1] = v; out[2] = c->n_allreduce; out[3] = c->n_other; out[4] = c->aborted ? 1 : 0;
    return WA_OK;
}

int wa_comm_info(const wa_comm *c, int32_t *rank, int32_t *world)
{
    if (!c) return WA_ERR_ARG;
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    return WA_OK;
}

int wa_acs_allreduce_best(wa_acs *s, wa_comm *c, int32_t gen0, int32_t count)
{
    if (!s || !c || gen0 < 0 || count < 1) return WA_ERR_ARG;
    wa_ctx *ctx = s->ctx;
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    COMM_LIVE(c);
    if (c->ctx->device != ctx->device) return fail(ctx, WA_ERR_ARG, "wa_acs_allreduce_best: solver and communicator live on different devices");
    const int64_t end = (int64_t)gen0 + count;
    if (!s->begun || end > s->D.trace_cap || end > s->gens_enqueued)
        return fail(ctx, WA_ERR_STATE, "wa_acs_allreduce_best: generations not enqueued yet");
    if (s->n_active > (1 << WA_OWNER_SLOT_BITS)) return fail(ctx, WA_ERR_ARG, "wa_acs_allreduce_best: more active slots than the owner word holds");
    if (end > c->gcap) {   // grow the history (rare: once per run length)
        { const int wrc = comm_wait(c, "wa_acs_allreduce_best"); if (wrc) return wrc; }
        int64_t cap = c->gcap ? c->gcap : 256;
        while (cap < end) cap *= 2;
        unsigned long long *fresh = nullptr;
        if (dalloc(&fresh, (size_t)cap)) return fail(ctx, WA_ERR_ALLOC, "wa_acs_allreduce_best: history");
        if (c->gkey) { HIPC(ctx, hipMemcpy(fresh, c->gkey, sizeof(unsigned long long) * c->gcap, hipMemcpyDeviceToDevice)); dev_free(c->gkey); }
        c->gkey = fresh;
        c->gcap = (int32_t)cap;
    }
    // the exchange waits for the generations enqueued so far and runs beside the ones enqueued after this call
    HIPC(ctx, hipEventRecord(c->ready, ctx->stream));
    HIPC(ctx, hipStreamWaitEvent(c->stream, c->ready, 0));
    k_min_key_over_slots<<<(count + 255) / 256, 256, 0, c->stream>>>(s->D.trBest, s->D.trace_cap, s->n_active, gen0, count, c->rank, c->gkey);
    HIPC(ctx, hipGetLastError());
    NCCLC(ctx, ncclAllReduce(c->gkey + gen0, c->gkey + gen0, (size_t)count, ncclUint64, ncclMin, c->nccl, c->stream));
    c->n_allreduce++;
    if ((int64_t)c->exchanged.size() < end) c->exchanged.resize((size_t)end, 0);
    for (int64_t g = gen0; g < end; g++) c->exchanged[(size_t)g] = 1;
    return WA_OK;
}

// wait for the exchanges enqueued so far and fetch keys [gen0, gen0 + count): only generations that HAVE been exchanged can be read
static int comm_read_keys(wa_comm *c, int32_t gen0, int32_t count, std::vector<unsigned long long> &keys)
{
    if (!c || gen0 < 0 || count < 1) return WA_ERR_ARG;
    const int64_t end = (int64_t)gen0 + count;
    if (end > (int64_t)c->exchanged.size()) return fail(c->ctx, WA_ERR_STATE, "wa_comm_read_best: range never exchanged");
    for (int64_t g = gen0; g < end; g++)
        if (!c->exchanged[(size_t)g]) return fail(c->ctx, WA_ERR_STATE, "wa_comm_read_best: range never exchanged");
    COMM_LIVE(c);
    { const int wrc = comm_wait(c, "wa_comm_read_best"); if (wrc) return wrc; }
    keys.resize((size_t)count);
    HIPC(c->ctx, hipMemcpy(keys.data(), c->gkey + gen0, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost));
    return WA_OK;
}

int wa_comm_read_best(wa_comm *c, int32_t gen0, int32_t count, float *out)
{
    if (!c || !out) return WA_ERR_ARG;
    return wa_comm_read_best_owner(c, gen0, count, out, nullptr, nullptr);
}

int wa_comm_read_best_owner(wa_comm *c, int32_t gen0, int32_t count, float *cost, int32_t *owner_rank, int32_t *owner_slot)
{
    if (!c) return WA_ERR_ARG;
    WaDevGuard dev_guard_(c->ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    std::vector<unsigned long long> keys;
    int rc = comm_read_keys(c, gen0, count, keys);
    if (rc) return rc;
    for (int32_t g = 0; g < count; g++)
        wa_comm_unpack_best_key((uint64_t)keys[(size_t)g], cost ? cost + g : nullptr, owner_rank ? owner_rank + g : nullptr, owner_slot ? owner_slot + g : nullptr);
    return WA_OK;
}

// ---- end of a sharded pair-planning run (ACSRank_3D.hpp:481-483 stores every pair's cost and path; ACS_GTSP.hpp:286-298 reads them
// all on one rank): the per-pair costs to every rank, the paths to the rank that stitches.  Both are size-prefixed: an all-gather of the
// counts first, then the padded records.
// The communicator's device staging block (the exchanges below are blocking and rare): ONE block that only grows -- a hipFree per call
// would stall whatever allocates next behind the driver's wipe (profiles/r04/alloc_after_free.txt).  The previous exchange has been
// waited for when this is called.
static int comm_scratch(wa_comm *c, size_t bytes, void **out)
{
    *out = nullptr;
    if (bytes < 16) bytes = 16;
#ifdef WA_TEST_KNOBS
    if (c->fail_scratch_in > 0 && --c->fail_scratch_in == 0) return fail(c->ctx, WA_ERR_ALLOC, "wa_comm: staging (forced failure: wa_test_comm_fail_scratch)");
#endif
    if (bytes > c->scratch_bytes) {
        dev_free(c->scratch);
        c->scratch = nullptr; c->scratch_bytes = 0;
        const size_t want = bytes + bytes / 2;
        if (dev_malloc(&c->scratch, want) != hipSuccess) return fail(c->ctx, WA_ERR_ALLOC, "wa_comm: staging");
        c->scratch_bytes = want;
    }
    *out = c->scratch;
    return WA_OK;
}

// Every exchange starts with an all-gather of a small header that ALSO carries each rank's verdict on its own arguments: a rank that
// finds its arguments bad still joins the header exchange (with the error flag set), and every rank leaves with an error together --
// a rank that returned before the collective would leave its peers blocked in it.  Nothing a rank does in front of the all-gather can
// keep it from joining (ADVICE / VERDICT r05): the rows live in a block allocated with the communicator, and this rank's row is filled
// with all-ones first -- every flag word set -- so that even a failed upload of its header reads as "this rank is in trouble" to the
// others.  A buffer whose size is only known after the headers is allocated by every rank and the verdicts exchanged the same way
// (comm_agree_alloc) before anybody enters the collective that needs it.  words: 4 or 8 per rank.
static int comm_headers_n(wa_comm *c, const long long *mine, int words, std::vector<long long> &all, const char *what)
{
    wa_ctx *ctx = c->ctx;
    const int32_t W = c->world;
    long long *d = c->hdr;
    all.assign((size_t)words * W, 0);
    hipError_t e = hipMemsetAsync(d + (size_t)words * W, 0xff, sizeof(long long) * (size_t)words, c->stream);
    { const hipError_t e2 = hipMemcpyAsync(d + (size_t)words * W, mine, sizeof(long long) * (size_t)words, hipMemcpyHostToDevice, c->stream); e = e ? e : e2; }
    const ncclResult_t nr = ncclAllGather(d + (size_t)words * W, d, (size_t)words, ncclInt64, c->nccl, c->stream);   // (joined whatever happened above)
    c->n_other++;
    { const hipError_t e2 = hipMemcpyAsync(all.data(), d, sizeof(long long) * (size_t)words * (size_t)W, hipMemcpyDeviceToHost, c->stream); e = e ? e : e2; }
    if (nr != ncclSuccess) { (void)hipStreamSynchronize(c->stream); return comm_fail(ctx, what, nr); }
    const int wrc = comm_wait(c, what);
    if (wrc) return wrc;
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_DEVICE, "wa_comm header exchange: %s", hipGetErrorString(e)); }
    return WA_OK;
}
static int comm_headers(wa_comm *c, const long long mine[4], std::vector<long long> &all, const char *what)
{
    return comm_headers_n(c, mine, 4, all, what);
}
// every rank tried to allocate what the next step needs (rc_mine = its own result): all of them go on, or all of them return WA_ERR_ALLOC
static int comm_agree_alloc(wa_comm *c, int rc_mine, const char *what)
{
    const long long v[4] = {rc_mine ? 1 : 0, 0, 0, 0};
    std::vector<long long> oks;
    const int rc = comm_headers(c, v, oks, what);
    if (rc) return rc;
    if (rc_mine) return rc_mine;   // (the message of this rank's own failure stands)
    for (int32_t r = 0; r < c->world; r++)
        if (oks[(size_t)4 * r]) return fail(c->ctx, WA_ERR_ALLOC, "wa_comm: another rank could not allocate its staging buffer");
    return WA_OK;
}

int wa_comm_allgather_costs(wa_comm *c, int32_t n_mine, const int32_t *index_mine, const float *cost_mine, int32_t n_total, float *all)
{
    if (!c) return WA_ERR_ARG;
    WaDevGuard dev_guard_(c->ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    COMM_LIVE(c);
    wa_ctx *ctx = c->ctx;
    const int32_t W = c->world;
    // this rank's verdict on its own arguments travels with its count
    const char *bad = nullptr;
    if (n_mine < 0 || n_total < 0 || (n_mine > 0 && (!index_mine || !cost_mine)) || (n_total > 0 && !all)) bad = "wa_comm_allgather_costs: bad argument";
    for (int32_t i = 0; !bad && i < n_mine; i++)
        if (index_mine[i] < 0 || index_mine[i] >= n_total) bad = "wa_comm_allgather_costs: index out of range";
    // 1. the headers: (count, error flag, n_total, 0)
    const long long hdr[4] = {bad ? 0 : n_mine, bad ? 1 : 0, n_total, 0};
    std::vector<long long> hs;
    int rc = comm_headers(c, hdr, hs, "ncclAllGather (counts)");
    if (rc) return rc;
    if (bad) return fail(ctx, WA_ERR_ARG, "%s", bad);
    int32_t maxn = 0;
    for (int32_t r = 0; r < W; r++) {
        if (hs[(size_t)4 * r + 1]) return fail(ctx, WA_ERR_ARG, "wa_comm_allgather_costs: another rank reported bad arguments");
        if (hs[(size_t)4 * r + 2] != n_total) return fail(ctx, WA_ERR_ARG, "wa_comm_allgather_costs: the ranks disagree on n_total");
        maxn = (int32_t)hs[(size_t)4 * r] > maxn ? (int32_t)hs[(size_t)4 * r] : maxn;
    }
    if (maxn == 0) return WA_OK;
    // 2. the records, padded to the largest count: (pair index << 32 | cost bits)
    std::vector<unsigned long long> mine((size_t)maxn, ~0ULL), got((size_t)maxn * W);
    for (int32_t i = 0; i < n_mine; i++) {
        uint32_t b;
        memcpy(&b, &cost_mine[i], 4);
        mine[(size_t)i] = ((unsigned long long)(uint32_t)index_mine[i] << 32) | b;
    }
    unsigned long long *d_rec = nullptr;
    rc = comm_agree_alloc(c, comm_scratch(c, sizeof(unsigned long long) * (size_t)maxn * (size_t)(W + 1), (void **)&d_rec), "ncclAllGather (cost staging)");
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(d_rec + (size_t)maxn * W, mine.data(), sizeof(unsigned long long) * (size_t)maxn, hipMemcpyHostToDevice, c->stream);
    const ncclResult_t nr = ncclAllGather(d_rec + (size_t)maxn * W, d_rec, (size_t)maxn, ncclUint64, c->nccl, c->stream);   // (joined even if the upload failed: the error is returned below)
    c->n_other++;
    { const hipError_t e2 = hipMemcpyAsync(got.data(), d_rec, sizeof(unsigned long long) * (size_t)maxn * W, hipMemcpyDeviceToHost, c->stream); e = e ? e : e2; }
    if (nr != ncclSuccess) { (void)hipStreamSynchronize(c->stream); return comm_fail(ctx, "ncclAllGather (costs)", nr); }
    rc = comm_wait(c, "wa_comm_allgather_costs");
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_comm_allgather_costs: %s", hipGetErrorString(e));
    for (int32_t r = 0; r < W; r++)
        for (int32_t i = 0; i < (int32_t)hs[(size_t)4 * r]; i++) {
            const unsigned long long k = got[(size_t)r * maxn + i];
            const uint32_t idx = (uint32_t)(k >> 32), b = (uint32_t)k;
            if (idx >= (uint32_t)n_total) return fail(ctx, WA_ERR_ARG, "wa_comm_allgather_costs: a rank sent an index outside n_total");
            memcpy(&all[idx], &b, 4);
        }
    return WA_OK;
}

int wa_comm_gather_paths(wa_comm *c, int32_t root, int32_t n_mine, const int32_t *index_mine, const int64_t *len_mine, const int32_t *ids_mine,
                         int64_t *n_paths_total, int64_t *n_ids_total)
{
    if (!c) return WA_ERR_ARG;
    WaDevGuard dev_guard_(c->ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    COMM_LIVE(c);
    wa_ctx *ctx = c->ctx;
    const int32_t W = c->world;
    c->gp_index.clear(); c->gp_len.clear(); c->gp_ids.clear();   // whatever happens below, the previous gather's paths are gone
    if (n_paths_total) *n_paths_total = 0;
    if (n_ids_total) *n_ids_total = 0;
    const char *bad = nullptr;
    if (root < 0 || root >= W || n_mine < 0 || (n_mine > 0 && (!index_mine || !len_mine))) bad = "wa_comm_gather_paths: bad argument";
    int64_t my_ids = 0;
    for (int32_t i = 0; !bad && i < n_mine; i++) {
        if (len_mine[i] < 0 || len_mine[i] > 0x7fffffff) bad = "wa_comm_gather_paths: path length";
        else my_ids += len_mine[i];
    }
    if (!bad && my_ids > 0 && !ids_mine) bad = "wa_comm_gather_paths: bad argument";
    // 1. the headers: (paths, ids, error flag, root) of every rank, to every rank
    const long long hdr[4] = {bad ? 0 : n_mine, bad ? 0 : my_ids, bad ? 1 : 0, root};
    std::vector<long long> cnt;
    int rc = comm_headers(c, hdr, cnt, "ncclAllGather (path counts)");
    if (rc) return rc;
    if (bad) return fail(ctx, WA_ERR_ARG, "%s", bad);
    int64_t tot_p = 0, tot_i = 0;
    for (int32_t r = 0; r < W; r++) {
        if (cnt[(size_t)4 * r + 2]) return fail(ctx, WA_ERR_ARG, "wa_comm_gather_paths: another rank reported bad arguments");
        if (cnt[(size_t)4 * r + 3] != root) return fail(ctx, WA_ERR_ARG, "wa_comm_gather_paths: the ranks disagree on the root");
        tot_p += cnt[(size_t)4 * r];
        tot_i += cnt[(size_t)4 * r + 1];
    }
    // 2. the tables (index, length as two int32) and the ids: every other rank sends, the root receives at its running offsets
    std::vector<int32_t> tab((size_t)2 * n_mine);
    for (int32_t i = 0; i < n_mine; i++) { tab[(size_t)2 * i] = index_mine[i]; tab[(size_t)2 * i + 1] = (int32_t)len_mine[i]; }
    // every rank allocates what its side of the transfer needs and the verdicts are exchanged BEFORE anybody sends or receives: a sender whose
    // partner had returned with "out of memory" would wait for ever
    const size_t words = (size_t)2 * tot_p + (size_t)tot_i;
    int32_t *d_buf = nullptr;
    {
        const size_t need = c->rank == root ? sizeof(int32_t) * words : sizeof(int32_t) * ((size_t)2 * n_mine + (size_t)my_ids);
        rc = comm_agree_alloc(c, comm_scratch(c, need, (void **)&d_buf), "ncclAllGather (path staging)");
        if (rc) return rc;
    }
    if (c->rank != root) {
        if (n_mine == 0) return WA_OK;
        hipError_t e = hipMemcpyAsync(d_buf, tab.data(), sizeof(int32_t) * 2 * (size_t)n_mine, hipMemcpyHostToDevice, c->stream);
        if (my_ids) { const hipError_t e2 = hipMemcpyAsync(d_buf + 2 * (size_t)n_mine, ids_mine, sizeof(int32_t) * (size_t)my_ids, hipMemcpyHostToDevice, c->stream); e = e ? e : e2; }
        const ncclResult_t nr = ncclSend(d_buf, (size_t)2 * n_mine + (size_t)my_ids, ncclInt32, root, c->nccl, c->stream);   // (sent even if an upload failed: the root is waiting)
        c->n_other++;
        if (nr != ncclSuccess) { (void)hipStreamSynchronize(c->stream); return comm_fail(ctx, "ncclSend (paths)", nr); }
        rc = comm_wait(c, "wa_comm_gather_paths (send)");
        if (rc) return rc;
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_comm_gather_paths: %s", hipGetErrorString(e));
        return WA_OK;
    }
    // root: one receive per sending rank (a rank's message = its table followed by its ids), grouped
    int32_t *d_all = d_buf;
    std::vector<size_t> off((size_t)W + 1, 0);
    for (int32_t r = 0; r < W; r++) off[(size_t)r + 1] = off[(size_t)r] + (size_t)2 * cnt[(size_t)4 * r] + (size_t)cnt[(size_t)4 * r + 1];
    ncclResult_t nr = ncclGroupStart();
    for (int32_t r = 0; r < W && nr == ncclSuccess; r++)
        if (r != root && cnt[(size_t)4 * r] > 0) { nr = ncclRecv(d_all + off[(size_t)r], off[(size_t)r + 1] - off[(size_t)r], ncclInt32, r, c->nccl, c->stream); c->n_other++; }
    { ncclResult_t ge = ncclGroupEnd(); nr = nr != ncclSuccess ? nr : ge; }
    std::vector<int32_t> all(words);
    hipError_t e = hipSuccess;
    if (words) e = hipMemcpyAsync(all.data(), d_all, sizeof(int32_t) * words, hipMemcpyDeviceToHost, c->stream);
    if (nr != ncclSuccess) { (void)hipStreamSynchronize(c->stream); return comm_fail(ctx, "ncclRecv (paths)", nr); }
    rc = comm_wait(c, "wa_comm_gather_paths (receive)");
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_comm_gather_paths: %s", hipGetErrorString(e));
    // (the root's own paths never leave the host)
    if (n_mine) memcpy(all.data() + off[(size_t)root], tab.data(), sizeof(int32_t) * 2 * (size_t)n_mine);
    if (my_ids) memcpy(all.data() + off[(size_t)root] + 2 * (size_t)n_mine, ids_mine, sizeof(int32_t) * (size_t)my_ids);
    std::vector<int32_t> gi, gd;
    std::vector<int64_t> gl;
    gi.reserve((size_t)tot_p); gl.reserve((size_t)tot_p); gd.reserve((size_t)tot_i);
    for (int32_t r = 0; r < W; r++) {
        const int32_t *t = all.data() + off[(size_t)r];
        const int64_t np = cnt[(size_t)4 * r];
        int64_t sum = 0;
        for (int64_t i = 0; i < np; i++) {
            if (t[2 * i + 1] < 0) return fail(ctx, WA_ERR_ARG, "wa_comm_gather_paths: a rank sent a negative length");
            gi.push_back(t[2 * i]);
            gl.push_back(t[2 * i + 1]);
            sum += t[2 * i + 1];
        }
        if (sum != cnt[(size_t)4 * r + 1]) return fail(ctx, WA_ERR_ARG, "wa_comm_gather_paths: a rank's lengths do not add up to its prefix");
        gd.insert(gd.end(), t + 2 * np, t + 2 * np + sum);
    }
    c->gp_index.swap(gi); c->gp_len.swap(gl); c->gp_ids.swap(gd);   // only a complete gather becomes readable
    if (n_paths_total) *n_paths_total = tot_p;
    if (n_ids_total) *n_ids_total = tot_i;
    return WA_OK;
}

// what the last wa_comm_gather_paths left on this rank (the root: every rank's paths; elsewhere 0, 0): size the buffers of
// wa_comm_gathered_paths_read by these
int wa_comm_gathered_paths_counts(const wa_comm *c, int64_t *n_paths, int64_t *n_ids)
{
    if (!c) return WA_ERR_ARG;
    if (n_paths) *n_paths = (int64_t)c->gp_index.size();
    if (n_ids) *n_ids = (int64_t)c->gp_ids.size();
    return WA_OK;
}

// ---- the occupancy grid to every rank (SURVEY 8(e): ncclBroadcast of occ + the three axis tables, once).  Rank `root` voxelised or
// read its grid (model_grid_map.hpp:223-268 is the O(triangles x voxels) step N1 replaced); the others receive a replica into a grid of
// their own instead of repeating that step: a 32-byte header first (dimensions, precision, wall, free count, the root's verdict), then
// the four arrays in one group.  grid = the root's grid (ignored elsewhere); *out = a new grid on every rank but the root (NULL there:
// the root keeps using its own).  Collective: every rank of the communicator calls it.
int wa_comm_broadcast_grid(wa_comm *c, int32_t root, const wa_grid *grid, wa_grid **out)
{
    if (!c || !out) return WA_ERR_ARG;
    *out = nullptr;
    WaDevGuard dev_guard_(c->ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    COMM_LIVE(c);
    wa_ctx *ctx = c->ctx;
    const bool am_root = c->rank == root;
    const bool bad = root < 0 || root >= c->world || (am_root && (!grid || grid->ctx->device != ctx->device));
    // header: nx, ny, nz, wall, precision bits, n_free, error flag, 0 -- every rank contributes its verdict, the root's row carries the grid
    long long hdr[8] = {0, 0, 0, 0, 0, 0, bad ? 1 : 0, 0};
    if (am_root && !bad) {
        uint32_t pb;
        memcpy(&pb, &grid->precision, 4);
        hdr[0] = grid->d.nx; hdr[1] = grid->d.ny; hdr[2] = grid->d.nz; hdr[3] = grid->wall; hdr[4] = pb; hdr[5] = grid->n_free;
    }
    const int32_t W = c->world;
    std::vector<long long> all;
    int rc = comm_headers_n(c, hdr, 8, all, "ncclAllGather (grid header)");
    if (rc) return rc;
    if (bad) return fail(ctx, WA_ERR_ARG, "wa_comm_broadcast_grid: bad argument");
    for (int32_t r = 0; r < W; r++)
        if (all[(size_t)8 * r + 6]) return fail(ctx, WA_ERR_ARG, "wa_comm_broadcast_grid: another rank reported bad arguments");
    const long long *h = all.data() + (size_t)8 * root;
    const int32_t nx = (int32_t)h[0], ny = (int32_t)h[1], nz = (int32_t)h[2];
    wa_grid *g = nullptr;
    if (!am_root) {
        // (every rank sees the same header: a grid the root could build is one this rank can describe; only the allocation can fail here,
        //  and that verdict is exchanged too, below, before anybody enters the broadcasts)
        std::vector<float> zx((size_t)nx, 0.f), zy((size_t)ny, 0.f), zz((size_t)nz, 0.f);
        uint32_t pb = (uint32_t)h[4];
        float precision;
        memcpy(&precision, &pb, 4);
        if (grid_alloc(ctx, nx, ny, nz, zx.data(), zy.data(), zz.data(), precision, (int32_t)h[3], &g) != WA_OK) g = nullptr;
    }
    const long long ok_hdr[4] = {(am_root || g) ? 0 : 1, 0, 0, 0};
    std::vector<long long> oks;
    rc = comm_headers(c, ok_hdr, oks, "ncclAllGather (grid allocation)");
    bool everybody = rc == WA_OK;
    for (int32_t r = 0; everybody && r < W; r++) everybody = oks[(size_t)4 * r] == 0;
    if (!everybody) {
        if (g) wa_grid_destroy(g);
        return rc ? rc : fail(ctx, WA_ERR_ALLOC, "wa_comm_broadcast_grid: a rank could not allocate its replica");
    }
    // the root's arrays may still be being written on its context's stream
    // (a failure here is reported AFTER the broadcasts: the other ranks are on their way into them)
    hipError_t pe = hipEventRecord(c->ready, ctx->stream);
    pe = pe ? pe : hipStreamWaitEvent(c->stream, c->ready, 0);
    const wa_grid *src = am_root ? grid : g;
    ncclResult_t nr = ncclGroupStart();
    if (nr == ncclSuccess) nr = ncclBroadcast(src->occ, src->occ, (size_t)nx * ny * nz, ncclUint8, root, c->nccl, c->stream);
    if (nr == ncclSuccess) nr = ncclBroadcast(src->cx, src->cx, (size_t)nx, ncclFloat32, root, c->nccl, c->stream);
    if (nr == ncclSuccess) nr = ncclBroadcast(src->cy, src->cy, (size_t)ny, ncclFloat32, root, c->nccl, c->stream);
    if (nr == ncclSuccess) nr = ncclBroadcast(src->cz, src->cz, (size_t)nz, ncclFloat32, root, c->nccl, c->stream);
    { ncclResult_t ge = ncclGroupEnd(); nr = nr != ncclSuccess ? nr : ge; }
    c->n_other += 4;
    if (nr != ncclSuccess) (void)hipStreamSynchronize(c->stream);
    const int wrc = nr != ncclSuccess ? comm_fail(ctx, "ncclBroadcast (grid)", nr) : comm_wait(c, "wa_comm_broadcast_grid");
    if (wrc || pe != hipSuccess) {
        if (g) wa_grid_destroy(g);
        return wrc ? wrc : fail(ctx, WA_ERR_DEVICE, "wa_comm_broadcast_grid: %s", hipGetErrorString(pe));
    }
    if (g) {
        g->n_free = h[5];
        *out = g;
    }
    return WA_OK;
}

int wa_comm_gathered_paths_read(wa_comm *c, int32_t *index_out, int64_t *len_out, int32_t *ids_out)
{
    if (!c) return WA_ERR_ARG;
    if (index_out && !c->gp_index.empty()) memcpy(index_out, c->gp_index.data(), sizeof(int32_t) * c->gp_index.size());
    if (len_out && !c->gp_len.empty()) memcpy(len_out, c->gp_len.data(), sizeof(int64_t) * c->gp_len.size());
    if (ids_out && !c->gp_ids.empty()) memcpy(ids_out, c->gp_ids.data(), sizeof(int32_t) * c->gp_ids.size());
    return WA_OK;
}

int wa_comm_allreduce_f64(wa_comm *c, double *inout, int32_t count, int32_t op)
{
    if (!c || !inout || count < 1 || op < WA_COMM_MIN || op > WA_COMM_SUM) return WA_ERR_ARG;
    WaDevGuard dev_guard_(c->ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;
    COMM_LIVE(c);
    if (count > c->tmp_cap) {
        { const int wrc = comm_wait(c, "wa_comm_allreduce_f64"); if (wrc) return wrc; }
        dev_free(c->d_tmp);
        c->d_tmp = nullptr; c->tmp_cap = 0;
        if (dalloc(&c->d_tmp, (size_t)count)) return fail(c->ctx, WA_ERR_ALLOC, "wa_comm_allreduce_f64: staging");
        c->tmp_cap = count;
    }
    const ncclRedOp_t nop = op == WA_COMM_MIN ? ncclMin : op == WA_COMM_MAX ? ncclMax : ncclSum;
    HIPC(c->ctx, hipMemcpyAsync(c->d_tmp, inout, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    NCCLC(c->ctx, ncclAllReduce(c->d_tmp, c->d_tmp, (size_t)count, ncclDouble, nop, c->nccl, c->stream));
    c->n_allreduce++;
    HIPC(c->ctx, hipMemcpyAsync(inout, c->d_tmp, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    return comm_wait(c, "wa_comm_allreduce_f64");
}

#ifdef WA_TEST_KNOBS
// (knobs build only, tests/test_gpu_mock_ranks.py) the n-th staging allocation of this communicator from now on fails: a rank that runs out of
// memory INSIDE an exchange, behind the first header round
int wa_test_comm_fail_scratch(wa_comm *c, int32_t n)
{
    if (!c) return WA_ERR_ARG;
    c->fail_scratch_in = n;
    return WA_OK;
}
#endif

int wa_comm_barrier(wa_comm *c)
{
    double one = 1.0;
    return wa_comm_allreduce_f64(c, &one, 1, WA_COMM_SUM);
}
