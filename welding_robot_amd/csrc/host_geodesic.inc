// host_geodesic.inc -- C ABI: exact hop counts and shortest paths on the 6-neighbour lattice of free voxels (included by weldacs.hip inside extern "C"),
// and the host driver of every level-synchronous search on the bitmaps of geodesic_kernels.hpp: host_weighted.inc runs on it too.
// Levels are enqueued in blocks of WA_GEO_BLOCK launches; the per-source words last[] / stop[] are read once per block.
static const int32_t WA_GEO_BLOCK = 32;
static const int32_t WA_GEO_MAX_CHUNK = 65535;   // sources per launch: gridDim.y

static WaGeoDims geo_dims(const wa_grid *g)
{
    WaGeoDims d;
    d.nx = g->d.nx; d.ny = g->d.ny; d.nz = g->d.nz;
    d.W = (g->d.nx + 63) / 64;
    d.nw = (int64_t)d.W * g->d.ny * g->d.nz;
    d.n = g->d.n;
    return d;
}

// builds g->fbits once (under the grid's lock, like the distance field)
static int grid_build_bits(const wa_grid *g)
{
    wa_ctx *ctx = g->ctx;
    std::lock_guard<std::mutex> lock(g->fbits_mu);
    if (g->fbits) return WA_OK;
    const WaGeoDims d = geo_dims(g);
    DevBuf<unsigned long long> b;
    if (b.alloc((size_t)d.nw) != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "geodesic: bit-packed occupancy");
    k_geo_pack<<<(unsigned)((d.nw + 3) / 4), 256, 0, ctx->stream>>>(g->occ, d, b);
    hipError_t e = hipGetLastError();
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "geodesic: packing the occupancy: %s", hipGetErrorString(e));
    g->fbits = b.detach();
    return WA_OK;
}

// ids inside the grid and on free voxels, else WA_ERR_ARG (nothing has been written anywhere at that point)
static int geo_check_ids(const wa_grid *g, const char *fn, const int64_t *const *lists, int n_lists, int64_t count)
{
    wa_ctx *ctx = g->ctx;
    for (int l = 0; l < n_lists; l++)
        for (int64_t i = 0; i < count; i++)
            if (lists[l][i] < 0 || lists[l][i] >= g->d.n) return fail(ctx, WA_ERR_ARG, "%s: id outside the grid", fn);
    const int64_t N = count * n_lists;
    if (N == 0) return WA_OK;
    DevBuf<long long> d_ids;
    DevBuf<uint8_t> d_f;
    std::vector<uint8_t> f((size_t)N);
    hipError_t e = d_ids.alloc((size_t)N);
    e = e ? e : d_f.alloc((size_t)N);
    for (int l = 0; e == hipSuccess && l < n_lists; l++)
        e = hipMemcpyAsync(d_ids + l * count, lists[l], sizeof(long long) * count, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        k_geo_gather_free<<<(unsigned)((N + 255) / 256), 256, 0, ctx->stream>>>(g->occ, d_ids, N, d_f);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(f.data(), d_f, (size_t)N, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: checking ids: %s", fn, hipGetErrorString(e));
    for (int64_t i = 0; i < N; i++)
        if (!f[i]) return fail(ctx, WA_ERR_ARG, "%s: a source, start or end lies on an occupied voxel", fn);
    return WA_OK;
}

// what every search call does once its arguments are checked: the ids, then (count > 0 only) the bit-packed occupancy and the dimensions.
// The caller returns when this fails or count == 0.
static int search_begin(const wa_grid *g, const char *fn, const int64_t *const *lists, int n_lists, int32_t count, WaGeoDims *d)
{
    int rc = geo_check_ids(g, fn, lists, n_lists, count);
    if (rc || count == 0) return rc;
    rc = grid_build_bits(g);
    *d = geo_dims(g);
    return rc;
}

// device state of one chunk of sources: per source the bitmap of the voxels the search has reached, `frontiers` frontier bitmaps (source s's
// begin at fronts + s * frontiers * nw for a ring, see SearchKind), a field and a matrix row when they are kept, and the words last / stop
struct SearchChunk {
    int32_t cap = 0;                       // sources the buffers hold
    DevBuf<unsigned long long> seen, fronts;
    DevBuf<int32_t> field, mat, last, stop;
    DevBuf<long long> src;
};

// What tells one search from another.  The driver runs: seed(c, ns), then launches level(c, ns, L, d_tgt, n_tgt) for L = first, first + 1, ...
// in blocks of WA_GEO_BLOCK, and goes on while a source has !stop[s] && last[s] >= L - window for the next L (what the level kernels ask
// themselves).  Both functions enqueue one kernel on the context's stream.  The driver does not look into the sources: they are the kind's
// keys (voxel ids for the searches over voxels; host_pose.inc packs a pin beside the id), copied to c.src and handed to seed.
struct SearchKind {
    const char *fn;        // the exported function, in front of every message
    int32_t frontiers;     // frontier bitmaps per source: 2 for hops, W + 1 for the weighted ring
    int32_t zeroed;        // how many of them a search needs zeroed (per source, the first ones): the level kernels write the others whole
    int32_t window;
    int64_t words, ints;   // the size of one bitmap in 64-bit words and of one source's field in int32: d.nw and d.n for the searches over voxels
    int64_t first, bound;  // the first level, and one the loop must not pass (WA_ERR_STATE)
    std::function<void(const SearchChunk &, int32_t)> seed;
    std::function<void(const SearchChunk &, int32_t, int64_t, const long long *, int32_t)> level;
};

// The memory rule (DESIGN 4j): a source costs frontiers + 1 bitmaps of k.words words, a field of k.ints int32 when one is kept and a matrix row; a
// chunk takes at most half of what wa_ctx_memory_info reports free behind the bit-packed occupancy, at least one source, at most
// WA_GEO_MAX_CHUNK, WA_GEO_CHUNK forces fewer, and is halved while the device refuses the allocation.
static int search_chunk_alloc(const wa_grid *g, const WaGeoDims &d, const SearchKind &k, int32_t n_src, bool with_field, int32_t n_tgt, SearchChunk *c)
{
    wa_ctx *ctx = g->ctx;
    int64_t free_b = 0;
    int rc = wa_ctx_memory_info(ctx, &free_b, nullptr);
    if (rc) return rc;
    const int64_t per = (int64_t)(k.frontiers + 1) * k.words * 8 + (with_field ? k.ints * 4 : 0) + (int64_t)n_tgt * 4 + 16;
    int64_t cap = (free_b / 2) / per;
    cap = std::max<int64_t>(1, std::min<int64_t>(cap, std::min<int64_t>(n_src, WA_GEO_MAX_CHUNK)));
    if (const int forced = env_int("WA_GEO_CHUNK", 0)) cap = std::max<int64_t>(1, std::min<int64_t>(cap, forced));   // (tests: several chunks on a small grid)
    for (;; cap = (cap + 1) / 2) {
        SearchChunk t;   // (a refused attempt gives back what it got when t goes)
        hipError_t e = t.seen.alloc((size_t)(cap * k.words));
        e = e ? e : t.fronts.alloc((size_t)(cap * k.frontiers * k.words));
        if (e == hipSuccess && with_field) e = t.field.alloc((size_t)(cap * k.ints));
        if (e == hipSuccess && n_tgt > 0) e = t.mat.alloc((size_t)(cap * n_tgt));
        e = e ? e : t.last.alloc((size_t)cap);
        e = e ? e : t.stop.alloc((size_t)cap);
        e = e ? e : t.src.alloc((size_t)cap);
        if (e == hipSuccess) { t.cap = (int32_t)cap; *c = std::move(t); return WA_OK; }
        (void)hipGetLastError();
        if (cap == 1) return fail(ctx, WA_ERR_ALLOC, "%s: the buffers of one source do not fit the device", k.fn);
    }
}

// the search from ns sources (host ids) in chunk c: fills c->field / c->mat rows 0 .. ns-1.  d_tgt: the matrix's targets on the device.
static int search_run(const wa_grid *g, const WaGeoDims &d, const SearchKind &k, const SearchChunk &c, const int64_t *src, int32_t ns,
                      const long long *d_tgt, int32_t n_tgt)
{
    wa_ctx *ctx = g->ctx;
    hipError_t e = hipMemcpyAsync(c.src, src, sizeof(long long) * ns, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(c.seen, 0, sizeof(unsigned long long) * (size_t)(ns * k.words), ctx->stream);
    e = e ? e : hipMemsetAsync(c.fronts, 0, sizeof(unsigned long long) * (size_t)((int64_t)ns * k.zeroed * k.words), ctx->stream);
    if (e == hipSuccess && c.field) e = hipMemsetAsync(c.field, 0xff, sizeof(int32_t) * (size_t)(ns * k.ints), ctx->stream);   // WA_HOPS_NONE / WA_DIST_NONE
    if (e == hipSuccess && c.mat) e = hipMemsetAsync(c.mat, 0xff, sizeof(int32_t) * (size_t)ns * n_tgt, ctx->stream);
    if (e == hipSuccess) {
        k.seed(c, ns);
        e = hipGetLastError();
    }
    std::vector<int32_t> last((size_t)ns), stop((size_t)ns);
    int64_t level = k.first;
    bool alive = true;
    while (e == hipSuccess && alive) {
        if (level > k.bound) return fail(ctx, WA_ERR_STATE, "%s: the search ran more levels than it can have", k.fn);
        for (int32_t i = 0; i < WA_GEO_BLOCK && e == hipSuccess; i++, level++) {
            k.level(c, ns, level, d_tgt, n_tgt);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(last.data(), c.last, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(stop.data(), c.stop, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        alive = false;
        for (int32_t s = 0; s < ns && !alive; s++) alive = !stop[s] && last[s] >= level - k.window;
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: the search: %s", k.fn, hipGetErrorString(e));
    return WA_OK;
}

// the loop of all six entry points: the sources in chunks, each chunk searched, then rows(c, s0, ns) takes what it wants of the ns rows
// of c.field / c.mat, which belong to sources s0 .. s0 + ns - 1
static int search_chunks(const wa_grid *g, const WaGeoDims &d, const SearchKind &k, const int64_t *src, int32_t n_src, bool with_field,
                         const long long *d_tgt, int32_t n_tgt, const std::function<int(const SearchChunk &, int32_t, int32_t)> &rows)
{
    SearchChunk c;
    int rc = search_chunk_alloc(g, d, k, n_src, with_field, n_tgt, &c);
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_src; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_src - s0);
        rc = search_run(g, d, k, c, src + s0, ns, d_tgt, n_tgt);
        rc = rc ? rc : rows(c, s0, ns);
    }
    return rc;
}

// the _fields (points == false: rows of d.n voxels) and _matrix (rows of n_src points, which are the targets too) calls behind their checks
static int search_rows(const wa_grid *g, const WaGeoDims &d, const SearchKind &k, const int64_t *src, int32_t n_src, bool points, int32_t *out)
{
    wa_ctx *ctx = g->ctx;
    DevBuf<long long> d_tgt;
    if (points) {
        hipError_t e = d_tgt.alloc((size_t)n_src);
        e = e ? e : hipMemcpyAsync(d_tgt, src, sizeof(long long) * n_src, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "%s: %s", k.fn, hipGetErrorString(e));
    }
    const int64_t row = points ? n_src : d.n;
    return search_chunks(g, d, k, src, n_src, !points, d_tgt, points ? n_src : 0, [&](const SearchChunk &c, int32_t s0, int32_t ns) {
        const hipError_t e = hipMemcpy(out + s0 * row, points ? c.mat : c.field, sizeof(int32_t) * (size_t)(ns * row), hipMemcpyDeviceToHost);
        return e == hipSuccess ? WA_OK : fail(ctx, WA_ERR_DEVICE, "%s: %s", k.fn, hipGetErrorString(e));
    });
}

// The two passes over the pairs of a chunk, which tell one _paths call from the other.  count enqueues what it needs and returns with
// the host arrays dist[] and len[] filled (len: the nodes of the path, anything where dist < 0); write enqueues the kernel that puts
// pair i's nodes at d_out + d_dst[i] (d_dst[i] < 0: nothing).
struct PathSteps {
    const char *need;   // how many ids a pair's range must hold, in the caller's terms (for the WA_ERR_CAPACITY message)
    std::function<hipError_t(const SearchChunk &, const int32_t *, const long long *, int32_t, int32_t *, int32_t *)> count;   // (c, d_slot, d_end, np, dist, len)
    std::function<hipError_t(const SearchChunk &, const int32_t *, const long long *, const long long *, int32_t, long long *)> write;   // (c, d_slot, d_end, d_dst, np, d_out)
};

// The PathSteps of a walk-back kernel that is both passes (host_weighted.inc, host_chamfer.inc): launch(c, d_slot, d_end, d_dst, np,
// d_dist, d_len, d_out) enqueues it, as the counting pass with d_dst = d_out = NULL.  The counts stay on the device in *counts, which the
// caller keeps until search_paths returns: the writing pass reads them there.
struct WalkbackCounts { DevBuf<int32_t> dist, len; };
typedef std::function<void(const SearchChunk &, const int32_t *, const long long *, const long long *, int32_t, int32_t *, int32_t *, long long *)> WalkbackLaunch;

static PathSteps walkback_steps(wa_ctx *ctx, WalkbackCounts *counts, const WalkbackLaunch &launch)
{
    PathSteps steps;
    steps.need = "len_out";
    steps.count = [=](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *dist, int32_t *len) {
        hipError_t e = counts->dist.alloc((size_t)np);
        e = e ? e : counts->len.alloc((size_t)np);
        if (e != hipSuccess) return e;
        launch(c, d_slot, d_end, nullptr, np, counts->dist, counts->len, nullptr);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(dist, counts->dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(len, counts->len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        return e ? e : hipStreamSynchronize(ctx->stream);
    };
    steps.write = [=](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        launch(c, d_slot, d_end, d_dst, np, counts->dist, counts->len, d_out);
        return hipGetLastError();
    };
    return steps;
}

// the _paths calls behind their checks: one field per distinct start; dist_out (and len_out, when not NULL) of every pair, then the nodes of
// the pairs whose range [off[p], off[p + 1]) holds them
static int search_paths(const wa_grid *g, const WaGeoDims &d, const SearchKind &k, const PathSteps &steps, const int64_t *start_ids,
                        const int64_t *end_ids, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    wa_ctx *ctx = g->ctx;
    // pairs grouped by start, in the order of first appearance
    std::vector<int64_t> starts;
    std::vector<std::vector<int32_t>> by_start;
    {
        std::unordered_map<int64_t, int32_t> seen;
        for (int32_t p = 0; p < n_pairs; p++) {
            const auto it = seen.emplace(start_ids[p], (int32_t)starts.size());
            if (it.second) { starts.push_back(start_ids[p]); by_start.emplace_back(); }
            by_start[it.first->second].push_back(p);
        }
    }
    bool short_range = false;
    std::vector<int32_t> pairs, slot, dist, len;
    std::vector<long long> ends, dst, out;
    const int rc = search_chunks(g, d, k, starts.data(), (int32_t)starts.size(), true, nullptr, 0, [&](const SearchChunk &c, int32_t s0, int32_t ns) {
        pairs.clear(); slot.clear(); ends.clear();
        for (int32_t s = 0; s < ns; s++)
            for (int32_t p : by_start[s0 + s]) { pairs.push_back(p); slot.push_back(s); ends.push_back(end_ids[p]); }
        const int32_t np = (int32_t)pairs.size();
        dist.resize((size_t)np); len.resize((size_t)np); dst.resize((size_t)np);
        DevBuf<int32_t> d_slot;
        DevBuf<long long> d_end, d_dst, d_out;
        hipError_t e = d_slot.alloc((size_t)np);
        e = e ? e : d_end.alloc((size_t)np);
        e = e ? e : d_dst.alloc((size_t)np);
        e = e ? e : hipMemcpyAsync(d_slot, slot.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, ctx->stream);
        e = e ? e : hipMemcpyAsync(d_end, ends.data(), sizeof(long long) * np, hipMemcpyHostToDevice, ctx->stream);
        e = e ? e : steps.count(c, d_slot, d_end, np, dist.data(), len.data());
        int64_t total = 0;
        if (e == hipSuccess) {
            for (int32_t i = 0; i < np; i++) {
                const int32_t p = pairs[i];
                dist_out[p] = dist[i];
                if (len_out) len_out[p] = len[i];
                dst[i] = -1;
                if (dist[i] < 0) continue;                                                     // unreachable: nothing to write, no error
                if ((int64_t)len[i] > off[p + 1] - off[p]) { short_range = true; continue; }   // reported once every pair has its counts
                dst[i] = total;
                total += len[i];
            }
            out.resize((size_t)total);
            e = d_out.alloc((size_t)std::max<int64_t>(total, 1));
            e = e ? e : hipMemcpyAsync(d_dst, dst.data(), sizeof(long long) * np, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e == hipSuccess && total > 0) {
            e = steps.write(c, d_slot, d_end, d_dst, np, d_out);
            e = e ? e : hipMemcpyAsync(out.data(), d_out, sizeof(long long) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
            e = e ? e : hipStreamSynchronize(ctx->stream);
        }
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "%s: %s", k.fn, hipGetErrorString(e));
        // only each pair's path: the rest of its range in the caller's buffer stays as it was
        for (int32_t i = 0; i < np; i++)
            if (dst[i] >= 0) memcpy(ids_out + off[pairs[i]], out.data() + dst[i], sizeof(int64_t) * (size_t)len[i]);
        return (int)WA_OK;
    });
    if (rc == WA_OK && short_range)
        return fail(ctx, WA_ERR_CAPACITY, "%s: a pair's range is shorter than its path (%s ids are needed)", k.fn, steps.need);
    return rc;
}

// the argument checks of a _paths call behind its NULL checks (the offsets, then search_begin on both id lists)
static int paths_begin(const wa_grid *g, const char *fn, const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs, const int64_t *off, WaGeoDims *d)
{
    for (int32_t p = 0; p < n_pairs; p++)
        if (off[p + 1] < off[p]) return fail(g->ctx, WA_ERR_ARG, "%s: offsets decrease", fn);
    const int64_t *lists[2] = {start_ids, end_ids};
    return search_begin(g, fn, lists, 2, n_pairs, d);
}

// breadth-first search: `seen` is the visited bitmap, the two frontiers of all sources lie behind one another (level L reads the one
// L - 1 wrote and writes the other whole, so only the first is zeroed)
static SearchKind geo_kind(const wa_grid *g, const WaGeoDims &d, const char *fn)
{
    SearchKind k;
    k.fn = fn;
    k.frontiers = 2; k.zeroed = 1; k.window = 1;
    k.words = d.nw; k.ints = d.n;
    // a search of F free voxels has at most F - 1 productive levels; one more launch looks at the last frontier
    k.first = 1; k.bound = g->n_free + 1;
    hipStream_t st = g->ctx->stream;
    k.seed = [=](const SearchChunk &c, int32_t ns) {
        k_geo_seed<<<(unsigned)((ns + 255) / 256), 256, 0, st>>>(c.src, ns, d, c.seen, c.fronts, c.field, c.last, c.stop);
    };
    k.level = [=](const SearchChunk &c, int32_t ns, int64_t level, const long long *d_tgt, int32_t n_tgt) {
        unsigned long long *fa = c.fronts, *fb = c.fronts + (int64_t)c.cap * d.nw;
        const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
        k_geo_level<<<grid, 256, 0, st>>>(g->fbits, d, (int32_t)level, c.seen, (level & 1) ? fa : fb, (level & 1) ? fb : fa, c.field, c.last, c.stop, d_tgt, n_tgt, c.mat);
    };
    return k;
}

// wa_grid_geodesic_fields (points == false) and _matrix behind their names
static int geo_rows_call(const char *fn, const wa_grid *g, const int64_t *ids, int32_t n, bool points, int32_t *hops_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (!ids || !hops_out || n < 0) return fail(g->ctx, WA_ERR_ARG, "%s: bad argument", fn);
    WaGeoDims d;
    const int rc = search_begin(g, fn, &ids, 1, n, &d);
    if (rc || n == 0) return rc;
    return search_rows(g, d, geo_kind(g, d, fn), ids, n, points, hops_out);
}

int wa_grid_geodesic_fields(const wa_grid *g, const int64_t *src_ids, int32_t n_src, int32_t *hops_out)
{
    return geo_rows_call("wa_grid_geodesic_fields", g, src_ids, n_src, false, hops_out);
}

int wa_grid_geodesic_matrix(const wa_grid *g, const int64_t *point_ids, int32_t n_pts, int32_t *hops_out)
{
    return geo_rows_call("wa_grid_geodesic_matrix", g, point_ids, n_pts, true, hops_out);
}

int wa_grid_geodesic_paths(const wa_grid *g, const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                           const int64_t *off, int64_t *ids_out, int32_t *hops_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!start_ids || !end_ids || !off || !ids_out || !hops_out || n_pairs < 0)
        return fail(ctx, WA_ERR_ARG, "wa_grid_geodesic_paths: bad argument");
    WaGeoDims d;
    const int rc = paths_begin(g, "wa_grid_geodesic_paths", start_ids, end_ids, n_pairs, off, &d);
    if (rc || n_pairs == 0) return rc;
    DevBuf<int32_t> d_hops;
    PathSteps steps;
    steps.need = "hops_out + 1";
    steps.count = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, int32_t np, int32_t *hops, int32_t *len) {
        hipError_t e = d_hops.alloc((size_t)np);
        if (e != hipSuccess) return e;
        k_geo_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, d.n, d_slot, d_end, np, d_hops);
        e = hipGetLastError();
        e = e ? e : hipMemcpyAsync(hops, d_hops, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        for (int32_t i = 0; i < np; i++) len[i] = hops[i] + 1;
        return e;
    };
    steps.write = [&](const SearchChunk &c, const int32_t *d_slot, const long long *d_end, const long long *d_dst, int32_t np, long long *d_out) {
        k_geo_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, d, d_slot, d_end, d_dst, np, d_out);
        return hipGetLastError();
    };
    return search_paths(g, d, geo_kind(g, d, "wa_grid_geodesic_paths"), steps, start_ids, end_ids, n_pairs, off, ids_out, hops_out, nullptr);
}
