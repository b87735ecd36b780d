// host_geodesic.inc -- C ABI: exact hop counts and shortest paths on the 6-neighbour lattice of free voxels (included by weldacs.hip inside extern "C")
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
    unsigned long long *b = nullptr;
    if (dalloc(&b, (size_t)d.nw) != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "geodesic: bit-packed occupancy");
    k_geo_pack<<<(unsigned)((d.nw + 3) / 4), 256, 0, ctx->stream>>>(g->occ, d, b);
    hipError_t e = hipGetLastError();
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { hipFree(b); return fail(ctx, WA_ERR_DEVICE, "geodesic: packing the occupancy: %s", hipGetErrorString(e)); }
    g->fbits = b;
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
    long long *d_ids = nullptr;
    uint8_t *d_f = nullptr;
    std::vector<uint8_t> f((size_t)N);
    hipError_t e = dalloc(&d_ids, (size_t)N);
    e = e ? e : dalloc(&d_f, (size_t)N);
    for (int l = 0; e == hipSuccess && l < n_lists; l++)
        e = hipMemcpyAsync(d_ids + l * count, lists[l], sizeof(long long) * count, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        k_geo_gather_free<<<(unsigned)((N + 255) / 256), 256, 0, ctx->stream>>>(g->occ, d_ids, N, d_f);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(f.data(), d_f, (size_t)N, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    hipFree(d_ids); hipFree(d_f);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "geodesic: checking ids: %s", hipGetErrorString(e));
    for (int64_t i = 0; i < N; i++)
        if (!f[i]) return fail(ctx, WA_ERR_ARG, "%s: a source, start or end lies on an occupied voxel", fn);
    return WA_OK;
}

// device state of one chunk of sources
struct GeoChunk {
    int32_t cap = 0;                       // sources the buffers hold
    unsigned long long *vis = nullptr, *fa = nullptr, *fb = nullptr;
    int32_t *field = nullptr, *mat = nullptr, *last = nullptr, *stop = nullptr;
    long long *src = nullptr;
    void release()
    {
        hipFree(vis); hipFree(fa); hipFree(fb); hipFree(field); hipFree(mat); hipFree(last); hipFree(stop); hipFree(src);
        vis = fa = fb = nullptr; field = mat = last = stop = nullptr; src = nullptr; cap = 0;
    }
};

// The memory rule (DESIGN 4j): a source costs three bitmaps (visited, two frontiers), a field of 4 bytes per voxel when one is kept and a
// matrix row; a chunk takes at most half of what wa_ctx_memory_info reports free behind the bit-packed occupancy, at least one source,
// at most WA_GEO_MAX_CHUNK, and is halved while the device refuses the allocation.
static int geo_chunk_alloc(const wa_grid *g, const WaGeoDims &d, int32_t n_src, bool with_field, int32_t n_tgt, GeoChunk *c)
{
    wa_ctx *ctx = g->ctx;
    int64_t free_b = 0;
    int rc = wa_ctx_memory_info(ctx, &free_b, nullptr);
    if (rc) return rc;
    const int64_t per = 3 * d.nw * 8 + (with_field ? d.n * 4 : 0) + (int64_t)n_tgt * 4 + 16;
    int64_t cap = (free_b / 2) / per;
    cap = std::max<int64_t>(1, std::min<int64_t>(cap, std::min<int64_t>(n_src, WA_GEO_MAX_CHUNK)));
    if (const int forced = env_int("WA_GEO_CHUNK", 0)) cap = std::max<int64_t>(1, std::min<int64_t>(cap, forced));   // (tests: several chunks on a small grid)
    for (;;) {
        hipError_t e = dalloc(&c->vis, (size_t)(cap * d.nw));
        e = e ? e : dalloc(&c->fa, (size_t)(cap * d.nw));
        e = e ? e : dalloc(&c->fb, (size_t)(cap * d.nw));
        if (e == hipSuccess && with_field) e = dalloc(&c->field, (size_t)(cap * d.n));
        if (e == hipSuccess && n_tgt > 0) e = dalloc(&c->mat, (size_t)(cap * n_tgt));
        e = e ? e : dalloc(&c->last, (size_t)cap);
        e = e ? e : dalloc(&c->stop, (size_t)cap);
        e = e ? e : dalloc(&c->src, (size_t)cap);
        if (e == hipSuccess) { c->cap = (int32_t)cap; return WA_OK; }
        (void)hipGetLastError();
        c->release();
        if (cap == 1) return fail(ctx, WA_ERR_ALLOC, "geodesic: the buffers of one source do not fit the device");
        cap = (cap + 1) / 2;
    }
}

// breadth-first search from ns sources (host ids) in chunk c: fills c->field / c->mat rows 0 .. ns-1.  d_tgt: the matrix's targets on the device.
static int geo_search(const wa_grid *g, const WaGeoDims &d, GeoChunk *c, const int64_t *src, int32_t ns, const long long *d_tgt, int32_t n_tgt)
{
    wa_ctx *ctx = g->ctx;
    hipError_t e = hipMemcpyAsync(c->src, src, sizeof(long long) * ns, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(c->vis, 0, sizeof(unsigned long long) * (size_t)(ns * d.nw), ctx->stream);
    e = e ? e : hipMemsetAsync(c->fa, 0, sizeof(unsigned long long) * (size_t)(ns * d.nw), ctx->stream);
    if (e == hipSuccess && c->field) e = hipMemsetAsync(c->field, 0xff, sizeof(int32_t) * (size_t)(ns * d.n), ctx->stream);   // WA_HOPS_NONE
    if (e == hipSuccess && c->mat) e = hipMemsetAsync(c->mat, 0xff, sizeof(int32_t) * (size_t)ns * n_tgt, ctx->stream);
    if (e == hipSuccess) {
        k_geo_seed<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(c->src, ns, d, c->vis, c->fa, c->field, c->last, c->stop);
        e = hipGetLastError();
    }
    std::vector<int32_t> last((size_t)ns), stop((size_t)ns);
    const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
    // a search of F free voxels has at most F - 1 productive levels; one more launch looks at the last frontier
    const int64_t bound = g->n_free + 1;
    int64_t level = 1;
    bool alive = true;
    while (e == hipSuccess && alive) {
        if (level > bound) return fail(ctx, WA_ERR_STATE, "geodesic: more levels than free voxels");
        for (int32_t k = 0; k < WA_GEO_BLOCK && e == hipSuccess; k++, level++) {
            unsigned long long *cur = (level & 1) ? c->fa : c->fb, *nxt = (level & 1) ? c->fb : c->fa;
            k_geo_level<<<grid, 256, 0, ctx->stream>>>(g->fbits, d, (int32_t)level, c->vis, cur, nxt, c->field, c->last, c->stop, d_tgt, n_tgt, c->mat);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(last.data(), c->last, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(stop.data(), c->stop, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        alive = false;
        for (int32_t s = 0; s < ns && !alive; s++) alive = !stop[s] && last[s] == level - 1;
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "geodesic search: %s", hipGetErrorString(e));
    return WA_OK;
}

int wa_grid_geodesic_fields(const wa_grid *g, const int64_t *src_ids, int32_t n_src, int32_t *hops_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!src_ids || !hops_out || n_src < 0) return fail(ctx, WA_ERR_ARG, "wa_grid_geodesic_fields: bad argument");
    int rc = geo_check_ids(g, "wa_grid_geodesic_fields", &src_ids, 1, n_src);
    if (rc || n_src == 0) return rc;
    rc = grid_build_bits(g);
    if (rc) return rc;
    const WaGeoDims d = geo_dims(g);
    GeoChunk c;
    rc = geo_chunk_alloc(g, d, n_src, true, 0, &c);
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_src; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_src - s0);
        rc = geo_search(g, d, &c, src_ids + s0, ns, nullptr, 0);
        if (rc == WA_OK) {
            const hipError_t e = hipMemcpy(hops_out + (int64_t)s0 * d.n, c.field, sizeof(int32_t) * (size_t)(ns * d.n), hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_geodesic_fields: %s", hipGetErrorString(e));
        }
    }
    c.release();
    return rc;
}

int wa_grid_geodesic_matrix(const wa_grid *g, const int64_t *point_ids, int32_t n_pts, int32_t *hops_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!point_ids || !hops_out || n_pts < 0) return fail(ctx, WA_ERR_ARG, "wa_grid_geodesic_matrix: bad argument");
    int rc = geo_check_ids(g, "wa_grid_geodesic_matrix", &point_ids, 1, n_pts);
    if (rc || n_pts == 0) return rc;
    rc = grid_build_bits(g);
    if (rc) return rc;
    const WaGeoDims d = geo_dims(g);
    long long *d_tgt = nullptr;
    hipError_t e = dalloc(&d_tgt, (size_t)n_pts);
    e = e ? e : hipMemcpyAsync(d_tgt, point_ids, sizeof(long long) * n_pts, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { hipFree(d_tgt); return fail(ctx, WA_ERR_ALLOC, "wa_grid_geodesic_matrix: %s", hipGetErrorString(e)); }
    GeoChunk c;
    rc = geo_chunk_alloc(g, d, n_pts, false, n_pts, &c);
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_pts; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_pts - s0);
        rc = geo_search(g, d, &c, point_ids + s0, ns, d_tgt, n_pts);
        if (rc == WA_OK) {
            e = hipMemcpy(hops_out + (int64_t)s0 * n_pts, c.mat, sizeof(int32_t) * (size_t)ns * n_pts, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_geodesic_matrix: %s", hipGetErrorString(e));
        }
    }
    c.release();
    hipFree(d_tgt);
    return rc;
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
    for (int32_t p = 0; p < n_pairs; p++)
        if (off[p + 1] < off[p]) return fail(ctx, WA_ERR_ARG, "wa_grid_geodesic_paths: offsets decrease");
    const int64_t *lists[2] = {start_ids, end_ids};
    int rc = geo_check_ids(g, "wa_grid_geodesic_paths", lists, 2, n_pairs);
    if (rc || n_pairs == 0) return rc;
    rc = grid_build_bits(g);
    if (rc) return rc;
    const WaGeoDims d = geo_dims(g);
    // pairs grouped by start: one field per distinct start, in the order of first appearance
    std::vector<int64_t> starts;
    std::vector<int32_t> pair_start((size_t)n_pairs);
    {
        std::unordered_map<int64_t, int32_t> seen;
        for (int32_t p = 0; p < n_pairs; p++) {
            auto it = seen.find(start_ids[p]);
            if (it == seen.end()) {
                it = seen.emplace(start_ids[p], (int32_t)starts.size()).first;
                starts.push_back(start_ids[p]);
            }
            pair_start[p] = it->second;
        }
    }
    const int32_t n_starts = (int32_t)starts.size();
    std::vector<std::vector<int32_t>> by_start((size_t)n_starts);
    for (int32_t p = 0; p < n_pairs; p++) by_start[pair_start[p]].push_back(p);
    GeoChunk c;
    rc = geo_chunk_alloc(g, d, n_starts, true, 0, &c);
    bool short_range = false;
    std::vector<int32_t> pairs, slot, hops;
    std::vector<long long> ends, dst, out;
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_starts; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_starts - s0);
        rc = geo_search(g, d, &c, starts.data() + s0, ns, nullptr, 0);
        if (rc) break;
        pairs.clear(); slot.clear(); ends.clear();
        for (int32_t s = 0; s < ns; s++)
            for (int32_t p : by_start[s0 + s]) { pairs.push_back(p); slot.push_back(s); ends.push_back(end_ids[p]); }
        const int32_t np = (int32_t)pairs.size();
        hops.resize((size_t)np); dst.resize((size_t)np);
        int32_t *d_slot = nullptr, *d_hops = nullptr;
        long long *d_end = nullptr, *d_dst = nullptr, *d_out = nullptr;
        hipError_t e = dalloc(&d_slot, (size_t)np);
        e = e ? e : dalloc(&d_hops, (size_t)np);
        e = e ? e : dalloc(&d_end, (size_t)np);
        e = e ? e : dalloc(&d_dst, (size_t)np);
        e = e ? e : hipMemcpyAsync(d_slot, slot.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, ctx->stream);
        e = e ? e : hipMemcpyAsync(d_end, ends.data(), sizeof(long long) * np, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            k_geo_pair_hops<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, d.n, d_slot, d_end, np, d_hops);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(hops.data(), d_hops, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        int64_t total = 0;
        if (e == hipSuccess) {
            for (int32_t i = 0; i < np; i++) {
                const int32_t p = pairs[i];
                hops_out[p] = hops[i];
                dst[i] = -1;
                if (hops[i] < 0) continue;                                                        // unreachable: nothing to write, no error
                if ((int64_t)hops[i] + 1 > off[p + 1] - off[p]) { short_range = true; continue; }   // reported once every pair has its hops
                dst[i] = total;
                total += (int64_t)hops[i] + 1;
            }
            out.resize((size_t)total);
            e = dalloc(&d_out, (size_t)std::max<int64_t>(total, 1));
            e = e ? e : hipMemcpyAsync(d_dst, dst.data(), sizeof(long long) * np, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e == hipSuccess && total > 0) {
            k_geo_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, d, d_slot, d_end, d_dst, np, d_out);
            e = hipGetLastError();
            e = e ? e : hipMemcpyAsync(out.data(), d_out, sizeof(long long) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
            e = e ? e : hipStreamSynchronize(ctx->stream);
        }
        hipFree(d_slot); hipFree(d_hops); hipFree(d_end); hipFree(d_dst); hipFree(d_out);
        if (e != hipSuccess) { rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_geodesic_paths: %s", hipGetErrorString(e)); break; }
        // only each pair's path: the rest of its range in the caller's buffer stays as it was
        for (int32_t i = 0; i < np; i++)
            if (dst[i] >= 0) memcpy(ids_out + off[pairs[i]], out.data() + dst[i], sizeof(int64_t) * ((size_t)hops[i] + 1));
    }
    c.release();
    if (rc == WA_OK && short_range)
        return fail(ctx, WA_ERR_CAPACITY, "wa_grid_geodesic_paths: a pair's range is shorter than its path (hops_out + 1 ids are needed)");
    return rc;
}
