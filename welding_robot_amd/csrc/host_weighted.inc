// host_weighted.inc -- C ABI: clearance costs, and exact shortest paths with per-voxel entry costs on the 6-neighbour lattice of free voxels
// (included by weldacs.hip inside extern "C", behind host_geodesic.inc whose helpers it shares: geo_dims, grid_build_bits, geo_check_ids,
// WA_GEO_BLOCK, WA_GEO_MAX_CHUNK).  The calls are stateless: the cost array is uploaded, checked and packed by every call.

int wa_grid_clearance_costs(const wa_grid *g, const int32_t *thr2, int32_t n_thr, uint8_t *cost_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!thr2 || !cost_out || n_thr < 0 || n_thr > WA_COST_MAX - 1) return fail(ctx, WA_ERR_ARG, "wa_grid_clearance_costs: bad argument");
    WaThr2 t;
    t.n = n_thr;
    for (int32_t k = 0; k < WA_COST_MAX - 1; k++) t.v[k] = 0;
    for (int32_t k = 0; k < n_thr; k++) {
        if (thr2[k] < 0 || thr2[k] >= WA_D2_NONE) return fail(ctx, WA_ERR_ARG, "wa_grid_clearance_costs: a threshold outside 0 .. WA_D2_NONE - 1");
        t.v[k] = thr2[k];
    }
    int rc = grid_build_d2(g);
    if (rc) return rc;
    const int64_t n = g->d.n;
    uint8_t *d_cost = nullptr;
    if (dalloc(&d_cost, (size_t)n) != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_grid_clearance_costs: the cost array");
    k_wgt_clearance_costs<<<(unsigned)((n + 1023) / 1024), 256, 0, ctx->stream>>>(g->occ, g->d2, n, t, d_cost);
    hipError_t e = hipGetLastError();
    e = e ? e : hipMemcpyAsync(cost_out, d_cost, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    hipFree(d_cost);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_clearance_costs: %s", hipGetErrorString(e));
    return WA_OK;
}

// what a call keeps of its cost array on the device: the bytes (the walk-back reads them), the three bit planes and W
struct WgtCosts {
    uint8_t *bytes = nullptr;
    unsigned long long *planes = nullptr;
    int32_t W = 0;
    void release() { hipFree(bytes); hipFree(planes); bytes = nullptr; planes = nullptr; }
};

// uploads and packs the costs; WA_ERR_ARG for a free voxel whose cost is outside 1 .. WA_COST_MAX and for a grid whose largest
// possible distance W * (n_free - 1) does not fit int32.  Needs g->fbits.
static int wgt_costs(const wa_grid *g, const WaGeoDims &d, const uint8_t *cost, const char *fn, WgtCosts *wc)
{
    wa_ctx *ctx = g->ctx;
    int32_t *d_info = nullptr;
    int32_t info[WA_COST_MAX + 1];
    hipError_t e = dalloc(&wc->bytes, (size_t)d.n);
    e = e ? e : dalloc(&wc->planes, (size_t)(3 * d.nw));
    e = e ? e : dalloc(&d_info, (size_t)(WA_COST_MAX + 1));
    if (e != hipSuccess) { (void)hipGetLastError(); hipFree(d_info); wc->release(); return fail(ctx, WA_ERR_ALLOC, "%s: the cost array does not fit the device", fn); }
    e = hipMemcpyAsync(wc->bytes, cost, (size_t)d.n, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(d_info, 0, sizeof info, ctx->stream);
    if (e == hipSuccess) {
        k_wgt_planes<<<(unsigned)((d.nw + 3) / 4), 256, 0, ctx->stream>>>(g->occ, wc->bytes, d, wc->planes, d_info);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    hipFree(d_info);
    if (e != hipSuccess) { wc->release(); return fail(ctx, WA_ERR_DEVICE, "weighted: packing the costs: %s", hipGetErrorString(e)); }
    if (info[0]) { wc->release(); return fail(ctx, WA_ERR_ARG, "%s: a free voxel's cost is outside 1 .. WA_COST_MAX", fn); }
    wc->W = 1;   // (a grid without a free voxel cannot get here: the ids are checked first)
    for (int32_t c = 1; c <= WA_COST_MAX; c++)
        if (info[c]) wc->W = c;
    if ((int64_t)wc->W * (g->n_free - 1) > (int64_t)INT32_MAX) {
        wc->release();
        return fail(ctx, WA_ERR_ARG, "%s: (largest cost) * (free voxels - 1) exceeds 2^31 - 1, a distance might not fit int32", fn);
    }
    return WA_OK;
}

// device state of one chunk of sources
struct WgtChunk {
    int32_t cap = 0;                       // sources the buffers hold
    unsigned long long *touched = nullptr, *ring = nullptr;
    int32_t *field = nullptr, *mat = nullptr, *last = nullptr, *stop = nullptr;
    long long *src = nullptr;
    void release()
    {
        hipFree(touched); hipFree(ring); hipFree(field); hipFree(mat); hipFree(last); hipFree(stop); hipFree(src);
        touched = ring = nullptr; field = mat = last = stop = nullptr; src = nullptr; cap = 0;
    }
};

// The memory rule (DESIGN 4k): a source costs W + 2 bitmaps (touched, a ring of W + 1 frontiers), a field of 4 bytes per voxel when one
// is kept and a matrix row; the chunk rule is geo_chunk_alloc's: at most half of what wa_ctx_memory_info reports free, at least one
// source, at most WA_GEO_MAX_CHUNK, WA_GEO_CHUNK forces fewer, halved while the device refuses the allocation.
static int wgt_chunk_alloc(const wa_grid *g, const WaGeoDims &d, int32_t W, int32_t n_src, bool with_field, int32_t n_tgt, WgtChunk *c)
{
    wa_ctx *ctx = g->ctx;
    int64_t free_b = 0;
    int rc = wa_ctx_memory_info(ctx, &free_b, nullptr);
    if (rc) return rc;
    const int64_t per = (int64_t)(W + 2) * d.nw * 8 + (with_field ? d.n * 4 : 0) + (int64_t)n_tgt * 4 + 16;
    int64_t cap = (free_b / 2) / per;
    cap = std::max<int64_t>(1, std::min<int64_t>(cap, std::min<int64_t>(n_src, WA_GEO_MAX_CHUNK)));
    if (const int forced = env_int("WA_GEO_CHUNK", 0)) cap = std::max<int64_t>(1, std::min<int64_t>(cap, forced));   // (tests: several chunks on a small grid)
    for (;;) {
        hipError_t e = dalloc(&c->touched, (size_t)(cap * d.nw));
        e = e ? e : dalloc(&c->ring, (size_t)(cap * (W + 1) * d.nw));
        if (e == hipSuccess && with_field) e = dalloc(&c->field, (size_t)(cap * d.n));
        if (e == hipSuccess && n_tgt > 0) e = dalloc(&c->mat, (size_t)(cap * n_tgt));
        e = e ? e : dalloc(&c->last, (size_t)cap);
        e = e ? e : dalloc(&c->stop, (size_t)cap);
        e = e ? e : dalloc(&c->src, (size_t)cap);
        if (e == hipSuccess) { c->cap = (int32_t)cap; return WA_OK; }
        (void)hipGetLastError();
        c->release();
        if (cap == 1) return fail(ctx, WA_ERR_ALLOC, "weighted: the buffers of one source do not fit the device");
        cap = (cap + 1) / 2;
    }
}

// the search from ns sources (host ids) in chunk c: fills c->field / c->mat rows 0 .. ns-1.  d_tgt: the matrix's targets on the device.
static int wgt_search(const wa_grid *g, const WaGeoDims &d, const WgtCosts &wc, WgtChunk *c, const int64_t *src, int32_t ns,
                      const long long *d_tgt, int32_t n_tgt)
{
    wa_ctx *ctx = g->ctx;
    const int32_t W = wc.W, R = W + 1;
    hipError_t e = hipMemcpyAsync(c->src, src, sizeof(long long) * ns, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(c->touched, 0, sizeof(unsigned long long) * (size_t)(ns * d.nw), ctx->stream);
    e = e ? e : hipMemsetAsync(c->ring, 0, sizeof(unsigned long long) * (size_t)((int64_t)ns * R * d.nw), ctx->stream);
    if (e == hipSuccess && c->field) e = hipMemsetAsync(c->field, 0xff, sizeof(int32_t) * (size_t)(ns * d.n), ctx->stream);   // WA_DIST_NONE
    if (e == hipSuccess && c->mat) e = hipMemsetAsync(c->mat, 0xff, sizeof(int32_t) * (size_t)ns * n_tgt, ctx->stream);
    if (e == hipSuccess) {
        k_wgt_seed<<<(unsigned)((ns + 255) / 256), 256, 0, ctx->stream>>>(c->src, ns, d, R, c->touched, c->ring, c->last, c->stop);
        e = hipGetLastError();
    }
    std::vector<int32_t> last((size_t)ns), stop((size_t)ns);
    const dim3 grid((unsigned)((d.nw + 255) / 256), (unsigned)ns);
    // the largest distance is at most W * (n_free - 1) <= 2^31 - 1 (wgt_costs); R more launches see the ring empty
    const int64_t bound = std::min<int64_t>((int64_t)W * (g->n_free - 1) + R + 1, (int64_t)INT32_MAX - WA_GEO_BLOCK);
    int64_t level = 0;
    bool alive = true;
    while (e == hipSuccess && alive) {
        if (level > bound) return fail(ctx, WA_ERR_STATE, "weighted: more levels than the largest possible distance");
        for (int32_t k = 0; k < WA_GEO_BLOCK && e == hipSuccess; k++, level++) {
            k_wgt_level<<<grid, 256, 0, ctx->stream>>>(g->fbits, wc.planes, d, (int32_t)level, (int32_t)(level % R), W, c->touched, c->ring,
                                                       c->field, c->last, c->stop, d_tgt, n_tgt, c->mat);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(last.data(), c->last, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(stop.data(), c->stop, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        alive = false;
        for (int32_t s = 0; s < ns && !alive; s++) alive = !stop[s] && last[s] >= level - R;   // what k_wgt_level asks of the next launch
    }
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "weighted search: %s", hipGetErrorString(e));
    return WA_OK;
}

int wa_grid_weighted_fields(const wa_grid *g, const uint8_t *cost, const int64_t *src_ids, int32_t n_src, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!cost || !src_ids || !dist_out || n_src < 0) return fail(ctx, WA_ERR_ARG, "wa_grid_weighted_fields: bad argument");
    int rc = geo_check_ids(g, "wa_grid_weighted_fields", &src_ids, 1, n_src);
    if (rc || n_src == 0) return rc;
    rc = grid_build_bits(g);
    if (rc) return rc;
    const WaGeoDims d = geo_dims(g);
    WgtCosts wc;
    rc = wgt_costs(g, d, cost, "wa_grid_weighted_fields", &wc);
    if (rc) return rc;
    WgtChunk c;
    rc = wgt_chunk_alloc(g, d, wc.W, n_src, true, 0, &c);
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_src; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_src - s0);
        rc = wgt_search(g, d, wc, &c, src_ids + s0, ns, nullptr, 0);
        if (rc == WA_OK) {
            const hipError_t e = hipMemcpy(dist_out + (int64_t)s0 * d.n, c.field, sizeof(int32_t) * (size_t)(ns * d.n), hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_weighted_fields: %s", hipGetErrorString(e));
        }
    }
    c.release();
    wc.release();
    return rc;
}

int wa_grid_weighted_matrix(const wa_grid *g, const uint8_t *cost, const int64_t *point_ids, int32_t n_pts, int32_t *dist_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!cost || !point_ids || !dist_out || n_pts < 0) return fail(ctx, WA_ERR_ARG, "wa_grid_weighted_matrix: bad argument");
    int rc = geo_check_ids(g, "wa_grid_weighted_matrix", &point_ids, 1, n_pts);
    if (rc || n_pts == 0) return rc;
    rc = grid_build_bits(g);
    if (rc) return rc;
    const WaGeoDims d = geo_dims(g);
    WgtCosts wc;
    rc = wgt_costs(g, d, cost, "wa_grid_weighted_matrix", &wc);
    if (rc) return rc;
    long long *d_tgt = nullptr;
    hipError_t e = dalloc(&d_tgt, (size_t)n_pts);
    e = e ? e : hipMemcpyAsync(d_tgt, point_ids, sizeof(long long) * n_pts, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { hipFree(d_tgt); wc.release(); return fail(ctx, WA_ERR_ALLOC, "wa_grid_weighted_matrix: %s", hipGetErrorString(e)); }
    WgtChunk c;
    rc = wgt_chunk_alloc(g, d, wc.W, n_pts, false, n_pts, &c);
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_pts; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_pts - s0);
        rc = wgt_search(g, d, wc, &c, point_ids + s0, ns, d_tgt, n_pts);
        if (rc == WA_OK) {
            e = hipMemcpy(dist_out + (int64_t)s0 * n_pts, c.mat, sizeof(int32_t) * (size_t)ns * n_pts, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_weighted_matrix: %s", hipGetErrorString(e));
        }
    }
    c.release();
    hipFree(d_tgt);
    wc.release();
    return rc;
}

int wa_grid_weighted_paths(const wa_grid *g, const uint8_t *cost, const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                           const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!cost || !start_ids || !end_ids || !off || !ids_out || !dist_out || !len_out || n_pairs < 0)
        return fail(ctx, WA_ERR_ARG, "wa_grid_weighted_paths: bad argument");
    for (int32_t p = 0; p < n_pairs; p++)
        if (off[p + 1] < off[p]) return fail(ctx, WA_ERR_ARG, "wa_grid_weighted_paths: offsets decrease");
    const int64_t *lists[2] = {start_ids, end_ids};
    int rc = geo_check_ids(g, "wa_grid_weighted_paths", lists, 2, n_pairs);
    if (rc || n_pairs == 0) return rc;
    rc = grid_build_bits(g);
    if (rc) return rc;
    const WaGeoDims d = geo_dims(g);
    WgtCosts wc;
    rc = wgt_costs(g, d, cost, "wa_grid_weighted_paths", &wc);
    if (rc) return rc;
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
    WgtChunk c;
    rc = wgt_chunk_alloc(g, d, wc.W, n_starts, true, 0, &c);
    bool short_range = false;
    std::vector<int32_t> pairs, slot, dist, len;
    std::vector<long long> ends, dst, out;
    for (int32_t s0 = 0; rc == WA_OK && s0 < n_starts; s0 += c.cap) {
        const int32_t ns = std::min(c.cap, n_starts - s0);
        rc = wgt_search(g, d, wc, &c, starts.data() + s0, ns, nullptr, 0);
        if (rc) break;
        pairs.clear(); slot.clear(); ends.clear();
        for (int32_t s = 0; s < ns; s++)
            for (int32_t p : by_start[s0 + s]) { pairs.push_back(p); slot.push_back(s); ends.push_back(end_ids[p]); }
        const int32_t np = (int32_t)pairs.size();
        dist.resize((size_t)np); len.resize((size_t)np); dst.resize((size_t)np);
        int32_t *d_slot = nullptr, *d_dist = nullptr, *d_len = nullptr;
        long long *d_end = nullptr, *d_dst = nullptr, *d_out = nullptr;
        hipError_t e = dalloc(&d_slot, (size_t)np);
        e = e ? e : dalloc(&d_dist, (size_t)np);
        e = e ? e : dalloc(&d_len, (size_t)np);
        e = e ? e : dalloc(&d_end, (size_t)np);
        e = e ? e : dalloc(&d_dst, (size_t)np);
        e = e ? e : hipMemcpyAsync(d_slot, slot.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, ctx->stream);
        e = e ? e : hipMemcpyAsync(d_end, ends.data(), sizeof(long long) * np, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {   // the counting pass: distances and node counts
            k_wgt_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, wc.bytes, d, d_slot, d_end, nullptr, np, d_dist, d_len, nullptr);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(dist.data(), d_dist, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipMemcpyAsync(len.data(), d_len, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        int64_t total = 0;
        if (e == hipSuccess) {
            for (int32_t i = 0; i < np; i++) {
                const int32_t p = pairs[i];
                dist_out[p] = dist[i];
                len_out[p] = len[i];
                dst[i] = -1;
                if (dist[i] < 0) continue;                                                // unreachable: nothing to write, no error
                if ((int64_t)len[i] > off[p + 1] - off[p]) { short_range = true; continue; }   // reported once every pair has its counts
                dst[i] = total;
                total += len[i];
            }
            out.resize((size_t)total);
            e = dalloc(&d_out, (size_t)std::max<int64_t>(total, 1));
            e = e ? e : hipMemcpyAsync(d_dst, dst.data(), sizeof(long long) * np, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e == hipSuccess && total > 0) {
            k_wgt_walkback<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(c.field, wc.bytes, d, d_slot, d_end, d_dst, np, d_dist, d_len, d_out);
            e = hipGetLastError();
            e = e ? e : hipMemcpyAsync(out.data(), d_out, sizeof(long long) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
            e = e ? e : hipStreamSynchronize(ctx->stream);
        }
        hipFree(d_slot); hipFree(d_dist); hipFree(d_len); hipFree(d_end); hipFree(d_dst); hipFree(d_out);
        if (e != hipSuccess) { rc = fail(ctx, WA_ERR_DEVICE, "wa_grid_weighted_paths: %s", hipGetErrorString(e)); break; }
        // only each pair's path: the rest of its range in the caller's buffer stays as it was
        for (int32_t i = 0; i < np; i++)
            if (dst[i] >= 0) memcpy(ids_out + off[pairs[i]], out.data() + dst[i], sizeof(int64_t) * (size_t)len[i]);
    }
    c.release();
    wc.release();
    if (rc == WA_OK && short_range)
        return fail(ctx, WA_ERR_CAPACITY, "wa_grid_weighted_paths: a pair's range is shorter than its path (len_out ids are needed)");
    return rc;
}
