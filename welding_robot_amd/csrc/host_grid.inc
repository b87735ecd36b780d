// host_grid.inc -- C ABI: STL input and the grid map (included by weldacs.hip inside extern "C")
// ------------------------------------------------------------------ STL (read_STL.hpp)
int64_t wa_stl_parse(const void *buf, size_t len, float *tris, int64_t cap_tris)
{
    const uint8_t *b = (const uint8_t *)buf;
    if (!b) return -WA_ERR_ARG;
    if (len < 80) return -WA_ERR_FILE;            // no byte 79 to sniff (:65 reads it regardless)
    if (b[79] != 0) return stl_parse_text(b, len, tris, cap_tris);   // ASCII sniff (:65-68)
    if (len < 84) return -WA_ERR_FILE;            // shorter than header + count
    int32_t n;
    memcpy(&n, b + 80, 4);                         // cpyint :158
    if (n < 0 || (size_t)n * 50 + 84 > len) return -WA_ERR_FILE;
    if (!tris) return n;
    if (cap_tris < n) return -WA_ERR_CAPACITY;
    const uint8_t *p = b + 84;
    for (int64_t i = 0; i < n; i++, p += 50) memcpy(tris + i * 12, p, 48);  // :142-151
    return n;
}
int64_t wa_stl_read_file(const char *path, float *tris, int64_t cap_tris)
{
    if (!path) return -WA_ERR_ARG;
    FILE *f = fopen(path, "rb");
    if (!f) return -WA_ERR_FILE;
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    rewind(f);
    std::vector<uint8_t> buf(sz > 0 ? (size_t)sz : 0);
    size_t got = sz > 0 ? fread(buf.data(), 1, (size_t)sz, f) : 0;
    fclose(f);
    if ((long)got != sz) return -WA_ERR_FILE;
    return wa_stl_parse(buf.data(), buf.size(), tris, cap_tris);
}

// ------------------------------------------------------------------ grid
int wa_axis_coords(float lo, float hi, float precision, int32_t wall, int32_t n, float *out)
{
    if (!out || n < 0) return WA_ERR_ARG;
    for (int32_t i = 0; i < n; i++)  // model_grid_map.hpp:204-211
        out[i] = i < wall ? lo - (float)(wall - i) * precision
                          : (i >= (n - wall) ? hi + (float)(i - n + wall) * precision : lo + (float)(i - wall) * precision);
    return WA_OK;
}

static int grid_alloc(wa_ctx *ctx, int32_t nx, int32_t ny, int32_t nz, const float *cx, const float *cy,
                      const float *cz, float precision, int32_t wall, wa_grid **out)
{
    if (nx < 1 || ny < 1 || nz < 1) return fail(ctx, WA_ERR_ARG, "grid dimensions must be >= 1");
    int64_t n = (int64_t)nx * ny * nz;
    if (n > (int64_t)WA_ID_MASK + 1) return fail(ctx, WA_ERR_ARG, "grid larger than 2^29 voxels");   // ids 0 .. 2^29 - 1 fit WA_ID_MASK
    wa_grid *g = new wa_grid();
    g->ctx = ctx;
    g->d.nx = nx; g->d.ny = ny; g->d.nz = nz; g->d.nxy = nx * ny; g->d.n = n;
    g->precision = precision;
    g->wall = wall;
    g->n_free = -1;
    g->cx = g->cy = g->cz = nullptr;
    g->occ = nullptr;
    if (dalloc(&g->cx, nx) || dalloc(&g->cy, ny) || dalloc(&g->cz, nz) || dalloc(&g->occ, n)) {
        wa_grid_destroy(g);
        return fail(ctx, WA_ERR_ALLOC, "grid device allocation failed");
    }
    hipError_t e = hipMemcpyAsync(g->cx, cx, sizeof(float) * nx, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(g->cy, cy, sizeof(float) * ny, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(g->cz, cz, sizeof(float) * nz, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { wa_grid_destroy(g); return fail(ctx, WA_ERR_DEVICE, "grid upload: %s", hipGetErrorString(e)); }
    *out = g;
    return WA_OK;
}

static int grid_count_free(wa_grid *g)
{
    wa_ctx *ctx = g->ctx;
    unsigned long long *d_cnt = nullptr, h = 0;
    hipError_t e = dalloc(&d_cnt, 1);
    e = e ? e : hipMemsetAsync(d_cnt, 0, 8, ctx->stream);
    if (e == hipSuccess) {
        k_count_free<<<1024, 256, 0, ctx->stream>>>(g->occ, g->d.n, d_cnt);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(&h, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    dev_free(d_cnt);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "free-voxel count: %s", hipGetErrorString(e));
    g->n_free = (int64_t)h;
    return WA_OK;
}

int wa_grid_from_mesh(wa_ctx *ctx, const float *tris, int64_t n_tris, float precision, int32_t wall,
                      wa_grid **out, float *bbox6_out)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx || !tris || !out || n_tris <= 0 || !(precision > 0) || wall < 0) return fail(ctx, WA_ERR_ARG, "wa_grid_from_mesh: bad argument");
    *out = nullptr;
    // bbox over all vertices (model_grid_map.hpp:165-181) and the ranges (:198-200)
    float mn[3] = {tris[3], tris[4], tris[5]}, mx[3] = {tris[3], tris[4], tris[5]};
    for (int64_t t = 0; t < n_tris; t++)
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++) {
                float q = tris[t * 12 + 3 + v * 3 + c];
                mx[c] = q > mx[c] ? q : mx[c];
                mn[c] = q < mn[c] ? q : mn[c];
            }
    int32_t dims[3];
    for (int c = 0; c < 3; c++) dims[c] = (int)((mx[c] - mn[c]) / precision) + 1 + 2 * wall;
    if (bbox6_out) for (int c = 0; c < 3; c++) { bbox6_out[c] = mn[c]; bbox6_out[3 + c] = mx[c]; }
    std::vector<float> ax[3];
    for (int c = 0; c < 3; c++) {
        if (dims[c] < 1) return fail(ctx, WA_ERR_ARG, "degenerate mesh extent");
        ax[c].resize(dims[c]);
        wa_axis_coords(mn[c], mx[c], precision, wall, dims[c], ax[c].data());
    }
    wa_grid *g = nullptr;
    int rc = grid_alloc(ctx, dims[0], dims[1], dims[2], ax[0].data(), ax[1].data(), ax[2].data(), precision, wall, &g);
    if (rc) return rc;
    DevBuf<float> d_tris;
    if (d_tris.alloc((size_t)n_tris * 12)) { wa_grid_destroy(g); return fail(ctx, WA_ERR_ALLOC, "triangle buffer"); }
    hipError_t ve = hipMemcpyAsync(d_tris, tris, sizeof(float) * 12 * n_tris, hipMemcpyHostToDevice, ctx->stream);
    if (ve == hipSuccess) {
        if (env_int("WA_VOXELIZE_DENSE", 0)) {   // the O(T*N^3) form, kept for comparison
            unsigned blocks = (unsigned)((g->d.n + 255) / 256);
            k_voxelize<<<blocks, 256, 0, ctx->stream>>>(d_tris, n_tris, precision, g->d, g->cx, g->cy, g->cz, g->occ);
        } else {
            ve = hipMemsetAsync(g->occ, 1, (size_t)g->d.n, ctx->stream);
            for (int64_t t0 = 0; ve == hipSuccess && t0 < n_tris; t0 += 1 << 20) {
                const int64_t cnt = n_tris - t0 < (1 << 20) ? n_tris - t0 : (1 << 20);
                k_voxelize_clip<<<dim3((unsigned)cnt, 4), 256, 0, ctx->stream>>>(d_tris.p + t0 * 12, cnt, precision, g->d, g->cx, g->cy, g->cz, g->occ);
            }
        }
        ve = ve ? ve : hipGetLastError();
    }
    if (ve == hipSuccess) ve = hipStreamSynchronize(ctx->stream);
    if (ve != hipSuccess) { wa_grid_destroy(g); return fail(ctx, WA_ERR_DEVICE, "voxelise: %s", hipGetErrorString(ve)); }
    rc = grid_count_free(g);
    if (rc) { wa_grid_destroy(g); return rc; }
    *out = g;
    return WA_OK;
}

int wa_grid_from_occupancy(wa_ctx *ctx, const uint8_t *free_, int32_t nx, int32_t ny, int32_t nz,
                           const float *cx, const float *cy, const float *cz, float precision,
                           int32_t wall, wa_grid **out)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx || !free_ || !cx || !cy || !cz || !out || !(precision > 0)) return fail(ctx, WA_ERR_ARG, "wa_grid_from_occupancy: bad argument");
    *out = nullptr;
    wa_grid *g = nullptr;
    int rc = grid_alloc(ctx, nx, ny, nz, cx, cy, cz, precision, wall, &g);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(g->occ, free_, (size_t)g->d.n, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { wa_grid_destroy(g); return fail(ctx, WA_ERR_DEVICE, "occupancy upload: %s", hipGetErrorString(e)); }
    rc = grid_count_free(g);
    if (rc) { wa_grid_destroy(g); return rc; }
    *out = g;
    return WA_OK;
}

void wa_grid_destroy(wa_grid *g)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!g) return;
    dev_free(g->cx); dev_free(g->cy); dev_free(g->cz); dev_free(g->occ); dev_free(g->d2); dev_free(g->fbits);
    delete g;
}
int wa_grid_info(const wa_grid *g, int32_t dims3[3], float *precision, int32_t *wall, int64_t *n_free)
{
    if (!g) return WA_ERR_ARG;
    if (dims3) { dims3[0] = g->d.nx; dims3[1] = g->d.ny; dims3[2] = g->d.nz; }
    if (precision) *precision = g->precision;
    if (wall) *wall = g->wall;
    if (n_free) *n_free = g->n_free;
    return WA_OK;
}
int wa_grid_read_occupancy(const wa_grid *g, uint8_t *free_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g || !free_out) return WA_ERR_ARG;
    HIPC(g->ctx, hipMemcpy(free_out, g->occ, (size_t)g->d.n, hipMemcpyDeviceToHost));
    return WA_OK;
}
int wa_grid_read_coords(const wa_grid *g, float *cx, float *cy, float *cz)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    if (cx) HIPC(g->ctx, hipMemcpy(cx, g->cx, sizeof(float) * g->d.nx, hipMemcpyDeviceToHost));
    if (cy) HIPC(g->ctx, hipMemcpy(cy, g->cy, sizeof(float) * g->d.ny, hipMemcpyDeviceToHost));
    if (cz) HIPC(g->ctx, hipMemcpy(cz, g->cz, sizeof(float) * g->d.nz, hipMemcpyDeviceToHost));
    return WA_OK;
}
// One point on the host mirror: k_resolve_points_clip's index box and scan, statement for statement (same fp32 subtraction, same
// comparisons; this translation unit is built without contraction and without fast-math like the kernels).
static int64_t resolve_on_host(const wa_grid *g, const float *q)
{
    const float t = (float)(1.2 * (double)g->precision);   // `float t = 1.2*precision` ACSRank_3D.hpp:544
    const float *ax[3] = {g->h_cx.data(), g->h_cy.data(), g->h_cz.data()};
    const int32_t dim[3] = {g->d.nx, g->d.ny, g->d.nz};
    int32_t lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = 0x7fffffff; hi[a] = -1;
        for (int32_t i = 0; i < dim[a]; i++) {
            float v = q[a] - ax[a][i];
            v = v > 0 ? v : -v;
            if (v < t) { if (i < lo[a]) lo[a] = i; if (i > hi[a]) hi[a] = i; }
        }
        if (hi[a] < lo[a]) return -1;
    }
    int64_t best = -1;
    for (int32_t z = lo[2]; z <= hi[2]; z++)
        for (int32_t y = lo[1]; y <= hi[1]; y++)
            for (int32_t x = lo[0]; x <= hi[0]; x++) {
                const int64_t id = (int64_t)z * g->d.nxy + (int64_t)y * g->d.nx + x;
                if (!g->h_occ[(size_t)id]) continue;
                float dx = q[0] - ax[0][x], dy = q[1] - ax[1][y], dz = q[2] - ax[2][z];
                dx = dx > 0 ? dx : -dx; dy = dy > 0 ? dy : -dy; dz = dz > 0 ? dz : -dz;
                if (dx < t && dy < t && dz < t && id > best) best = id;   // the LAST free match in raster order (:545-561)
            }
    return best;
}

// ACS_Rank::setPoints resolves two points per call (ACSRank_3D.hpp:537-565) and a host that loops over pairs calls it per pair: a
// launch + synchronise + copy per call (35 us, profiles/r04/scalar_calls.txt) is what that loop would wait for.  Up to
// WA_RESOLVE_HOST_MAX points are therefore resolved on a host mirror of the grid (axis tables + occupancy, fetched once per grid on the
// first such call); larger batches run k_resolve_points_clip.  WA_RESOLVE_HOST=0 sends everything to the device; the GPU tests hold
// both against the oracle.
#define WA_RESOLVE_HOST_MAX 16
int wa_grid_resolve_points(const wa_grid *g, const float *pts_xyz, int32_t n_pts, int64_t *ids_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g || !pts_xyz || !ids_out || n_pts < 0) return WA_ERR_ARG;
    if (n_pts == 0) return WA_OK;
    wa_ctx *ctx = g->ctx;
    if (n_pts <= WA_RESOLVE_HOST_MAX && env_int("WA_RESOLVE_HOST", 1) && !env_int("WA_RESOLVE_DENSE", 0)) {
        // (filled once, under the grid's lock: the drop-in's shard threads may resolve points of one grid concurrently -- ADVICE r05)
        {
        std::lock_guard<std::mutex> mirror_lock(g->h_mu);
        if (!g->h_valid) {
            g->h_cx.resize((size_t)g->d.nx); g->h_cy.resize((size_t)g->d.ny); g->h_cz.resize((size_t)g->d.nz); g->h_occ.resize((size_t)g->d.n);
            hipError_t e = hipStreamSynchronize(ctx->stream);     // (whatever built the grid has finished)
            e = e ? e : hipMemcpy(g->h_cx.data(), g->cx, sizeof(float) * g->d.nx, hipMemcpyDeviceToHost);
            e = e ? e : hipMemcpy(g->h_cy.data(), g->cy, sizeof(float) * g->d.ny, hipMemcpyDeviceToHost);
            e = e ? e : hipMemcpy(g->h_cz.data(), g->cz, sizeof(float) * g->d.nz, hipMemcpyDeviceToHost);
            e = e ? e : hipMemcpy(g->h_occ.data(), g->occ, (size_t)g->d.n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_resolve_points: %s", hipGetErrorString(e));
            g->h_valid = true;
        }
        }
        for (int32_t i = 0; i < n_pts; i++) ids_out[i] = resolve_on_host(g, pts_xyz + 3 * (size_t)i);
        return WA_OK;
    }
    DevBuf<float> d_pts;
    DevBuf<long long> d_ids;
    std::vector<long long> h(n_pts);
    hipError_t e = d_pts.alloc((size_t)n_pts * 3);
    e = e ? e : d_ids.alloc((size_t)n_pts);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "resolve buffers");
    e = hipMemcpyAsync(d_pts, pts_xyz, sizeof(float) * 3 * n_pts, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemsetAsync(d_ids, 0xff, sizeof(long long) * n_pts, ctx->stream);  // -1
    if (e == hipSuccess) {
        if (env_int("WA_RESOLVE_DENSE", 0)) {   // thread per voxel x every point, kept for comparison
            unsigned blocks = (unsigned)((g->d.n + 255) / 256);
            k_resolve_points<<<blocks, 256, 0, ctx->stream>>>(g->d, g->cx, g->cy, g->cz, g->occ, g->precision, d_pts, n_pts, d_ids);
        } else {
            k_resolve_points_clip<<<(unsigned)n_pts, 256, 0, ctx->stream>>>(g->d, g->cx, g->cy, g->cz, g->occ, g->precision, d_pts, n_pts, d_ids);
        }
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(h.data(), d_ids, sizeof(long long) * n_pts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_resolve_points: %s", hipGetErrorString(e));
    for (int32_t i = 0; i < n_pts; i++) ids_out[i] = h[i];
    return WA_OK;
}

