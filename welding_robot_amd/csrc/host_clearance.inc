// host_clearance.inc -- C ABI: distance field, inflated grids and the trajectory check (included by weldacs.hip inside extern "C")
// ------------------------------------------------------------------ distance field
// builds g->d2 once (under the grid's lock: grids are shared read-only between threads, see wa_grid_resolve_points)
static int grid_build_d2(const wa_grid *g)
{
    wa_ctx *ctx = g->ctx;
    std::lock_guard<std::mutex> lock(g->d2_mu);
    if (g->d2) return WA_OK;
    const int64_t bound = (int64_t)(g->d.nx - 1) * (g->d.nx - 1) + (int64_t)(g->d.ny - 1) * (g->d.ny - 1) + (int64_t)(g->d.nz - 1) * (g->d.nz - 1);
    if (bound >= ((int64_t)1 << 31))
        return fail(ctx, WA_ERR_ARG, "wa_grid_distance_field: squared grid diagonal >= 2^31 does not fit int32");
    // (2^31 - 1 = WA_D2_NONE is 7 mod 8, so no sum of three squares: a real distance never equals the marker)
    const int64_t n = g->d.n;
    DevBuf<int32_t> d2;
    DevBuf<int2> env;
    hipError_t e = d2.alloc((size_t)n);
    e = e ? e : env.alloc((size_t)n);
    if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "distance field buffers");
    const int64_t rows = (int64_t)g->d.ny * g->d.nz;
    k_edt_x<<<(unsigned)((rows + 3) / 4), 256, 0, ctx->stream>>>(g->occ, g->d, d2);
    e = hipGetLastError();
    if (e == hipSuccess && g->d.ny > 1) {   // y: columns (x, z), element j at z*nxy + j*nx + x
        const int64_t nc = (int64_t)g->d.nx * g->d.nz;
        k_edt_cols<<<(unsigned)((nc + 255) / 256), 256, 0, ctx->stream>>>(d2, env, nc, g->d.ny, g->d.nx, g->d.nx, g->d.nxy);
        e = hipGetLastError();
    }
    if (e == hipSuccess && g->d.nz > 1) {   // z: columns (x, y), element j at j*nxy + y*nx + x
        const int64_t nc = g->d.nxy;
        k_edt_cols<<<(unsigned)((nc + 255) / 256), 256, 0, ctx->stream>>>(d2, env, nc, g->d.nz, g->d.nxy, g->d.nxy, 0);
        e = hipGetLastError();
    }
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_grid_distance_field: %s", hipGetErrorString(e));
    g->d2 = d2.detach();   // the grid's from here
    return WA_OK;
}

// The grid as the trajectory stages look a sample up in it: the distance field (built if need be) and, once per grid, each axis
// table's range and whether it is non-decreasing (binary search) -- the hi-side seam of the wall is where a table built by
// wa_axis_coords can hold one value twice, which is still non-decreasing.  A grid never changes after it is built.
static int grid_field(const wa_grid *g, WaField *F)
{
    int rc = grid_build_d2(g);
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> lock(g->d2_mu);
        if (!g->axes_valid) {
            const float *dev[3] = {g->cx, g->cy, g->cz};
            const int32_t len[3] = {g->d.nx, g->d.ny, g->d.nz};
            for (int c = 0; c < 3; c++) {
                std::vector<float> ax((size_t)len[c]);
                HIPC(g->ctx, hipMemcpy(ax.data(), dev[c], sizeof(float) * ax.size(), hipMemcpyDeviceToHost));
                float lo = ax[0], hi = ax[0];
                int mono = 1;
                for (size_t j = 1; j < ax.size(); j++) {
                    const float v = ax[j];
                    lo = v < lo ? v : lo;
                    hi = v > hi ? v : hi;
                    if (!(v >= ax[j - 1])) mono = 0;
                }
                if (lo != lo || hi != hi) mono = 0;
                g->axes.lo[c] = lo; g->axes.hi[c] = hi; g->axes.mono[c] = mono;
            }
            g->axes_valid = true;
        }
    }
    *F = WaField{g->d, g->cx, g->cy, g->cz, g->axes, g->d2};
    return WA_OK;
}

int wa_grid_distance_field(const wa_grid *g, int32_t *d2_out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    int rc = grid_build_d2(g);
    if (rc) return rc;
    if (d2_out) HIPC(g->ctx, hipMemcpy(d2_out, g->d2, sizeof(int32_t) * (size_t)g->d.n, hipMemcpyDeviceToHost));
    return WA_OK;
}

// ------------------------------------------------------------------ inflated planning grid
int wa_grid_inflate(const wa_grid *g, float radius, const int64_t *keep_ids, int32_t n_keep, wa_grid **out)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!out || !(radius >= 0) || isinf(radius) || n_keep < 0 || (n_keep > 0 && !keep_ids))
        return fail(ctx, WA_ERR_ARG, "wa_grid_inflate: bad argument");
    *out = nullptr;
    int rc = grid_build_d2(g);
    if (rc) return rc;
    std::vector<float> ax[3] = {std::vector<float>((size_t)g->d.nx), std::vector<float>((size_t)g->d.ny), std::vector<float>((size_t)g->d.nz)};
    rc = wa_grid_read_coords(g, ax[0].data(), ax[1].data(), ax[2].data());
    if (rc) return rc;
    std::vector<uint8_t> keep_free;
    if (n_keep > 0) {
        for (int32_t k = 0; k < n_keep; k++)
            if (keep_ids[k] < 0 || keep_ids[k] >= g->d.n) return fail(ctx, WA_ERR_ARG, "wa_grid_inflate: keep id outside the grid");
        keep_free.resize((size_t)n_keep);
        for (int32_t k = 0; k < n_keep; k++) HIPC(ctx, hipMemcpy(&keep_free[k], g->occ + keep_ids[k], 1, hipMemcpyDeviceToHost));
        for (int32_t k = 0; k < n_keep; k++)
            if (!keep_free[k]) return fail(ctx, WA_ERR_ARG, "wa_grid_inflate: keep id is not a free voxel");
    }
    wa_grid *ng = nullptr;
    rc = grid_alloc(ctx, g->d.nx, g->d.ny, g->d.nz, ax[0].data(), ax[1].data(), ax[2].data(), g->precision, g->wall, &ng);
    if (rc) return rc;
    const double r2 = (double)radius * (double)radius, rk = (double)radius + 1.0;
    k_inflate<<<2048, 256, 0, ctx->stream>>>(g->occ, g->d2, g->d.n, r2, ng->occ);
    hipError_t e = hipGetLastError();
    DevBuf<long long> d_keep;
    if (e == hipSuccess && n_keep > 0) {
        e = d_keep.alloc((size_t)n_keep);
        e = e ? e : hipMemcpyAsync(d_keep, keep_ids, sizeof(long long) * n_keep, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            // half-width of the bubble's box, capped by the grid: |v - k|^2 <= (radius + 1)^2 needs every |v_c - k_c| <= radius + 1
            const double hmax = (double)std::max(g->d.nx, std::max(g->d.ny, g->d.nz));
            const int32_t h = (int32_t)std::min(floor(rk), hmax);
            k_inflate_keep<<<(unsigned)n_keep, 256, 0, ctx->stream>>>(g->occ, g->d, d_keep, h, rk * rk, ng->occ);
            e = hipGetLastError();
        }
    }
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { wa_grid_destroy(ng); return fail(ctx, WA_ERR_DEVICE, "wa_grid_inflate: %s", hipGetErrorString(e)); }
    rc = grid_count_free(ng);
    if (rc) { wa_grid_destroy(ng); return rc; }
    *out = ng;
    return WA_OK;
}

// ------------------------------------------------------------------ trajectory check
static void clr_summary_from(const unsigned long long acc[4], wa_clearance_summary *sum)
{
    sum->min_d2 = (int32_t)(acc[0] >> 33);
    sum->argmin = (int64_t)(acc[0] & ((1ull << 33) - 1));
    sum->first_hit = acc[1] == ~0ull ? -1 : (int64_t)acc[1];
    sum->n_hit = (int64_t)acc[2];
    sum->n_outside = (int64_t)acc[3];
}

int wa_traj_clearance(const wa_grid *g, const wa_traj *t, int64_t *ids_out, int32_t *d2_out, uint8_t *hit_out, wa_clearance_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!t || !sum) return fail(ctx, WA_ERR_ARG, "wa_traj_clearance: bad argument");
    if (t->ctx != ctx) return fail(ctx, WA_ERR_ARG, "wa_traj_clearance: trajectory and grid belong to different contexts");
    const int64_t n = t->n;
    if (n > ((int64_t)1 << 33)) return fail(ctx, WA_ERR_ARG, "wa_traj_clearance: more than 2^33 samples");
    WaField F;
    int rc = grid_field(g, &F);
    if (rc) return rc;
    sum->min_d2 = WA_D2_NONE; sum->argmin = -1; sum->first_hit = -1; sum->n_hit = 0; sum->n_outside = 0;
    if (n == 0) return WA_OK;
    DevBuf<long long> d_ids;
    DevBuf<int32_t> d_d2;
    DevBuf<uint8_t> d_hit;
    DevBuf<unsigned long long> d_acc;
    unsigned long long init[4], acc[4];
    clr_acc_init(init);
    hipError_t e = d_ids.alloc((size_t)n);
    e = e ? e : d_d2.alloc((size_t)n);
    e = e ? e : d_hit.alloc((size_t)(n > 1 ? n - 1 : 1));
    e = e ? e : d_acc.alloc(4);
    e = e ? e : hipMemcpyAsync(d_acc, init, sizeof init, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        k_clr_samples<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(t->xyz, n, F, d_ids, d_d2, d_acc);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n > 1) {
        k_clr_segments<<<(unsigned)((n - 1 + 255) / 256), 256, 0, ctx->stream>>>(d_ids, n, g->d, g->occ, d_hit, d_acc);
        e = hipGetLastError();
    }
    e = e ? e : hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && ids_out) e = hipMemcpyAsync(ids_out, d_ids, sizeof(long long) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && d2_out) e = hipMemcpyAsync(d2_out, d_d2, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && hit_out && n > 1) e = hipMemcpyAsync(hit_out, d_hit, (size_t)(n - 1), hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_clearance: %s", hipGetErrorString(e));
    clr_summary_from(acc, sum);
    return WA_OK;
}
