// host_seamtour.inc -- C ABI: wa_gtsp_seam_tour / wa_gtsp_seam_tour_exact, order and direction of two-ended weld seams (DESIGN §4n; included by
// weldacs.hip inside extern "C").  The host checks and quantises the costs (the only floating-point step), the device does the rest in
// integers on the context's stream; device blocks come from and go back to the context's memory cache.
static const double WA_ST_Q = 1048576.0;   // 2^20 quanta per unit of cost

// W (2M x 2M, symmetric, zero on the diagonal, within a seam and on the dummy's rows) from the upper triangle of dist (2m x 2m)
static int st_quantise(wa_ctx *ctx, const char *who, const double *dist, int m, int M, std::vector<int64_t> &W, bool *narrow)
{
    const int n = 2 * m, N2 = 2 * M;
    W.assign((size_t)N2 * N2, 0);
    *narrow = true;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) {
            if ((i >> 1) == (j >> 1)) continue;
            const double d = dist[(size_t)i * n + j] * WA_ST_Q;
            if (!(d >= 0.0) || !std::isfinite(d)) return fail(ctx, WA_ERR_ARG, "%s: a cost is negative or not finite", who);
            const double r = rint(d);
            if (!(r < 1099511627776.0)) return fail(ctx, WA_ERR_ARG, "%s: a cost reaches 2^40 quanta", who);
            const int64_t w = (int64_t)r;
            if (w >> 32) *narrow = false;
            W[(size_t)i * N2 + j] = W[(size_t)j * N2 + i] = w;
        }
    return WA_OK;
}

// the closed tour on M seams (in-endpoints E) as the caller sees it: seam 0 first, or, when open, the seam behind the dummy first and
// the dummy dropped
static void st_emit(const uint16_t *E, int m, int M, int32_t *order_out, uint8_t *dir_out)
{
    const int first = M == m ? 0 : m;
    int at = 0;
    for (int k = 0; k < M; k++)
        if ((E[k] >> 1) == first) at = k;
    if (M != m) at++;
    for (int k = 0; k < m; k++) {
        const uint16_t e = E[(at + k) % M];
        order_out[k] = e >> 1;
        dir_out[k] = (uint8_t)(e & 1);
    }
}

static int64_t st_cost(const std::vector<int64_t> &W, const uint16_t *E, int M)
{
    int64_t c = 0;
    for (int k = 0; k < M; k++) c += W[(size_t)(E[k] ^ 1) * 2 * M + E[(k + 1) % M]];
    return c;
}

extern "C++" {
template <typename WT, bool W_LDS, int TEAM>
static hipError_t st_launch(wa_ctx *ctx, const WaStArgs &a, size_t lds)
{
    hipError_t e = hipFuncSetAttribute((const void *)k_seam_descend<WT, W_LDS, TEAM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int teams = WA_ST_BLOCK / TEAM;
    const long long want = ((long long)a.n_starts + teams - 1) / teams;
    const long long per_cu = std::min<long long>(32 / (WA_ST_BLOCK / 64), std::max<long long>(1, (long long)(160 * 1024 / lds)));
    const long long cap = (long long)std::max(1, ctx->prop.multiProcessorCount) * per_cu;   // resident blocks: each loops over its starts
    k_seam_descend<WT, W_LDS, TEAM><<<(unsigned)std::min(want, cap), WA_ST_BLOCK, lds, ctx->stream>>>(a);
    return hipGetLastError();
}
}

int wa_gtsp_seam_tour(wa_ctx *ctx, const double *dist, int32_t m, const wa_seam_params *prm, const int32_t *order0, const uint8_t *dir0,
                 int32_t *order_out, uint8_t *dir_out, int64_t *start_cost_q_out, int32_t *start_passes_out, wa_seam_summary *sum)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx) return WA_ERR_ARG;
    if (!dist || !prm || !order_out || !dir_out || !sum) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour: NULL dist, params, outputs or summary");
    if (m < 1 || m > 1024) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour: 1 .. 1024 seams");
    if (prm->or_len < 0 || prm->or_len > 3 || prm->n_starts < 1 || prm->n_starts > (1 << 20) || prm->max_passes < 1 || prm->max_passes > (1 << 20))
        return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour: or_len 0 .. 3, n_starts and max_passes 1 .. 2^20");
    const int M = prm->closed ? m : m + 1, N2 = 2 * M, n_starts = prm->n_starts;
    std::vector<uint16_t> e0((size_t)M);
    {
        std::vector<uint8_t> seen((size_t)m, 0);
        for (int k = 0; k < m; k++) {
            const int32_t s = order0 ? order0[k] : k;
            if (s < 0 || s >= m || seen[(size_t)s]) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour: order0 is not a permutation of the seams");
            seen[(size_t)s] = 1;
            if (dir0 && dir0[k] > 1) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour: dir0 entries are 0 or 1");
            e0[(size_t)k] = (uint16_t)(2 * s + (dir0 ? dir0[k] : 0));
        }
        if (M != m) e0[(size_t)m] = (uint16_t)(2 * m);
    }
    std::vector<int64_t> W;
    bool narrow = true;
    int rc = st_quantise(ctx, "wa_gtsp_seam_tour", dist, m, M, W, &narrow);
    if (rc) return rc;

    // where W lives and who holds a descent: a wavefront up to 64 positions (W always fits LDS then), the workgroup above
    const int Mpad = (M + 7) & ~7;
    const bool wave = M <= 64;
    const size_t state = (size_t)(wave ? 4 : 1) * 2 * Mpad * sizeof(uint16_t) + (WA_ST_BLOCK / 64) * 16;
    const size_t w_narrow = ((size_t)N2 * N2 * 4 + 15) & ~(size_t)15, w_wide = ((size_t)N2 * N2 * 8 + 15) & ~(size_t)15;
    const size_t lds_max = 160 * 1024;
    const bool w_lds = wave || (narrow && w_narrow + state <= lds_max);
    const size_t lds = state + (w_lds ? (narrow ? w_narrow : w_wide) : 0);

    CtxBuf<unsigned char> dW(ctx);   // uint32_t or long long entries
    CtxBuf<uint16_t> dE0(ctx);
    CtxBuf<long long> dCost(ctx);
    CtxBuf<int32_t> dPass(ctx);
    CtxBuf<uint8_t> dCap(ctx);
    CtxBuf<uint16_t> dTours(ctx);
    hipError_t e = dW.alloc((size_t)N2 * N2 * (narrow ? 4 : 8));
    e = e ? e : dE0.alloc((size_t)M);
    e = e ? e : dCost.alloc((size_t)n_starts);
    e = e ? e : dPass.alloc((size_t)n_starts);
    e = e ? e : dCap.alloc((size_t)n_starts);
    e = e ? e : dTours.alloc((size_t)n_starts * M);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_ALLOC, "wa_gtsp_seam_tour: device buffers"); }
    std::vector<uint32_t> W32;
    if (narrow) {
        W32.resize(W.size());
        for (size_t k = 0; k < W.size(); k++) W32[k] = (uint32_t)W[k];
        e = hipMemcpyAsync(dW, W32.data(), W32.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    } else {
        e = hipMemcpyAsync(dW, W.data(), W.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    }
    e = e ? e : hipMemcpyAsync(dE0, e0.data(), sizeof(uint16_t) * M, hipMemcpyHostToDevice, ctx->stream);
    WaStArgs a;
    a.W = dW;
    a.e0 = dE0;
    a.M = M; a.or_len = prm->or_len; a.n_starts = n_starts; a.max_passes = prm->max_passes;
    a.seed = prm->seed;
    a.cost = dCost; a.passes = dPass; a.capped = dCap; a.tours = dTours;
    if (e == hipSuccess) {
        if (wave) e = narrow ? st_launch<uint32_t, true, 64>(ctx, a, lds) : st_launch<long long, true, 64>(ctx, a, lds);
        else if (w_lds) e = st_launch<uint32_t, true, 256>(ctx, a, lds);
        else e = narrow ? st_launch<uint32_t, false, 256>(ctx, a, lds) : st_launch<long long, false, 256>(ctx, a, lds);
    }
    std::vector<int64_t> cost((size_t)n_starts);
    std::vector<int32_t> passes((size_t)n_starts);
    std::vector<uint8_t> capped((size_t)n_starts);
    e = e ? e : hipMemcpyAsync(cost.data(), dCost, sizeof(int64_t) * n_starts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipMemcpyAsync(passes.data(), dPass, sizeof(int32_t) * n_starts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipMemcpyAsync(capped.data(), dCap, (size_t)n_starts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour: %s", hipGetErrorString(e));
    wa_seam_summary s;
    memset(&s, 0, sizeof s);
    s.m = m; s.M = M; s.n_starts = n_starts;
    for (int r = 0; r < n_starts; r++) {
        if (cost[(size_t)r] < cost[(size_t)s.best_start]) s.best_start = r;
        s.n_capped += capped[(size_t)r];
        s.passes_total += passes[(size_t)r];
    }
    s.cost_q = cost[(size_t)s.best_start];
    s.start0_cost_q_in = st_cost(W, e0.data(), M);
    s.start0_cost_q_out = cost[0];
    std::vector<uint16_t> best((size_t)M);
    e = hipMemcpyAsync(best.data(), dTours.p + (size_t)s.best_start * M, sizeof(uint16_t) * M, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour: %s", hipGetErrorString(e));
    st_emit(best.data(), m, M, order_out, dir_out);
    if (start_cost_q_out) memcpy(start_cost_q_out, cost.data(), sizeof(int64_t) * n_starts);
    if (start_passes_out) memcpy(start_passes_out, passes.data(), sizeof(int32_t) * n_starts);
    *sum = s;
    return WA_OK;
}

int wa_gtsp_seam_tour_exact(wa_ctx *ctx, const double *dist, int32_t m, int32_t closed, int32_t *order_out, uint8_t *dir_out, int64_t *cost_q)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx) return WA_ERR_ARG;
    if (!dist || !order_out || !dir_out || !cost_q) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_exact: NULL dist or outputs");
    if (m < 1 || m > 1024) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_exact: 1 .. 1024 seams");
    const int M = closed ? m : m + 1, N2 = 2 * M, n = M - 1, ne = 2 * n;
    if (M > WA_ST_MAX_EXACT) return fail(ctx, WA_ERR_CAPACITY, "wa_gtsp_seam_tour_exact: more than 16 seams (the dummy of an open tour included)");
    std::vector<int64_t> W;
    bool narrow = true;
    int rc = st_quantise(ctx, "wa_gtsp_seam_tour_exact", dist, m, M, W, &narrow);
    if (rc) return rc;
    std::vector<uint16_t> E((size_t)M);
    E[0] = 0;
    int64_t opt = 0;
    if (n > 0) {
        const size_t cells = ((size_t)1 << n) * ne;
        CtxBuf<long long> dW(ctx), dF(ctx);
        hipError_t e = dW.alloc(W.size());
        e = e ? e : dF.alloc(cells);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_ALLOC, "wa_gtsp_seam_tour_exact: device buffers"); }
        e = hipMemcpyAsync(dW, W.data(), sizeof(int64_t) * W.size(), hipMemcpyHostToDevice, ctx->stream);
        for (int level = 1; level <= n && e == hipSuccess; level++) {
            k_seam_dp_level<<<(unsigned)((cells + 255) / 256), 256, 0, ctx->stream>>>(dW, M, level, dF);
            e = hipGetLastError();
        }
        std::vector<int64_t> f(cells);
        e = e ? e : hipMemcpyAsync(f.data(), dF, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_exact: %s", hipGetErrorString(e));
        // backtracking from the end: the lowest endpoint among equal values at every step
        unsigned S = (1u << n) - 1;
        int cur = -1;
        opt = WA_ST_INF;
        for (int e2 = 0; e2 < ne; e2++) {
            const int64_t v = f[(size_t)S * ne + e2] + W[(size_t)(e2 + 2) * N2 + 0];
            if (v < opt) { opt = v; cur = e2; }
        }
        for (int k = M - 1; k >= 1; k--) {
            E[(size_t)k] = (uint16_t)((cur ^ 1) + 2);   // cur is where the seam is left: it is entered at its other end
            const int64_t here = f[(size_t)S * ne + cur];
            const int in = (cur ^ 1) + 2;
            S ^= 1u << (cur >> 1);
            if (S == 0) break;
            int prev = -1;
            for (int e2 = 0; e2 < ne && prev < 0; e2++)
                if (((S >> (e2 >> 1)) & 1u) && f[(size_t)S * ne + e2] + W[(size_t)(e2 + 2) * N2 + in] == here) prev = e2;
            if (prev < 0) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_exact: the table does not backtrack");
            cur = prev;
        }
    }
    st_emit(E.data(), m, M, order_out, dir_out);
    *cost_q = opt;
    return WA_OK;
}
