// host_gtsp.inc -- C ABI: ACS-TSP seam ordering (included by weldacs.hip inside extern "C")
// ------------------------------------------------------------------ GTSP
int wa_gtsp_solve(wa_ctx *ctx, const double *dist, int32_t n, int32_t cnt, int32_t n_instances,
                  const wa_gtsp_params *p, int32_t *rand_state36, int32_t *tour_edges,
                  double *tour_cost, int32_t *iterations, double *pheromone_out)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx || !dist || !p || !tour_edges || n < 2 || n_instances < 1) return fail(ctx, WA_ERR_ARG, "wa_gtsp_solve: bad argument");
    if (p->rng_mode == WA_RNG_REF && n_instances != 1) return fail(ctx, WA_ERR_ARG, "wa_gtsp_solve: REF mode runs one instance");
    const size_t I = (size_t)n_instances, nn = (size_t)n * n;
    WaGtspDev G;
    memset(&G, 0, sizeof G);
    double *d_dist = nullptr;
    hipError_t e = hipSuccess;
    e = e ? e : dalloc(&d_dist, I * nn);
    e = e ? e : dalloc(&G.pher, I * nn);
    e = e ? e : dalloc(&G.h6, I * nn);
    e = e ? e : dalloc(&G.info, I * (size_t)257 * n + I * nn);
    e = e ? e : dalloc(&G.antL, I * n);
    e = e ? e : dalloc(&G.tours, I * nn * 2);
    e = e ? e : dalloc(&G.best, I * n * 2);
    e = e ? e : dalloc(&G.inJ, I * nn);
    e = e ? e : dalloc(&G.rbuf, nn);
    e = e ? e : dalloc(&G.rng, 1);
    e = e ? e : dalloc(&G.out_cost, I);
    e = e ? e : dalloc(&G.out_iters, I);
    auto cleanup = [&]() {
        dev_free(d_dist); dev_free(G.pher); dev_free(G.h6); dev_free(G.info); dev_free(G.antL); dev_free(G.tours);
        dev_free(G.best); dev_free(G.inJ); dev_free(G.rbuf); dev_free(G.rng); dev_free(G.out_cost); dev_free(G.out_iters);
    };
    if (e != hipSuccess) { cleanup(); return fail(ctx, WA_ERR_ALLOC, "wa_gtsp_solve: %s", hipGetErrorString(e)); }
    G.dist = d_dist;
    G.n = n; G.cnt = cnt; G.max_iterations = p->max_iterations; G.rng_mode = p->rng_mode;
    G.seed = p->seed; G.stream0 = p->stream;
    WaGlibcRand r;
    if (rand_state36) { memcpy(r.r, rand_state36, sizeof(int32_t) * 34); r.f = rand_state36[34]; r.b = rand_state36[35]; }
    else wa_glibc_seed(&r, 1);
    hipError_t h = hipMemcpyAsync(d_dist, dist, sizeof(double) * I * nn, hipMemcpyHostToDevice, ctx->stream);
    h = h ? h : hipMemcpyAsync(G.rng, &r, sizeof r, hipMemcpyHostToDevice, ctx->stream);
    h = h ? h : hipMemsetAsync(G.best, 0, sizeof(int32_t) * I * n * 2, ctx->stream);
    if (h == hipSuccess) {
        // fast path: lanes = ants, info matrix in LDS (rows padded to the mask width, odd stride) when
        // it fits; for n <= 64 the per-ant prefix sums live there too (binary-search second pass)
        const int nw = n <= 64 ? 1 : (n <= 128 ? 2 : 4);
        const size_t ld = (size_t)(64 * nw + 1);
        const size_t info_bytes = sizeof(double) * ld * n;
        const bool in_lds = info_bytes <= 140 * 1024;
        const unsigned threads = (unsigned)(((n + 63) / 64) * 64);
        const bool prefix = nw == 1;
        // one instance (or a few): spread each ant over a wavefront; many instances already fill the GPU with the
        // lanes-as-ants kernel (64 instances x 64 cities: 48 ms vs 82 ms), so the choice goes by the wave count
        const bool wave_path = env_int("WA_GTSP_WAVE", (int64_t)n_instances * n <= 1024 ? 1 : 0) != 0;
        if (n <= 256 && wave_path && env_int("WA_GTSP_GENERIC", 0) == 0) {
            // wave-per-ant path: lanes = cities, grid = (ants, instances); construct -> update per iteration
            WaGtspWave W;
            W.G = G;
            W.state = nullptr;
            W.valid = nullptr;
            h = dalloc(&W.state, I);
            h = h ? h : dalloc(&W.valid, I * n);
            // cities per lane: the n ordered additions are sequential whatever the layout, but a lane-to-lane hop
            // (two DPP moves) costs several additions, so few lanes with many cities each win (n/NC hops per step)
            const int nc = n <= 128 ? 8 : 16;
            const size_t info_bytes_w = sizeof(double) * nn;
            const bool stage = info_bytes_w <= 128 * 1024;
            const size_t shm_w = stage ? info_bytes_w : 0;
            const int32_t max_it = p->max_iterations > 0 ? p->max_iterations : n * n;
            std::vector<WaGtspState> hst(I);
#define WA_GTSPW_CONSTRUCT(NC, ST)                                                                                            \
    do {                                                                                                                      \
        if (!attr_set) h = hipFuncSetAttribute((const void *)k_gtspw_construct<NC, ST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_w); \
        if (h == hipSuccess) k_gtspw_construct<NC, ST><<<dim3((unsigned)n, (unsigned)n_instances), 64, shm_w, ctx->stream>>>(W, it);           \
    } while (0)
            if (h == hipSuccess) {
                k_gtspw_init<<<(unsigned)n_instances, 256, 0, ctx->stream>>>(W);
                h = hipGetLastError();
            }
            bool attr_set = false;
            for (int32_t it = 0; h == hipSuccess && it < max_it; it++) {
                if (nc == 8) { if (stage) WA_GTSPW_CONSTRUCT(8, true); else WA_GTSPW_CONSTRUCT(8, false); }
                else { if (stage) WA_GTSPW_CONSTRUCT(16, true); else WA_GTSPW_CONSTRUCT(16, false); }
                attr_set = true;
                if (h == hipSuccess) k_gtspw_update<<<(unsigned)n_instances, 256, 0, ctx->stream>>>(W, it);
                if ((it & 7) == 7 || it == max_it - 1) {   // poll the stagnation stop (:263)
                    h = h ? h : hipMemcpyAsync(hst.data(), W.state, sizeof(WaGtspState) * I, hipMemcpyDeviceToHost, ctx->stream);
                    h = h ? h : hipStreamSynchronize(ctx->stream);
                    bool all = true;
                    for (auto &x : hst) all = all && x.stop != 0;
                    if (all) break;
                }
            }
#undef WA_GTSPW_CONSTRUCT
            if (h == hipSuccess) h = hipGetLastError();
            h = h ? h : hipStreamSynchronize(ctx->stream);
            dev_free(W.state);
            dev_free(W.valid);
        } else if (n <= 256 && env_int("WA_GTSP_GENERIC", 0) == 0) {
            size_t shm = (in_lds ? info_bytes : 0) + (prefix ? sizeof(double) * ld * threads : 0);
#define WA_GTSP_LAUNCH(NW, LDS, PFX)                                                                                     \
    do {                                                                                                                 \
        h = hipFuncSetAttribute((const void *)k_gtsp_fast<NW, LDS, PFX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
        if (h == hipSuccess) k_gtsp_fast<NW, LDS, PFX><<<(unsigned)n_instances, threads, shm, ctx->stream>>>(G);         \
    } while (0)
            if (nw == 1) WA_GTSP_LAUNCH(1, true, true);
            else if (nw == 2 && in_lds) WA_GTSP_LAUNCH(2, true, false);
            else if (nw == 2) WA_GTSP_LAUNCH(2, false, false);
            else WA_GTSP_LAUNCH(4, false, false);
#undef WA_GTSP_LAUNCH
        } else {
            k_gtsp<<<(unsigned)n_instances, 256, 0, ctx->stream>>>(G);
        }
        if (h == hipSuccess) h = hipGetLastError();
    }
    std::vector<double> cost(I);
    std::vector<int32_t> its(I);
    h = h ? h : hipMemcpyAsync(tour_edges, G.best, sizeof(int32_t) * I * n * 2, hipMemcpyDeviceToHost, ctx->stream);
    h = h ? h : hipMemcpyAsync(cost.data(), G.out_cost, sizeof(double) * I, hipMemcpyDeviceToHost, ctx->stream);
    h = h ? h : hipMemcpyAsync(its.data(), G.out_iters, sizeof(int32_t) * I, hipMemcpyDeviceToHost, ctx->stream);
    h = h ? h : hipMemcpyAsync(&r, G.rng, sizeof r, hipMemcpyDeviceToHost, ctx->stream);
    if (pheromone_out) h = h ? h : hipMemcpyAsync(pheromone_out, G.pher, sizeof(double) * I * nn, hipMemcpyDeviceToHost, ctx->stream);
    h = h ? h : hipStreamSynchronize(ctx->stream);
    cleanup();
    if (h != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_solve: %s", hipGetErrorString(h));
    for (size_t i = 0; i < I; i++) {
        if (tour_cost) tour_cost[i] = cost[i];
        if (iterations) iterations[i] = its[i];
    }
    if (rand_state36 && p->rng_mode == WA_RNG_REF) { memcpy(rand_state36, r.r, sizeof(int32_t) * 34); rand_state36[34] = r.f; rand_state36[35] = r.b; }
    return WA_OK;
}

