// host_seamrules.inc -- C ABI: wa_gtsp_seam_tour_rules / wa_gtsp_seam_tour_rules_exact / wa_gtsp_seam_rules_check, seam tours under precedences
// and one-way seams (DESIGN §4aa; included by weldacs.hip inside extern "C", behind host_seamtour.inc whose st_quantise, st_emit and
// st_cost it shares).  The host checks the rules (range, duplicates, cycles), quantises the costs and validates start 0; the search,
// the repair of every drawn start and the subset programme run on the device in integers, on the context's stream.
extern "C++" {
struct SrRules {
    int M = 0, anchor = 0, n_pairs = 0, n_fixed = 0;
    std::vector<int32_t> succ_at, succ, pred_at, pred;   // the distinct pairs as lists by seam (M + 1 offsets each)
    std::vector<uint8_t> fixed;                          // M bytes, the dummy's 0
};

// NULL, or what is wrong with the rules
static const char *sr_rules(int m, int closed, const int32_t *before, const int32_t *after, int n_prec, const uint8_t *fixed, SrRules &R)
{
    if (m < 1 || m > 1024) return "1 .. 1024 seams";
    if (n_prec < 0 || n_prec > 65536) return "n_prec is 0 .. 65536";
    if (n_prec > 0 && (!before || !after)) return "NULL before / after with n_prec > 0";
    const int M = closed ? m : m + 1;
    R.M = M;
    R.anchor = closed ? 0 : m;
    R.fixed.assign((size_t)M, 0);
    R.n_fixed = 0;
    for (int s = 0; s < m && fixed; s++) {
        if (fixed[s] > 2) return "a fixed byte is 0, 1 or 2";
        R.fixed[(size_t)s] = fixed[s];
        R.n_fixed += fixed[s] != 0;
    }
    std::vector<uint32_t> key((size_t)n_prec);
    for (int k = 0; k < n_prec; k++) {
        const int32_t a = before[k], b = after[k];
        if (a < 0 || a >= m || b < 0 || b >= m) return "a pair names a seam outside 0 .. m-1";
        if (a == b) return "a seam before itself";
        if (closed && b == 0) return "a closed tour starts with seam 0: nothing goes before it";
        key[(size_t)k] = ((uint32_t)a << 16) | (uint32_t)b;
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    const int n = (int)key.size();
    R.n_pairs = n;
    R.succ_at.assign((size_t)M + 1, 0);
    R.pred_at.assign((size_t)M + 1, 0);
    R.succ.assign((size_t)std::max(n, 1), 0);
    R.pred.assign((size_t)std::max(n, 1), 0);
    for (int k = 0; k < n; k++) {
        R.succ_at[(size_t)(key[(size_t)k] >> 16) + 1]++;
        R.pred_at[(size_t)(key[(size_t)k] & 0xffff) + 1]++;
    }
    for (int s = 0; s < M; s++) {
        R.succ_at[(size_t)s + 1] += R.succ_at[(size_t)s];
        R.pred_at[(size_t)s + 1] += R.pred_at[(size_t)s];
    }
    std::vector<int32_t> fill(R.pred_at.begin(), R.pred_at.end() - 1);
    for (int k = 0; k < n; k++) {   // (sorted by `before`: the successor lists fill in order)
        R.succ[(size_t)k] = (int32_t)(key[(size_t)k] & 0xffff);
        R.pred[(size_t)fill[(size_t)(key[(size_t)k] & 0xffff)]++] = (int32_t)(key[(size_t)k] >> 16);
    }
    // a cycle leaves seams that never become ready
    std::vector<int32_t> left((size_t)M), ready;
    for (int s = 0; s < M; s++) {
        left[(size_t)s] = R.pred_at[(size_t)s + 1] - R.pred_at[(size_t)s];
        if (!left[(size_t)s]) ready.push_back(s);
    }
    int done = 0;
    while (!ready.empty()) {
        const int s = ready.back();
        ready.pop_back();
        done++;
        for (int q = R.succ_at[(size_t)s]; q < R.succ_at[(size_t)s + 1]; q++)
            if (--left[(size_t)R.succ[(size_t)q]] == 0) ready.push_back(R.succ[(size_t)q]);
    }
    if (done != M) return "the pairs hold a cycle";
    return nullptr;
}

// the repair of the identity order: the anchor, then always the lowest seam whose predecessors are placed
static void sr_identity(const SrRules &R, std::vector<int32_t> &order)
{
    const int M = R.M;
    std::vector<int32_t> left((size_t)M);
    for (int s = 0; s < M; s++) left[(size_t)s] = R.pred_at[(size_t)s + 1] - R.pred_at[(size_t)s];
    order.clear();
    for (int step = 0; step < M; step++) {
        int s = R.anchor;
        if (step)
            for (s = 0; s < M && left[(size_t)s] != 0; s++) {}
        left[(size_t)s] = -1;
        for (int q = R.succ_at[(size_t)s]; q < R.succ_at[(size_t)s + 1]; q++) left[(size_t)R.succ[(size_t)q]]--;
        order.push_back(s);
    }
}

// pairs out of order in a state read from position 0 (every distinct pair once)
static int sr_bad_pairs(const SrRules &R, const uint16_t *E)
{
    std::vector<int32_t> pos((size_t)R.M);
    for (int k = 0; k < R.M; k++) pos[(size_t)(E[k] >> 1)] = k;
    int bad = 0;
    for (int s = 0; s < R.M; s++)
        for (int q = R.succ_at[(size_t)s]; q < R.succ_at[(size_t)s + 1]; q++) bad += pos[(size_t)s] >= pos[(size_t)R.succ[(size_t)q]];
    return bad;
}

template <typename WT, bool W_LDS, int TEAM>
static hipError_t sr_launch(wa_ctx *ctx, const WaSrArgs &a, size_t lds)
{
    hipError_t e = hipFuncSetAttribute((const void *)k_seam_descend_rules<WT, W_LDS, TEAM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int teams = WA_ST_BLOCK / TEAM;
    const long long want = ((long long)a.st.n_starts + teams - 1) / teams;
    const long long per_cu = std::min<long long>(32 / (WA_ST_BLOCK / 64), std::max<long long>(1, (long long)(160 * 1024 / lds)));
    const long long cap = (long long)std::max(1, ctx->prop.multiProcessorCount) * per_cu;   // resident blocks: each loops over its starts
    k_seam_descend_rules<WT, W_LDS, TEAM><<<(unsigned)std::min(want, cap), WA_ST_BLOCK, lds, ctx->stream>>>(a);
    return hipGetLastError();
}
}

int wa_gtsp_seam_tour_rules(wa_ctx *ctx, const double *dist, int32_t m, const wa_seam_params *prm, const int32_t *before, const int32_t *after,
                            int32_t n_prec, const uint8_t *fixed, const int32_t *order0, const uint8_t *dir0, int32_t *order_out, uint8_t *dir_out,
                            int64_t *start_cost_q_out, int32_t *start_passes_out, wa_seam_rules_summary *sum)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx) return WA_ERR_ARG;
    if (!dist || !prm || !order_out || !dir_out || !sum) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: NULL dist, params, outputs or summary");
    if (prm->or_len < 0 || prm->or_len > 3 || prm->n_starts < 1 || prm->n_starts > (1 << 20) || prm->max_passes < 1 || prm->max_passes > (1 << 20))
        return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: or_len 0 .. 3, n_starts and max_passes 1 .. 2^20");
    SrRules R;
    if (const char *why = sr_rules(m, prm->closed, before, after, n_prec, fixed, R)) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: %s", why);
    const int M = R.M, N2 = 2 * M, n_starts = prm->n_starts;
    // start 0: the anchor at position 0, then order0 / dir0 as given (they must be admissible) or the repair of the identity
    std::vector<uint16_t> e0((size_t)M);
    {
        std::vector<int32_t> ident;
        if (!order0) sr_identity(R, ident);
        std::vector<uint8_t> seen((size_t)m, 0);
        const int shift = M - m;
        if (shift) e0[0] = (uint16_t)(2 * m);
        for (int k = 0; k < m; k++) {
            const int32_t s = order0 ? order0[k] : ident[(size_t)(k + shift)];
            if (s < 0 || s >= m || seen[(size_t)s]) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: order0 is not a permutation of the seams");
            seen[(size_t)s] = 1;
            if (dir0 && dir0[k] > 1) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: dir0 entries are 0 or 1");
            const int fx = R.fixed[(size_t)s], d = dir0 ? dir0[k] : (fx ? fx - 1 : 0);
            if (fx && d != fx - 1) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: dir0 enters a one-way seam at the wrong end");
            e0[(size_t)(k + shift)] = (uint16_t)(2 * s + d);
        }
        if ((e0[0] >> 1) != R.anchor) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: order0 of a closed tour starts with seam 0");
        if (sr_bad_pairs(R, e0.data())) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules: order0 breaks a precedence");
    }
    std::vector<int64_t> W;
    bool narrow = true;
    int rc = st_quantise(ctx, "wa_gtsp_seam_tour_rules", dist, m, M, W, &narrow);
    if (rc) return rc;

    // where W lives and who holds a descent: §4n's rule with the wider state (a wavefront up to 64 positions, the workgroup above)
    const int Mpad = (M + 7) & ~7;
    const bool wave = M <= 64;
    const size_t state = (size_t)(wave ? 4 : 1) * WA_SR_WORDS * Mpad * sizeof(uint16_t) + (WA_ST_BLOCK / 64) * 16;
    const size_t w_narrow = ((size_t)N2 * N2 * 4 + 15) & ~(size_t)15, w_wide = ((size_t)N2 * N2 * 8 + 15) & ~(size_t)15;
    const size_t lds_max = 160 * 1024;
    const bool w_lds = wave || (narrow && w_narrow + state <= lds_max);
    const size_t lds = state + (w_lds ? (narrow ? w_narrow : w_wide) : 0);

    CtxBuf<unsigned char> dW(ctx);   // uint32_t or long long entries
    CtxBuf<uint16_t> dE0(ctx), dTours(ctx);
    CtxBuf<long long> dCost(ctx);
    CtxBuf<int32_t> dPass(ctx), dSuccAt(ctx), dSucc(ctx), dPredAt(ctx), dPred(ctx);
    CtxBuf<uint8_t> dCap(ctx), dFixed(ctx);
    hipError_t e = dW.alloc((size_t)N2 * N2 * (narrow ? 4 : 8));
    e = e ? e : dE0.alloc((size_t)M);
    e = e ? e : dCost.alloc((size_t)n_starts);
    e = e ? e : dPass.alloc((size_t)n_starts);
    e = e ? e : dCap.alloc((size_t)n_starts);
    e = e ? e : dTours.alloc((size_t)n_starts * M);
    e = e ? e : dSuccAt.alloc(R.succ_at.size());
    e = e ? e : dPredAt.alloc(R.pred_at.size());
    e = e ? e : dSucc.alloc(R.succ.size());
    e = e ? e : dPred.alloc(R.pred.size());
    e = e ? e : dFixed.alloc(R.fixed.size());
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_ALLOC, "wa_gtsp_seam_tour_rules: device buffers"); }
    std::vector<uint32_t> W32;
    if (narrow) {
        W32.resize(W.size());
        for (size_t k = 0; k < W.size(); k++) W32[k] = (uint32_t)W[k];
        e = hipMemcpyAsync(dW, W32.data(), W32.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    } else {
        e = hipMemcpyAsync(dW, W.data(), W.size() * 8, hipMemcpyHostToDevice, ctx->stream);
    }
    e = e ? e : hipMemcpyAsync(dE0, e0.data(), sizeof(uint16_t) * M, hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(dSuccAt, R.succ_at.data(), sizeof(int32_t) * R.succ_at.size(), hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(dPredAt, R.pred_at.data(), sizeof(int32_t) * R.pred_at.size(), hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(dSucc, R.succ.data(), sizeof(int32_t) * R.succ.size(), hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(dPred, R.pred.data(), sizeof(int32_t) * R.pred.size(), hipMemcpyHostToDevice, ctx->stream);
    e = e ? e : hipMemcpyAsync(dFixed, R.fixed.data(), R.fixed.size(), hipMemcpyHostToDevice, ctx->stream);
    WaSrArgs a;
    a.st.W = dW;
    a.st.e0 = dE0;
    a.st.M = M; a.st.or_len = prm->or_len; a.st.n_starts = n_starts; a.st.max_passes = prm->max_passes;
    a.st.seed = prm->seed;
    a.st.cost = dCost; a.st.passes = dPass; a.st.capped = dCap; a.st.tours = dTours;
    a.succ_at = dSuccAt; a.succ = dSucc; a.pred_at = dPredAt; a.pred = dPred; a.fixed = dFixed;
    a.anchor = R.anchor;
    if (e == hipSuccess) {
        if (wave) e = narrow ? sr_launch<uint32_t, true, 64>(ctx, a, lds) : sr_launch<long long, true, 64>(ctx, a, lds);
        else if (w_lds) e = sr_launch<uint32_t, true, 256>(ctx, a, lds);
        else e = narrow ? sr_launch<uint32_t, false, 256>(ctx, a, lds) : sr_launch<long long, false, 256>(ctx, a, lds);
    }
    std::vector<int64_t> cost((size_t)n_starts);
    std::vector<int32_t> passes((size_t)n_starts);
    std::vector<uint8_t> capped((size_t)n_starts);
    e = e ? e : hipMemcpyAsync(cost.data(), dCost, sizeof(int64_t) * n_starts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipMemcpyAsync(passes.data(), dPass, sizeof(int32_t) * n_starts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipMemcpyAsync(capped.data(), dCap, (size_t)n_starts, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_rules: %s", hipGetErrorString(e));
    wa_seam_rules_summary s;
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
    s.n_prec = R.n_pairs;
    s.n_fixed = R.n_fixed;
    std::vector<uint16_t> best((size_t)M);
    e = hipMemcpyAsync(best.data(), dTours.p + (size_t)s.best_start * M, sizeof(uint16_t) * M, hipMemcpyDeviceToHost, ctx->stream);
    e = e ? e : hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_rules: %s", hipGetErrorString(e));
    st_emit(best.data(), m, M, order_out, dir_out);
    if (start_cost_q_out) memcpy(start_cost_q_out, cost.data(), sizeof(int64_t) * n_starts);
    if (start_passes_out) memcpy(start_passes_out, passes.data(), sizeof(int32_t) * n_starts);
    *sum = s;
    return WA_OK;
}

int wa_gtsp_seam_tour_rules_exact(wa_ctx *ctx, const double *dist, int32_t m, int32_t closed, const int32_t *before, const int32_t *after, int32_t n_prec,
                                  const uint8_t *fixed, int32_t *order_out, uint8_t *dir_out, int64_t *cost_q)
{
    WaDevGuard dev_guard_(ctx);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!ctx) return WA_ERR_ARG;
    if (!dist || !order_out || !dir_out || !cost_q) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules_exact: NULL dist or outputs");
    SrRules R;
    if (const char *why = sr_rules(m, closed, before, after, n_prec, fixed, R)) return fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_tour_rules_exact: %s", why);
    const int M = R.M, N2 = 2 * M, n = M - 1, ne = 2 * n;
    if (M > WA_ST_MAX_EXACT) return fail(ctx, WA_ERR_CAPACITY, "wa_gtsp_seam_tour_rules_exact: more than 16 seams (the dummy of an open tour included)");
    std::vector<int64_t> W;
    bool narrow = true;
    int rc = st_quantise(ctx, "wa_gtsp_seam_tour_rules_exact", dist, m, M, W, &narrow);
    if (rc) return rc;
    // the anchor becomes seam 0 of the programme: an open tour's dummy moves to the front and seam s becomes s + 1
    std::vector<int> seam_of((size_t)M), label((size_t)M);
    for (int t = 0; t < M; t++) seam_of[(size_t)t] = closed ? t : (t ? t - 1 : m);
    for (int t = 0; t < M; t++) label[(size_t)seam_of[(size_t)t]] = t;
    std::vector<uint32_t> predmask((size_t)std::max(n, 1), 0);
    std::vector<uint8_t> fx((size_t)std::max(n, 1), 0);
    for (int t = 0; t < n; t++) {
        const int s = seam_of[(size_t)t + 1];
        fx[(size_t)t] = R.fixed[(size_t)s];
        for (int q = R.pred_at[(size_t)s]; q < R.pred_at[(size_t)s + 1]; q++)
            if (label[(size_t)R.pred[(size_t)q]] >= 1) predmask[(size_t)t] |= 1u << (label[(size_t)R.pred[(size_t)q]] - 1);
    }
    std::vector<uint16_t> E((size_t)M), Ebest((size_t)M);
    int64_t opt = WA_ST_INF;
    CtxBuf<long long> dW(ctx), dF(ctx);
    CtxBuf<uint32_t> dMask(ctx);
    CtxBuf<uint8_t> dFx(ctx);
    const size_t cells = n > 0 ? ((size_t)1 << n) * ne : 0;
    std::vector<int64_t> f(cells), Wa(W.size());
    if (n > 0) {
        hipError_t e = dW.alloc(W.size());
        e = e ? e : dF.alloc(cells);
        e = e ? e : dMask.alloc(predmask.size());
        e = e ? e : dFx.alloc(fx.size());
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, WA_ERR_ALLOC, "wa_gtsp_seam_tour_rules_exact: device buffers"); }
        e = hipMemcpyAsync(dMask, predmask.data(), sizeof(uint32_t) * predmask.size(), hipMemcpyHostToDevice, ctx->stream);
        e = e ? e : hipMemcpyAsync(dFx, fx.data(), fx.size(), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_rules_exact: %s", hipGetErrorString(e));
    }
    // one table per permitted direction of the anchor (the dummy has one); of equal costs the d = 0 table wins
    for (int d = 0; d < (closed ? 2 : 1); d++) {
        if (closed && R.fixed[0] && R.fixed[0] - 1 != d) continue;
        if (n == 0) {
            E[0] = (uint16_t)d;
            if (0 < opt) { opt = 0; Ebest = E; }
            continue;
        }
        // W with the programme's labels; for d = 1 the anchor's two endpoints change places
        auto src = [&](int x) { const int t = x >> 1, b = (x & 1) ^ (t == 0 ? d : 0); return 2 * seam_of[(size_t)t] + b; };
        for (int x = 0; x < N2; x++)
            for (int y = 0; y < N2; y++) Wa[(size_t)x * N2 + y] = W[(size_t)src(x) * N2 + src(y)];
        hipError_t e = hipMemcpyAsync(dW, Wa.data(), sizeof(int64_t) * Wa.size(), hipMemcpyHostToDevice, ctx->stream);
        for (int level = 1; level <= n && e == hipSuccess; level++) {
            k_seam_rules_dp_level<<<(unsigned)((cells + 255) / 256), 256, 0, ctx->stream>>>(dW, M, level, dMask, dFx, dF);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(f.data(), dF, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, ctx->stream);
        e = e ? e : hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_rules_exact: %s", hipGetErrorString(e));
        // backtracking from the end: the lowest endpoint among equal values at every step
        unsigned S = (1u << n) - 1;
        int cur = -1;
        int64_t c = WA_ST_INF;
        for (int e2 = 0; e2 < ne; e2++) {
            const int64_t p = f[(size_t)S * ne + e2];
            if (p < WA_ST_INF && p + Wa[(size_t)(e2 + 2) * N2 + 0] < c) { c = p + Wa[(size_t)(e2 + 2) * N2 + 0]; cur = e2; }
        }
        if (cur < 0) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_rules_exact: the table holds no tour");
        E[0] = 0;
        for (int k = M - 1; k >= 1; k--) {
            E[(size_t)k] = (uint16_t)((cur ^ 1) + 2);   // cur is where the seam is left: it is entered at its other end
            const int64_t here = f[(size_t)S * ne + cur];
            const int in = (cur ^ 1) + 2;
            S ^= 1u << (cur >> 1);
            if (S == 0) break;
            int prev = -1;
            for (int e2 = 0; e2 < ne && prev < 0; e2++) {
                const int64_t p = f[(size_t)S * ne + e2];
                if (((S >> (e2 >> 1)) & 1u) && p < WA_ST_INF && p + Wa[(size_t)(e2 + 2) * N2 + in] == here) prev = e2;
            }
            if (prev < 0) return fail(ctx, WA_ERR_DEVICE, "wa_gtsp_seam_tour_rules_exact: the table does not backtrack");
            cur = prev;
        }
        if (c < opt) {
            opt = c;
            for (int k = 0; k < M; k++) Ebest[(size_t)k] = (uint16_t)src(E[(size_t)k]);   // back to the caller's endpoints
        }
    }
    st_emit(Ebest.data(), m, M, order_out, dir_out);
    *cost_q = opt;
    return WA_OK;
}

int wa_gtsp_seam_rules_check(wa_ctx *ctx, int32_t m, int32_t closed, const int32_t *before, const int32_t *after, int32_t n_prec, const uint8_t *fixed,
                             const int32_t *order, const uint8_t *dir, int64_t *n_bad_prec_out, int64_t *n_bad_dir_out)
{
    // (host only: no device guard, and a NULL context is fine -- it only keeps the text for wa_last_error)
    if (!order || !dir || !n_bad_prec_out || !n_bad_dir_out) return ctx ? fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_rules_check: NULL tour or outputs") : WA_ERR_ARG;
    SrRules R;
    if (const char *why = sr_rules(m, closed, before, after, n_prec, fixed, R)) return ctx ? fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_rules_check: %s", why) : WA_ERR_ARG;
    // the tour as the caller holds it, read from its anchor: seam 0 of a closed tour, the start of an open one
    std::vector<int32_t> pos((size_t)m, -1);
    int at = 0;
    for (int k = 0; k < m; k++) {
        if (order[k] < 0 || order[k] >= m || pos[(size_t)order[k]] >= 0 || dir[k] > 1)
            return ctx ? fail(ctx, WA_ERR_ARG, "wa_gtsp_seam_rules_check: order is a permutation of the seams, dir entries are 0 or 1") : WA_ERR_ARG;
        pos[(size_t)order[k]] = k;
        if (closed && order[k] == 0) at = k;
    }
    int64_t bad_p = 0, bad_d = 0;
    for (int k = 0; k < n_prec; k++)   // every given pair counts, a duplicate as often as it is given
        bad_p += (pos[(size_t)before[k]] - at + m) % m >= (pos[(size_t)after[k]] - at + m) % m;
    for (int k = 0; k < m; k++) bad_d += R.fixed[(size_t)order[k]] && dir[k] != R.fixed[(size_t)order[k]] - 1;
    *n_bad_prec_out = bad_p;
    *n_bad_dir_out = bad_d;
    return WA_OK;
}
