// host_torch.inc -- C ABI: wa_traj_tool_axes and wa_traj_tool_check, the torch-axis planner (included by weldacs.hip inside extern "C").
// The host quantises the float inputs (rule 1) and checks the arguments; feasibility, the sequences and the counters stay on the
// device, on the context's stream; the host reads ONE WaTorchRec and the leg costs before it copies any output.

// Rule 1.  false: a component is not finite or the length is 0.
static bool torch_quantise(const float *v, short4 *out)
{
    const double x = v[0], y = v[1], z = v[2];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return false;
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0)) return false;
    out->x = (short)(int32_t)rint((x / len) * 16384.0);
    out->y = (short)(int32_t)rint((y / len) * 16384.0);
    out->z = (short)(int32_t)rint((z / len) * 16384.0);
    out->w = 1;
    return true;
}

// the tool as the device sees it; false: a value out of range
static bool torch_tool_dev(const wa_tool_beads *tool, int32_t near_add, WaTorchTool *out)
{
    memset(out, 0, sizeof *out);
    if (tool->n_beads < 1 || tool->n_beads > WA_TORCH_MAX_BEADS || near_add > (1 << 30)) return false;
    out->n_beads = tool->n_beads;
    for (int32_t j = 0; j < tool->n_beads; j++) {
        if (tool->dist16[j] < 0 || tool->dist16[j] > 65536 || tool->r2[j] < 0 || tool->r2[j] > (1 << 30)) return false;
        out->dist16[j] = tool->dist16[j];
        out->r2[j] = (uint32_t)tool->r2[j];
        out->rn[j] = (uint32_t)tool->r2[j] + (near_add >= 0 ? (uint32_t)near_add : 0u);
    }
    return true;
}

static const WaTorchRec TORCH_REC0 = {0, 0, 0, 0, ~0ull, 0, 0, 0, 0};

struct TorchBuffers {
    DevBuf<short4> q, wish;
    DevBuf<WaTorchTool> tool;
    DevBuf<WaTorchRec> rec;
    DevBuf<long long> off, leg_cost;
    DevBuf<int32_t> pin_first, pin_last, dir;
    CtxBuf<uint8_t> feas, back;   // n * K bytes each, from the context's arena
    DevBuf<uint8_t> blocked, near_;
    explicit TorchBuffers(wa_ctx *c) : feas(c), back(c) {}
};

static void torch_summary_from(const WaTorchRec &rec, int64_t n, wa_tool_summary *s)
{
    memset(s, 0, sizeof *s);
    s->n = n;
    s->n_outside = (int64_t)rec.n_outside;
    s->n_blocked_pairs = (int64_t)rec.n_blocked_pairs;
    s->n_no_dir = (int64_t)rec.n_no_dir;
    s->n_chosen_blocked = (int64_t)rec.n_chosen_blocked;
    s->first_chosen_blocked = rec.first_chosen_blocked == ~0ull ? -1 : (int64_t)rec.first_chosen_blocked;
    s->n_chosen_near = (int64_t)rec.n_chosen_near;
    s->n_over_turn = (int64_t)rec.n_over_turn;
    s->max_turn_taken = (int64_t)rec.max_turn_taken;
}

int wa_traj_tool_axes(const wa_grid *g, const wa_traj *t, const float *dirs, int32_t K, const wa_tool_beads *tool,
                      const wa_tool_weights *weights, const float *want, const int64_t *off, int32_t n_legs, const int32_t *pin_first,
                      const int32_t *pin_last, int32_t *dir_out, uint8_t *feas_out, int64_t *leg_cost, wa_tool_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!t || !dirs || !tool || !weights || !off || !sum) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: NULL argument");
    if (t->ctx != ctx) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: trajectory and grid belong to different contexts");
    if (K < 1 || K > WA_TORCH_MAX_DIRS) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: K must be 1 .. 256");
    if (n_legs < 0) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: negative number of legs");
    const wa_tool_weights W = *weights;
    if (W.w_near < 0 || W.w_near > 1024 || W.w_want < 0 || W.w_want > 1024 || W.w_turn < 0 || W.w_turn > 1024)
        return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: weights must be 0 .. 1024");
    WaTorchTool dt;
    if (!torch_tool_dev(tool, W.near_add, &dt)) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: n_beads, dist16, r2 or near_add out of range");
    const int64_t n = t->n;
    if (off[0] != 0 || off[n_legs] != n) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: off must run from 0 to the number of samples");
    bool long_leg = false;
    for (int32_t l = 0; l < n_legs; l++) {
        if (off[l + 1] < off[l]) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: off must not decrease");
        long_leg |= off[l + 1] - off[l] > ((int64_t)1 << 22);
        if ((pin_first && (pin_first[l] < -1 || pin_first[l] >= K)) || (pin_last && (pin_last[l] < -1 || pin_last[l] >= K)))
            return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: a pin must be -1 .. K-1");
    }
    std::vector<short4> hq((size_t)K), hw;
    for (int32_t k = 0; k < K; k++)
        if (!torch_quantise(dirs + 3 * (size_t)k, &hq[(size_t)k]))
            return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: a direction is not finite or has zero length");
    if (want) {
        hw.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const float *v = want + 3 * (size_t)i;
            if (v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f) hw[(size_t)i] = make_short4(0, 0, 0, 0);
            else if (!torch_quantise(v, &hw[(size_t)i])) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: a want entry is not finite");
        }
    }
    if (long_leg) return fail(ctx, WA_ERR_CAPACITY, "wa_traj_tool_axes: a leg holds more than 2^22 samples");
    if (n > (((int64_t)1 << 33) / K)) return fail(ctx, WA_ERR_CAPACITY, "wa_traj_tool_axes: n * K exceeds 2^33");
    WaField F;
    int rc = grid_field(g, &F);
    if (rc) return rc;
    WaTorchRec rec = TORCH_REC0;
    std::vector<int64_t> costs((size_t)n_legs, 0);
    TorchBuffers B(ctx);
    if (n > 0) {
        const size_t lds = (size_t)K * (size_t)dt.n_beads * sizeof(short4);
        if (lds > ((size_t)48 << 10)) {   // (the limit belongs to the function, per device: raised to the most a call can ask for)
            const hipError_t a = hipFuncSetAttribute((const void *)k_torch_nodes, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(WA_TORCH_MAX_DIRS * WA_TORCH_MAX_BEADS * sizeof(short4)));
            if (a != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_tool_axes: dynamic LDS limit: %s", hipGetErrorString(a));
        }
        const size_t nk = (size_t)n * (size_t)K;
        hipError_t e = B.q.alloc((size_t)K);
        e = e ? e : B.tool.alloc(1);
        e = e ? e : B.rec.alloc(1);
        e = e ? e : B.off.alloc((size_t)n_legs + 1);
        e = e ? e : B.leg_cost.alloc((size_t)n_legs);
        e = e ? e : B.dir.alloc((size_t)n);
        if (want) e = e ? e : B.wish.alloc((size_t)n);
        if (pin_first) e = e ? e : B.pin_first.alloc((size_t)n_legs);
        if (pin_last) e = e ? e : B.pin_last.alloc((size_t)n_legs);
        e = e ? e : B.feas.alloc(nk);
        e = e ? e : B.back.alloc(nk);
        if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_traj_tool_axes: device buffers");
        hipStream_t st = ctx->stream;
        e = hipMemcpyAsync(B.q, hq.data(), sizeof(short4) * (size_t)K, hipMemcpyHostToDevice, st);
        e = e ? e : hipMemcpyAsync(B.tool, &dt, sizeof dt, hipMemcpyHostToDevice, st);
        e = e ? e : hipMemcpyAsync(B.rec, &rec, sizeof rec, hipMemcpyHostToDevice, st);
        e = e ? e : hipMemcpyAsync(B.off, off, sizeof(long long) * ((size_t)n_legs + 1), hipMemcpyHostToDevice, st);
        if (want) e = e ? e : hipMemcpyAsync(B.wish, hw.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
        if (pin_first) e = e ? e : hipMemcpyAsync(B.pin_first, pin_first, sizeof(int32_t) * (size_t)n_legs, hipMemcpyHostToDevice, st);
        if (pin_last) e = e ? e : hipMemcpyAsync(B.pin_last, pin_last, sizeof(int32_t) * (size_t)n_legs, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            const unsigned tiles = (unsigned)((n + WA_TORCH_TILE - 1) / WA_TORCH_TILE);
            k_torch_nodes<<<tiles, 256, lds, st>>>(t->xyz, n, F, B.q, K, B.tool, B.feas, B.rec);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            const WaTorchDp P = {K, W.w_near, W.w_want, W.w_turn, W.max_turn};
            k_torch_dp<<<(unsigned)n_legs, (unsigned)((K + 63) / 64 * 64), 0, st>>>(B.q, B.wish, B.feas, B.off, B.pin_first, B.pin_last, P, B.back,
                                                                                    B.dir, B.leg_cost, B.rec);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(&rec, B.rec, sizeof rec, hipMemcpyDeviceToHost, st);
        e = e ? e : hipMemcpyAsync(costs.data(), B.leg_cost, sizeof(long long) * (size_t)n_legs, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_tool_axes: %s", hipGetErrorString(e));
        if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_axes: a coordinate of the trajectory is not finite");
        // (every WA_ERR_ARG has been answered by now: nothing was written before this line)
        if (dir_out) e = hipMemcpyAsync(dir_out, B.dir, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st);
        if (feas_out) e = e ? e : hipMemcpyAsync(feas_out, B.feas, nk, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_tool_axes: %s", hipGetErrorString(e));
        if (feas_out)
            for (size_t p = 0; p < nk; p++) feas_out[p] = (feas_out[p] & 0x80) ? 255 : feas_out[p];   // the kernels' byte -> rule 7
    }
    wa_tool_summary s;
    torch_summary_from(rec, n, &s);
    for (int32_t l = 0; l < n_legs; l++)
        if (costs[(size_t)l] < WA_TORCH_INF) s.cost = std::min<int64_t>(s.cost + costs[(size_t)l], WA_TORCH_INF);
    if (leg_cost) memcpy(leg_cost, costs.data(), sizeof(int64_t) * (size_t)n_legs);
    *sum = s;
    return WA_OK;
}

int wa_traj_tool_check(const wa_grid *g, const wa_traj *t, const float *axes, const wa_tool_beads *tool, int32_t near_add,
                       uint8_t *blocked_out, uint8_t *near_out, wa_tool_summary *sum)
{
    WaDevGuard dev_guard_(g ? g->ctx : nullptr);
    if (!dev_guard_.ok) return WA_ERR_DEVICE;   // the context's device could not be made current
    if (!g) return WA_ERR_ARG;
    wa_ctx *ctx = g->ctx;
    if (!t || !axes || !tool || !sum) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_check: NULL argument");
    if (t->ctx != ctx) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_check: trajectory and grid belong to different contexts");
    WaTorchTool dt;
    if (!torch_tool_dev(tool, near_add, &dt)) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_check: n_beads, dist16, r2 or near_add out of range");
    const int64_t n = t->n;
    if (n > ((int64_t)1 << 33)) return fail(ctx, WA_ERR_CAPACITY, "wa_traj_tool_check: more than 2^33 samples");
    std::vector<short4> hq((size_t)n);
    for (int64_t i = 0; i < n; i++)
        if (!torch_quantise(axes + 3 * (size_t)i, &hq[(size_t)i]))
            return fail(ctx, WA_ERR_ARG, "wa_traj_tool_check: an axis is not finite or has zero length");
    WaField F;
    int rc = grid_field(g, &F);
    if (rc) return rc;
    WaTorchRec rec = TORCH_REC0;
    if (n > 0) {
        TorchBuffers B(ctx);
        hipError_t e = B.q.alloc((size_t)n);
        e = e ? e : B.tool.alloc(1);
        e = e ? e : B.rec.alloc(1);
        e = e ? e : B.blocked.alloc((size_t)n);
        e = e ? e : B.near_.alloc((size_t)n);
        if (e != hipSuccess) return fail(ctx, WA_ERR_ALLOC, "wa_traj_tool_check: device buffers");
        hipStream_t st = ctx->stream;
        e = hipMemcpyAsync(B.q, hq.data(), sizeof(short4) * (size_t)n, hipMemcpyHostToDevice, st);
        e = e ? e : hipMemcpyAsync(B.tool, &dt, sizeof dt, hipMemcpyHostToDevice, st);
        e = e ? e : hipMemcpyAsync(B.rec, &rec, sizeof rec, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            k_torch_check<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t->xyz, n, F, B.q, B.tool, B.blocked, B.near_, B.rec);
            e = hipGetLastError();
        }
        e = e ? e : hipMemcpyAsync(&rec, B.rec, sizeof rec, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_tool_check: %s", hipGetErrorString(e));
        if (rec.bad & 1) return fail(ctx, WA_ERR_ARG, "wa_traj_tool_check: a coordinate of the trajectory is not finite");
        if (blocked_out) e = hipMemcpyAsync(blocked_out, B.blocked, (size_t)n, hipMemcpyDeviceToHost, st);
        if (near_out) e = e ? e : hipMemcpyAsync(near_out, B.near_, (size_t)n, hipMemcpyDeviceToHost, st);
        e = e ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(ctx, WA_ERR_DEVICE, "wa_traj_tool_check: %s", hipGetErrorString(e));
    }
    wa_tool_summary s;
    torch_summary_from(rec, n, &s);
    s.n_blocked_pairs = s.n_no_dir = s.n_chosen_blocked;
    *sum = s;
    return WA_OK;
}
