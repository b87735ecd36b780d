// acs_plan.hpp -- the ACS solver's device memory, written down ONCE: every block a solver takes from the context's allocator is a row
// of the plan, in the order it is asked for.  acs_create_once (host_acs.inc) walks the rows to allocate, fill and later free them;
// wa_acs_memory_estimate and wa_acs_straggler_pool_bytes are sums over the same rows.  A new array of the solver is one row here and one
// pointer assignment there.  Plain host C++14 without a HIP header: tests/cpp/acs_plan_check.cpp builds it with g++ and the sanitizers.
// (The trace buffers, the result staging block and the diagnostic hash log grow on demand outside the allocator: not in the plan.)
#pragma once
#include <stdint.h>

#include <vector>

// what the kernels' headers call WA_REF_SPEC_LEN, WA_REF_SUPER, WA_RESUME_MAX, WA_POOL_REC (acs_dev.hpp) and WA_ROW26 (acs_nb26.hpp):
// host_acs.inc holds the two sets against each other
constexpr int64_t WA_PLAN_REF_SPEC_LEN = 4096, WA_PLAN_REF_SUPER = 1024, WA_PLAN_RESUME_MAX = 256, WA_PLAN_POOL_REC = 4, WA_PLAN_ROW26 = 32;

struct WaPlanIn {
    int64_t n;                    // voxels of the grid
    int32_t nxy, n_slots, max_colony;   // nxy: nx * ny
    int32_t fields0;              // heuristic fields the pool starts with (the rule: host_acs.inc acs_plan_in, mirrored by tests/test_wide_batch_rules.py)
    int64_t path_capacity;        // as asked for (<= 0: the default)
    int32_t nb, lazy;             // 6 or 26 neighbours; lazy evaporation
    int32_t mask_u64, replay, ref_spec, stragglers, straggler_slots;   // WA_MASK_U64 (0), WA_REPLAY (1), WA_REF_SPEC (1), WA_STRAGGLERS (1), WA_STRAGGLER_SLOTS (16)
    int64_t sizeof_ctl, sizeof_rng;                                     // sizeof(WaSlotCtl), sizeof(WaGlibcRand)
};

enum WaFill { WA_FILL_NONE, WA_FILL_ZERO, WA_FILL_ONES };   // what a block holds when the solver is created: anything, 0x00 bytes, 0xff bytes

struct WaPlanRow {
    const char *name;
    int64_t elem;                        // bytes per element
    int64_t per_slot, per_field, once;   // elements: per slot, per heuristic field (the pool's row only), once per solver (guard bands, pads, per-solver tables)
    WaFill fill;
    bool upper_half;                     // the fill covers the second half of the block only (the replay flags behind the ants' lengths: ONE block, one granule)
    bool pool;                           // the straggler group: optional as a whole, a solver that cannot have all of it runs without the hand-over
};

struct WaAcsPlan {
    int64_t n_slots, fields0;            // fields0: heuristic fields the pool starts with
    int64_t cap, pher_stride, guard, sguard, vbits_words, vbits_rows;   // guard / sguard: elements in front of AND behind the field / stamp blocks
    bool ref_spec, pools;
    std::vector<WaPlanRow> rows;
    int64_t bytes(const WaPlanRow &r, int64_t fields) const { return r.elem * (r.per_slot * n_slots + r.per_field * fields + r.once); }
    int64_t bytes(const WaPlanRow &r) const { return bytes(r, fields0); }   // as the solver is created
    int64_t heur_row;                    // the pool of heuristic fields: the one row that grows at run time (heur_pool_grow), per field + its guard bands
};

inline WaAcsPlan wa_acs_plan(const WaPlanIn &in)
{
    WaAcsPlan P;
    const int64_t n = in.n, C = in.max_colony, nb = in.nb;
    const int32_t n_slots = in.n_slots;
    const bool lazy = in.lazy != 0;
    P.n_slots = n_slots;
    P.cap = in.path_capacity;
    if (P.cap <= 0) P.cap = n < (1 << 18) ? n : (1 << 18);
    if (P.cap > n) P.cap = n;
    if (P.cap < 2) P.cap = 2;
    const int64_t cap = P.cap;
    P.pher_stride = ((nb * n + 63) / 64) * 64;
    P.vbits_words = (n + 31) / 32;
    // The walk's inner loop reads records up to two lattice hops away from the current voxel without clamping the
    // address (an out-of-bounds neighbour is never walked to, its record is only fetched): every pheromone /
    // heuristic allocation therefore carries a guard band of 2*nx*ny records (+ slack) in front and behind.
    P.guard = nb == 6 ? (((int64_t)2 * in.nxy * 6 + 64 + 63) / 64) * 64 : 0;   // floats
    P.sguard = lazy ? (((int64_t)in.nxy + 64 + 63) / 64) * 64 : 0;             // entries: the walk fetches its six neighbours' stamps unclamped
    // REF mode, converged colonies: the stream generated ahead for a generation, the kept states, the per-ant verdicts (see k_ref_draws).
    // Only solvers that can run REF speculation carry them (6 neighbours, dense, WA_REF_SPEC != 0): ~24 KB per ant otherwise unused
    P.ref_spec = in.ref_spec != 0 && nb == 6 && !lazy;
    // stragglers (see WaAcsDev): dense searches (6 or 26 neighbours) of at most 256 ants, lists and pools PER SLOT (0.5 GB per slot at
    // path_capacity 2^18), for solvers of up to WA_STRAGGLER_SLOTS (16) slots; WA_STRAGGLERS=0 switches the mechanism off
    P.pools = n_slots <= in.straggler_slots && !lazy && in.max_colony <= 256 && in.stragglers != 0;
    P.vbits_rows = C + (P.pools ? WA_PLAN_RESUME_MAX : 0);          // (+ the rows of the resume blocks)
    P.fields0 = in.fields0;

    const WaFill N = WA_FILL_NONE, Z = WA_FILL_ZERO;
    auto row = [&P](const char *name, int64_t elem, int64_t per_slot, int64_t once, WaFill fill = WA_FILL_NONE, bool pool = false) {
        P.rows.push_back(WaPlanRow{name, elem, per_slot, 0, once, fill, false, pool});
    };
    // the order is the order of the requests: which kept block of the context's arena serves which request depends on it
    row("pher0", 4, P.pher_stride, 2 * P.guard, Z);
    if (!lazy) row("pher1", 4, P.pher_stride, 2 * P.guard, Z);   // the dense sweep is out of place: two fields; the lazy one in place
    if (lazy) {
        row("stamp", 4, n, 2 * P.sguard, Z);
        row("dirty_list", 4, n, 0);
        row("dcount", 4, 2, 0, Z);
    }
    P.heur_row = (int64_t)P.rows.size();
    P.rows.push_back(WaPlanRow{"heur", 4, 0, P.pher_stride, 2 * P.guard, N, false, false});   // (heur_pool_grow clears the guard bands)
    row("ltab", 4, 0, cap + 1);
    // rank masks: a bit per depositing rank and edge.  At most 0.2 * colony + 1 ranks deposit (:200), so a solver for colonies
    // of up to 39 ants (pair planning: 24) gets by with one BYTE per edge instead of a u64 (805 -> 101 MB per slot at 256^3);
    // the byte array is padded to a multiple of 4 (the marks are 32-bit atomic ORs on the containing word)
    if ((int32_t)(0.2 * in.max_colony) + 1 <= 8 && in.mask_u64 == 0) row("mask8", 1, P.pher_stride, 4, Z);
    else row("mask", 8, P.pher_stride, 0, Z);
    row("bestmark", 4, n, 0, Z);
    row("bestpath", 4, cap, 0);
    row("bestpos", 4, n, 0);
    row("besttabu", 1, cap, 0);
    if (lazy || in.replay != 0) row("rtab", 4, cap * (nb == 6 ? 8 : WA_PLAN_ROW26), 256);   // replay table: 8 floats per best-path node (6 neighbours) / 32 (26 neighbours)
    // ants' paths; solvers that hand stragglers over keep two such arrays (paths2 below) and alternate by generation: a straggler's walk so far
    // stays where it is and its resume block walks on in place while the next generation's ants write the other array
    row("paths", 4, C * cap, 0);
    row("antL", 4, C, 0);
    row("antLen", 4, 2 * C, 0, Z);   // (+ the replay flags behind the lengths)
    P.rows.back().upper_half = true;
    for (const char *name : {"perm", "depA"}) row(name, 4, C, 0);
    row("sortk", 4, 2 * C, 0);
    row("vbits", 4, P.vbits_rows * P.vbits_words, 0, Z);
    row("ctl", in.sizeof_ctl, 1, 0, Z);
    row("rng", in.sizeof_rng, 0, 1);
    row("dbg", 8, 0, 16, Z);
    if (P.ref_spec) {
        row("ref_draws", 4, 0, C * WA_PLAN_REF_SPEC_LEN);
        row("ref_state", 4, 0, (C * WA_PLAN_REF_SPEC_LEN / 64 + 2 * (WA_PLAN_REF_SUPER / 64) + 2) * 32);
    }
    row("ref_ok", 4, 0, C + 2, Z);
    if (P.ref_spec) row("ref_jump", 4, 0, 31 * 31);
    if (P.pools) {
        row("paths2", 4, C * cap, 0, N, true);   // the second paths array
        row("arr_len", 4, 256, 0, WA_FILL_ONES, true);
        row("arr_n", 4, 1, 0, Z, true);
        row("pool_rec", 4, 2 * WA_PLAN_RESUME_MAX * WA_PLAN_POOL_REC, 0, N, true);
        row("pool_n", 4, 2, 0, Z, true);
        row("strag_cnt", 8, 2, 0, Z, true);
    }
    for (const char *name : {"d_starts", "d_ends"}) row(name, 8, 1, 0);                            // per search: what wa_acs_begin uploads
    for (const char *name : {"d_streams", "d_hslot", "d_hlist", "d_hends"}) row(name, 4, 1, 0);
    return P;
}

// the rows added up: per slot / per heuristic field / once per solver, and the bytes of the solver as it is created
struct WaPlanSums { int64_t per_slot, per_field, fixed, total; };
inline WaPlanSums wa_plan_sums(const WaPlanIn &in)
{
    const WaAcsPlan P = wa_acs_plan(in);
    WaPlanSums s = {0, 0, 0, 0};
    for (const WaPlanRow &r : P.rows) {
        s.per_slot += r.elem * r.per_slot;
        s.per_field += r.elem * r.per_field;
        s.fixed += r.elem * r.once;
        s.total += P.bytes(r);
    }
    return s;
}
// what wa_acs_memory_estimate returns: the solver WITHOUT the straggler group; wa_acs_straggler_pool_bytes: what the group adds to it, its own
// blocks + the resume blocks' rows of the spill bitmap
inline WaPlanSums wa_plan_estimate(WaPlanIn in) { in.stragglers = 0; return wa_plan_sums(in); }
inline int64_t wa_plan_pool_bytes(const WaPlanIn &in) { return wa_plan_sums(in).total - wa_plan_estimate(in).total; }
