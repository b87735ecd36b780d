// acs_plan_check.cpp -- the ACS solver's memory plan (csrc/acs_plan.hpp) on its own: prints, for a list of solver shapes, the plan's
// rows and the four totals the library's estimate entry points return.  tests/test_acs_plan.py builds this with g++ and the sanitizers
// and holds the output against the formulas the estimate used before there was a plan.
//   shape <nx> <ny> <nz> <nb> <lazy> <ants> <slots> <capacity asked>
//   plan  <cap> <pher_stride> <guard> <sguard> <fields0> <pools> <rows>
//   row   <name> <elem bytes> <per slot> <per field> <once> <fill> <upper half> <pool group> <bytes>
//   sums  <per slot> <per field> <fixed> <pool bytes>
#include "../../welding_robot_amd/csrc/acs_plan.hpp"

#include <stdio.h>

// sizeof(WaSlotCtl) and sizeof(WaGlibcRand) of csrc/wa_device.h (a HIP header: the library passes its own)
static const int64_t SIZEOF_CTL = 104, SIZEOF_RNG = 144;

static void shape(const int *g, int nb, int lazy, int ants, int slots, int64_t cap)
{
    const int64_t n = (int64_t)g[0] * g[1] * g[2];
    const int fields0 = slots >= 32 ? (slots / 8 < 8 ? 8 : slots / 8 > 24 ? 24 : slots / 8) : (slots < 4 ? slots : 4);   // (the library's rule: host_acs.inc)
    const WaPlanIn in = {n, g[0] * g[1], slots, ants, fields0, cap, nb, lazy, 0, 1, 1, 1, 16, SIZEOF_CTL, SIZEOF_RNG};
    const WaAcsPlan P = wa_acs_plan(in);
    printf("shape %d %d %d %d %d %d %d %lld\n", g[0], g[1], g[2], nb, lazy, ants, slots, (long long)cap);
    printf("plan %lld %lld %lld %lld %lld %d %zu\n", (long long)P.cap, (long long)P.pher_stride, (long long)P.guard, (long long)P.sguard,
           (long long)P.fields0, P.pools ? 1 : 0, P.rows.size());
    for (const WaPlanRow &r : P.rows)
        printf("row %s %lld %lld %lld %lld %d %d %d %lld\n", r.name, (long long)r.elem, (long long)r.per_slot, (long long)r.per_field, (long long)r.once,
               (int)r.fill, r.upper_half ? 1 : 0, r.pool ? 1 : 0, (long long)P.bytes(r));
    const WaPlanSums s = wa_plan_estimate(in);
    printf("sums %lld %lld %lld %lld\n", (long long)s.per_slot, (long long)s.per_field, (long long)s.fixed, (long long)wa_plan_pool_bytes(in));
}

int main()
{
    static const int grids[5][3] = {{24, 24, 24}, {96, 96, 96}, {128, 128, 128}, {256, 256, 256}, {40, 24, 56}};
    // {neighbours, lazy, ants, slots}
    static const int kinds[][4] = {
        {6, 0, 24, 1}, {6, 0, 24, 16}, {6, 0, 24, 17}, {6, 0, 24, 32}, {6, 0, 24, 224},
        {6, 0, 35, 1}, {6, 0, 36, 1}, {6, 0, 39, 1}, {6, 0, 40, 1},                                  // byte masks: (int)(0.2 * ants) + 1 <= 8, up to 39 ants
        {6, 0, 256, 1}, {6, 0, 256, 16}, {6, 0, 256, 17}, {6, 0, 257, 1}, {6, 0, 257, 16}, {6, 0, 257, 17},   // pool edge
        {6, 0, 2048, 1},
        {26, 0, 64, 1}, {26, 0, 64, 2},
        {6, 1, 24, 1}, {6, 1, 24, 224}, {6, 1, 2048, 1}, {6, 1, 2048, 224},
        {26, 1, 24, 1},
    };
    for (const auto &g : grids)
        for (const auto &k : kinds) {
            const int64_t n = (int64_t)g[0] * g[1] * g[2];
            for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)7, n + 5}) shape(g, k[0], k[1], k[2], k[3], cap);
        }
    return 0;
}
