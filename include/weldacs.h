/* include/weldacs.h -- C ABI of libweldacs.so (MI355X / gfx950 HIP backend).
 *
 * The reference (mhsitu/welding_robot) has no FFI: its planning path lives behind the public
 * members of header-only C++ classes.  This header is the boundary a maintainer
 * binds instead; each entry point names the reference interface it replaces.  The drop-in C++
 * headers under welding_robot_amd/include/core/ (same class names as the reference) are written
 * purely on top of this ABI, and tests/bench reach it through ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, caller-allocated outputs, opaque handles.
 *   - every function returns a wa_status (0 = ok) unless it returns a count; wa_last_error()
 *     gives the text.  The library never exit()s and never prints (the reference does both:
 *     read_STL.hpp:34-59, ACSRank_3D.hpp:239).
 *   - there is NO CPU fallback: with no HIP device wa_ctx_create fails with WA_ERR_DEVICE.
 *   - lattice: voxel id = (z*ny + y)*nx + x  (model_grid_map.hpp:203-216);
 *     edge k of a voxel: 0:z-1 1:y-1 2:x-1 3:x+1 4:y+1 5:z+1  (ACSRank_3D.hpp:355-365).
 *   - a wa_ctx and everything created from it is used from one host thread at a time.
 */
#ifndef WELDACS_H
#define WELDACS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    WA_OK = 0,
    WA_ERR_ARG = 1,       /* bad argument / null pointer / size                          */
    WA_ERR_DEVICE = 2,    /* no HIP device, HIP runtime error                            */
    WA_ERR_ALLOC = 3,     /* host or device allocation failed                            */
    WA_ERR_FILE = 4,      /* cannot open / short read (read_STL.hpp:34-59 exit(1..3))    */
    WA_ERR_FORMAT = 5,    /* an ASCII STL the reference's reader never returns from     */
    WA_ERR_POINT = 6,     /* a route point resolves to no free voxel (ACSRank_3D.hpp:491) */
    WA_ERR_CAPACITY = 7,  /* a walk outgrew path_capacity / more ants than max_colony     */
    WA_ERR_STATE = 8      /* call order (e.g. results before a solve)                     */
} wa_status;

typedef struct wa_ctx wa_ctx;
typedef struct wa_grid wa_grid;
typedef struct wa_acs wa_acs;
typedef struct wa_traj wa_traj;       /* device-resident polyline, n x 3 floats */
typedef struct wa_bspline wa_bspline;

/* ---- context --------------------------------------------------------------------------- */
const char *wa_version(void);
/* visible HIP devices (0 when there is none or no runtime): the drop-in ACS_Rank shards its pair searches over all of
 * them, one wa_ctx per device (ACSRank_3D.hpp:472-499 is a loop over independent searches) */
int wa_device_count(void);
/* free / total memory of the context's device in bytes (either pointer may be NULL): what the slot count of a solver for many
 * pair searches is sized by, and what a caller can poll after another process has just released the GPU */
int wa_ctx_memory_info(wa_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
/* A context keeps the device memory (blocks of 1 MiB and up) of the solvers destroyed on it and builds the next solver from it: the
 * reference never frees anything (SURVEY 8(b) ownership; ACSRank_3D.hpp:456-460 allocates once) and creates its search once per
 * process; a host that runs searchBestPathOfPoints per job would otherwise pay the driver's wipe of the freed memory before every
 * re-allocation (seconds for a C5-sized solver).  Where the device supports virtual memory management the memory is kept as an ARENA
 * of physical chunks (512 MiB and 32 MiB) that are mapped into a fresh address range for every block of 32 MiB and up, so a solver of
 * ANY shape is served from what solvers of other shapes gave back; smaller blocks, and every block without that support
 * (WA_DEV_ARENA=0), are whole allocations reused for requests of nearly their size.  Kept bytes count as free in wa_ctx_memory_info;
 * at most WA_DEV_KEEP_PCT (95) percent of the device's memory is kept; when the device runs out, kept memory goes back to the driver
 * -- as much as is needed --, as it does on wa_ctx_trim and with the context.  Other PROCESSES on the same GPU cannot have those bytes
 * until then: a host that shares its GPU trims after its last job.  WA_DEV_CACHE=0 in the environment switches the mechanism off. */
int wa_ctx_cached_bytes(wa_ctx *ctx, int64_t *bytes);
int wa_ctx_trim(wa_ctx *ctx);
/* counters since the context was created: [0] blocks asked for (1 MiB and up), [1] bytes served from kept memory, [2] bytes newly
 * obtained from the driver, [3] bytes given back to the driver, [4] blocks served ENTIRELY from kept memory, [5] out-of-memory events
 * handled by releasing kept memory, [6] milliseconds spent building arena blocks, [7] 1 when the arena is in use, 2 when it is but its
 * address window is used up (blocks kept so far go on serving, new shapes come as whole allocations) */
int wa_ctx_cache_stats(wa_ctx *ctx, int64_t out[8]);
/* Debug read-out of WA_DEV_POISON=1 (read at wa_ctx_create): every device block the library allocates for a call on such a context is
 * filled with WA_DEV_POISON_BYTE (0 .. 255, default 255) before it is used, so that a kernel which reads a word nobody wrote reads that
 * pattern and not the zeros of fresh device memory.  [0] blocks and [1] bytes filled through the context's allocator (the solvers'
 * memory), [2] blocks and [3] bytes filled through the plain one (grids, trajectories, every planning call's scratch).  All 0 without
 * the knob. */
int wa_ctx_poison_stats(wa_ctx *ctx, int64_t out[4]);
/* Debug read-out of WA_DEV_GUARD=1 (read at wa_ctx_create): every plain device block the library allocates for a call on such a context
 * (grids, trajectories, splines, every planning call's scratch, the whole blocks of the context's allocator; not the blocks the arena
 * builds from chunks) stands between two red zones of 4096 bytes filled with WA_DEV_GUARD_BYTE (0 .. 255, default 0xa5).  The back zone
 * starts behind the bytes that were asked for.  When the block is given back the device is waited for and both zones are compared byte
 * by byte.  [0] blocks handed out with zones, [1] blocks freed and checked, [2] blocks live now, [3] requested bytes live now, [4] blocks
 * freed with a damaged front zone, [5] with a damaged back zone, [6] requested size of the first damaged block (-1: none), [7] distance
 * in bytes of its first damaged byte from the block: >= 0 behind its end, < 0 in front of its start.  All 0 / -1 without the knob.
 * WA_ERR_ARG for a NULL argument. */
int wa_ctx_guard_stats(wa_ctx *ctx, int64_t out[8]);
/* The proof that the check above fires, on a block of the library's own: allocates a guarded block of `bytes`, writes one byte (the
 * complement of the guard byte) at `offset` from the block's start with hipMemsetAsync on the context's stream, and frees the block.
 * No kernel is launched.  WA_ERR_ARG for bytes < 0 or an offset outside [-4096, bytes + 4096): the write never leaves the allocation.
 * WA_ERR_STATE on a context created without WA_DEV_GUARD=1. */
int wa_ctx_guard_selftest(wa_ctx *ctx, int64_t bytes, int64_t offset);
/* Every call on a context (and on anything created from it) runs on that context's device regardless of the calling
 * thread's current HIP device, and restores the caller's current device before returning. */
int wa_ctx_create(int device_ordinal, wa_ctx **out);
void wa_ctx_destroy(wa_ctx *ctx);
const char *wa_last_error(const wa_ctx *ctx);
int wa_ctx_device_name(const wa_ctx *ctx, char *buf, size_t cap);
int wa_ctx_sync(wa_ctx *ctx);
/* the HIP stream every kernel of this context is launched on (hipStream_t as void*) */
void *wa_ctx_stream(wa_ctx *ctx);

/* ---- mesh input: replaces STLReader::readFile + TriangleList (read_STL.hpp:26-77,:88,:131-156)
 * tris = n x 12 floats (normal, v0, v1, v2).  Returns the triangle count (>= 0) or -wa_status.
 * Pass tris = NULL to query the count.  Byte 79 != 0 selects the ASCII branch (:65-68, :99-129), read with the reference's stream
 * semantics: normals stay (0, 0, 0), an unreadable vertex keeps the previous triangle's value, a text without a
 * "facet" word where the reader expects one gives 0 triangles.  WA_ERR_FORMAT: the text ends directly behind a "facet" word (the
 * reference's loop does not end on it); WA_ERR_FILE: shorter than the 80 bytes the sniff reads / a truncated binary file. */
int64_t wa_stl_parse(const void *buf, size_t len, float *tris, int64_t cap_tris);
int64_t wa_stl_read_file(const char *path, float *tris, int64_t cap_tris);

/* ---- grid map: replaces GridMap<float>::creatGridMap / readGridMap / ptr_grid_map
 *      (model_grid_map.hpp:151-298, :300-356, :358) -------------------------------------- */
/* voxelise a mesh on the device (bbox :165-181, ranges :198-200, coords :204-211, occupancy
 * :223-268).  bbox6_out (optional) = min xyz, max xyz of the mesh. */
int wa_grid_from_mesh(wa_ctx *ctx, const float *tris, int64_t n_tris, float precision, int32_t wall,
                      wa_grid **out, float *bbox6_out);
/* adopt an existing occupancy (free_[id] != 0 <=> isFree) with per-axis node coordinates --
 * the readGridMap path and the synthetic benchmark grids.  Grids up to 2^29 voxels (ids 0 .. 2^29 - 1); WA_ERR_ARG above. */
int wa_grid_from_occupancy(wa_ctx *ctx, const uint8_t *free_, int32_t nx, int32_t ny, int32_t nz,
                           const float *cx, const float *cy, const float *cz, float precision,
                           int32_t wall, wa_grid **out);
/* model_grid_map.hpp:204-211 / :321-328 piecewise axis coordinates (host helper, n values) */
int wa_axis_coords(float lo, float hi, float precision, int32_t wall, int32_t n, float *out);
void wa_grid_destroy(wa_grid *g);
int wa_grid_info(const wa_grid *g, int32_t dims3[3], float *precision, int32_t *wall, int64_t *n_free);
int wa_grid_read_occupancy(const wa_grid *g, uint8_t *free_out /* nx*ny*nz */);
int wa_grid_read_coords(const wa_grid *g, float *cx, float *cy, float *cz);
/* ACS_Rank::setPoints / checkRoutePoints (ACSRank_3D.hpp:537-565, :511-535): for each point the
 * LAST free voxel in raster order within +-(float)(1.2*precision) on every axis; -1 if none.  Calls with up to 16 points (setPoints
 * resolves two) are answered from a host mirror of the grid's axis tables and occupancy, fetched once per grid (0.2 us per call instead
 * of a launch + synchronise + copy); larger batches by the kernel; WA_RESOLVE_HOST=0: always the kernel.  Same ids either way. */
int wa_grid_resolve_points(const wa_grid *g, const float *pts_xyz, int32_t n_pts, int64_t *ids_out);

/* ---- rank-based ACS: replaces ACS_Rank::initFromGridMap / computeSolution / reset /
 *      searchBestPathOfPoints' pair loop / getSolution (ACSRank_3D.hpp:220-504) ----------- */
enum { WA_RNG_REF = 0, WA_RNG_DEV = 1 };
/* WA_RNG_REF: glibc rand() stream shared sequentially by all ants and all problems, libstdc++
 *             std::sort tie order -- bit-identical to the reference, ants walk one after another
 *             (a parity mode, one wavefront per problem).
 * WA_RNG_DEV: counter-based draw keyed (seed, stream, generation, ant, step), ranks ties by ant
 *             index -- the parallel production mode, one wavefront per ant. */
typedef struct {
    int32_t alpha;          /* pheromone exponent, reference 1       (ACSRank_3D.hpp:319) */
    float beta;             /* heuristic weight, reference 0.6       (:320)               */
    float rho;              /* evaporation factor, reference 0.8     (:321)               */
    float pheromone_0;      /* reference 1                           (:324)               */
    int32_t max_iteration;  /* generations, reference 150            (:322)               */
    float predict;          /* computeSolution(predict_path_len)     (:220)               */
    int32_t fixed_colony;   /* 0: reference-adaptive colony (:247); >0: pinned ant count   */
    int32_t rng_mode;       /* WA_RNG_REF / WA_RNG_DEV                                     */
    uint64_t seed;          /* DEV counter key (REF: use wa_acs_srand)                     */
} wa_acs_params;
void wa_acs_default_params(wa_acs_params *p);

/* n_slots independent problems can be in flight.  Each owns a pheromone field (24 B/voxel, two of them with the dense
 * sweep: it is out of place), best-path stamps (8 B/voxel), deposit rank masks (6 B/voxel when max_colony <= 35 --
 * at most 8 ranks deposit, ACSRank_3D.hpp:200 -- 48 B/voxel otherwise) and its ants' paths (4 B * max_colony *
 * path_capacity); the heuristic fields (24 B/voxel) are a pool shared by the slots: one per distinct END point in use,
 * computed by wa_acs_begin when the pool does not hold it yet.  max_colony bounds the ants per generation,
 * path_capacity the nodes per walk (<= number of voxels).  Grids up to 89,478,485 voxels (the walk addresses a field with
 * signed 32-bit byte offsets: 24 B * voxels < 2^31); WA_ERR_ARG above. */
int wa_acs_create(wa_ctx *ctx, const wa_grid *grid, int32_t n_slots, int32_t max_colony,
                  int64_t path_capacity, wa_acs **out);
/* Same with an explicit neighbourhood: 6 = face neighbours (what wa_acs_create builds, the reference as
 * shipped), 26 = faces + edges + corners -- the variant the reference's initFromGridMap walks but stubs
 * out by setting the two extra distances to 0 (ACSRank_3D.hpp:361-388); here they carry the values the
 * reference keeps in comments (precision*1.414f, precision*1.732f) and evaporation / reset cover all 26
 * edges.  Edge index k of a voxel follows the reference's cube loop: offsets z, y, x in {-1,0,1}, z outermost,
 * centre skipped (k = 0 is (-1,-1,-1), k = 25 is (+1,+1,+1)).  Fields are [N][26]; grids up to 2^27 voxels.
 * Every other wa_acs_* call is unchanged; wa_acs_read_pheromone then fills nvox*26 floats and
 * wa_acs_result's `choices` are 0..25. */
int wa_acs_create_nb(wa_ctx *ctx, const wa_grid *grid, int32_t n_slots, int32_t max_colony,
                     int64_t path_capacity, int32_t neighbourhood, wa_acs **out);
/* Same results as wa_acs_create, evaporation evaluated LAZILY: a voxel none of whose outgoing edges ever received a
 * deposit is never swept -- after g evaporations each of its in-bounds edges holds pheromone_0*rho*...*rho in the
 * reference's own fp32 rounding, which the solver carries as one scalar -- and only the voxels on deposited paths
 * are multiplied by rho every generation (ACSRank_3D.hpp:268-272 restricted to where it can differ).  Every value
 * any kernel reads, and wa_acs_read_pheromone's output, is bit-identical to the dense sweep.  A generation then
 * costs O(deposited voxels) instead of 48 B/voxel and reset_pheromone O(deposited voxels) instead of 24 B/voxel:
 * meant for many pair searches on large grids (BASELINE config C5).  DEV mode, <= 2048 ants and
 * <= 64 depositing ranks only (WA_ERR_ARG at wa_acs_begin otherwise); wa_acs_evaporate is not available. */
int wa_acs_create_lazy(wa_ctx *ctx, const wa_grid *grid, int32_t n_slots, int32_t max_colony,
                       int64_t path_capacity, wa_acs **out);
/* ... with 6 or 26 neighbours (round 5): the 26-neighbour variant the reference stubs out (ACSRank_3D.hpp:361-388) swept 26 x 8 B x N
 * per search and generation in its dense form -- 3.5 GB at 256^3 -- which kept it a small-grid feature; lazily evaporated it runs at
 * pair-planning scale.  Same restrictions as wa_acs_create_lazy. */
int wa_acs_create_lazy_nb(wa_ctx *ctx, const wa_grid *grid, int32_t n_slots, int32_t max_colony,
                          int64_t path_capacity, int32_t neighbourhood, wa_acs **out);
void wa_acs_destroy(wa_acs *s);
/* device bytes a solver of this shape takes: per slot, per heuristic field (the pool holds one per distinct END point of a
 * batch, at least min(n_slots, 4) -- from 32 slots on n_slots / 8, between 8 and 24) and once per solver; the per-generation trace (20 B per slot and generation) comes on top.
 * Nothing is allocated.  The drop-in ACS_Rank sizes the concurrent pair searches of a device from this and
 * wa_ctx_memory_info (ACSRank_3D.hpp:472-499 runs them one after another).  The straggler pools of small dense solvers come on top:
 * wa_acs_straggler_pool_bytes.  Both are sums over the list of blocks the solver itself is created from (csrc/acs_plan.hpp), so every
 * block is counted at its size: bytes_fixed holds the guard bands (a lazy solver's stamp guard included), the L table, the pads of the
 * replay table (1 024 B) and of the byte masks (4 B), the REF stream, the debug counters, the per-ant REF verdicts and the REF
 * speculation buffers; a dense solver created under WA_REPLAY=0 has no replay table and none is counted.  (Until the plan existed the
 * small blocks were a guessed 4 096 B and the stamp guard and the pads were left out: bytes_per_slot and bytes_per_heuristic_field
 * are what they were, bytes_fixed moved by less than a megabyte.) */
int wa_acs_memory_estimate(const wa_grid *grid, int32_t max_colony, int64_t path_capacity, int32_t neighbourhood, int32_t lazy,
                           int64_t *bytes_per_slot, int64_t *bytes_per_heuristic_field, int64_t *bytes_fixed);
/* A dense solver (6 or 26 neighbours) of at most 256 ants and at most 16 slots (WA_STRAGGLER_SLOTS) additionally holds, PER SLOT, the
 * arrival list and what the straggler hand-over needs (see wa_acs_debug_counters): a second array of ants' paths (max_colony x
 * path_capacity words: stragglers walk on in place while the next generation writes the other array) + 256 spill-bitmap rows
 * (0.33 GB per slot at 128^3 with 256 ants and the default path capacity) + the small lists and counters.  *bytes = what a solver of this
 * shape holds in total -- its plan with the group minus its plan without -- 0 when it gets none (lazy, larger colonies, more slots,
 * WA_STRAGGLERS=0). */
int wa_acs_straggler_pool_bytes(const wa_grid *grid, int32_t n_slots, int32_t max_colony, int64_t path_capacity, int32_t neighbourhood,
                                int32_t lazy, int64_t *bytes);
/* initFromGridMap :343-408: in-bounds edges pheromone_0, out-of-bounds edges 0. slot<0: all */
int wa_acs_init_pheromone(wa_acs *s, int32_t slot, float pheromone_0);
/* reset() :307-315: every edge pheromone_0 */
int wa_acs_reset_pheromone(wa_acs *s, int32_t slot, float pheromone_0);
/* REF mode libc state: srand(seed) (:327); get/set = 34 words + 2 indices, to hand the stream
 * on to wa_gtsp_solve exactly as the reference's process-global rand() does */
int wa_acs_srand(wa_acs *s, uint32_t seed);
int wa_acs_rand_state(wa_acs *s, int32_t state36_inout[36], int32_t set);

/* start n_problems searches on slots 0..n-1 (setPoints already resolved to voxel ids; streams[i]
 * is the DEV-mode stream key of problem i, NULL = 0..n-1), then advance all of them by
 * n_generations (enqueued on the context stream, asynchronous), then wait.
 * wa_acs_run returns when everything is enqueued -- for a lone search whose converged generations run in windows (wa_acs_converged_info), once
 * the last window of the call has reported to the host (wa_acs_converged_host_info): the call then waits, a bounded time, for the work in front
 * of that window. */
int wa_acs_begin(wa_acs *s, const wa_acs_params *p, int32_t n_problems, const int64_t *start_ids,
                 const int64_t *end_ids, const uint32_t *streams);
int wa_acs_run(wa_acs *s, int32_t n_generations);
int wa_acs_sync(wa_acs *s);
/* Pipelined groups.  The searches of a batch are independent (ACSRank_3D.hpp:472-499 is a loop over searches with a pheromone
 * reset in between, :481): wa_acs_run splits the active slots into `groups` contiguous groups that advance on HIP streams of
 * their own, so that one group's HBM-bound evaporation sweep (:268-272) runs under another group's latency-bound walk
 * (:252-261).  The groups are forked from the context's stream when wa_acs_run starts and joined into it before it returns,
 * so everything enqueued on the context afterwards is ordered behind all of them.  Every slot's own launch sequence is the
 * single-stream one: results do not depend on the split.  groups = 0: by rule (WA_PIPE_GROUPS, read at creation, overrides
 * the rule); 1: everything on the context's stream.  wa_acs_pipeline_info: the groups the last wa_acs_run used. */
int wa_acs_set_pipeline(wa_acs *s, int32_t groups);
int wa_acs_pipeline_info(const wa_acs *s, int32_t *groups_last_run);
/* begin + run(max_iteration) + sync */
int wa_acs_solve(wa_acs *s, const wa_acs_params *p, int32_t n_problems, const int64_t *start_ids,
                 const int64_t *end_ids, const uint32_t *streams);

/* best-so-far of a slot (Agent<float> best: L, path ids, edge choices = nodeIndex()).  When no
 * ant has arrived cost = +inf (a valid result) and len = 0.  The first read behind a run (wa_acs_run / wa_acs_solve)
 * fetches every slot's result to the host in one go; wa_acs_result / wa_acs_result_batch* are served from that copy until the next
 * wa_acs_begin / wa_acs_run (a per-slot read in a host loop, getSolution :506-509, costs a host array access). */
int wa_acs_result(wa_acs *s, int32_t slot, float *cost, int64_t *len, int32_t *path_ids,
                  int8_t *choices, int64_t cap);
/* the same for slots 0 .. n_slots-1 in one round trip (batched pair searches): costs[q], lens[q] (0 when the cost is
 * +inf), and -- if path_ids is not NULL -- slot q's path ids at path_ids[q*path_stride ...]; WA_ERR_CAPACITY when a
 * path is longer than path_stride (lens is filled in either way: call again with a larger buffer). */
int wa_acs_result_batch(wa_acs *s, int32_t n_slots, float *costs, int64_t *lens, int32_t *path_ids, int64_t path_stride);
/* ... and the edge choices (Agent::nodeIndex(), as wa_acs_result's `choices`): slot q's lens[q] - 1 edge indices at choices[q*path_stride ...] */
int wa_acs_result_batch_choices(wa_acs *s, int32_t n_slots, float *costs, int64_t *lens, int32_t *path_ids, int8_t *choices, int64_t path_stride);
/* per-generation history the reference computes and discards (:295-296).  Arrays of
 * generations_done entries; any pointer may be NULL. */
int wa_acs_trace(wa_acs *s, int32_t slot, int32_t *generations_done, float *best_L, float *iter_best_L,
                 int32_t *colony, int32_t *finite, int64_t *steps);
/* device-to-device copy (on the context stream) of best_L[gen0 .. gen0+count) of every active
 * slot into dst_device[slot*count + g] -- feeds the RCCL MIN all-reduce of the global best */
int wa_acs_export_trace(wa_acs *s, void *dst_device, int32_t gen0, int32_t count);
int wa_acs_read_pheromone(wa_acs *s, int32_t slot, float *out /* nvox*6 */);
/* the agents[] of the generation walked last (ACSRank_3D.hpp:251-261): per ant L (+inf = dead end, :88-91) and node
 * count (Agent::getPath()->size()); *colony = ants of that generation, of which min(colony, cap) are written. */
int wa_acs_read_ants(wa_acs *s, int32_t slot, int32_t *colony, float *L, int32_t *len, int32_t cap);
/* the node ids one ant of that generation visited, start first (Agent::getPath(), ACSRank_3D.hpp:34,75-77): *len = node
 * count, of which min(*len, cap) ids are written. */
int wa_acs_read_ant_path(wa_acs *s, int32_t slot, int32_t ant, int32_t *ids, int32_t cap, int32_t *len);
int wa_acs_last_params(wa_acs *s, int32_t slot, int32_t *colony, float *lambda, float *Q);

/* kernel timing with HIP events on the context stream.  Enable before wa_acs_run; afterwards
 * ms[i]/launches[i] hold the summed event time and launch count of kernel class i. */
enum { WA_K_WALK = 0, WA_K_RANK = 1, WA_K_EVAPORATE = 2, WA_K_DEPOSIT = 3, WA_K_COUNT = 4 };
/* enable: 0 off; 1 every sample_every-th generation has all its launches stamped; 3 = the same, and the launch that carries the
 * evaporation sweep is stamped in EVERY generation (per-dispatch start/stop events of hipExtLaunchKernelGGL: no extra stream
 * operation, so the timed loop is not perturbed -- what bench.py's roofline figure uses); bit 2 (value 4) added to either: every
 * stamped sweep-carrying launch is preceded by a no-op dispatch with events of its own -- a dispatch with events directly behind one
 * without (the walk) reports 1.6-2 us that belong to that transition, not to the kernel (profiles/r06/sweep_gap.txt) */
int wa_acs_profile(wa_acs *s, int32_t enable, int32_t sample_every);
/* what the last DEV walk launch of a 6-neighbour solver ran with (the visited set of ACSRank_3D.hpp:70, :144-146 lives in LDS, one table per
 * walking ant): [0] log2 of the table's slots, [1] 1 if it kept 16-bit entries (saturated launches of grids whose voxel ids an entry can name;
 * WA_TAB16=0 in the environment switches them off, =1 forces them), [2] bytes of LDS per walk block -- min(163840 / [2], 16) blocks are resident
 * per CU --, [3] 1 if the loop carried touch loads (a lone search) */
int wa_acs_walk_info(const wa_acs *s, int32_t out[4]);
int wa_acs_profile_read(wa_acs *s, double ms[WA_K_COUNT], int64_t launches[WA_K_COUNT]);
/* diagnostic counters.  Product build: out16[9] = ants handed over as stragglers, out16[7] = stragglers finished by a resume block (the two
 * are equal after wa_acs_run returns), out16[6] = REF-mode ants confirmed by the converged-colony speculation (below), everything else zero; the cycle counters of the walk's inner loop only exist in the diagnostic
 * builds (-DWA_STAMPS / -DWA_ANT_TIME, tools/).
 * Stragglers (dense searches of at most 256 ants in solvers of at most 16 slots, 6 or 26 neighbours, DEV mode, alpha == 1, the first 64
 * generations of a search): only the ranks o <= lambda - 1 deposit (ACSRank_3D.hpp:200) and only the shortest ant can become the best path
 * (:263-264), so an ant that is already longer than floor(lambda - 1) + 1 arrivals of its generation (26 neighbours: whose L so far
 * already exceeds theirs) can change neither (about 140 of 256 ants per exploratory generation); at one of the loop's checks (every 64
 * nodes, every 16 once shorter ants have arrived) it leaves the walk launch -- which lasts as long as its longest ant -- and a resume
 * block of the NEXT generation's walk launch finishes the same walk on the previous generation's field (intact until the next sweep),
 * adding its arrival and its steps to its own generation's trace entry.  Lists and pools are per slot: every search of a batch hands
 * its own stragglers over.  The last generation of a wa_acs_run call hands over too once calls have been seen to follow each other
 * without a read in between (chunked runs, generation-by-generation loops; behind a lone call it would only add a launch to what the
 * caller waits for); its stragglers are finished by the next call's first walk launch or -- when results are read first
 * (wa_acs_sync, wa_acs_result, wa_acs_trace, wa_acs_read_ants ...) -- by a launch of resume blocks only, which also puts the finished
 * walks back into agents[] (WA_STRAGGLER_DRAIN=0: the last generation of a call never hands over, as in round 3).  agents[] and the
 * trace are complete whenever they are read.  Results are bit-identical with the mechanism on or off (WA_STRAGGLERS=0, read at
 * wa_acs_create; wa_acs_set_stragglers(s, 0) at run time).
 * REF mode once the colony has converged (6 neighbours, alpha == 1; WA_REF_SPEC=0 switches it off): the shared libc stream forces the ants
 * to walk one after another because an ant's first draw is the previous ants' total step count -- but when every ant re-walks the best path
 * that count is known.  The stream of the whole generation is generated ahead, every ant checks IN PARALLEL (replay table) that it follows
 * the whole best path with the draws it would be dealt, and the sequential walk starts at the first ant that does not, with the stream taken
 * to exactly that ant's first draw.  Same draws, same results, same stream position as the reference (BASELINE config 3, 500 REF generations: 8.7 -> 1.25 s). */
int wa_acs_debug_counters(wa_acs *s, uint64_t out16[16], int32_t reset);
/* the same two counts per slot (ants handed over / stragglers finished by a resume block; equal whenever they are read) */
int wa_acs_straggler_counters(wa_acs *s, int32_t slot, uint64_t *handed_over, uint64_t *resumed, int32_t reset);
/* generations of a search during which its ants may be handed over (default 64, WA_STRAGGLER_GENS; 0: off; < 0: back to the default) */
int wa_acs_set_stragglers(wa_acs *s, int32_t generations);
/* Converged generations in one launch (dense 6-neighbour solvers on the fused DEV loop; WA_CONVERGED_RUN=0, read at wa_acs_create, switches it off;
 * WA_CONVERGED_WINDOW: generations a window covers at most).  out: [0] windows enqueued for `slot` since the solver was created, [1] windows
 * committed whole, [2] windows cut short by an ant that left the best path, [3] generations committed.  Results are bit-identical with the
 * mechanism on or off.  Waits for the work enqueued so far. */
int wa_acs_converged_info(wa_acs *s, int32_t slot, uint64_t out[4]);
/* A lone search (one active slot): every window of three generations or more reports the generations it committed to the host, through a word of pinned
 * host memory, and wa_acs_run does not enqueue the launches of committed generations that would only return at their top (WA_CONVERGED_READBACK=0, read at
 * wa_acs_create: enqueue them all, as for batches).  The host waits for a verdict at most WA_CONVERGED_WAIT_US microseconds (default 200000; 0: never) and no
 * longer than the stream takes to drain; a wait given up enqueues every generation of the window, which is right whatever the window committed.
 * Behind a window that committed whole the next window's flush (the two launches behind the walk of its last generation) is enqueued directly behind the
 * window kernel, before the verdict: it flushes if that window commits whole too and returns at once otherwise (WA_CONVERGED_SPECULATE=0: never).
 * out: [0] verdicts the host went to read since the solver was created, [1] generations whose launches were not enqueued, [2] speculative launches
 * (flushes, or walk launches: wa_acs_converged_carried_info) cancelled because their window did not commit whole, [3] waits given up, of [0].  Results are bit-identical with the read-back on or off.  Does not wait. */
int wa_acs_converged_host_info(wa_acs *s, uint64_t out[4]);
/* Owed evaporations, on the same path (a lone search whose verdicts the host reads; WA_CONVERGED_OWED=0, read at wa_acs_create: never).  A window that
 * commits whole in front of a generation that is enqueued in full whatever happens -- the last of the call, or one stamped for wa_acs_profile -- also
 * tests that generation: if every ant of it replays the best path too, nothing reads the field in between, the window is CARRIED and its flush leaves
 * the pass over the field out; the sweep of the generation behind it multiplies every value once more than the window committed generations, one
 * rounding each.  out: [0] whole windows the host read "carried" of since the solver was created, [1] generations enqueued whose sweep paid a carried
 * window's evaporations with its own, [2] whole windows that were not carried (an ant leaves the path behind them: flushed as ever), [3] / [4]: of [1],
 * the sweeps that ran out of place / in place.  Results are bit-identical with the switch on or off.  Does not wait. */
int wa_acs_converged_owed_info(wa_acs *s, uint64_t out[5]);
/* The carried walk, where owed evaporations apply (WA_CONVERGED_CARRIED_WALK=0, read at wa_acs_create: never).  The flush of a carried window has one reader,
 * the walk of the generation behind it, and the window has already tested that generation's ants: the flush is not enqueued at all, and the walk launch
 * delivers every ant as a whole replay of the best path without reading the replay table.  Behind a window that committed whole that walk launch goes
 * out in front of the next window's verdict and returns at its top unless the window turns out carried (WA_CONVERGED_SPECULATE=0: never ahead).
 * out: [0] walk launches that took the carried path since the solver was created, [1] rows launches of carried windows that were not enqueued,
 * [2] walk launches enqueued ahead of a verdict, [3] of [2], those cancelled.  Results are bit-identical with the switch on or off.  Waits for the
 * work enqueued so far. */
int wa_acs_converged_carried_info(wa_acs *s, uint64_t out[4]);
/* evaporation sweep alone (ACSRank_3D.hpp:268-272) over `slot` -- for roofline measurements */
int wa_acs_evaporate(wa_acs *s, int32_t slot, float rho, int32_t repeats);

/* ---- multi-GPU: problems shard one set per GPU (main.cpp:268-283 is a loop over independent searches, and so is a
 *      multi-start batch); the only exchange is the global-best path cost per generation -- what each rank's
 *      ACSRank_3D.hpp:263-264 would publish -- as an RCCL all-reduce (ncclMin) over xGMI.  One wa_comm per wa_ctx
 *      (= per device, per process or host thread); libweldacs.so links librccl itself, no torch / MPI needed. ---- */
#define WA_COMM_ID_BYTES 128
typedef struct wa_comm wa_comm;
/* rank 0 creates the id (ncclGetUniqueId) and ships the bytes to the other ranks by any means it has
 * (a file, a socket, MPI_Bcast, a torch.distributed store ...) */
int wa_comm_unique_id(uint8_t id_out[WA_COMM_ID_BYTES]);
/* collective over all `world` ranks (ncclCommInitRank); the communicator runs its exchanges on its own stream */
int wa_comm_create(wa_ctx *ctx, int32_t rank, int32_t world, const uint8_t id[WA_COMM_ID_BYTES], wa_comm **out);
void wa_comm_destroy(wa_comm *c);
int wa_comm_info(const wa_comm *c, int32_t *rank, int32_t *world);
/* Every wait of the exchanges below is bounded and watches the communicator (ncclCommGetAsyncError): a peer that died, or that does not
 * answer within WA_COMM_TIMEOUT_S seconds (environment, read by wa_comm_create; default 600, 0 = wait for ever), makes the call give the
 * communicator up (ncclCommAbort) and return WA_ERR_DEVICE instead of blocking; every later call on it returns WA_ERR_STATE.
 * wa_comm_abort does the same on request (a host that has learnt by other means that a peer is gone); wa_comm_destroy is still due.
 * The reference has no counterpart (its pair loop is one process: ACSRank_3D.hpp:472-499); the convention is SURVEY 8(b)'s: status
 * codes, never a hang.
 * wa_comm_stats: [0] ranks as RCCL counts them (ncclCommCount), [1] RCCL's version code (ncclGetVersion), [2] all-reduce calls issued on
 * this communicator, [3] other collectives / sends / receives issued, [4] 1 once the communicator has been aborted. */
int wa_comm_abort(wa_comm *c);
int wa_comm_stats(wa_comm *c, int64_t out[5]);
/* global_best[g] = MIN over all ranks and all active slots of best_L[g] for g in [gen0, gen0 + count), together with WHO holds it:
 * one ncclAllReduce(ncclUint64, ncclMin) of the packed key (float bits of the cost << 32 | rank << 16 | slot; costs are non-negative
 * or +inf, so the bits order like the values; ties go to the lowest rank, then the lowest slot).  Asynchronous -- waits (event) for
 * the generations enqueued so far, runs on the communicator's stream beside the generations enqueued afterwards.  Every rank must
 * call it with the same (gen0, count) sequence.  The global best is published, never fed back into a problem's own colony / Q, so
 * per-problem results equal the single-GPU run.  At most 65 536 active slots per rank. */
int wa_acs_allreduce_best(wa_acs *s, wa_comm *c, int32_t gen0, int32_t count);
/* wait for the exchanges enqueued so far, then copy global_best[gen0 .. gen0 + count) to the host; WA_ERR_STATE for a generation that
 * has not been through wa_acs_allreduce_best.  ..._owner: also the rank and the slot whose search holds that cost (its path:
 * wa_acs_result on that rank; wa_comm_gather_paths brings it to one rank); any output may be NULL. */
int wa_comm_read_best(wa_comm *c, int32_t gen0, int32_t count, float *out);
int wa_comm_read_best_owner(wa_comm *c, int32_t gen0, int32_t count, float *cost, int32_t *owner_rank, int32_t *owner_slot);
/* the packed key itself, for a host that runs the reduction through another transport (host-side helpers, no device work) */
int wa_comm_pack_best_key(float cost, int32_t rank, int32_t slot, uint64_t *key);
int wa_comm_unpack_best_key(uint64_t key, float *cost, int32_t *rank, int32_t *slot);
/* End of a sharded pair-planning run (every rank ran its share of ACSRank_3D.hpp:472-499; ACS_GTSP.hpp:224-253 wants all costs,
 * :286-298 all paths on one rank).  Both are blocking and size-prefixed (an all-gather of the counts, then the padded records).
 * wa_comm_allgather_costs: all[index_mine[i]] = cost_mine[i] for every rank's pairs, on every rank (entries nobody owns keep what
 * the caller put there).
 * wa_comm_gather_paths: rank `root` receives every rank's paths (path i: global index index_mine[i], len_mine[i] node ids, all ids
 * back to back in ids_mine) by ncclSend / ncclRecv; on the root the totals come back and wa_comm_gathered_paths_read copies them out
 * in rank order (index_out / len_out: n_paths_total entries, ids_out: n_ids_total); on the other ranks the totals are 0. */
int wa_comm_allgather_costs(wa_comm *c, int32_t n_mine, const int32_t *index_mine, const float *cost_mine, int32_t n_total, float *all);
int wa_comm_gather_paths(wa_comm *c, int32_t root, int32_t n_mine, const int32_t *index_mine, const int64_t *len_mine, const int32_t *ids_mine,
                         int64_t *n_paths_total, int64_t *n_ids_total);
int wa_comm_gathered_paths_read(wa_comm *c, int32_t *index_out, int64_t *len_out, int32_t *ids_out);
/* paths / node ids the last wa_comm_gather_paths left on this rank (the root: every rank's; elsewhere 0): what the three buffers of
 * wa_comm_gathered_paths_read must hold.  A gather that failed leaves nothing readable (0, 0). */
int wa_comm_gathered_paths_counts(const wa_comm *c, int64_t *n_paths, int64_t *n_ids);
/* The occupancy grid to every rank, once: rank `root` built its grid -- wa_grid_from_mesh is the reference's O(triangles x
 * voxels) creatGridMap, model_grid_map.hpp:223-268 -- and every other rank receives a replica (occupancy + the three axis tables:
 * ncclBroadcast over xGMI; 16 MiB at 256^3) instead of repeating that step.  `grid`: the root's grid (ignored elsewhere).  *out: a new
 * grid owned by the caller on every rank but the root, NULL on the root (which keeps using its own).  Collective: every rank calls it;
 * a rank whose arguments are bad still takes part in the header exchange, so that all ranks return an error together. */
int wa_comm_broadcast_grid(wa_comm *c, int32_t root, const wa_grid *grid, wa_grid **out);
/* bookkeeping helpers for a C++ launcher (timing max over ranks, totals): blocking all-reduce of host doubles */
enum { WA_COMM_MIN = 0, WA_COMM_MAX = 1, WA_COMM_SUM = 2 };
int wa_comm_allreduce_f64(wa_comm *c, double *inout, int32_t count, int32_t op);
int wa_comm_barrier(wa_comm *c);

/* ---- weld-seam ordering: replaces ACS_GTSP::readFromGraphFile's init + computeSolution
 *      (ACS_GTSP.hpp:187-218, :224-253, :255-284) ----------------------------------------- */
typedef struct {
    int32_t rng_mode;        /* WA_RNG_REF / WA_RNG_DEV */
    uint64_t seed;           /* DEV */
    uint32_t stream;         /* DEV */
    int32_t max_iterations;  /* <= 0: city_num^2 (:216) */
} wa_gtsp_params;
/* dist = n x n row-major symmetric doubles (diagonal ignored), cnt = distance count of the graph
 * header (:229).  n_instances problems laid out back to back (dist, tour_edges 2*n each, cost,
 * iters).  REF mode: rand_state36 (inout, may be NULL -> srand(1)) continues the libc stream
 * and n_instances must be 1. */
int wa_gtsp_solve(wa_ctx *ctx, const double *dist, int32_t n, int32_t cnt, int32_t n_instances,
                  const wa_gtsp_params *p, int32_t *rand_state36, int32_t *tour_edges,
                  double *tour_cost, int32_t *iterations, double *pheromone_out);

/* ---- path post-processing: what main.cpp:283-352 does with the planned path ----
 * wa_traj_stitch replaces ACS_GTSP::read_all_segments / read_segment (ACS_GTSP.hpp:286-312): segment s
 * is the node ids seg_ids[seg_off[s] .. seg_off[s+1]) (n_seg+1 offsets); coordinates come from the
 * grid's axis tables on the device.  reverse (may be NULL) flips individual segments -- the reference
 * appends best_matrix[i][j] as stored even when the tour runs j -> i. */
int wa_traj_stitch(const wa_grid *g, const int64_t *seg_ids, const int64_t *seg_off, int32_t n_seg,
                   const uint8_t *reverse, wa_traj **out);
int wa_traj_from_points(wa_ctx *ctx, const float *xyz, int64_t n, wa_traj **out);
int64_t wa_traj_size(const wa_traj *t);
int wa_traj_read(const wa_traj *t, float *xyz /* n x 3 */);
void wa_traj_destroy(wa_traj *t);

/* BS_Basic<float, DIM, DEGREE, CONST_LEVEL_INI, CONST_LEVEL_FIN> (BSplineBasic.h:33-56); the template
 * arguments are run-time values.  WA_ERR_ARG where the reference indexes out of bounds: dim outside
 * 1..16, degree outside 0..7, a constraint level above the degree, or NumKnots < 2*(DEGREE+1) (:53-55). */
int wa_bspline_create(wa_ctx *ctx, int32_t dim, int32_t degree, int32_t level_ini, int32_t level_fin,
                      int64_t n_middle, wa_bspline **out);
void wa_bspline_destroy(wa_bspline *b);
/* The reference reads heap cells it never wrote when level_fin + 1 > degree (c_mat[idx][CL+1],
 * BSplineBasic.h:414-431 -- BS_Basic<float,3,2,2,2> at main.cpp:337 does): their value is an input
 * here, as a 32-bit float pattern.  Default 0 (a fresh zeroed heap). */
int wa_bspline_set_uninit(wa_bspline *b, uint32_t float_bits);
/* SetParam (:72-78).  init / fin: (level+1) x dim floats (position, velocity, acceleration ...);
 * middle: n_middle rows of `stride` floats, the first dim of each are used (:458-464).  fin_time > 0. */
int wa_bspline_set_param(wa_bspline *b, const float *init, const float *fin, const float *middle,
                         int64_t stride, float fin_time);
/* same with the middle points already on the device (dim must be 3, wa_traj_size == n_middle) */
int wa_bspline_set_param_traj(wa_bspline *b, const float *init, const float *fin, const wa_traj *middle,
                              float fin_time);
int wa_bspline_info(const wa_bspline *b, int64_t *n_knots, int64_t *n_cps);
int wa_bspline_read(const wa_bspline *b, float *knots, float *cps /* n_cps x dim */);
/* getCurvePoint (:87-112, der = 0) / getCurveDerPoint (:122-146, der >= 1) for `count` times at once.
 * ok[i] (may be NULL) = the reference's bool result; rows with ok = 0 are zero-filled (the reference
 * leaves `ret` untouched). */
int wa_bspline_eval(wa_bspline *b, const float *u, int64_t count, int32_t der, float *out /* count x dim */,
                    uint8_t *ok);
/* ONE time, evaluated on the host from a mirror of the knots and control points (fetched once per SetParam) by the same fp32
 * operations in the same order as the kernel: bit-identical to wa_bspline_eval, ~0.1-0.2 us per call instead of a launch +
 * synchronise + copy.  What the drop-in BS_Basic::getCurvePoint / getCurveDerPoint use: main.cpp:302-316 / :341-351 call them once per
 * sample inside clock()-paced loops whose sample count depends on how long a call takes.  out: dim floats (zeros when *ok = 0). */
int wa_bspline_eval_host(wa_bspline *b, float u, int32_t der, float *out /* dim */, uint8_t *ok);
/* fixed-rate sampling u_i = t0 + (float)i * dt (fp32), replacing main.cpp's clock()-paced loops
 * (:302-316, :341-351).  out / ok may be NULL; out_traj (may be NULL, needs dim == 3 and der == 0 or
 * any der) receives the samples as a device-resident polyline, e.g. as the next spline's middle points. */
int wa_bspline_sample(wa_bspline *b, float t0, float dt, int64_t count, int32_t der, float *out,
                      uint8_t *ok, wa_traj **out_traj);

/* ---- obstacle clearance (not in the reference: its planner treats the torch as a point) ----
 * Distances are in voxel-INDEX units.  The axis tables are uniform at `precision` except at the hi-side seam of the wall
 * (model_grid_map.hpp:204-211, wa_axis_coords), so sqrt(d2) * precision is a distance in metres only up to that seam.
 *
 * wa_grid_distance_field: for every voxel v, min over occupied voxels o of (vx-ox)^2 + (vy-oy)^2 + (vz-oz)^2 (integers, exact);
 * 0 on occupied voxels; WA_D2_NONE everywhere when the grid has no occupied voxel.  Space outside the grid is not an obstacle.
 * Computed on the first call (or the first wa_grid_inflate / wa_traj_clearance) and kept on the device with the grid (freed by
 * wa_grid_destroy).  d2_out (n = nx*ny*nz int32 in raster order, like wa_grid_read_occupancy) may be NULL: then it only builds the
 * field.  WA_ERR_ARG when (nx-1)^2 + (ny-1)^2 + (nz-1)^2 >= 2^31 (a degenerate grid: the field would not fit int32). */
#define WA_D2_NONE 0x7fffffff
int wa_grid_distance_field(const wa_grid *g, int32_t *d2_out);
/* New grid (same dims, axis tables, precision, wall; own buffers; n_free recounted): voxel v is free iff g's v is free AND
 * (double)d2[v] > (double)radius * radius (WA_D2_NONE: no obstacle, farther than any radius) -- except inside keep bubbles: for each
 * keep id k (must be a free voxel of g, else WA_ERR_ARG), every voxel v with |v-k|^2 <= (radius+1)^2 (index units, double) keeps
 * g's state.  radius in voxels (>= 0, finite; 0 reproduces g's occupancy exactly).  g is not modified.  The result is an ordinary
 * grid for every other entry point.  Keep bubbles exist for weld points on the workpiece's surface (pass the ids resolved on g);
 * a bubble does not guarantee that a point in a concave corner connects to the free corridor around the part. */
int wa_grid_inflate(const wa_grid *g, float radius, const int64_t *keep_ids, int32_t n_keep, wa_grid **out);
typedef struct {
    int32_t min_d2;           /* over samples (WA_D2_NONE if no obstacle, or no sample) */
    int64_t argmin;           /* lowest sample index attaining it (-1 without samples) */
    int64_t first_hit;        /* lowest segment index whose supercover meets an occupied voxel, -1 if none */
    int64_t n_hit;            /* segments that do */
    int64_t n_outside;        /* samples outside the grid's coordinate range on some axis */
} wa_clearance_summary;
/* Checks a trajectory t (t's n points; t and g from one context) against g.  Voxel of a sample: per axis, p is clamped into
 * [smallest, largest] value of the axis table (NaN to the smallest; such samples count in n_outside), then the voxel index is the
 * lowest j minimising |p - c[j]| (fp32 subtraction).  d2 of a sample = the distance field at its voxel.  Segment i = samples i, i+1;
 * it hits iff some voxel of the 3-D supercover between their voxels a, b is occupied, where with d = b - a, per axis c the set of
 * t is every t when d_c = 0 and v_c = a_c (none if v_c != a_c), else the closed interval between (2(v_c-a_c)-1)/(2d_c) and
 * (2(v_c-a_c)+1)/(2d_c); v is in the supercover iff [0,1] and the three sets share a t (the segment between the voxel centres touches
 * v's closed cube: conservative at edges and corners).  A stitched path of 6-neighbour free voxels has no hit as long as every node
 * maps back to itself, which fails where an axis table holds one coordinate twice: at the hi seam when (hi - lo) / precision is an
 * exact integer, lowest-j-on-ties maps the upper node to the one below it.  ids_out / d2_out (n) and hit_out (n-1) may be NULL;
 * sum may not.  At most 2^33 samples. */
int wa_traj_clearance(const wa_grid *g, const wa_traj *t, int64_t *ids_out, int32_t *d2_out, uint8_t *hit_out,
                      wa_clearance_summary *sum);

/* ---- any-angle path shortening (not in the reference: its paths are lattice staircases) ----
 * A path is a sequence of node ids v_0 ... v_{L-1}, raster ids of grid g, L >= 1.
 * visible(a, b): the 3-D supercover between voxels a and b contains no occupied voxel of g.  This is exactly the segment test of
 *   wa_traj_clearance: same events, tied axes stepped together, the full product set at a tie, voxel a itself included.
 * Greedy shortcut with a span cap max_span >= 1: start with w_0 = 0.  From an anchor a < L-1, next(a) is the largest j in
 *   [a+1, min(a+max_span, L-1)] such that visible(v_a, v_k) holds for EVERY k in (a, j] (prefix visibility, not just the last node);
 *   if no such j exists, next(a) = a+1 (a 26-neighbour diagonal step that grazes an occupied edge, or an occupied node).  Stop when
 *   L-1 is reached: the first and last nodes are always kept.
 * Length: the sum over consecutive waypoints of sqrt(dx^2 + dy^2 + dz^2), in float64 on the fp32 axis-table coordinates
 *   (wa_grid_read_coords), every operation correctly rounded on its own (no contraction; (dx*dx + dy*dy) + dz*dz), summed
 *   sequentially in waypoint order.
 *
 * n_paths paths back to back: path p = ids[off[p] .. off[p+1]) (n_paths+1 offsets, off[0] = 0, non-decreasing, empty paths allowed).
 * wp_idx (off[n_paths] entries): for path p, its waypoints as indices INTO path p, written at wp_idx[off[p] .. off[p] + wp_count[p]);
 * later entries of its range are left untouched.  length_out (may be NULL): the shortened length in metres.
 * WA_ERR_ARG: NULL g/ids/off/wp_idx/wp_count, n_paths < 0, max_span < 1 or > 4096, off not non-decreasing, an id outside the grid. */
int wa_grid_path_shortcut(const wa_grid *g, const int64_t *ids, const int64_t *off, int32_t n_paths, int32_t max_span,
                          int64_t *wp_idx, int32_t *wp_count, double *length_out);

/* ---- exact shortest-path fields (not in the reference: its planner is the colony alone) ----
 * The graph: the free voxels of g (wa_grid_read_occupancy != 0); voxel (x, y, z) has raster id x + nx * (y + ny * z).  Two free voxels are
 * joined iff they differ by 1 in exactly one coordinate (the 6-neighbour lattice), every step costs 1.  Neighbours are taken in the fixed
 * order -x, +x, -y, +y, -z, +z; a neighbour outside the grid does not exist.  26-neighbour lattices need a different algorithm (unit
 * steps make this breadth-first search): see "exact shortest paths with diagonal moves" below, which takes integer step weights.
 * hops(s, v): the number of steps of a shortest such path from s to v; 0 for v = s; WA_HOPS_NONE when there is none (v lies in another
 *   component, or is occupied).  An int32, exact at any length a grid allows (also beyond 65 535).
 * path(s, e), for hops(s, e) = h >= 0: the h + 1 ids p_0 ... p_h with p_h = e and, for k = h ... 1, p_{k-1} = the first neighbour
 *   n of p_k in the order above that is inside the grid, free and has hops(s, n) = k - 1.  With s == e it is the one id.
 * Sources, starts and ends must be free voxels: an occupied one is WA_ERR_ARG (wa_last_error says so), like an id outside the grid, a
 * NULL id array (also with a count of 0), a NULL output or a negative count; on WA_ERR_ARG no output has been written.  Counts of 0
 * with valid pointers succeed and write nothing.
 *
 * Everything runs on the context's stream and g is not modified; a bit-packed copy of its occupancy (one bit per voxel, rows in x
 * padded to 64) is built by the first call and kept with the grid like the distance field (freed by wa_grid_destroy).  Per source the
 * search keeps three such bitmaps on the device, and a field of 4 bytes per voxel where one is needed (_fields, _paths); sources are
 * processed in chunks of at most half of what wa_ctx_memory_info reports free over that cost, at least 1, at most 65 535
 * (WA_ERR_ALLOC when one source does not fit).  Results do not depend on the chunking and are the same bytes on every call.
 *
 * wa_grid_geodesic_fields: hops_out[s * n + v] = hops(src_ids[s], v) for every voxel v (n = nx * ny * nz; n_src * n int32 on the host).
 * wa_grid_geodesic_matrix: hops_out[i * n_pts + j] = hops(point_ids[i], point_ids[j]): symmetric, 0 on the diagonal, WA_HOPS_NONE where
 *   the two points are not connected.  No field is stored; a point's search ends as soon as every point has been reached.
 * wa_grid_geodesic_paths: pair p = (start_ids[p], end_ids[p]); off holds n_pairs + 1 non-decreasing offsets (off[0] need not be 0) and
 *   gives pair p the range ids_out[off[p] .. off[p+1]).  hops_out[p] = hops(start, end) is filled for every pair.  A pair with
 *   hops >= 0 whose range holds at least hops + 1 ids gets path(start, end) at ids_out[off[p] .. off[p] + hops]; later entries of its
 *   range are left untouched.  An unreachable pair writes nothing and is no error.  If some reachable pair's range is too short, nothing
 *   is written into that pair's range, all other pairs are written as usual and the call returns WA_ERR_CAPACITY: size off from
 *   hops_out (or from the matrix) and call again.  Pairs that share a start share one field, in whatever order they come.
 *   Also WA_ERR_ARG: off decreasing. */
#define WA_HOPS_NONE (-1)
int wa_grid_geodesic_fields(const wa_grid *g, const int64_t *src_ids, int32_t n_src, int32_t *hops_out);
int wa_grid_geodesic_matrix(const wa_grid *g, const int64_t *point_ids, int32_t n_pts, int32_t *hops_out);
int wa_grid_geodesic_paths(const wa_grid *g, const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                           const int64_t *off, int64_t *ids_out, int32_t *hops_out);

/* ---- clearance-weighted exact shortest paths (not in the reference) ----
 * The graph is the one of the section above: the free voxels of g on the 6-neighbour lattice, neighbours in the fixed order -x, +x, -y,
 * +y, -z, +z.  Here ENTERING voxel v costs cost[v], a small integer, instead of 1.
 * WA_COST_MAX = 8.  A cost array is n = nx * ny * nz bytes on the host in raster order, like wa_grid_read_occupancy.  Every free voxel
 *   must hold a value in 1 .. WA_COST_MAX; the bytes of occupied voxels are ignored.
 * dist(s, v): the minimum, over lattice paths of free voxels s = p_0, p_1 ... p_h = v, of cost[p_1] + ... + cost[p_h].  The start is not
 *   paid for, so dist(s, s) = 0.  WA_DIST_NONE where there is no such path or v is occupied.  With every cost 1 this is hops(s, v), bit
 *   for bit.  It is not symmetric: dist(s, e) - dist(e, s) = cost[e] - cost[s]; cost[s] + dist(s, e) is.
 * path(s, e), for dist(s, e) >= 0: walking back from e, the predecessor of a node p with dist(s, p) = D > 0 is the first neighbour q in
 *   the order above that is inside the grid, free and has dist(s, q) = D - cost[p]; the walk ends at s (D = 0).  The path is returned
 *   start first.  Its number of nodes is an output of its own: it does not follow from the distance.
 * Clearance costs: cost[v] = 0 on occupied voxels, else 1 + #{k < n_thr : d2[v] <= thr2[k]} with d2 the field of
 *   wa_grid_distance_field.  0 <= n_thr <= WA_COST_MAX - 1, every 0 <= thr2[k] < WA_D2_NONE, in any order.  Thresholds 1, 4, 9 give
 *   cost 4 next to an obstacle, then 3, 2, and 1 from a distance of more than 3 voxels on (and everywhere on a grid without obstacles).
 *
 * The calls are stateless: the cost array comes in with each call and nothing about it is kept with the grid; an array from
 * wa_grid_clearance_costs and a hand-made one are treated alike.  WA_ERR_ARG, before any output is written: a NULL pointer (also with a
 * count of 0), a negative count, an id outside the grid or on an occupied voxel, decreasing offsets, a free voxel whose cost is 0 or
 * above WA_COST_MAX, a threshold out of range, n_thr above WA_COST_MAX - 1, and a grid for which (largest cost present on a free
 * voxel) * (n_free - 1) exceeds 2^31 - 1: a distance might not fit int32.  Counts of 0 with valid pointers succeed and write nothing
 * (the cost array is not looked at then).
 *
 * Memory: a call keeps the cost bytes (n) and three bitmaps of them on the device; with W the largest cost present, a source costs W + 2
 * bitmaps of n / 8 bytes (rows in x padded to 64 voxels), plus 4 n bytes where a field is kept (_fields, _paths), plus its matrix row.
 * Sources are processed in chunks by the rule of the section above (half of the free memory, at least 1, at most 65 535, WA_ERR_ALLOC
 * when one source does not fit).  Results do not depend on the chunking and are the same bytes on every call.
 *
 * wa_grid_clearance_costs: cost_out[v] (n bytes on the host) by the rule above; builds the distance field if the grid has none yet.
 * wa_grid_weighted_fields: dist_out[s * n + v] = dist(src_ids[s], v) for every voxel v (n_src * n int32 on the host).
 * wa_grid_weighted_matrix: dist_out[i * n_pts + j] = dist(point_ids[i], point_ids[j]); 0 on the diagonal, WA_DIST_NONE where the two
 *   points are not connected.  No field is stored; a point's search ends as soon as its row is full.
 * wa_grid_weighted_paths: the protocol of wa_grid_geodesic_paths.  Pair p = (start_ids[p], end_ids[p]); off holds n_pairs + 1
 *   non-decreasing offsets and gives pair p the range ids_out[off[p] .. off[p+1]).  dist_out[p] = dist(start, end) and len_out[p] = the
 *   nodes of path(start, end) (0 when unreachable) are filled for every pair.  A reachable pair whose range holds at least len_out[p] ids
 *   gets its path at ids_out[off[p] .. off[p] + len_out[p]); later entries of its range are left untouched.  An unreachable pair writes
 *   nothing and is no error.  If some reachable pair's range is too short, nothing is written into that pair's range, all other pairs
 *   are written as usual and the call returns WA_ERR_CAPACITY: size off from len_out and call again.  Pairs that share a start share one
 *   field, in whatever order they come. */
#define WA_COST_MAX 8
#define WA_DIST_NONE (-1)
int wa_grid_clearance_costs(const wa_grid *g, const int32_t *thr2, int32_t n_thr, uint8_t *cost_out);
int wa_grid_weighted_fields(const wa_grid *g, const uint8_t *cost, const int64_t *src_ids, int32_t n_src, int32_t *dist_out);
int wa_grid_weighted_matrix(const wa_grid *g, const uint8_t *cost, const int64_t *point_ids, int32_t n_pts, int32_t *dist_out);
int wa_grid_weighted_paths(const wa_grid *g, const uint8_t *cost, const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                           const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out);

/* ---- exact shortest paths with diagonal moves: 26-neighbour chamfer fields (not in the reference) ----
 * The graph: the nodes are the free voxels of g.  A move changes each coordinate by -1, 0 or +1, at least one of them; its class a in
 * {1, 2, 3} is the number of coordinates that change (face, edge, corner).  The move u -> v exists iff all 2^a voxels of the box
 * {u.x, v.x} x {u.y, v.y} x {u.z, v.z} are inside the grid and free, and it costs step[a - 1].  For two 26-neighbours the box rule is
 * visible(u, v) of wa_grid_path_shortcut and the segment test of wa_traj_clearance (the full product set at a tie), so a returned path
 * has no hit in wa_traj_clearance, under the proviso stated there for 6-neighbour paths.  The rule is symmetric, and so is dist.
 * WA_STEP_MAX = 16.  step holds three int32 on the host, each in 1 .. WA_STEP_MAX; no order among them is required (3, 4, 5 approximates
 *   the Euclidean 1, sqrt 2, sqrt 3 within 8 %; every distance stays an integer).
 * dist(s, v): the least sum of step costs over such paths from s to v; 0 for v = s; WA_DIST_NONE where there is no path or v is occupied.
 * path(s, e), for dist(s, e) >= 0: walking back from e, the predecessor of a node p with dist(s, p) = D > 0 is q = p + o for the first
 *   offset o, in the fixed order below, such that the move q -> p exists and dist(s, q) = D - step[class(o) - 1]; the walk ends at s.
 *   The order: the six face offsets -x, +x, -y, +y, -z, +z, then the 12 edge offsets, then the 8 corner offsets, edge and corner offsets
 *   each sorted by (dz, dy, dx) ascending.  The path is returned start first; its number of nodes is an output of its own.
 * Identities that follow from the definition:
 *   step = {1, 2, 3}: dist equals hops of wa_grid_geodesic_fields bit for bit (a diagonal exists only where the face detours through its
 *     box exist, so it never wins), and by the face-first order path equals wa_grid_geodesic_paths' path.
 *   step = {1, 1, 1} on a grid without obstacles: dist is the Chebyshev distance max(|dx|, |dy|, |dz|).
 *   step = {3, 4, 5} on a grid without obstacles: with the sorted |differences| a >= b >= c, dist = 3 (a - b) + 4 (b - c) + 5 c.
 *
 * The calls are stateless and repeatable: the same bytes on every call, whatever ran before on the grid.  WA_ERR_ARG, before any output
 * is written: a NULL pointer (step included, also with a count of 0), a negative count, a step outside 1 .. WA_STEP_MAX, a grid for
 * which max(step) * (n_free - 1) exceeds 2^31 - 1 (a distance might not fit int32; refused before any search), an id outside the grid
 * or on an occupied voxel, decreasing offsets.  Counts of 0 with valid arguments succeed and write nothing.
 *
 * Memory: with R = max(step) + 1, a source costs R + 1 bitmaps of n / 8 bytes (rows in x padded to 64 voxels), plus 4 n bytes where a
 * field is kept (_fields, _paths), plus its matrix row.  Sources are processed in chunks by the rule of the geodesic section (half of
 * the free memory, at least 1, at most 65 535, WA_ERR_ALLOC when one source does not fit); results do not depend on the chunking.
 *
 * wa_grid_chamfer_fields: dist_out[s * n + v] = dist(src_ids[s], v) for every voxel v (n_src * n int32 on the host).
 * wa_grid_chamfer_matrix: dist_out[i * n_pts + j] = dist(point_ids[i], point_ids[j]): symmetric, 0 on the diagonal, WA_DIST_NONE where
 *   the two points are not connected.  No field is stored; a point's search ends as soon as its row is full.
 * wa_grid_chamfer_paths: the protocol of wa_grid_weighted_paths.  Pair p = (start_ids[p], end_ids[p]); off holds n_pairs + 1
 *   non-decreasing offsets and gives pair p the range ids_out[off[p] .. off[p+1]).  dist_out[p] and len_out[p] (the nodes of the path, 0
 *   when unreachable) are filled for every pair.  A reachable pair whose range holds at least len_out[p] ids gets its path at
 *   ids_out[off[p] .. off[p] + len_out[p]); later entries of its range are left untouched.  An unreachable pair writes nothing and is no
 *   error.  If some reachable pair's range is too short, nothing is written into that pair's range, all other pairs are written as
 *   usual and the call returns WA_ERR_CAPACITY: size off from len_out and call again.  Pairs that share a start share one field. */
#define WA_STEP_MAX 16
int wa_grid_chamfer_fields(const wa_grid *g, const int32_t step[3], const int64_t *src_ids, int32_t n_src, int32_t *dist_out);
int wa_grid_chamfer_matrix(const wa_grid *g, const int32_t step[3], const int64_t *point_ids, int32_t n_pts, int32_t *dist_out);
int wa_grid_chamfer_paths(const wa_grid *g, const int32_t step[3], const int64_t *start_ids, const int64_t *end_ids, int32_t n_pairs,
                          const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out);

/* ---- exact shortest paths with diagonal moves and clearance penalties (not in the reference) ----
 * The graph, the box rule for a move, the three classes, step[3] in 1 .. WA_STEP_MAX and the order of the 26 offsets are exactly those
 * of the section above.  New is a penalty per voxel, paid on entry, which keeps paths off the metal where there is room and still lets
 * them through gaps that wa_grid_inflate would close.
 * WA_PEN_MAX = 31.  pen is n = nx * ny * nz bytes on the host in raster order, like wa_grid_read_occupancy.  Every free voxel holds a
 *   value in 0 .. WA_PEN_MAX; the bytes of occupied voxels are ignored.
 * The move u -> v costs step[class - 1] + pen[v].  The penalty is per voxel ENTERED, not per length: a corner move pays it once, like a
 *   face move.  The start is not paid for.
 * dist(s, v): the least sum of move costs over paths from s to v; dist(s, s) = 0; WA_DIST_NONE where there is no path or v is occupied.
 * path(s, e), for dist(s, e) >= 0: walking back from e, the predecessor of a node p with dist(s, p) = D > 0 is q = p + o for the first
 *   offset o, in the order of the section above, such that the move exists and dist(s, q) = D - pen[p] - step[class(o) - 1] >= 0; the walk
 *   ends at s.  The path is returned start first; its number of nodes is an output of its own.
 * Identities that follow from the definition:
 *   (a) pen = 0 on every free voxel: dist, the matrix and the paths are the bytes of wa_grid_chamfer_fields / _matrix / _paths, for any step.
 *   (b) pen = c on every free voxel: they are those of the chamfer calls with step[k] + c, where these fit WA_STEP_MAX.
 *   (c) dist(s, e) - dist(e, s) = pen[e] - pen[s] (a path reversed enters the same voxels but for its two ends), so the matrix is NOT
 *       symmetric; pen[s] + dist(s, e) is.  Reachability is symmetric.
 *
 * The calls are stateless and repeatable: the penalty array comes in with each call, nothing about it is kept with the grid, and the
 * same bytes come back on every call, in any chunking.  WA_ERR_ARG, before any output is written: everything the section above refuses
 * (a NULL pointer, step included, also with a count of 0; a negative count; a step outside 1 .. WA_STEP_MAX; max(step) * (n_free - 1)
 * above 2^31 - 1; an id outside the grid or on an occupied voxel; decreasing offsets), a NULL pen (also with a count of 0), a free voxel
 * whose penalty is above WA_PEN_MAX, and a grid for which (max(step) + the largest penalty present on a free voxel) * (n_free - 1)
 * exceeds 2^31 - 1 (a distance might not fit int32; refused before any search).  Counts of 0 with valid pointers succeed, write nothing
 * and do not look at pen.
 *
 * Memory: a call keeps the penalty bytes (n) and five bitmaps of them on the device.  With R = max(step) + P + 1, P the largest penalty
 * present on a free voxel, a source costs R + 1 bitmaps of n / 8 bytes (rows in x padded to 64 voxels), plus 4 n bytes where a field is
 * kept (_fields, _paths), plus its matrix row.  Sources are processed in chunks by the rule of the geodesic section (half of the free
 * memory, at least 1, at most 65 535, WA_ERR_ALLOC when one source does not fit); results do not depend on the chunking.
 *
 * wa_grid_chamfer_weighted_fields: dist_out[s * n + v] = dist(src_ids[s], v) for every voxel v (n_src * n int32 on the host).
 * wa_grid_chamfer_weighted_matrix: dist_out[i * n_pts + j] = dist(point_ids[i], point_ids[j]): 0 on the diagonal, WA_DIST_NONE where the
 *   two points are not connected, not symmetric (identity (c)).  No field is stored; a point's search ends as soon as its row is full.
 * wa_grid_chamfer_weighted_paths: the protocol of wa_grid_chamfer_paths, WA_ERR_CAPACITY and what it leaves untouched included. */
#define WA_PEN_MAX 31
int wa_grid_chamfer_weighted_fields(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *src_ids, int32_t n_src, int32_t *dist_out);
int wa_grid_chamfer_weighted_matrix(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *point_ids, int32_t n_pts, int32_t *dist_out);
int wa_grid_chamfer_weighted_paths(const wa_grid *g, const int32_t step[3], const uint8_t *pen, const int64_t *start_ids, const int64_t *end_ids,
                                   int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dist_out, int32_t *len_out);

/* ---- trajectory fit that refines the spline until it clears the grid (not in the reference: main.cpp:337 fits through the path
 *      points as they are) ----
 * A B-spline of degree D lies in the convex hull of D + 1 consecutive control points.  Control points placed ON a collision-free
 * polyline, closely enough where the curve hits, pull the curve onto that polyline.  The call does that on the device: control
 * polygon -> fit -> sample -> check -> blame -> refine, until no segment of the sampled curve hits or nothing can be refined.
 *
 * g is the grid the curve is CHECKED against (the metal, not an inflated planning grid).  poly holds n >= 2 points; leg k joins
 * points k and k + 1, k = 0 .. n - 2; zero-length legs are legal.  Every leg k has a level s_k, 0 at the start.  One round:
 * 1. Pieces.  len_k = the length of leg k as wa_grid_path_shortcut defines one: float64 on the fp32 coordinates, dx = (double)b_x -
 *    (double)a_x and so on, sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded on its own.  In float64, each operation rounded on its
 *    own: q = (len_k * (double)(1 << s_k)) / (double)spacing; m_k = (int64)ceil(q) if ceil(q) >= 1, else 1.
 * 2. Control polygon.  Leg k (from a to b) contributes j = 0 .. m_k - 1: per axis a + (b - a) * ((float)j / (float)m_k), in fp32, each of
 *    the four operations rounded on its own (no contraction); behind the last leg comes the polyline's last point.  Point 0 is the
 *    spline's initial position, the last point its final position, all points between are its middle points, in order.
 *    owner[c] = the leg control point c came from; the constrained control points at either end belong to the first / the last leg.
 * 3. Fit.  BS_Basic<float, 3, D, D-1, D-1> (D = degree, 2 or 3) on those points, end derivatives of every constrained level zero,
 *    fin_time = (float)(number of knot spans) = (float)(middle points + D): the knot step is exactly 1.0f and knot i is the integer
 *    min(max(i - D, 0), fin_time).  A fit of more than 2^24 control points (in any round) is refused with WA_ERR_ARG.
 * 4. Sample and check.  u_i = (float)i * dt, dt = fin_time / (float)(n_samples - 1) (fp32), i = 0 .. n_samples - 1, evaluated as
 *    wa_bspline_sample(b, 0, dt, n_samples) does; then wa_traj_clearance of those samples against g: the same voxel lookup, the same
 *    segment test.  No hit: the loop ends.
 * 5. Blame.  For a hit segment i, take the knot span the evaluation used for u_i and for u_(i+1) (_findSpan, BSplineBasic.h:358-385,
 *    after the clamp into the knot range); the control points with a non-zero basis there are span - D .. span; every leg that owns
 *    one of them is marked.
 * 6. Refine.  n_legs_at_cap = the marked legs with s_k = max_level.  Every marked leg with s_k < max_level gets s_k + 1.  If no level
 *    changed, or this was round 32, the loop ends (in round 32 no level is raised); otherwise the next round starts at 1.
 * max_level is in 0 .. 8 (0: one plain fit on the given spacing).  Every round but the last raises at least one leg, so the loop ends.
 *
 * Results: *spline_out = the last round's spline, an ordinary wa_bspline owned by the caller (eval, derivatives, wa_bspline_read);
 * *samples_out (may be NULL) = its n_samples samples as a device-resident polyline owned by the caller; leg_level_out (n - 1 int32, may
 * be NULL) = the levels that spline was built with; *sum as below.  The call does NOT promise final.n_hit == 0: the segment test is
 * conservative (two consecutive samples in diagonal voxels test the whole product set), so a curve arbitrarily close to a visible leg
 * can still be reported, and inside the keep bubbles of wa_grid_inflate a path touches the metal by design.  rounds == 32 or
 * n_legs_at_cap > 0 with final.n_hit > 0 tell the caller so.  Where control points are dense the curve is slow (time runs one knot
 * span per unit): the fit shapes the curve, it does not re-time it.
 *
 * WA_ERR_ARG, before anything is written: NULL g / poly / sum / spline_out, poly and g from different contexts, n < 2, degree outside
 * {2, 3}, spacing not finite or <= 0, max_level outside 0 .. 8, n_samples < 2 or > 2^33, a coordinate of poly that is not finite.
 * Same bytes on every call; everything runs on the context's stream. */
typedef struct {
    int32_t rounds;         /* fits made (>= 1) */
    int32_t max_level_used; /* the highest level of any leg */
    int64_t n_legs;         /* n - 1 */
    int64_t n_legs_at_cap;  /* legs at max_level that were still blamed in the last round */
    int64_t n_cps;          /* control points of the final spline */
    int64_t n_hit_first;    /* hit segments of round 1: the unrefined fit on the same control spacing */
    wa_clearance_summary final; /* of the final samples against g: n_hit == 0 is the success case */
} wa_fit_summary;
int wa_grid_fit_trajectory(const wa_grid *g, const wa_traj *poly, int32_t degree, float spacing, int32_t max_level, int64_t n_samples,
                           int32_t *leg_level_out, wa_bspline **spline_out, wa_traj **samples_out, wa_fit_summary *sum);

/* ---- re-timing a sampled trajectory: speed caps, ramps, controller ticks (not in the reference: main.cpp:341-351 and :117-131 pace
 *      their loops by clock()) ----
 * t holds samples p_0 ... p_(n-1) (fp32, 2 <= n <= 2^31), segment i joins p_i and p_(i+1).  The call finds the fastest speed profile along
 * the samples that starts and ends at rest, stays below every cap and within the tangential acceleration / deceleration limits, the
 * time at which every sample is reached, and the positions at a fixed controller period.  Everything is defined in integers of
 * Q = 2^30 quanta per unit (of length, of squared speed, of time) so that the result is the same bytes whatever computes it.
 * "double" is IEEE float64, every operation rounded on its own (no contraction); rint rounds ties to even.
 * 1. Lengths.  ds_i = the length of segment i as wa_grid_path_shortcut defines one (double on the fp32 coordinates,
 *    sqrt((dx*dx + dy*dy) + dz*dz)).  L_i = (int64)rint(ds_i * Q), A_i = (int64)rint(((2 * acc) * ds_i) * Q), D_i likewise with dec (each 2^61
 *    where the product is 2^61 or more); where L_i > 0 both A_i and D_i are raised to at least 1, where L_i = 0 both are 0.  GA, GD = the
 *    exclusive prefix sums of A, D over segments (GA_0 = 0, n entries).
 * 2. Caps, as squared speeds in double, per sample; the cap of a sample is the minimum, its kind the lowest-numbered kind attaining it.
 *    Kind 0: samples 0 and n-1 have cap 0 (rest to rest).  Kind 1: m * m with m = min(v_max, (double)v_limit[i]).  Kind 2, interior
 *    samples only and only when a_lat is finite and not 0: with u = p_i - p_(i-1), v = p_(i+1) - p_i, w = p_(i+1) - p_(i-1) in double,
 *    c = |u x v| (components u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x; every norm sqrt((x*x + y*y) + z*z)),
 *    den = (|u| * |v|) * |w|: if c > 0 and den > 0 the cap is a_lat / ((2 * c) / den) (Menger curvature), else none.  Kind 3, when g is given
 *    and near_d2 >= 0: the sample's voxel by the lookup of wa_traj_clearance; if its d2 <= near_d2 the cap is v_near * v_near.
 *    C_i = (int64)floor(cap * Q), and 2^61 where that product is infinite or >= 2^61.
 * 3. Forward and backward pass.  F_0 = C_0, F_i = min(C_i, F_(i-1) + A_(i-1)); B_(n-1) = F_(n-1), B_i = min(F_i, B_(i+1) + D_i).  In integers
 *    these are exactly F_i = min_(j <= i) (C_j - GA_j) + GA_i and B_i = min_(j >= i) (F_j + GD_j) - GD_i, a prefix and a suffix minimum, which
 *    is what the device computes.  w_q_out[i] = B_i, the squared speed at sample i.
 * 4. bound_out[i]: bit 0 B_i = C_i; bit 1 i > 0 and B_i - B_(i-1) = A_(i-1); bit 2 i < n-1 and B_i - B_(i+1) = D_i; bits 4-5 the kind of the
 *    sample's cap.  Every sample has at least one of bits 0-2: the profile is on a cap or on a ramp everywhere, which is what makes it
 *    the fastest one.
 * 5. Times.  v_i = sqrt((double)B_i / Q).  (a) L_i = 0: dt_i = 0.  (b) L_i > 0 and v_i + v_(i+1) = 0 (a segment from rest to rest):
 *    w_p = (((2 * ds_i) * acc) * dec) / (acc + dec), t_up = sqrt(w_p) / acc, dt_i = t_up + sqrt(w_p) / dec.  (c) otherwise
 *    dt_i = (2 * ds_i) / (v_i + v_(i+1)).  T_i = (int64)rint(dt_i * Q); time_q_out = the exclusive prefix sum of T (entry 0 is 0, entry n-1
 *    the duration).
 * 6. Ticks.  tick_q = (int64)rint(tick * Q), in 1 .. 2^61.  Outputs at tau_k = k * tick_q for k = 0 .. floor(duration / tick_q), and one
 *    more at the duration if that is no multiple of tick_q.  For a tau: i = the largest index in 0 .. n-2 with time_q[i] <= tau;
 *    e = (double)(tau - time_q[i]) / Q.  If tau >= time_q[i+1] the output is p_(i+1) exactly; else if L_i = 0 it is p_i exactly.  Else, in
 *    case (c), s = (v_i * e) + ((0.5 * a) * e) * e with a = ((double)(B_(i+1) - B_i) / Q) / (2 * ds_i); in case (b) s = ((0.5 * acc) * e) * e for
 *    e <= t_up, else ds_i - ((0.5 * dec) * r) * r with r = dt_i - e.  lambda = s / ds_i clamped into [0, 1]; per axis
 *    out = (float)((double)a_c + ((double)b_c - (double)a_c) * lambda) with a = p_i, b = p_(i+1).  *ticks_out is an ordinary device-resident
 *    wa_traj owned by the caller: wa_traj_clearance can check what the controller will actually be sent.
 * 7. Errors.  WA_ERR_ARG before anything is written: NULL t / lim / sum, g and t from different contexts, n < 2 or > 2^31, v_max / acc /
 *    dec not finite or <= 0, a_lat negative or NaN, v_near not finite or <= 0 where it is used (g given and near_d2 >= 0), a v_limit
 *    entry not finite or <= 0, a coordinate that is not finite, tick not finite or tick_q outside 1 .. 2^61, the sum of L, of A, of D or
 *    of T reaching 2^61.  More than 2^31 ticks: WA_ERR_CAPACITY with *sum and the per-sample outputs filled and *ticks_out = NULL.
 * time_q_out, w_q_out, bound_out (n entries each, host) and ticks_out may be NULL.  Same bytes on every call; everything runs on the
 * context's stream; g and t are not modified.  g may be NULL: then there is no clearance cap and n_outside is 0.
 * (Stops inside the motion -- arc start, crater fill, a turn in place: wa_traj_retime_stops, rules 40 - 42 at the end of this header.) */
typedef struct {
    double v_max;     /* speed cap everywhere, coordinate units per second, > 0, finite */
    double acc, dec;  /* tangential acceleration / deceleration, > 0, finite */
    double a_lat;     /* lateral (centripetal) acceleration allowed; +inf or 0: no curvature cap */
    double v_near;    /* speed cap where the distance field says "near the metal"; ignored when g == NULL or near_d2 < 0 */
    int32_t near_d2;  /* "near": d2 of the sample's voxel <= near_d2 (voxel-index units squared, as wa_traj_clearance reports); < 0: off */
} wa_retime_limits;
typedef struct {
    int64_t n, n_ticks;          /* samples in, positions out */
    int64_t length_q, time_q;    /* total arc length and duration in quanta of 2^-30 (units, seconds) */
    int64_t n_bound[4];          /* samples whose cap is of kind: 0 an end point, 1 v_max / v_limit, 2 curvature, 3 clearance */
    int64_t n_on_cap, n_on_ramp; /* samples with B == C; samples with a tight ramp on either side (may overlap) */
    int64_t n_triangle;          /* segments travelled rest -> peak -> rest (rule 5b) */
    int64_t n_outside;           /* as wa_clearance_summary (0 when g == NULL) */
    int64_t peak_w_q;            /* largest squared speed reached, in quanta */
} wa_retime_summary;
int wa_traj_retime(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit, double tick,
                   int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out, wa_retime_summary *sum);

/* ---- seam tours: order and direction of two-ended weld seams (not in the reference: ACS_GTSP orders points) ----
 * m seams, 2m endpoints: seam s has endpoints 2s and 2s+1.  The torch enters a seam at one end, leaves it at the other and travels to the
 * next seam; the calls choose the order of the seams and the direction of each so that the travel between seams is short.  Everything
 * is defined in integers so that the result is the same bytes whatever computes it (DESIGN 4n holds the full text).
 * 1. Costs.  dist is 2m x 2m doubles, row-major; only i < j is read (and mirrored), the diagonal and the entries (2s, 2s+1) are ignored
 *    (a seam's own length is constant).  W[i][j] = (int64)rint(dist[i][j] * 2^20), ties to even; every entry read must be finite, >= 0 and
 *    give W < 2^40.
 * 2. Open tours.  closed == 0 appends a dummy seam m whose endpoints cost 0 to every endpoint; M = m + 1 (else M = m).  The result is the
 *    closed tour on M seams with the dummy removed, starting with the seam behind it.  A closed result starts with seam 0.
 * 3. State.  Positions 0 .. M-1 (taken mod M) hold seam P[k] and direction d[k]: in(k) = 2 P[k] + d[k], out(k) = 2 P[k] + 1 - d[k],
 *    cost = sum_k W[out(k)][in(k+1)].  dir_out[k] = d[k]: 0 enters seam order_out[k] at its even endpoint.
 * 4. Moves.  A, Reverse(i, j), 0 <= i <= j <= M-1, j - i <= M-2: positions i..j reversed, their d flipped; number i*M + j.
 *    B, Move(i, L, g, r), 1 <= L <= min(or_len, M-2), i + L - 1 <= M-1, g outside the block and not i-1 mod M: the block i..i+L-1 leaves
 *    the array and goes in directly behind the element that stood at g (reversed and flipped when r = 1);
 *    number M*M + (((i*3 + L-1)*M + g)*2 + r).  A pass evaluates every move, takes the smallest cost change (the lowest number among
 *    equals) and applies it if it is negative; otherwise the start has ended.  A start also ends after max_passes passes (n_capped).
 * 5. Starts.  Start 0 is order0 / dir0 (NULL: the identity order / all 0; the dummy stands last).  Start r >= 1 is drawn from a
 *    splitmix64 stream seeded with seed ^ (r * 0xD1B54A32D192ED03): Fisher-Yates from the identity for k = M-1 .. 1 with
 *    j = ((draw >> 32) * (k+1)) >> 32, then d[k] = draw >> 63 for k = 0 .. M-1.  The start with the smallest final cost wins, the lowest
 *    index among equals.
 * 6. wa_gtsp_seam_tour_exact: the optimum by dynamic programming over subsets, M <= 16 (WA_ERR_CAPACITY above); of equal tours the one that
 *    backtracking from the end with the lowest endpoint at every step finds, seam 0 first with d = 0 before the open/closed handling.
 * WA_ERR_ARG, before anything is written: a NULL pointer (order0, dir0, start_cost_q_out, start_passes_out may be NULL), m outside
 * 1 .. 1024, or_len outside 0 .. 3, n_starts or max_passes outside 1 .. 2^20, an order0 that is no permutation of 0 .. m-1, a dir0 entry
 * above 1, a cost that breaks rule 1.  order_out / dir_out hold m entries, start_cost_q_out / start_passes_out n_starts entries (host).
 * Same bytes on every call; everything runs on the context's stream.  (The calls carry the order stage's wa_gtsp_ prefix: they take
 * a context like wa_gtsp_solve and stand where it stands in the pipeline.) */
typedef struct {
    int32_t closed;       /* != 0: the tour returns to its first seam */
    int32_t or_len;       /* longest block that move B takes, 0 .. 3 (0: reversals only) */
    int32_t n_starts;     /* 1 .. 2^20 */
    int32_t max_passes;   /* 1 .. 2^20 per start */
    uint64_t seed;
} wa_seam_params;
typedef struct {
    int32_t m, M, n_starts, best_start, n_capped;
    int64_t cost_q;                                /* cost of the returned tour, quanta of 2^-20 */
    int64_t start0_cost_q_in, start0_cost_q_out;   /* start 0 as given / after its descent */
    int64_t passes_total;
} wa_seam_summary;
int wa_gtsp_seam_tour(wa_ctx *ctx, const double *dist, int32_t m, const wa_seam_params *params, const int32_t *order0, const uint8_t *dir0,
                 int32_t *order_out, uint8_t *dir_out, int64_t *start_cost_q_out, int32_t *start_passes_out, wa_seam_summary *sum);
int wa_gtsp_seam_tour_exact(wa_ctx *ctx, const double *dist, int32_t m, int32_t closed, int32_t *order_out, uint8_t *dir_out, int64_t *cost_q);

/* ---- seam tours under job rules: precedences between seams and one-way seams (DESIGN 4aa holds the full text) ----
 * Costs, closed, the dummy seam of an open tour, the state and the cost are rules 1 - 3 above.  Two more inputs: before[k] / after[k],
 * k < n_prec (0 .. 65 536; duplicates allowed): seam before[k] is welded earlier in the tour than seam after[k]; and fixed[s], m bytes
 * (NULL: all 0): 0 free, 1 the seam is entered at its even endpoint (d = 0), 2 at its odd endpoint (d = 1).
 *  7. Anchor.  A tour is read from its anchor seam: the dummy when the tour is open, seam 0 when it is closed.  The anchor stands at
 *     position 0 of every state and never leaves it.  (A caller who wants a home position makes it a degenerate seam 0.)
 *  8. Admissible state.  The anchor stands at position 0, pos(before[k]) < pos(after[k]) for every pair, every fixed seam has its d.
 *  9. Moves.  Rule 4's moves with rule 4's numbers, but i >= 1 (the one exception is Reverse(0, 0), which flips the anchor seam alone),
 *     and a move counts only if the state it produces is admissible.  A pass takes the smallest cost change among the admissible moves,
 *     the lowest number among equals, and applies it if it is negative; ends and max_passes as in rule 4.
 * 10. Starts.  Rule 5's draw, then a repair: the anchor goes first; then, step by step, the seam that stands earliest in the drawn order
 *     among the seams whose `before` seams have all been placed; the drawn d stays unless fixed forces the other.  Start 0 is order0 /
 *     dir0 as given: they must be admissible and a closed order0[0] must be 0.  A NULL order0 is the repair of the identity, a NULL dir0
 *     is 0 where a seam is free.
 * 11. wa_gtsp_seam_tour_rules_exact: rule 6's subset programme with the anchor first, M <= 16.  A subset carries a value only if it is
 *     closed under `before`, and an entry only where fixed permits it.  Closed: one table per permitted d of seam 0, the d = 0 table
 *     wins on equal cost; open: one table.  Backtracking takes the lowest endpoint at every step.
 * 12. wa_gtsp_seam_rules_check (host only: nothing runs on the device, and ctx may be NULL -- like every wa_gtsp_ call it takes the context
 *     first, here only so that wa_last_error can say what was refused): order / dir hold a tour of m seams as the calls return it; it is read from
 *     seam 0 when closed, from its first entry when open.  n_bad_prec_out counts the given pairs (a duplicate as often as it is given)
 *     whose `before` seam does not come first, n_bad_dir_out the fixed seams entered at the wrong end.
 * WA_ERR_ARG, before anything is written: everything the calls above refuse; n_prec outside 0 .. 65 536 or NULL before / after with
 * n_prec > 0; a seam index outside 0 .. m-1; before[k] == after[k]; a cycle; after[k] == 0 on a closed tour; a fixed byte above 2;
 * an order0 / dir0 that is not admissible.  wa_seam_rules_summary is wa_seam_summary, then the number of distinct pairs and of fixed
 * seams. */
typedef struct {
    int32_t m, M, n_starts, best_start, n_capped;
    int64_t cost_q;
    int64_t start0_cost_q_in, start0_cost_q_out;
    int64_t passes_total;
    int32_t n_prec, n_fixed;                       /* distinct pairs, seams with fixed != 0 */
} wa_seam_rules_summary;
int wa_gtsp_seam_tour_rules(wa_ctx *ctx, const double *dist, int32_t m, const wa_seam_params *params, const int32_t *before, const int32_t *after,
                            int32_t n_prec, const uint8_t *fixed, const int32_t *order0, const uint8_t *dir0, int32_t *order_out, uint8_t *dir_out,
                            int64_t *start_cost_q_out, int32_t *start_passes_out, wa_seam_rules_summary *sum);
int wa_gtsp_seam_tour_rules_exact(wa_ctx *ctx, const double *dist, int32_t m, int32_t closed, const int32_t *before, const int32_t *after, int32_t n_prec,
                                  const uint8_t *fixed, int32_t *order_out, uint8_t *dir_out, int64_t *cost_q);
int wa_gtsp_seam_rules_check(wa_ctx *ctx, int32_t m, int32_t closed, const int32_t *before, const int32_t *after, int32_t n_prec, const uint8_t *fixed,
                             const int32_t *order, const uint8_t *dir, int64_t *n_bad_prec_out, int64_t *n_bad_dir_out);

/* ---- torch axis along a trajectory: which way the torch body may point, sample by sample (not in the reference: Usr_SendToSimulation
 *      holds alpha, beta, gamma at constants, main.cpp:393-405) ----
 * t holds n samples, the torch TIP.  The call picks, for every sample, one of K given directions for the torch body so that the body
 * stays clear of the metal of g and the direction changes little from sample to sample: a shortest path over (sample, direction).
 * Everything the device sees is an integer, so the result is the same bytes whatever computes it.  "double" is IEEE float64, every
 * operation rounded on its own (no contraction); rint rounds ties to even; integer division is floor division, >> is arithmetic.
 * 1. Directions.  A direction points from the tip INTO the torch body.  A float triple (x, y, z) is quantised once, on the host:
 *    len = sqrt((x*x + y*y) + z*z) in double, q_c = (int32)rint((c / len) * 16384) per component; all three components must be finite
 *    and len > 0.  The device sees q only.  U(a, b) = ((a_x-b_x)^2 + (a_y-b_y)^2 + (a_z-b_z)^2) >> 10, at most 3 * 2^20: the turn measure.
 * 2. Tool.  n_beads beads (1 .. WA_TORCH_MAX_BEADS); bead j sits dist16[j] sixteenths of a voxel behind the tip (0 .. 65536) and must
 *    keep a squared clearance above r2[j] (0 .. 2^30, the voxel-index units of wa_grid_distance_field).  Its offset from the sample's
 *    voxel is, per axis, o_c = floor((q_c * dist16[j] + 2^17) / 2^18); the sample's voxel comes from the lookup of wa_traj_clearance
 *    (samples outside the coordinate range are clamped and counted in n_outside).  A bead whose voxel lies outside the grid passes:
 *    space outside the grid is no obstacle.  Otherwise, with v its voxel: the bead is BLOCKED iff d2[v] <= r2[j]; it is NEAR iff it is
 *    not blocked, near_add >= 0 and d2[v] <= r2[j] + near_add (near_add <= 2^30; negative: off).  A direction is blocked at a sample iff
 *    any bead is; near(i, k) = the number of near beads (of all beads, whether or not another one is blocked).  On a grid without
 *    obstacles d2 is WA_D2_NONE everywhere and nothing is blocked.
 * 3. Node cost.  N(i, k) = BLOCK * [blocked] + w_near * near(i, k) + w_want * U(q_k, qw_i), BLOCK = 2^36; qw_i = the quantised wish
 *    want[i]; the wish term is 0 when want is NULL or the triple is all zero.  Weights are 0 .. 1024.
 * 4. Legs.  off[0 .. n_legs] splits the n samples into independent legs: off[0] = 0, non-decreasing, off[n_legs] = n; empty legs are
 *    allowed, a leg holds at most 2^22 samples.  pin_first[l] / pin_last[l]: a direction index the leg must start / end with, or -1;
 *    a NULL array means all -1; the pins of an empty leg are ignored.
 * 5. Sequence.  Per leg with samples s .. e; every sum saturates at INF = 2^62 (finite sums stay below 2^61 by the bounds above).
 *    alpha_s(k) = N(s, k), or INF for k != pin_first when that is given.
 *    alpha_i(k) = N(i, k) + min over k' of (alpha_(i-1)(k') + w_turn * U(q_k', q_k) + BLOCK * [max_turn >= 0 and U(q_k', q_k) > max_turn]);
 *    back_i(k) = the lowest k' attaining the minimum.  The last state is pin_last if given, else the lowest k minimising alpha_e; the
 *    sequence follows back from there.  dir_out[i] = the direction index of sample i; leg_cost[l] = alpha_e(last state), 0 for an
 *    empty leg.  Every transition is finite, so an end pin is always reached finitely from the sample before; leg_cost is INF only
 *    for a leg of ONE sample whose two pins differ (pin_last wins).  There is always a full sequence: a sample where every direction
 *    is blocked shows up in the summary, not as an error.
 * 6. Summary.  n, n_outside; n_blocked_pairs = blocked (sample, direction) pairs; n_no_dir = samples where every direction is blocked;
 *    n_chosen_blocked = samples whose chosen direction is blocked, first_chosen_blocked the lowest of them (-1: none); n_chosen_near =
 *    samples whose chosen direction is not blocked and has near >= 1; n_over_turn = chosen transitions inside a leg with max_turn >= 0
 *    and U > max_turn; max_turn_taken = the largest U of a chosen transition (0 without one); cost = the sum of the leg costs below
 *    INF, itself saturating at INF.
 * 7. wa_traj_tool_axes.  dirs: K x 3 floats, 1 <= K <= WA_TORCH_MAX_DIRS; want: n x 3 floats or NULL; dir_out (int32 n), feas_out
 *    (uint8 n x K: feas_out[i * K + k] = 255 if direction k is blocked at sample i, else near(i, k)) and leg_cost (int64 n_legs) are on
 *    the host and may be NULL; sum may not.
 * 8. wa_traj_tool_check applies rule 2 to ONE given axis per sample (axes: n x 3 floats, quantised by rule 1): a caller who
 *    interpolates between planned key poses has the interpolated poses checked by the very device function the planner uses.
 *    blocked_out[i] = 0 / 1, near_out[i] = near of that axis (each uint8 n, host, may be NULL).  Its summary treats the given axis as the
 *    chosen one of a single direction: n, n_outside, n_blocked_pairs = n_no_dir = n_chosen_blocked, first_chosen_blocked,
 *    n_chosen_near are filled, the other fields are 0.
 *    (Axes at every controller TICK, interpolated and checked on the device: wa_traj_tick_axes, rules 24 - 26 at the end of this header.)
 * 9. Errors.  WA_ERR_ARG, before anything is written: a NULL required pointer (g, t, dirs / axes, tool, weights, off, sum), g and t from
 *    different contexts, K, n_beads, n_legs (< 0), a weight, dist16, r2 or near_add out of range, off that breaks rule 4, a pin outside
 *    -1 .. K-1, a direction or axis that is not finite or has zero length, a want entry or a coordinate of t that is not finite.
 *    WA_ERR_CAPACITY: a leg above 2^22 samples, n * K above 2^33 (wa_traj_tool_check: n above 2^33).
 * Same bytes on every call; everything runs on the context's stream; g and t are not modified.  The feasibility bytes and the back
 * pointers (n * K bytes each) live in blocks of the context's arena for the duration of the call.
 * (The C names say "tool", the Python wrappers torch_axes / torch_check: no declaration of this header may carry the name of the
 * tensor library, which tests/test_abi.py checks letter by letter.) */
#define WA_TORCH_MAX_DIRS 256
#define WA_TORCH_MAX_BEADS 64
#define WA_TORCH_INF ((int64_t)1 << 62)
typedef struct {
    int32_t n_beads;                       /* 1 .. WA_TORCH_MAX_BEADS */
    int32_t dist16[WA_TORCH_MAX_BEADS];    /* sixteenths of a voxel behind the tip, 0 .. 65536 */
    int32_t r2[WA_TORCH_MAX_BEADS];        /* squared clearance the bead must exceed, 0 .. 2^30 */
} wa_tool_beads;
typedef struct {
    int32_t w_near, w_want, w_turn;        /* 0 .. 1024 */
    int32_t near_add;                      /* rule 2; < 0: no bead is near */
    int32_t max_turn;                      /* rule 5; < 0: no turn limit */
} wa_tool_weights;
typedef struct {
    int64_t n, n_outside;
    int64_t n_blocked_pairs, n_no_dir;
    int64_t n_chosen_blocked, first_chosen_blocked, n_chosen_near;
    int64_t n_over_turn, max_turn_taken;
    int64_t cost;
} wa_tool_summary;
int wa_traj_tool_axes(const wa_grid *g, const wa_traj *t, const float *dirs, int32_t K, const wa_tool_beads *tool,
                       const wa_tool_weights *weights, const float *want, const int64_t *off, int32_t n_legs, const int32_t *pin_first,
                       const int32_t *pin_last, int32_t *dir_out, uint8_t *feas_out, int64_t *leg_cost, wa_tool_summary *sum);
int wa_traj_tool_check(const wa_grid *g, const wa_traj *t, const float *axes, const wa_tool_beads *tool, int32_t near_add,
                        uint8_t *blocked_out, uint8_t *near_out, wa_tool_summary *sum);

/* ---- torch-fit planning grids: rule 2 above for EVERY voxel of a grid, so that a planner can be told where the torch fits before it
 *      plans (wa_traj_tool_axes tells it afterwards).  The rules continue the numbering above; directions, q, the offsets
 *      o_c = floor((q_c * dist16[j] + 2^17) / 2^18) and wa_tool_beads are those of rules 1 and 2, near is not used.
 *      K = 1 .. WA_TORCH_MAX_DIRS directions, W = ceil(K / 64), n = nx * ny * nz, v = (x, y, z) a voxel of g, o(k, j) the offset of
 *      bead j under direction k.
 * 10. blocked(v, k) iff some bead j has v + o(k, j) inside the grid and d2[v + o(k, j)] <= r2[j].  A bead outside the grid passes; on a
 *     grid without obstacles nothing is blocked.  open(v, k) = v is free in g AND not blocked(v, k): an occupied voxel has no open
 *     direction, whatever the beads say.
 * 11. count[v] = the number of open directions, 0 .. K (uint16, raster order).  mask is word-plane-major: bit (k & 63) of
 *     mask[(k >> 6) * n + v] is open(v, k); the unused high bits of the last plane are 0.
 * 12. wa_reach_summary: n_free = free voxels of g; n_no_dir = free voxels with count 0; n_all_dirs = free voxels with count K;
 *     n_blocked_pairs = the sum over free voxels of K - count.
 * 13. wa_grid_tool_reach copies the masks (W * n uint64) and the counts (n uint16) to the host; either may be NULL, sum may not.  The
 *     mask planes are a block of the context's arena, taken only when mask_out is given.
 * 14. wa_grid_tool_fit builds a new planning grid like wa_grid_inflate (same dims, axis tables, precision and wall; its own buffers;
 *     n_free recounted; destroyed with wa_grid_destroy): v is free in it iff v is free in g AND count[v] >= min_dirs (1 .. K) -- except
 *     inside keep bubbles: for each keep id k (a free voxel of g), every voxel v with |v - k|^2 <= keep_r2 (integer index units,
 *     0 .. 2^30) keeps the state it has in g.  The counts never leave the device between the count and the new occupancy.  sum (of g,
 *     rule 12) may be NULL.  *out is written on success only.
 * 15. wa_grid_tool_penalties writes a penalty array for wa_grid_chamfer_weighted_*: n bytes on the host in raster order, 0 on occupied
 *     voxels, on free voxels the number of t with count[v] < thr[t].  0 <= n_thr <= WA_PEN_MAX (thr may be NULL when n_thr is 0),
 *     every threshold 0 .. 65535, in any order, repeats allowed.
 * 16. Errors.  WA_ERR_ARG, before anything is written: a NULL required pointer (g, dirs, tool, sum / out / pen_out, keep_ids with
 *     n_keep > 0, thr with n_thr > 0); K, n_beads, dist16, r2, min_dirs, n_thr, a threshold or keep_r2 out of range; a direction that is
 *     not finite or has zero length; a keep id outside the grid or on an occupied voxel; a negative n_keep.  WA_ERR_ALLOC when the
 *     device blocks do not fit.
 * Same bytes on every call; everything runs on the context's stream; g is not modified; the distance field is built on the first use,
 * as by wa_grid_inflate.  EVERY call recomputes the counts: nothing is cached with the grid, so a caller who wants the fit grid and
 * the penalties of one tool pays for the count twice. */
typedef struct {
    int64_t n_free, n_no_dir, n_all_dirs, n_blocked_pairs;
} wa_reach_summary;
int wa_grid_tool_reach(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, uint64_t *mask_out, uint16_t *count_out,
                       wa_reach_summary *sum);
int wa_grid_tool_fit(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t min_dirs, const int64_t *keep_ids,
                     int32_t n_keep, int32_t keep_r2, wa_grid **out, wa_reach_summary *sum);
int wa_grid_tool_penalties(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, const int32_t *thr, int32_t n_thr,
                           uint8_t *pen_out);

/* ---- exact pose paths: shortest lattice paths over the states (voxel, direction) with a turn limit, so that a planner knows BEFORE it
 *      plans whether a turn-limited SEQUENCE of directions exists along a path (a free voxel of wa_grid_tool_fit only promises one open
 *      direction per voxel).  The rules continue the numbering above; directions, q, U(a, b), wa_tool_beads, open(v, k),
 *      K = 1 .. WA_TORCH_MAX_DIRS and W = ceil(K / 64) are those of rules 1, 2, 10 and 11.  Integers only.
 * 17. States are the pairs (v, k) with open(v, k).  adj(k, k') holds iff max_turn < 0 or U(q_k, q_k') <= max_turn; it is symmetric and
 *     holds for k' = k.  max_turn is -1 or 0 .. 3 * 2^20.
 * 18. One step goes from (v, k) to (v', k'): v' is a 6-neighbour of v inside the grid, adj(k, k') and open(v', k') hold.  There is no
 *     turn in place: a path is a lattice path of distinct consecutive voxels with one direction index per node.
 * 19. The seed of a source s with pin p: every open direction of s when p = -1, otherwise the one state (s, p) if it is open.  An
 *     empty seed is not an error: nothing is reached, the source itself included.
 * 20. level(s; v, k) = the breadth-first level of the state from the seed, WA_HOPS_NONE (-1) where there is none.  hops(s; v) = the
 *     minimum over k of level(s; v, k); hops(s; t, pin) restricts that minimum to the pinned direction (pin = -1: no restriction).
 * 21. The path of a pair is defined, not only its length D = hops(start; end, end pin).  Its end state is the lowest k allowed by the end
 *     pin with level D.  Walking back from (p, k) at level L > 0, the predecessor voxel is the first neighbour in the order -x, +x, -y,
 *     +y, -z, +z that is inside the grid and has some k' with level L - 1 and adj(k', k); the predecessor direction is the lowest such k'
 *     of that voxel.  The path is returned start first: D + 1 voxel ids and D + 1 direction indices.
 * 22. wa_grid_pose_fields: hops_out[s * n + v] = hops(s; v); state_out (may be NULL) [(s * K + k) * n + v] = level(s; v, k).
 *     wa_grid_pose_matrix: hops_out[i * n_pts + j] = hops from point i, seeded with its pin, to point j restricted to ITS pin; with the same
 *     pins on both sides the matrix is symmetric.  wa_grid_pose_paths follows wa_grid_geodesic_paths: pair p owns the range
 *     [off[p], off[p + 1]) of ids_out AND of dir_out (int32); hops_out[p] = D or WA_HOPS_NONE, len_out[p] (may be NULL) = D + 1 (0 for no
 *     path); the counts reach the caller for every pair first, WA_ERR_CAPACITY is reported once every pair has its counts, only a pair's
 *     own D + 1 entries are written, and an unreachable pair is no error.  The pin arrays may be NULL (all -1).
 *     With max_turn < 0 and no pins, or with K = 1, hops equals wa_grid_geodesic_* on wa_grid_tool_fit(min_dirs = 1, no keep ids); on a
 *     grid without obstacles it equals wa_grid_geodesic_* on g.
 * 23. Errors.  WA_ERR_ARG, before anything is written: the errors of rule 16 for g, dirs, K and the tool; a NULL id, offset or output
 *     array other than those named optional; a negative count; decreasing offsets; max_turn out of range; a pin outside -1 .. K - 1;
 *     an id outside the grid or on an occupied voxel.  WA_ERR_ALLOC when the buffers of one source do not fit, WA_ERR_STATE past
 *     K * n_free + 1 levels.
 * Same bytes on every call; everything runs on the context's stream; g is not modified.  The masks are recomputed by every call, in a
 * block of the context's arena (rule 16).  A source costs 3 * W * 8 * n bytes of bitmaps and 4 * n bytes of hops, and 4 * K * n bytes
 * more where states are kept (_paths always, _fields with state_out); sources are searched in chunks as for wa_grid_geodesic_*. */
int wa_grid_pose_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *src_ids,
                        const int32_t *src_pin, int32_t n_src, int32_t *hops_out, int32_t *state_out);
int wa_grid_pose_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *point_ids,
                        const int32_t *point_pin, int32_t n_pts, int32_t *hops_out);
int wa_grid_pose_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn, const int64_t *start_ids,
                       const int64_t *end_ids, const int32_t *pin_start, const int32_t *pin_end, int32_t n_pairs, const int64_t *off,
                       int64_t *ids_out, int32_t *dir_out, int32_t *hops_out, int32_t *len_out);

/* ---- tool poses at controller ticks: smoothed axes, a turn-rate limit for the timing, one axis per tick (not in the reference) ----
 *      wa_traj_retime gives the tip position at every controller tick, wa_traj_tool_axes one of K directions per SAMPLE.  The three
 *      calls below join them: they spread the direction changes along the path, turn them into a per-sample speed limit for
 *      wa_traj_retime, and give the axis at every tick, checked against the metal by rule 2.  The rules continue the numbering above;
 *      q, U(a, b), wa_tool_beads and "blocked" are those of rules 1 and 2, Q = 2^30, ds_i, L_i and rule 6 those of the retime section.
 *      Integers and individually rounded doubles only: the same bytes whatever computes it.
 *      Axes travel between these calls as QUANTISED INTEGERS: q is int32, n x 3, rule 1's rint((c / len) * 16384) (api.quantise_axes);
 *      every |q_c| <= 16384 and no triple is all zero (WA_ERR_ARG otherwise).  Floats do not round-trip: quantising q / 16384 again by
 *      rule 1 can move a component by 1, because the length of a quantised triple is not exactly 16384.  Keep the integers.
 * 24. wa_traj_axes_smooth.  L_i as retime rule 1, GL = its exclusive prefix sum (n entries); a total of 2^61 or more is WA_ERR_ARG.
 *     h_q = (int64)rint(h * Q) with h finite, >= 0 and h_q <= 2^61; max_level is 0 .. 8.  Legs follow rule 4 (off[0 .. n_legs], n_legs >= 1, a
 *     leg of at most 2^22 samples, WA_ERR_CAPACITY above); a window never crosses a leg.  The candidate axis of sample i at level
 *     l < max_level: J = the samples j of i's leg with |GL_j - GL_i| <= (h_q >> l), a contiguous range; S = the sum of q_j over J per
 *     component (int64).  If S = (0, 0, 0) the candidate is q_i.  Otherwise, S_c converted exactly to double,
 *     len = sqrt((S_x*S_x + S_y*S_y) + S_z*S_z) and the candidate is (int32)rint((S_c / len) * 16384) per component.  At level max_level the
 *     candidate is q_i itself.  A candidate is blocked by rule 2 at sample i's voxel (near is not used).  level_out[i] = the lowest l in
 *     0 .. max_level whose candidate is not blocked, max_level if all are; q_out[i] = that level's candidate; blocked_out[i] = whether it
 *     is blocked.  A sample's result depends on the inputs only, never on another sample's output: no rounds, no order.  g and tool
 *     may both be NULL (one alone is WA_ERR_ARG): nothing is blocked, every level is 0, n_outside is 0.  Summary: n, n_outside,
 *     n_level[l] = samples with level l, n_blocked and first_blocked (-1: none) over blocked_out, n_zero_sum = samples whose chosen level
 *     had S = 0, max_turn_in / max_turn_out = the largest U between consecutive samples inside a leg before / after.  q_out (int32 n x 3),
 *     level_out and blocked_out (uint8 n) are on the host; the last two may be NULL.  n is 1 .. 2^31.
 * 25. wa_traj_axes_limits.  Legs play no part: the trajectory is one motion.  Per segment i: D_i = the sum over c of
 *     (q_i,c - q_(i+1),c)^2, an exact integer <= 3 * 2^30; psi_i = sqrt((double)D_i) / 16384, the CHORD of the two unit axes -- omega caps
 *     the rate of the chord, not of the angle: the chord understates the angle by 1.2 % at 30 degrees and by 11 % at 90.  If D_i > 0 and
 *     L_i > 0: m_i = (ds_i * omega) / psi_i.  If D_i > 0 and L_i = 0 no speed makes room for the turn: counted in n_jump, no limit from it.
 *     Per sample: lim_i = min(v_cap, m_(i-1), m_i, (double)v_limit_in[i]) over those that exist; f_i = the largest float <= lim_i
 *     (convert, one step down if the float is greater); if (double)f_i < v_floor then f_i = the smallest float >= v_floor, counted in
 *     n_floored.  v_limit_out (n floats, host) is ready to be passed to wa_traj_retime as v_limit.  WA_ERR_ARG: omega, v_cap or v_floor
 *     not finite or <= 0, v_floor > v_cap or beyond the floats, a v_limit_in entry not finite or <= 0 (v_limit_in may be NULL).
 *     Summary: n, n_turning (D_i > 0), n_jump, n_floored, n_limited ((double)f_i < v_cap), min_limit (the smallest f_i).
 *     Property: with v_limit_out among the limits of wa_traj_retime, every segment with D_i > 0, L_i > 0 and neither end floored takes
 *     T_i >= floor(psi_i / omega * Q * (1 - 2^-40)) - 1 quanta.  n is 1 .. 2^31.
 * 26. wa_traj_tick_axes.  time_q and w_q (n int64 each, host) are what wa_traj_retime returned for the same t, acc and dec; checked:
 *     time_q[0] = 0, non-decreasing, below 2^61; 0 <= w_q <= 2^61.  The tick set, and per tick the segment i and lambda, are exactly rule
 *     6 (lambda = 1 where the tick is p_(i+1) exactly, 0 where it is p_i exactly); the tick position is rule 6's, the bytes of
 *     ticks_out.  The axis: v_c = (double)q_i,c + ((double)q_(i+1),c - (double)q_i,c) * lambda; if v is all zero the axis is q_i, else v
 *     quantised by rule 1 to qt.  *axes_out (may be NULL) is an ordinary device-resident wa_traj of n_ticks points
 *     (float)(qt_c / 16384.0), exact in fp32, owned by the caller.  blocked_out (one byte per tick, host, may be NULL): rule 2 with qt at
 *     the voxel of the tick POSITION (the lookup of wa_traj_clearance on the fp32 position).  g and tool may both be NULL: no check.
 *     Summary: n_ticks, n_outside, n_blocked, first_blocked (-1: none), n_near = ticks not blocked with a near bead, max_tick_turn = the
 *     largest U between the axes of consecutive ticks (0 with one tick).  WA_ERR_ARG as rule 7 of the retime section for n, acc, dec,
 *     tick and the coordinates, as rule 9 for the tool and near_add.  More than 2^31 ticks: WA_ERR_CAPACITY, *axes_out = NULL and
 *     nothing else written.
 * Every WA_ERR_ARG is answered before anything is written.  Same bytes on every call; everything runs on the context's stream; g and
 * t are not modified.  The scans of rule 24 live in blocks of the context's arena for the duration of the call. */
typedef struct {
    int64_t n, n_outside;
    int64_t n_level[9];
    int64_t n_blocked, first_blocked, n_zero_sum;
    int64_t max_turn_in, max_turn_out;
} wa_axes_smooth_summary;
typedef struct {
    int64_t n, n_turning, n_jump, n_floored, n_limited;
    double min_limit;
} wa_axes_limits_summary;
typedef struct {
    int64_t n_ticks, n_outside, n_blocked, first_blocked, n_near, max_tick_turn;
} wa_tick_axes_summary;
int wa_traj_axes_smooth(const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, const int64_t *off, int32_t n_legs,
                        double h, int32_t max_level, int32_t *q_out, uint8_t *level_out, uint8_t *blocked_out, wa_axes_smooth_summary *sum);
int wa_traj_axes_limits(const wa_traj *t, const int32_t *q, double omega, double v_cap, double v_floor, const float *v_limit_in,
                        float *v_limit_out, wa_axes_limits_summary *sum);
int wa_traj_tick_axes(const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, int32_t near_add, double acc, double dec,
                      double tick, const int64_t *time_q, const int64_t *w_q, wa_traj **axes_out, uint8_t *blocked_out,
                      wa_tick_axes_summary *sum);

/* ---- pose-aware path shortening: any-angle shortcuts of (voxel, direction) paths that keep the torch clear (not in the reference) ----
 *      wa_grid_pose_paths returns a staircase of 6-neighbour hops with one open direction per node; wa_grid_path_shortcut straightens a
 *      staircase but knows the occupancy only.  This call shortens where the torch body stays clear along the WHOLE straight segment
 *      under a direction the plan already chose, keeps the turn limit at the waypoints and returns the direction held on every segment.
 *      The rules continue the numbering above; dirs, q, U(a, b), wa_tool_beads, open(v, k), adj(k, k') and max_turn are those of rules 1,
 *      2, 10 and 17, K = 1 .. WA_TORCH_MAX_DIRS.  The supercover is the one of wa_traj_clearance and wa_grid_path_shortcut: tied axes
 *      stepped together, the full product set at a tie, voxel a itself included.  Integers only, except the length.
 * 27. Input.  n_paths paths back to back as for wa_grid_path_shortcut: path p = the nodes off[p] .. off[p + 1] - 1 (n_paths + 1 offsets,
 *     off[0] = 0, non-decreasing, empty paths allowed), node i has voxel v_i = ids[i] and direction index k_i = ks[i] in 0 .. K - 1.  The
 *     paths need not come from wa_grid_pose_paths and are not checked for being pose paths.  For nodes a < m of one path:
 *     cover_open(a, m, k) holds iff open(w, k) for EVERY voxel w of the supercover between v_a and v_m (which includes that w is free);
 *     ok(a, m) holds iff adj(k_a, k_m) and (cover_open(a, m, k_a) or cover_open(a, m, k_m)).
 * 28. Greedy rule: that of wa_grid_path_shortcut with ok in place of visible.  Indices are relative to the path, L its node count, w_0 = 0.
 *     From an anchor a < L - 1, next(a) is the largest j in [a + 1, min(a + max_span, L - 1)] such that ok(a, m) holds for EVERY m in
 *     (a, j] (prefix form); if there is none, next(a) = a + 1.  Stop when L - 1 is reached: the first and last nodes are always kept.
 *     The hold of the segment a -> j = next(a): if ok(a, j) does not hold (only possible for the fallback j = a + 1) the hold is -1, and
 *     the hop carries whatever guarantee the input had -- for a path of wa_grid_pose_paths the lattice step of rule 18.  Otherwise the
 *     hold is k_a if cover_open(a, j, k_a): the torch travels with the anchor's direction and turns on arrival; else it is k_j: the
 *     torch turns on departure.  A segment with a hold >= 0 is HELD.
 *     Consequences.  Along a held segment one direction is open in every voxel that the straight line between the two voxel centres
 *     touches.  Every turn at a waypoint of a held segment is between adjacent directions, both open at the waypoint's voxel (k_a -> k_j
 *     at j, or k_a -> k_j at a: both voxels belong to the cover); up to two such turns meet at one waypoint, the arrival of one segment
 *     and the departure of the next.
 *     Identities.  (a) With a tool of one bead with dist16 = 0 and r2 = 0 and max_turn = -1, open(v, k) = v is free, so wp_idx, wp_count
 *     and length_out are the bytes of wa_grid_path_shortcut whatever ks holds.  (b) max_span = 1 makes every node a waypoint.  (c) With
 *     max_turn = 0 and pairwise distinct quantised directions a held segment joins two nodes of EQUAL direction.
 * 29. Outputs.  wp_idx[off[p] .. off[p] + wp_count[p]) = the waypoints of path p as indices INTO path p; hold_out (int32, may be NULL)
 *     uses the same ranges: entry t is the hold of the segment that leaves waypoint t, the last waypoint's entry is -1.  Later entries of
 *     both ranges stay untouched.  length_out (may be NULL) is exactly wa_grid_path_shortcut's float64 length of the waypoints.  Summary
 *     (required): n_paths, n_nodes = off[n_paths], n_waypoints = the sum of wp_count; the segments counted by their hold -- n_held_start
 *     (the hold is k_a, also when k_j equals it), n_held_end (the hold is k_j and differs from k_a), n_unheld (-1); max_hold_turn = the
 *     largest U(q_h, q_h') over the holds h, h' of two CONSECUTIVE segments of one path that are both held, 0 without such a pair.
 *     WA_ERR_ARG, before anything is written: the errors of rule 16 for g, dirs, K and the tool; max_turn outside -1 .. 3 * 2^20; a NULL
 *     ids, ks, off, wp_idx, wp_count or sum; n_paths < 0; max_span outside 1 .. 4096; off[0] != 0 or decreasing offsets; an id outside the
 *     grid; a ks entry outside 0 .. K - 1; a path of 2^31 nodes or more; more than 2^33 nodes.  WA_ERR_ALLOC when the device blocks do
 *     not fit.
 * Same bytes on every call; everything runs on the context's stream; g is not modified.  The masks are recomputed by every call, in a
 * block of the context's arena (W * 8 * n bytes, rule 16); nothing is cached with the grid. */
typedef struct {
    int64_t n_paths, n_nodes, n_waypoints;
    int64_t n_held_start, n_held_end, n_unheld;  /* segments by rule 28's hold */
    int64_t max_hold_turn;                       /* largest U between the holds of consecutive held segments of one path; 0 without one */
} wa_pose_shortcut_summary;
int wa_grid_pose_shortcut(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                          const int64_t *ids, const int32_t *ks, const int64_t *off, int32_t n_paths, int32_t max_span,
                          int64_t *wp_idx, int32_t *hold_out, int32_t *wp_count, double *length_out, wa_pose_shortcut_summary *sum);

/* ---- turn-cost pose paths: cheapest lattice paths over the states (voxel, direction) where a change of direction and a voxel near the
 *      metal cost something (not in the reference).  wa_grid_pose_paths minimises hops and takes the lowest direction index among equally
 *      short paths, so the torch swings for no reason; here a step is charged by how far it turns the torch and by the voxel it enters.
 *      The rules continue the numbering above.  States, open(v, k), adj(k, k'), steps, seeds, pins and keys are those of rules 17 - 19,
 *      unchanged; U(a, b) is rule 2's.  Integers only.
 * 30. The cost description wa_pose_costs.  hop_cost = 1 .. 8.  n_bands = B = 0 .. WA_POSE_MAX_BANDS (4).  turn_band[0 .. B - 1]: strictly
 *     ascending, each 0 .. 3 * 2^20.  turn_cost[0 .. B]: non-decreasing, each 0 .. WA_POSE_COST_MAX (15), turn_cost[0] = 0.  Entries of
 *     both arrays behind those are ignored.  pen: one byte per voxel, 0 .. WA_POSE_COST_MAX on free voxels, an occupied voxel's byte is
 *     ignored; NULL means all zero.  It is the array wa_grid_tool_penalties gives, or wa_grid_clearance_costs minus 1.
 * 31. Turn class: class(k, k') = the number of bands b with U(q_k, q_k') > turn_band[b]; it is symmetric and class(k, k) = 0.
 *     A step (v, k) -> (v', k') of rule 18 costs hop_cost + turn_cost[class(k, k')] + pen[v'] (at least 1).
 * 32. dist(s; v, k) = the cheapest total over the paths from the seed of s to the state, WA_DIST_NONE (-1) where there is none (the seed's
 *     states have 0: the start is not paid for).  cost(s; v) = the minimum over k of dist(s; v, k); cost(s; t, pin) restricts that
 *     minimum to the pinned direction (pin = -1: no restriction), as in rule 20.
 * 33. The path of a pair is defined, not only its cost D = cost(start; end, end pin).  Its end state is the lowest k allowed by the end
 *     pin with dist D.  Walking back from (v, k) at dist L > 0, the predecessor voxel is the first neighbour in the order -x, +x, -y,
 *     +y, -z, +z that is inside the grid and has some k' with adj(k', k) and dist(k') + hop_cost + turn_cost[class(k', k)] + pen[v] == L;
 *     the predecessor direction is the lowest such k' of that voxel.  The path is returned start first.
 * 34. wa_grid_pose_weighted_fields: cost_out[s * n + v] = cost(s; v); state_out (may be NULL) [(s * K + k) * n + v] = dist(s; v, k).
 *     wa_grid_pose_weighted_matrix: cost_out[i * n_pts + j] = the cost from point i, seeded with its pin, to point j restricted to ITS
 *     pin.  Without pen and with the same pins on both sides the matrix is symmetric; with pen and no pins
 *     d(i, j) - pen[j] == d(j, i) - pen[i].  wa_grid_pose_weighted_paths: as wa_grid_pose_paths, pair p owns the range
 *     [off[p], off[p + 1]) of ids_out and of dir_out; cost_out[p] = D or WA_DIST_NONE; len_out[p] (REQUIRED: the node count is not D + 1)
 *     = the nodes of the path, 0 for no path.  The counts reach the caller for every pair first, WA_ERR_CAPACITY is reported once every
 *     pair has its counts, only a pair's own len_out[p] entries are written, and an unreachable pair is no error.
 *     Identities.  With hop_cost = 1, no pen, and n_bands = 0 or every turn_cost 0, all three calls return the bytes of wa_grid_pose_*
 *     (len_out = D + 1).  Multiplying hop_cost, every turn_cost and every pen byte by one factor multiplies every distance by it and
 *     keeps every path.  Two descriptions with the same classes of equal cost (a band between two classes of one cost) give the same bytes.
 * 35. Errors.  Rule 23's apply (len_out is required here).  WA_ERR_ARG, before anything is written, also for: costs NULL; hop_cost,
 *     n_bands, a band or a turn cost out of range; bands not strictly ascending; turn costs decreasing; turn_cost[0] != 0; a pen byte
 *     above WA_POSE_COST_MAX on a free voxel.  WA_ERR_STATE past (hop_cost + max turn_cost + P) * (K * n_free - 1) + R + 1 levels (capped
 *     at 2^31 - 33), P and R as in rule 36.
 * 36. Memory.  The search is level-synchronous with the level the distance: R = hop_cost + max turn_cost + P + 1 settled sets per source,
 *     P = the largest pen byte present on a free voxel.  A source costs (R + 1) * W * 8 * n bytes of bitmaps, 4 * n bytes of costs, and
 *     4 * K * n bytes more where states are kept (_paths always, _fields with state_out): at 256^3, K = 64 and R = 12 about 1.7 GB per
 *     source without states.  Sources are searched in chunks as for wa_grid_geodesic_* (WA_GEO_CHUNK and the chunk rule unchanged).
 * Same bytes on every call; everything runs on the context's stream; g is not modified.  The masks, the step matrices (one K x W bit
 * matrix per distinct step weight) and the device copy of pen are rebuilt by every call; nothing is cached with the grid. */
#define WA_POSE_MAX_BANDS 4
#define WA_POSE_COST_MAX 15
typedef struct {
    int32_t hop_cost;                          /* 1 .. 8 */
    int32_t n_bands;                           /* B = 0 .. WA_POSE_MAX_BANDS */
    int32_t turn_band[WA_POSE_MAX_BANDS];      /* [0 .. B - 1], strictly ascending, 0 .. 3 * 2^20 */
    int32_t turn_cost[WA_POSE_MAX_BANDS + 1];  /* [0 .. B], non-decreasing, 0 .. WA_POSE_COST_MAX, [0] = 0 */
    const uint8_t *pen;                        /* n bytes (host), 0 .. WA_POSE_COST_MAX on free voxels; NULL: all zero */
} wa_pose_costs;
int wa_grid_pose_weighted_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                 const wa_pose_costs *costs, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *cost_out,
                                 int32_t *state_out);
int wa_grid_pose_weighted_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                 const wa_pose_costs *costs, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *cost_out);
int wa_grid_pose_weighted_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                                const wa_pose_costs *costs, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                                const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out,
                                int32_t *cost_out, int32_t *len_out);

/* ---- pose-aware trajectory fit: refine the spline until a planned direction stays open along it (not in the reference) ----
 *      wa_grid_pose_shortcut returns waypoints and, per segment between them, the direction (hold) that is open in every voxel the
 *      straight segment touches.  wa_grid_fit_trajectory turns waypoints into the B-spline the robot drives but checks the sampled curve
 *      against the occupancy only: the curve cuts corners inside the hull of its control points, through voxels where no planned
 *      direction fits the torch body.  This call is the loop of wa_grid_fit_trajectory with "a planned direction is open along this
 *      piece of curve" in place of "this piece of curve is free", and it returns the direction it found for every segment.
 *      The rules continue the numbering above; dirs, q, U(a, b), wa_tool_beads and open(v, k) are those of rules 1, 2 and 10, K = 1 ..
 *      WA_TORCH_MAX_DIRS; "step n" is step n of wa_grid_fit_trajectory.  Integers only, except what the fit computes.
 * 37. Input.  g, poly, degree, spacing, max_level and n_samples are wa_grid_fit_trajectory's, with the same rules; dirs, K and tool are
 *     wa_grid_pose_shortcut's, with the same rules.  leg_hold: n - 1 int32 (host), one per leg of poly, each -1 or 0 .. K - 1: what rule
 *     29's hold_out gives for the segments between waypoints; paths stitched end to start simply concatenate their holds.
 *     Definition.  Steps 1 - 3, 5 and 6 of wa_grid_fit_trajectory, unchanged.  Step 4 samples the same way and looks the samples' voxels
 *     up as wa_traj_clearance does; it then tests each segment i (samples i and i + 1):
 *     Candidates.  Take the knot span step 5 would use for u_i, then the one for u_(i+1) (the same _findSpan after the same clamp; a
 *     sample is skipped under the conditions step 5 skips it: _findSpan refuses, span - D < 0 or span >= the number of control points).
 *     For each span take the control points span - D .. span in ascending order, and of each the hold of its owner leg (step 2's
 *     owner).  Drop -1; keep the first occurrence of each value.  That leaves at most 2 (D + 1) = 8 candidates, in a defined order.
 *     With at least one candidate, the segment's direction is the FIRST candidate c with open(w, c) for EVERY voxel w of the supercover
 *     between the two samples' voxels (the supercover of wa_traj_clearance: tied axes stepped together, the full product set at a tie,
 *     voxel a itself included).  If no candidate qualifies the segment is BLOCKED and its direction is -1.
 *     Without a candidate (every owner unheld) the segment is blocked iff wa_traj_clearance would report a hit there; its direction
 *     is -1, and it carries whatever guarantee the input had, as rule 28 says of an unheld hop.
 *     Loop.  Blocked segments take the place of hit segments in steps 4 - 6: the loop ends when no segment is blocked, when no level
 *     rose, or after round 32.
 * 38. Outputs.  *spline_out, *samples_out (may be NULL) and leg_level_out (may be NULL) as wa_grid_fit_trajectory returns them.
 *     seg_dir_out (n_samples - 1 int32, host, may be NULL): the direction of every segment of the last round, -1 where it has none.
 *     blocked_out (n_samples - 1 bytes, host, may be NULL): 1 where that segment is blocked.  Summary (required): rounds,
 *     max_level_used, n_legs, n_legs_at_cap, n_cps as in wa_fit_summary with "blamed" meaning blamed for a blocked segment;
 *     n_blocked_first = the blocked segments of round 1; final = the OCCUPANCY clearance summary of the final samples, exactly what
 *     wa_traj_clearance reports for them; n_blocked and first_blocked (-1 without one) of the last round; n_no_candidate = its segments
 *     without a candidate; n_dir_changes = the pairs of consecutive segments whose directions are both >= 0 and differ; max_dir_turn =
 *     the largest U(q_c, q_c') over such pairs, 0 without one.  As for the fit, n_blocked == 0 is not promised: rounds == 32 or
 *     n_legs_at_cap > 0 with n_blocked > 0 tell the caller so.
 *     Identities.  (a) With a tool of one bead with dist16 = 0 and r2 = 0 and every hold >= 0, open(v, k) = v is free, so the spline,
 *     the samples, the levels, rounds, n_cps, n_legs_at_cap, n_blocked_first (= n_hit_first) and final are the bytes of
 *     wa_grid_fit_trajectory.  (b) The same holds with every hold -1, whatever the tool.  (c) A segment that is not blocked and has a
 *     direction c >= 0 has c open on its whole cover, so every voxel of the cover is free.
 * 39. Errors.  WA_ERR_ARG, before anything is written: every argument error of wa_grid_fit_trajectory (NULL g / poly / sum /
 *     spline_out, different contexts, n < 2, degree, spacing, max_level, n_samples, a coordinate that is not finite, more than 2^24
 *     control points); the errors of rule 16 for dirs, K and the tool; a NULL leg_hold; a hold outside -1 .. K - 1.  WA_ERR_ALLOC when
 *     the masks or the device buffers do not fit.
 * Same bytes on every call; everything runs on the context's stream; g is not modified.  The masks are recomputed by every call, once,
 * before round 1, in a block of the context's arena (W * 8 * n bytes, rule 16); nothing is cached with the grid. */
typedef struct {
    int32_t rounds;          /* fits made (>= 1) */
    int32_t max_level_used;  /* the highest level of any leg */
    int64_t n_legs;          /* n - 1 */
    int64_t n_legs_at_cap;   /* legs at max_level that were still blamed in the last round */
    int64_t n_cps;           /* control points of the final spline */
    int64_t n_blocked_first; /* blocked segments of round 1: the unrefined fit on the same control spacing */
    wa_clearance_summary final; /* of the final samples against g's occupancy */
    int64_t n_blocked;       /* blocked segments of the last round: 0 is the success case */
    int64_t first_blocked;   /* the first of them, -1 without one */
    int64_t n_no_candidate;  /* segments of the last round whose owner legs are all unheld */
    int64_t n_dir_changes;   /* consecutive segments with directions >= 0 that differ */
    int64_t max_dir_turn;    /* largest U over those pairs; 0 without one */
} wa_pose_fit_summary;
int wa_grid_pose_fit_trajectory(const wa_grid *g, const wa_traj *poly, int32_t degree, float spacing, int32_t max_level, int64_t n_samples,
                                const float *dirs, int32_t K, const wa_tool_beads *tool, const int32_t *leg_hold, int32_t *leg_level_out,
                                wa_bspline **spline_out, wa_traj **samples_out, int32_t *seg_dir_out, uint8_t *blocked_out,
                                wa_pose_fit_summary *sum);

/* ---- weld passes in the timed trajectory: stops, dwells and tick tags (not in the reference) ----
 *      wa_traj_retime knows one motion, rest to rest.  A job that welds has to stop at a seam's start to strike the arc, wait, weld at
 *      weld speed, stop for the crater fill and travel on; and a torch that must re-orient between a travel leg and a seam needs a
 *      place to do it (rule 25's n_jump).  A STOP is a segment without length (L_i = 0) that has a duration.  The three calls below take
 *      stops into the timing, turn the torch in place while one lasts, tag every tick with what the caller put on its segment, and size
 *      a dwell from a turn rate.  The rules continue the retime section (its rules 1 - 7 are meant by "retime rule k") and rules
 *      24 - 26; Q, ds_i, L_i, q, U, D_i and psi_i are theirs.  Integers and individually rounded doubles only.
 * 40. wa_traj_retime_stops.  dwell: n - 1 doubles on the host, or NULL.  dwell[i] < 0: segment i is an ordinary segment.  dwell[i] >= 0:
 *     segment i is a stop of that many seconds (0 is legal: come to rest, then go); dq_i = (int64)rint(dwell[i] * Q).  WA_ERR_ARG before
 *     anything is written: an entry that is not finite, dq_i >= 2^61, a stop on a segment with L_i > 0, a NULL stops.  Retime rule 2
 *     gains one line: both samples of a stop get a kind-0 cap of 0 (kind 0 is the lowest number, so it is the kind reported, and
 *     n_bound[0] counts these samples).  Retime rules 3 and 4 apply as they stand: a cap of 0 resets the prefix and the suffix minimum, so
 *     the profile on either side of a stop is the rest-to-rest profile of that piece alone.  Retime rule 5 (a) becomes: L_i = 0:
 *     T_i = dq_i on a stop, else 0; the sum of T stays below 2^61.  Retime rule 6 is unchanged, word for word: i is the LARGEST index
 *     with time_q[i] <= tau, so a tick inside a dwell finds the stop and is p_i by the L_i = 0 clause.  Errors as retime rule 7.
 *     wa_stops_summary: n_stops = entries >= 0, n_stop_samples = samples at either end of a stop (one between two stops counts once),
 *     dwell_q = the sum of dq.  With dwell == NULL every output is the bytes of wa_traj_retime and *stops is all zero.
 * 41. wa_traj_tick_axes_stops.  Rule 26 with two additions.  (a) Dwell: a located segment i with L_i = 0, time_q[i+1] > time_q[i] and
 *     tau < time_q[i+1] -- this is how the call recognises a dwell; it takes no dwell array.  The position is p_i (retime rule 6); the
 *     axis is rule 26's formula, all-zero case included, with lambda = (double)(tau - time_q[i]) / (double)(time_q[i+1] - time_q[i]) (each
 *     conversion rounded to nearest even, one division) clamped into [0, 1]: the torch turns in place, linear in time; the bead check
 *     runs at the voxel of p_i with that axis.  (b) Tags: seg_tag (n - 1 bytes, host, may be NULL) carries whatever the caller put on
 *     a segment, arc on or off and a seam number for instance; tag_out[k] = seg_tag[i] for the segment i that retime rule 6 located for
 *     tick k, the final tick that is p_(i+1) exactly included.  tag_out (n_ticks bytes, host) may be NULL and must be with seg_tag NULL.
 *     wa_tick_stops_summary: n_dwell_ticks = ticks located in a dwell; n_tagged = ticks whose tag is not 0 (0 without seg_tag);
 *     max_dwell_turn = the largest U between the axes of tick k - 1 and tick k over the ticks k > 0 located in a dwell.  Without a
 *     segment of no length and positive duration *axes_out, blocked_out and *sum are the bytes of wa_traj_tick_axes.  Errors as rule
 *     26, and WA_ERR_ARG for a NULL stops.
 * 42. wa_traj_axes_dwells gives the dwell a turn needs.  Per segment i, with D_i, psi_i and L_i exactly as in rule 25 and
 *     given = dwell_in ? dwell_in[i] : -1:  L_i > 0: given must be < 0 (WA_ERR_ARG otherwise), dwell_out[i] = -1.  L_i = 0 and D_i = 0:
 *     dwell_out[i] = given if given >= 0, else -1.  L_i = 0 and D_i > 0 (rule 25's jump): need = psi_i / omega (one division);
 *     dwell_out[i] = need if given < need, else given.  WA_ERR_ARG as rule 25 for omega, the axes and the coordinates, and for a
 *     dwell_in entry that is not finite.  Summary: n, n_jump, n_stops (dwell_out[i] >= 0), n_raised (jumps with given < need), max_need
 *     (the largest need, 0 without a jump).  dwell_out (n - 1 doubles, host) is ready to be passed to wa_traj_retime_stops as dwell.
 *     Property: there every jump segment takes T_i >= floor(psi_i / omega * Q) quanta.  As in rule 25 omega bounds the CHORD of the two
 *     axes: in a wide turn the interpolated axis of rule 41 moves faster in the middle of the dwell than at its ends; max_dwell_turn
 *     shows by how much, and a caller who minds inserts intermediate samples (more, smaller turns).  n is 1 .. 2^31.
 * Every WA_ERR_ARG is answered before anything is written.  Same bytes on every call; everything runs on the context's stream; g and
 * t are not modified.  Not covered: stops on segments that have a length, angular acceleration, slerp.  (A jerk limit:
 * wa_traj_retime_jerk, rules 48 - 55 at the end of this header.) */
typedef struct {
    int64_t n_stops, n_stop_samples, dwell_q;
} wa_stops_summary;
typedef struct {
    int64_t n_dwell_ticks, n_tagged, max_dwell_turn;
} wa_tick_stops_summary;
typedef struct {
    int64_t n, n_jump, n_stops, n_raised;
    double max_need;
} wa_axes_dwells_summary;
int wa_traj_retime_stops(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit,
                         const double *dwell /* n-1, host, may be NULL */, double tick,
                         int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                         wa_retime_summary *sum, wa_stops_summary *stops);
int wa_traj_tick_axes_stops(const wa_grid *g, const wa_traj *t, const int32_t *q, const wa_tool_beads *tool, int32_t near_add,
                            double acc, double dec, double tick, const int64_t *time_q, const int64_t *w_q,
                            const uint8_t *seg_tag /* n-1, host, may be NULL */,
                            wa_traj **axes_out, uint8_t *blocked_out, uint8_t *tag_out /* n_ticks, host, may be NULL */,
                            wa_tick_axes_summary *sum, wa_tick_stops_summary *stops);
int wa_traj_axes_dwells(const wa_traj *t, const int32_t *q, double omega, const double *dwell_in /* n-1 or NULL */,
                        double *dwell_out /* n-1, host */, wa_axes_dwells_summary *sum);

/* ---- diagonal pose paths: 26-neighbour moves over the states (voxel, direction) (not in the reference) ----
 *      wa_grid_pose_* and wa_grid_pose_weighted_* move along the six axes only, so a path for which a sequence of open directions is
 *      known to exist is a Manhattan staircase; wa_grid_chamfer_* moves diagonally but knows nothing of the torch.  Here the states and
 *      the face steps are those of the turn-cost pose paths, and a diagonal move is added that keeps the direction.  The rules continue
 *      the numbering of the torch section.  States, open(v, k), adj(k, k'), seeds, pins and keys are those of rules 17 - 19, unchanged;
 *      the turn classes are rule 31's; U(a, b) is rule 2's.  Integers only.
 * 43. The cost description wa_pose_diag_costs.  step[0 .. 2]: the face, edge and corner move, each 1 .. 16.  n_bands, turn_band,
 *     turn_cost and pen exactly as in rule 30.
 *     A move changes each coordinate by -1, 0 or +1; its class c = 1 .. 3 is the number of coordinates that change.
 *     c = 1: the step (v, k) -> (v', k') of rule 18 (adj(k, k') and open(v', k')); it costs step[0] + turn_cost[class(k, k')] + pen[v'].
 *     c = 2 or 3: (v, k) -> (v', k), the SAME direction; it exists iff all 2^c voxels of the box that v and v' span are inside the grid
 *     and have k open (the box rule of wa_grid_chamfer_*, on open(., k) in place of free); it costs step[c - 1] + pen[v'].
 *     The torch does not turn during a diagonal move, nor in place.  The rule is symmetric: the reverse of a move is a move.
 * 44. dist(s; v, k), cost(s; v), the pinned minimum cost(s; t, pin), WA_DIST_NONE and the end state of a pair are rules 32 and 33's with
 *     the moves of rule 43.  Walking back from (v, k) at dist L > 0 the predecessors are tried in this order: first the six faces in
 *     the order -x, +x, -y, +y, -z, +z, of the first such voxel inside the grid that has some k' with adj(k', k) and
 *     dist(k') + step[0] + turn_cost[class(k', k)] + pen[v] == L the lowest such k' (rule 33); then the 12 edge offsets, then the 8
 *     corner offsets, each group sorted by (dz, dy, dx) ascending (the order of wa_grid_chamfer_paths): the first offset o for which the
 *     move (v + o, k) -> (v, k) exists and dist(s; v + o, k) == L - step[c - 1] - pen[v].  The path is returned start first.
 * 45. wa_grid_pose_diag_fields, _matrix and _paths take the arguments of wa_grid_pose_weighted_fields, _matrix and _paths with a
 *     wa_pose_diag_costs, and return what rule 34 says with these distances and paths (len_out REQUIRED, the capacity protocol unchanged).
 *     Identities.  (1) With step = {h, 2h, 3h}, h = 1 .. 5, and no pen, all three calls return the bytes of wa_grid_pose_weighted_* with
 *     hop_cost = h and the same bands and turn costs: a diagonal exists only where its face detour with the direction kept exists at the
 *     same price, and faces are asked first; with h = 1 and zero turn costs these are the bytes of wa_grid_pose_*.  (2) With K = 1 the
 *     bytes are those of wa_grid_chamfer_weighted_* with the same step and pen on the grid wa_grid_tool_fit gives for min_dirs = 1 and
 *     no keep ids, every direction index 0.  (3) With max_turn = 0, pairwise distinct q and no pins, dist(s; ., k) is the
 *     wa_grid_chamfer_weighted_fields distance from s on the grid whose free voxels are {v : open(v, k)}, all WA_DIST_NONE where
 *     open(s, k) does not hold.  (4) Multiplying every step, turn cost and pen byte by one factor multiplies every distance by it and
 *     keeps every path.  (5) Without pen and with the same pins on both sides the matrix is symmetric; with pen and no pins
 *     d(i, j) - pen[j] == d(j, i) - pen[i].
 * 46. Errors.  Rules 23 and 35 apply, with a step[i] outside 1 .. 16 in the place of hop_cost.  WA_ERR_STATE past
 *     (R - 1) * (K * n_free - 1) + R + 1 levels (capped at 2^31 - 33), R as in rule 47.
 * 47. Memory.  R = max(step[0] + max turn_cost, step[1], step[2]) + P + 1 settled sets per source, P = the largest pen byte present on a
 *     free voxel; a source costs (R + 1) * W * 8 * n bytes of bitmaps plus the fields of rule 36; chunks as in rule 36.
 * Same bytes on every call; everything runs on the context's stream; g is not modified.  The masks, the step matrices and the device
 * copy of pen are rebuilt by every call; nothing is cached with the grid.  Not covered: turns during a diagonal move, turns in place,
 * per-edge costs. */
typedef struct {
    int32_t step[3];                           /* face, edge, corner move: each 1 .. 16 */
    int32_t n_bands;                           /* as wa_pose_costs */
    int32_t turn_band[WA_POSE_MAX_BANDS];
    int32_t turn_cost[WA_POSE_MAX_BANDS + 1];
    const uint8_t *pen;                        /* as wa_pose_costs: 0 .. WA_POSE_COST_MAX on free voxels, NULL = zero */
} wa_pose_diag_costs;
int wa_grid_pose_diag_fields(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                             const wa_pose_diag_costs *costs, const int64_t *src_ids, const int32_t *src_pin, int32_t n_src, int32_t *cost_out,
                             int32_t *state_out);
int wa_grid_pose_diag_matrix(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                             const wa_pose_diag_costs *costs, const int64_t *point_ids, const int32_t *point_pin, int32_t n_pts, int32_t *cost_out);
int wa_grid_pose_diag_paths(const wa_grid *g, const float *dirs, int32_t K, const wa_tool_beads *tool, int32_t max_turn,
                            const wa_pose_diag_costs *costs, const int64_t *start_ids, const int64_t *end_ids, const int32_t *pin_start,
                            const int32_t *pin_end, int32_t n_pairs, const int64_t *off, int64_t *ids_out, int32_t *dir_out,
                            int32_t *cost_out, int32_t *len_out);

/* ---- jerk-limited controller ticks: a moving average along the arc length (not in the reference) ----
 *      The profile of wa_traj_retime / wa_traj_retime_stops is bang-bang: where a ramp meets a cap the acceleration jumps by up to
 *      acc + dec within one tick.  wa_traj_retime_jerk averages the last W ticks, not in x, y and z but in the ARC LENGTH, so the torch
 *      stays on the polyline that wa_traj_clearance and the fit stages proved clear, and the third difference of the arc length is
 *      bounded by 2 / W of the second difference the unfiltered ticks have.  An average carries speed into slow zones and eats the
 *      first W - 1 ticks of a dwell: the caps are lowered over the distance a window can span before the profile is computed, and the
 *      dwells are extended.  The rules continue the numbering above; Q = 2^30, tick_q, ds_i, L_i, A_i, D_i, the caps and kinds are those
 *      of the retime section ("retime rule k"), stops and dq_i those of rule 40.  GL = the exclusive prefix sum of L (n entries),
 *      length_q = GL_(n-1).  Integers and individually rounded doubles only.
 * 48. Window and reach.  window = W, 1 .. 2^20 ticks.  step_q = (int64)floor((v_max * tick) * Q) + 1, R_q = (W - 1) * step_q: the farthest the
 *     W ticks of one window can lie apart.  WA_ERR_ARG before anything is written: W out of range, R_q >= 2^61, (W - 1) * tick_q >= 2^61, a
 *     dq_i + (W - 1) * tick_q >= 2^61, W * length_q >= 2^62, tag_out without seg_tag, a NULL stops or jerk, and everything retime rule 7 and
 *     rule 40 refuse.
 * 49. Lowered caps.  For EVERY sample, end points and stop samples included, cap13_j = retime rule 2's minimum over the kinds 1 - 3 only,
 *     with its kind; C13_j its quanta by retime rule 2's floor.  The window of sample j is every sample m with
 *     GL_max(j-1, 0) - R_q <= GL_m <= GL_min(j+1, n-1) + R_q.  C'_j = the minimum of C13 over the window, its kind the lowest-numbered kind
 *     among the window's samples that attain it.  With R_q = 0 nothing is lowered: C' = C13.  Retime rule 2's kind 0 is then applied as
 *     ever: samples 0 and n-1 and both samples of every stop get cap 0.  bound_out gains bit 6: C'_j < C13_j, the cap was lowered.
 *     (The neighbours j-1 and j+1 belong to the interval because a filtered tick on segment i averages speeds taken on every segment
 *     that meets [GL_i - R_q, GL_(i+1) + R_q], the speed on a segment is bounded by the caps at both of its ends, and with this window at
 *     least one of C_i and C_(i+1) lies in the window of each of those ends.  [GL_j - R_q, GL_j + R_q] alone is not enough where samples
 *     lie farther apart than R_q.)
 * 50. Extended dwells.  On a stop dq'_i = dq_i + (W - 1) * tick_q.  stops->dwell_q reports the caller's own sum.
 * 51. The underlying profile.  Retime rules 3 - 5 and rule 40 on (C', dq') give B, bound, T and time_q: what time_q_out, w_q_out and
 *     bound_out return and *sum describes (sum->n_ticks = n_u of rule 52).  With W = 1 they are the bytes of wa_traj_retime_stops.
 * 52. Unfiltered arc lengths.  n_u = retime rule 6's tick count on that profile; for k = 0 .. n_u - 1 tau_k = min(k * tick_q, duration), i
 *     and lambda retime rule 6's for tau_k, U_k = GL_i + x with x = L_i if the tick is p_(i+1) exactly, 0 if L_i = 0, else
 *     (int64)rint(lambda * (double)L_i).  U_k = 0 for k < 0 and length_q for k >= n_u.
 * 53. The filter.  n_ticks = n_u + W - 1; S_k = floor((U_k + U_(k-1) + ... + U_(k-W+1)) / W) for k = 0 .. n_ticks - 1; s_q_out[k] = S_k (the
 *     last one is length_q).  More than 2^31 output ticks: WA_ERR_CAPACITY as in retime rule 7, with the summaries and the per-sample
 *     outputs filled, the tick fields of *jerk (max_d1 .. n_back) 0 and *ticks_out = NULL.
 * 54. Where a tick lies.  (a) Rest tick: if some stop segment i has GL_i = S_k, the tick takes the lowest-numbered such stop, sits at p_i
 *     and carries seg_tag[i]: stops in a row act as one stop with the sum of their dwells and the first one's tag.  (b) Otherwise
 *     i = the largest index in 0 .. n-2 with GL_i <= S_k; if S_k >= GL_(i+1) the tick is p_(i+1); else if L_i = 0 it is p_i; else
 *     lambda = (double)(S_k - GL_i) / (double)L_i and the position retime rule 6's per-axis expression.  tag_out[k] = seg_tag[i].
 * 55. wa_jerk_summary.  window, reach_q = R_q; n_lowered = samples with bit 6; n_in = n_u, n_ticks; max_d1, max_d2, max_d3 = the largest
 *     absolute first, second and third difference of S (quanta per tick, tick^2, tick^3); in_max_d2 = the largest absolute second
 *     difference of U over k = -W .. n_u + W; n_rest_ticks; n_short_rests = groups of stops sharing one GL whose rest ticks number
 *     fewer than floor(sum of their dq / tick_q); n_back = steps with S_(k+1) < S_k.  Property: max_d3 <= 2 * in_max_d2 / W + 4.
 * wa_traj_jerk_window: W = max(1, ceil((2 * max(acc, dec)) / (jerk * tick))), the window that bounds the jerk along the path by `jerk`;
 * WA_ERR_ARG for an argument that is not finite and > 0, a NULL window_out, a W above 2^20.  Host only; t may be NULL and is not read: like
 * every wa_traj_ call it takes the trajectory first, whose context receives the error text.
 * time_q_out, w_q_out, bound_out (n entries, host), ticks_out (a device-resident wa_traj of the filtered positions, owned by the
 * caller), s_q_out (int64 per output tick, host), tag_out (one byte per output tick, host), dwell, v_limit, seg_tag (n - 1 bytes, host)
 * and g may be NULL; s_q_out and tag_out hold jerk->n_ticks entries, which a call without them reports.  Same bytes on every call; everything runs on the context's stream; g and t are not modified.  The range minima of
 * rule 49 take 8 * n bytes per power of two in the widest window; WA_ERR_ALLOC where that cannot be had.  Not covered: a reach
 * tighter than rule 48's, cascaded windows (a bound on the snap), per-stop tags for stops in a row.  (Torch axes at the filtered ticks:
 * wa_traj_retime_jerk_axes, rules 56 - 60 below.) */
typedef struct {
    int64_t window, reach_q, n_lowered, n_in, n_ticks;
    int64_t max_d1, max_d2, max_d3, in_max_d2;
    int64_t n_rest_ticks, n_short_rests, n_back;
} wa_jerk_summary;
int wa_traj_retime_jerk(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit,
                        const double *dwell /* n-1, host, may be NULL */, double tick, int32_t window,
                        const uint8_t *seg_tag /* n-1, host, may be NULL */,
                        int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                        int64_t *s_q_out /* n_ticks, host, may be NULL */, uint8_t *tag_out /* n_ticks, host, may be NULL */,
                        wa_retime_summary *sum, wa_stops_summary *stops, wa_jerk_summary *jerk);
int wa_traj_jerk_window(const wa_traj *t /* may be NULL */, double acc, double dec, double jerk, double tick, int32_t *window_out);

/* ---- torch axes at jerk-limited ticks: poses for the filtered trajectory (not in the reference) ----
 *      wa_traj_tick_axes and wa_traj_tick_axes_stops locate a tick by TIME (retime rule 6); the ticks of wa_traj_retime_jerk are a moving
 *      average along the ARC LENGTH: they lie at other places, under other tick numbers, and there are W - 1 more of them.
 *      wa_traj_retime_jerk_axes is wa_traj_retime_jerk with one checked torch axis per filtered tick; S of rule 53 never leaves the
 *      device.  The rules continue the numbering above; q, U(a, b), wa_tool_beads and "blocked" are those of rules 1 and 2, the axes
 *      travel as quantised integers as in rule 24's preamble, GL, S_k and rule 54 are those of the section above.
 * 56. Every output wa_traj_retime_jerk has is returned with that call's bytes, *ticks_out included, and everything it refuses is
 *     refused.  q (int32, n x 3, host): every |q_c| <= 16384 and no triple all zero; tool and near_add as rule 9; g and tool may both be
 *     NULL (no check: nothing is blocked, n_outside is 0), one alone is WA_ERR_ARG; a NULL q or a NULL axes summary is WA_ERR_ARG.  g
 *     serves both the caps of retime rule 2 and the check of rule 59.  Every WA_ERR_ARG is answered before anything is written.  More
 *     than 2^31 output ticks: WA_ERR_CAPACITY as in rule 53, and *axes_out = NULL, blocked_out untouched, *axes all zero.
 * 57. Moving tick (rule 54 (b) gave segment i).  lambda = 1 where the tick is p_(i+1) exactly, 0 where L_i = 0, else rule 54's
 *     (double)(S_k - GL_i) / (double)L_i.  The axis is rule 26's expression: v_c = (double)q_i,c + ((double)q_(i+1),c - (double)q_i,c) * lambda;
 *     if v is all zero the axis is q_i, else v quantised by rule 1 to qt.  The axis belongs to the POSITION the tick has on the
 *     polyline: the set of (position, axis) pairs is the one rule 26 visits, only the pace along it changes.
 * 58. Rest tick (rule 54 (a) gave the head stop f).  a = the lowest and e = the highest sample index with GL = GL_f (e <= n - 1): the
 *     whole run of coincident samples turns as one, whatever un-stopped segments without length it holds, so the moving tick in front
 *     of the rest approaches q_a and the one behind it leaves from q_e.  first_f = the lowest tick index that is a rest tick of f,
 *     R_f = the number of rest ticks of f -- both by counting, not by assuming that S never falls (n_back exists because that is not
 *     proved).  lambda = (double)(k - first_f) / (double)R_f clamped into [0, 1]; the axis is rule 57's expression between q_a and q_e, q_a
 *     where v is all zero.  The position stays rule 54's p_f.  The torch turns in place, linear in the tick number, over exactly the
 *     ticks during which the filtered position rests; rule 50's extension gives a stop of dq at least floor(dq / tick_q) of them unless
 *     n_short_rests says otherwise.
 * 59. Check.  blocked_out[k] (one byte per tick, 0 or 1, host, may be NULL) = rule 2 with qt at the voxel of the tick's fp32 position (the
 *     lookup of wa_traj_clearance).  *axes_out (may be NULL) is a device-resident wa_traj of n_ticks points (float)(qt_c / 16384.0), owned
 *     by the caller.
 * 60. wa_jerk_axes_summary.  n_ticks, n_outside, n_blocked, first_blocked (-1: none), n_near, max_tick_turn as wa_tick_axes_summary, over
 *     the filtered ticks.  n_rest_ticks = jerk->n_rest_ticks.  n_turning_rests = groups of stops sharing one GL with q_a != q_e;
 *     min_turn_ticks = the smallest R_f among them (0 without one): psi / (R_f * tick) is the chord rate of that turn.  max_rest_turn =
 *     the largest U between the axes of tick k - 1 and tick k over the rest ticks k > 0.
 * Same bytes on every call; everything runs on the context's stream; g and t are not modified.  Not covered: a limit on the angular
 * acceleration at the ends of a rest, slerp, cascaded windows. */
typedef struct {
    int64_t n_ticks, n_outside, n_blocked, first_blocked, n_near, max_tick_turn;
    int64_t n_rest_ticks, n_turning_rests, min_turn_ticks, max_rest_turn;
} wa_jerk_axes_summary;
int wa_traj_retime_jerk_axes(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit,
                             const double *dwell /* n-1, host, may be NULL */, double tick, int32_t window,
                             const uint8_t *seg_tag /* n-1, host, may be NULL */,
                             const int32_t *q /* n x 3, host */, const wa_tool_beads *tool, int32_t near_add,
                             int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                             int64_t *s_q_out /* n_ticks, host, may be NULL */, uint8_t *tag_out /* n_ticks, host, may be NULL */,
                             wa_traj **axes_out, uint8_t *blocked_out /* n_ticks, host, may be NULL */,
                             wa_retime_summary *sum, wa_stops_summary *stops, wa_jerk_summary *jerk, wa_jerk_axes_summary *axes);

/* ---- tool frames and the weld weave at jerk-limited ticks (not in the reference) ----
 *      An axis fixes two of a tool frame's three rotational degrees of freedom; the third is the direction ACROSS the seam,
 *      perpendicular to the torch and to the direction of travel (the lateral).  A weave is a small periodic offset along the lateral
 *      during a weld pass, tapered in at arc start and out at crater fill.  It moves the tip OFF the polyline that wa_traj_clearance and
 *      the fit stages proved clear, so the offset and the bead check at the displaced position belong where the tick's place on the path
 *      is known: wa_traj_retime_jerk_frames is wa_traj_retime_jerk_axes with a lateral per tick and, with a weave, woven positions
 *      checked where they are.  With window = 1 it covers the unfiltered ticks of wa_traj_retime_stops.  The rules continue the numbering
 *      above; Q = 2^30, GL, S_k, rules 54, 57 and 58 are those of the two sections above, rule 1 and U(a, b) those of the tool section
 *      (DESIGN 4ad).  Integers and individually rounded doubles only, no contraction.
 * 61. Bytes that stay.  With weave == NULL, amp_q = 0 or no weaving segment every output of wa_traj_retime_jerk_axes has that call's
 *     bytes and *lat_out is the only new array.  With a weave only *ticks_out, blocked_out and n_outside, n_blocked, first_blocked and
 *     n_near of *axes may differ; time_q_out, w_q_out, bound_out, s_q_out, tag_out, *axes_out, *sum, *stops, *jerk, max_tick_turn and
 *     the rest counters of rule 60 keep their bytes.  Refused with WA_ERR_ARG before anything is written, beyond rule 56: a NULL frames;
 *     a weave without seg_tag; an amplitude or a taper that is not finite or < 0; a wavelength that is not finite; wl_q outside
 *     1 .. 2^50 (so phi < 2^50 is a double as it stands and phi * P < 2^62); amp_q or taper_q >= 2^61; P outside 2 .. 4096; a NULL
 *     pattern; a pattern entry outside -16384 .. 16384; pattern[0] != 0; tag_mask == 0.  More than 2^31 output ticks: as rule 56, and
 *     *lat_out = NULL, *frames all zero.
 * 62. Travel direction per sample.  lo(j) = the highest m < j with GL_m < GL_j, hi(j) = the lowest m > j with GL_m > GL_j; a = p_lo if
 *     it exists, else p_j; b = p_hi if it exists, else p_j; T_j = (double)b_c - (double)a_c per axis; tau_j = T_j quantised by rule 1,
 *     and (0, 0, 0) where T_j is all zero.  All samples of a run of coincident samples share lo and hi, so they share tau.
 * 63. Lateral per tick.  Moving tick (rule 54 (b), segment i, rule 57's lambda): t = rule 57's expression between tau_i and tau_(i+1),
 *     tau_i where it is all zero.  Rest tick (rule 58, run a .. e): t = tau_a.  z = the tick's own quantised axis qt of rule 57 / 58.
 *     y = z x t = (z_y t_z - z_z t_y, z_z t_x - z_x t_z, z_x t_y - z_y t_x), every product and difference rounded on its own (they
 *     are integers below 2^30: exact).  If y is all zero the lateral is undefined: ql = (0, 0, 0), counted in n_no_lateral; else
 *     ql = rule 1 of y.  *lat_out (may be NULL) is a device-resident wa_traj of n_ticks points (float)(ql_c / 16384.0), owned by the
 *     caller.  The third frame axis is ql x qt and is left to the caller.  Sign: with the torch body up (+z) and travel along +x the
 *     lateral is +y, left of travel.
 * 64. Runs.  Segment i weaves iff (seg_tag[i] & tag_mask) == tag_value.  A run r is a maximal stretch of consecutive weaving segments
 *     lo_r .. hi_r; O_r = GL_(lo_r), E_r = GL_(hi_r + 1).  A tick weaves iff the segment rule 54 gave it weaves (a rest tick: its head
 *     stop) and belongs to that segment's run.  A stop inside a pass must carry a weaving tag to keep the run whole: that is the
 *     caller's business.
 * 65. Offset.  amp_q, wl_q, taper_q = rint(amplitude * Q), rint(wavelength * Q), rint(taper * Q).  For a weaving tick with S = S_k:
 *     d = S - O_r, phi = d mod wl_q; x = ((double)phi * (double)P) / (double)wl_q, j = floor(x) capped at P - 1, f = x - j;
 *     w = pat[j] + (pat[(j+1) mod P] - pat[j]) * f in doubles.  Envelope: m = min(d, E_r - S); env = 1 if taper_q = 0 or m >= taper_q,
 *     else (double)m / (double)taper_q.  off = ((((double)amp_q / Q) * env) * w) / 16384; off_q = (int64)rint(off * Q).  A tick that
 *     does not weave has off = 0.  pattern[0] = 0: with a taper the offset is 0 at both ends of a run, so the position is continuous
 *     into the stops of rule 40.  |off| <= amp_q / Q.
 * 66. Position and check.  If off != 0 and ql is not all zero: out_c = (float)((double)tick_c + ((double)ql_c / 16384.0) * off), tick_c
 *     rule 54's fp32 position; otherwise the position is rule 54's bytes.  *ticks_out holds the woven positions, and rule 59's voxel
 *     lookup and bead check run at the WOVEN position.
 * 67. wa_frames_summary.  n_ticks; n_no_lateral; n_weave_runs; n_weave_ticks; n_weave_blocked = weaving ticks that are blocked;
 *     max_offset_q = the largest |off_q|; max_offset_step_q = the largest |off_q_k - off_q_(k-1)|, k > 0: the lateral speed the weave
 *     adds, which the jerk filter knows nothing of; max_lat_turn = the largest U between the laterals of consecutive ticks where both
 *     are defined.
 * Same bytes on every call; everything runs on the context's stream; g and t are not modified; the pattern is read during the call
 * only.  Not covered: slerp, Euler angles or quaternions, inverse kinematics, a limit on the lateral acceleration of the weave. */
typedef struct {
    double amplitude, wavelength, taper;
    const int16_t *pattern; /* P entries, host, one period; pattern[0] = 0 */
    int32_t P;
    uint8_t tag_mask, tag_value;
} wa_weave;
typedef struct {
    int64_t n_ticks, n_no_lateral, n_weave_runs, n_weave_ticks, n_weave_blocked;
    int64_t max_offset_q, max_offset_step_q, max_lat_turn;
} wa_frames_summary;
int wa_traj_retime_jerk_frames(const wa_grid *g, const wa_traj *t, const wa_retime_limits *lim, const float *v_limit,
                               const double *dwell /* n-1, host, may be NULL */, double tick, int32_t window,
                               const uint8_t *seg_tag /* n-1, host, may be NULL without a weave */,
                               const int32_t *q /* n x 3, host */, const wa_tool_beads *tool, int32_t near_add,
                               const wa_weave *weave /* may be NULL */,
                               int64_t *time_q_out, int64_t *w_q_out, uint8_t *bound_out, wa_traj **ticks_out,
                               int64_t *s_q_out /* n_ticks, host, may be NULL */, uint8_t *tag_out /* n_ticks, host, may be NULL */,
                               wa_traj **axes_out, uint8_t *blocked_out /* n_ticks, host, may be NULL */,
                               wa_traj **lat_out /* may be NULL */,
                               wa_retime_summary *sum, wa_stops_summary *stops, wa_jerk_summary *jerk, wa_jerk_axes_summary *axes,
                               wa_frames_summary *frames);

#ifdef __cplusplus
}
#endif
#endif /* WELDACS_H */
