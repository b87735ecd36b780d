#!/usr/bin/env python3
"""BASELINE config C5 in miniature or at full size: P weld points on an n^3 grid, all P(P-1)/2
pair searches (ACS_Rank::searchBestPathOfPoints' loop, ACSRank_3D.hpp:472-499) batched across the
slots of each GPU and dealt longest-first across ranks, then the weld-seam order by the ACS-TSP
kernel (ACS_GTSP.hpp:255-284) from the in-memory cost matrix (no graph.in round trip), then on rank 0
the tour's segments stitched and smoothed on the device (main.cpp:283-352).

    python examples/plan_batch.py --grid 256 --points 64 --generations 150          # 1 GPU
    torchrun --nproc-per-node 8 examples/plan_batch.py --grid 256 --points 64       # 8 GPUs (torchrun only starts the processes)

Every pair uses its GLOBAL pair index as DEV-mode stream key, so the cost matrix -- and the tour --
do not depend on the number of ranks or slots.  One process per GPU; the exchanges at the end are the library's own
(RCCL behind the C ABI, no torch): wa_comm_broadcast_grid ships rank 0's grid to the others, wa_comm_allgather_costs brings every pair's cost to every rank (8 KB at P = 64) and
wa_comm_gather_paths every pair's path to rank 0, which orders the seams and stitches (ACS_GTSP.hpp:286-298 needs all of
best_matrix on one rank).  WA_FORCE_DIST=1 runs the same exchanges with the one rank a 1-GPU box has.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from welding_robot_amd import api, synth  # noqa: E402
from welding_robot_amd import dist as wd  # noqa: E402


def plan(ctx, grid, point_ids, generations, predict, seed, slots, rank=0, world=1, fixed_colony=0, lazy=False, neighbourhood=6,
         shortcut=0, skip=()):
    """skip: pairs (i, j) known to have no path (--geodesic): not searched, their cost is +inf and their path empty"""
    P = len(point_ids)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    # dealing and order: longest-processing-time-first over end-point groups (welding_robot_amd/dist.py: deal_pairs -- the rule
    # of the drop-in C++ pair loop).  Results do not depend on either: every search draws from the stream of its global pair index.
    nx, nxy = grid.nx, grid.nx * grid.ny
    vox = [(int(v) // nxy, (int(v) // nx) % grid.ny, int(v) % nx) for v in point_ids]
    weights = [1 + sum(abs(a - b) for a, b in zip(vox[i], vox[j])) for i, j in pairs]
    shards, _ = wd.deal_pairs(pairs, weights, world)
    mine = shards[rank]
    if skip:
        mine = [k for k in mine if pairs[k] not in skip]
    colony = fixed_colony or max(1, int(0.35 * predict / float(grid.precision)))
    by_length = os.environ.get("WA_PLAN_ORDER", "") == "length"
    if by_length:   # experiment (round 6): batches of searches of similar length -- a batch-generation lasts as long as its longest walk
        mine = sorted(mine, key=lambda k: (-weights[k], pairs[k][1], k))
    if not slots:   # sized by rule: free memory, footprint limit, whole batches
        slots, _ = api.pair_slots_by_rule(ctx, grid, colony, max(1, len(mine)), len({pairs[k][1] for k in mine}), generations, lazy=lazy, neighbourhood=neighbourhood,
                                          all_fields=by_length)
    plan.last_slots = slots
    t_create = time.perf_counter()
    solver = api.AcsSolver(ctx, grid, n_slots=slots, max_colony=colony, lazy=lazy, neighbourhood=neighbourhood)
    ctx.sync()
    plan.last_create_s = time.perf_counter() - t_create   # device allocation + field initialisation (one-off for a service)
    p = api.default_params(max_iteration=generations, predict=predict, fixed_colony=fixed_colony,
                           rng_mode=api.RNG_DEV, seed=seed)
    cost = np.zeros((P, P), np.float64)
    paths = {}
    for i, j in skip:
        cost[i, j] = cost[j, i] = np.inf
        if pairs.index((i, j)) in shards[rank]:
            paths[(i, j)] = np.zeros(0, np.int32)
    plan.last_batch_s = []                             # seconds per batch: solve / reset / read-back (tools/walk_direct_ab.py --batches)
    plan.last_shortcut = {ij: paths[ij] for ij in paths} if shortcut else {}   # shortcut > 0: {(i, j): waypoint node ids} (the pair's cost is then their length)
    for b0 in range(0, len(mine), slots):
        idx = mine[b0:b0 + slots] if by_length else wd.order_batch(mine[b0:b0 + slots], weights)   # (longest searches first in each half of the slots)
        tb = [time.perf_counter()]
        solver.solve(p, [point_ids[pairs[k][0]] for k in idx], [point_ids[pairs[k][1]] for k in idx], streams=idx)
        tb.append(time.perf_counter())
        solver.reset_pheromone(1.0)  # reset() between problems (:481)
        tb.append(time.perf_counter())
        costs, ids_all = solver.results(len(idx))      # one round trip for the whole batch
        tb.append(time.perf_counter())
        if shortcut:   # the batch's paths shortened by line of sight on the planning grid, in one call (wa_grid_path_shortcut)
            wps, lengths = api.shortcut_paths(grid, ids_all, shortcut)
            costs = np.where(np.isfinite(costs), lengths, costs)
        plan.last_batch_s.append([round(tb[i + 1] - tb[i], 4) for i in range(3)])
        for q, k in enumerate(idx):
            i, j = pairs[k]
            cost[i, j] = cost[j, i] = costs[q]
            paths[(i, j)] = ids_all[q]
            if shortcut:
                plan.last_shortcut[(i, j)] = wps[q]
    solver.close()
    return cost, paths, len(mine)


def plan_exact(grid, point_ids, rank=0, world=1, shortcut=0):
    """--exact-paths: the pair paths from the exact planner (wa_grid_geodesic_paths: one breadth-first field per start point) instead of
    the colony; a pair's cost is the length of its path in metres (span-1 length from shortcut_paths), or of its shortened path.
    Same return values as plan(); pair k belongs to rank k % world."""
    P = len(point_ids)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    mine = [k for k in range(len(pairs)) if k % world == rank]
    hops, ids_all = api.geodesic_paths(grid, [point_ids[pairs[k][0]] for k in mine], [point_ids[pairs[k][1]] for k in mine])
    ids_all = [np.zeros(0, np.int64) if p is None else p for p in ids_all]
    wps, lengths = api.shortcut_paths(grid, ids_all, shortcut or 1)
    cost = np.zeros((P, P), np.float64)
    paths = {}
    plan.last_slots, plan.last_create_s, plan.last_batch_s, plan.last_shortcut = 0, 0.0, [], {}
    for q, k in enumerate(mine):
        i, j = pairs[k]
        cost[i, j] = cost[j, i] = lengths[q] if hops[q] >= 0 else np.inf
        paths[(i, j)] = ids_all[q]
        if shortcut:
            plan.last_shortcut[(i, j)] = wps[q]
    return cost, paths, len(mine)


def turn_totals(dirs, ids_all, ks_all):
    """over all pair paths: the hops, the changes of direction and the sum of the turn measure U over the steps"""
    q = api.quantise_axes(dirs).astype(np.int64)
    hops = changes = turn = 0
    for ids, ks in zip(ids_all, ks_all):
        if ks is None or len(ks) < 2:
            continue
        d = q[ks[:-1]] - q[ks[1:]]
        hops += len(ids) - 1
        changes += int((ks[:-1] != ks[1:]).sum())
        turn += int(((d * d).sum(1) >> 10).sum())
    return dict(hops=hops, direction_changes=changes, turn_sum=turn)


def pose_path_totals(grid, dirs, tool, max_turn, ids_all, ks_all, shortcut, pose_shortcut):
    """of a batch of (voxel, direction) paths (empty arrays for pairs without one): the nodes, the moves by class, the length of the
    lattice paths, and with a shortcut span the shortened length (wa_grid_pose_shortcut's with pose_shortcut, else the plain one's)"""
    nx, nxy = grid.nx, grid.nx * grid.ny
    by_class = np.zeros(4, np.int64)
    for p in ids_all:
        a, b = p[:-1], p[1:]
        by_class += np.bincount((a % nx != b % nx).astype(np.int64) + ((a // nx) % grid.ny != (b // nx) % grid.ny) + (a // nxy != b // nxy), minlength=4)
    q = dict(nodes_total=int(sum(len(p) for p in ids_all)), moves_by_class=[int(v) for v in by_class[1:]],
             length_total=float(api.shortcut_paths(grid, ids_all, 1)[1].sum()))
    if shortcut and pose_shortcut:
        q.update(shortened_length_total=float(api.pose_shortcut_paths(grid, dirs, tool, max_turn, ids_all, ks_all, shortcut)[3].sum()))
    elif shortcut:
        q.update(shortened_length_total=float(api.shortcut_paths(grid, ids_all, shortcut)[1].sum()))
    return q


def plan_pose(grid, point_ids, dirs, tool, max_turn, rank=0, world=1, shortcut=0, pose_shortcut=False, costs=None, diag=None):
    """--pose-paths MAX_TURN: the pair paths from the exact search over (voxel, torch direction) (wa_grid_pose_paths): every node has a
    direction in which the torch body clears the metal, and from node to node the torch turns by at most MAX_TURN.  Costs and return
    values as plan_exact; the directions per node are left in plan_pose.last_dirs.  A path shortened by line of sight (shortcut alone,
    wa_grid_path_shortcut) leaves the planned voxels, so the guarantee then holds for the lattice path only.  With pose_shortcut the
    waypoints and the costs come from wa_grid_pose_shortcut instead: a stretch is straightened only where one of its two end directions
    stays open in every voxel the straight segment touches, the turns at the waypoints keep MAX_TURN, and a hop that cannot be held
    stays the lattice step it was.  Its summary, its total length and the total of the plain shortcut of the same paths (this rank's
    pairs) are left in plan_pose.last_pose_shortcut, the hold of every shortened segment in plan_pose.last_holds (what --pose-fit fits with).
    costs (--pose-turn-costs, an api.pose_costs): the pair paths come from wa_grid_pose_weighted_paths instead, which charges every
    step its turn and the voxel it enters; the pair costs stay lengths.  plan_pose.last_totals holds turn_totals per planner (this
    rank's pairs): of wa_grid_pose_paths always, of the weighted planner beside it when it is used.
    diag (--pose-diagonal, an api.pose_diag_costs): the pair paths come from wa_grid_pose_diag_paths instead, which moves on the
    26-neighbour lattice and keeps the direction on a diagonal move; wa_grid_pose_diag_matrix gives the same pairs' costs, and every
    path must cost what the matrix says.  The planner it replaces has run above: plan_pose.last_diagonal holds both planners' totals."""
    P = len(point_ids)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    mine = [k for k in range(len(pairs)) if k % world == rank]
    starts, ends = [point_ids[pairs[k][0]] for k in mine], [point_ids[pairs[k][1]] for k in mine]
    t0 = time.perf_counter()
    hops, ids_all, ks_all = grid.pose_paths(dirs, tool, max_turn, starts, ends)
    plan_pose.last_totals = dict(pose_paths=dict(turn_totals(dirs, ids_all, ks_all), t_s=time.perf_counter() - t0))
    if costs is not None:
        t0 = time.perf_counter()
        hops, ids_all, ks_all = grid.pose_weighted_paths(dirs, tool, max_turn, costs, starts, ends)
        plan_pose.last_totals.update(pose_weighted_paths=dict(turn_totals(dirs, ids_all, ks_all), t_s=time.perf_counter() - t0,
                                                              cost_total=int(hops[hops >= 0].sum())))
    ids_all = [np.zeros(0, np.int64) if p is None else p for p in ids_all]
    ks_some = [np.zeros(0, np.int32) if k is None else k for k in ks_all]
    plan_pose.last_diagonal = None
    if diag is not None:
        stairs = dict(pose_path_totals(grid, dirs, tool, max_turn, ids_all, ks_some, shortcut, pose_shortcut),
                      planner="wa_grid_pose_weighted_paths" if costs is not None else "wa_grid_pose_paths", pairs_reached=int((hops >= 0).sum()))
        t0 = time.perf_counter()
        matrix = grid.pose_diag_matrix(dirs, tool, max_turn, diag, point_ids)
        t1 = time.perf_counter()
        hops, ids_all, ks_all = grid.pose_diag_paths(dirs, tool, max_turn, diag, starts, ends)
        t2 = time.perf_counter()
        if [int(matrix[pairs[k]]) for k in mine] != hops.tolist():
            raise SystemExit("wa_grid_pose_diag_paths and wa_grid_pose_diag_matrix disagree on a pair's cost")
        ids_all = [np.zeros(0, np.int64) if p is None else p for p in ids_all]
        ks_some = [np.zeros(0, np.int32) if k is None else k for k in ks_all]
        plan_pose.last_totals.update(pose_diag_paths=dict(turn_totals(dirs, ids_all, ks_all), t_s=t2 - t1, cost_total=int(hops[hops >= 0].sum())))
        plan_pose.last_diagonal = dict(pose_path_totals(grid, dirs, tool, max_turn, ids_all, ks_some, shortcut, pose_shortcut),
                                       step=[int(v) for v in diag.c.step], t_matrix_s=t1 - t0, t_paths_s=t2 - t1,
                                       pairs_reached=int((hops >= 0).sum()), cost_total=int(hops[hops >= 0].sum()), staircase=stairs)
    wps, lengths = api.shortcut_paths(grid, ids_all, shortcut or 1)
    plan_pose.last_pose_shortcut, holds = None, None
    if pose_shortcut:
        plain_total = float(lengths.sum())
        wps, _, holds, lengths, summary = api.pose_shortcut_paths(grid, dirs, tool, max_turn, ids_all, ks_some, shortcut)
        plan_pose.last_pose_shortcut = dict({k: summary[k] for k in ("n_waypoints", "n_held_start", "n_held_end", "n_unheld", "max_hold_turn")},
                                            length_total=float(lengths.sum()), plain_length_total=plain_total)
    cost = np.zeros((P, P), np.float64)
    paths = {}
    plan.last_slots, plan.last_create_s, plan.last_batch_s, plan.last_shortcut, plan_pose.last_dirs, plan_pose.last_holds = 0, 0.0, [], {}, {}, {}
    for q, k in enumerate(mine):
        i, j = pairs[k]
        cost[i, j] = cost[j, i] = lengths[q] if hops[q] >= 0 else np.inf
        paths[(i, j)] = ids_all[q]
        plan_pose.last_dirs[(i, j)] = ks_all[q]
        if shortcut:
            plan.last_shortcut[(i, j)] = wps[q]
        if holds is not None:
            plan_pose.last_holds[(i, j)] = holds[q]
    return cost, paths, len(mine)


def plan_safe(grid, point_ids, radius, rank=0, world=1, shortcut=0):
    """--safe-paths R: the pair paths that minimise the sum of clearance costs (wa_grid_clearance_costs with bands at 1^2 .. R^2, then
    wa_grid_weighted_paths) instead of the number of steps: they keep away from the metal where there is room and squeeze through where
    there is not.  A pair's cost for the seam order is a length, as in plan_exact (the weighted distance is not one).
    Same return values as plan(); pair k belongs to rank k % world."""
    P = len(point_ids)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    mine = [k for k in range(len(pairs)) if k % world == rank]
    bands = [k * k for k in range(1, radius + 1)]
    t0 = time.perf_counter()
    costs = grid.clearance_costs(bands)
    t1 = time.perf_counter()
    dist, lens, ids_all = api.weighted_paths(grid, costs, [point_ids[pairs[k][0]] for k in mine], [point_ids[pairs[k][1]] for k in mine])
    plan.last_safe = dict(t_costs_s=t1 - t0, t_paths_s=time.perf_counter() - t1, bands=bands)
    ids_all = [np.zeros(0, np.int64) if p is None else p for p in ids_all]
    wps, lengths = api.shortcut_paths(grid, ids_all, shortcut or 1)
    cost = np.zeros((P, P), np.float64)
    paths = {}
    plan.last_slots, plan.last_create_s, plan.last_batch_s, plan.last_shortcut = 0, 0.0, [], {}
    for q, k in enumerate(mine):
        i, j = pairs[k]
        cost[i, j] = cost[j, i] = lengths[q] if dist[q] >= 0 else np.inf
        paths[(i, j)] = ids_all[q]
        if shortcut:
            plan.last_shortcut[(i, j)] = wps[q]
    return cost, paths, len(mine)


def plan_diagonal(grid, point_ids, step, rank=0, world=1, shortcut=0):
    """--diagonal-paths A B C: the pair paths from the exact planner with diagonal moves (wa_grid_chamfer_paths: face, edge and corner
    moves cost A, B, C; a diagonal move needs the whole box it spans free) instead of the colony.  The chamfer matrix of the points comes
    first (what a seam order in this metric would start from; here it is held against the paths' distances).  A pair's cost for the
    seam order is a length in metres, as in plan_exact.  Same return values as plan(); pair k belongs to rank k % world."""
    P = len(point_ids)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    mine = [k for k in range(len(pairs)) if k % world == rank]
    t0 = time.perf_counter()
    matrix = grid.chamfer_matrix(step, point_ids)
    t1 = time.perf_counter()
    dist, lens, ids_all = api.chamfer_paths(grid, step, [point_ids[pairs[k][0]] for k in mine], [point_ids[pairs[k][1]] for k in mine])
    plan.last_diagonal = dict(step=[int(v) for v in step], t_matrix_s=t1 - t0, t_paths_s=time.perf_counter() - t1)
    assert all(matrix[pairs[k]] == dist[q] for q, k in enumerate(mine)), "matrix and paths are two routes to the same distances"
    ids_all = [np.zeros(0, np.int64) if p is None else p for p in ids_all]
    wps, lengths = api.shortcut_paths(grid, ids_all, shortcut or 1)
    cost = np.zeros((P, P), np.float64)
    paths = {}
    plan.last_slots, plan.last_create_s, plan.last_batch_s, plan.last_shortcut = 0, 0.0, [], {}
    for q, k in enumerate(mine):
        i, j = pairs[k]
        cost[i, j] = cost[j, i] = lengths[q] if dist[q] >= 0 else np.inf
        paths[(i, j)] = ids_all[q]
        if shortcut:
            plan.last_shortcut[(i, j)] = wps[q]
    return cost, paths, len(mine)


def plan_safe_diagonal(grid, point_ids, radius, step, gain, rank=0, world=1, shortcut=0, extra_pen=None):
    """--safe-paths R with --diagonal-paths A B C: the pair paths from the exact planner with diagonal moves AND clearance penalties
    (wa_grid_chamfer_weighted_paths): a move costs its step plus gain * (the number of bands 1^2 .. R^2 the voxel entered lies within),
    so the paths are short like the diagonal ones and keep off the metal like the safe ones where there is room.  The matrix of the
    points comes first and is held against the paths' distances.  A pair's cost for the seam order is a length in metres, as in
    plan_exact.  extra_pen (--torch-grid): penalties of Grid.torch_penalties, added and the sum clamped at WA_PEN_MAX.
    Same return values as plan(); pair k belongs to rank k % world."""
    P = len(point_ids)
    pairs = [(i, j) for i in range(P) for j in range(i + 1, P)]
    mine = [k for k in range(len(pairs)) if k % world == rank]
    bands = [k * k for k in range(1, radius + 1)]
    t0 = time.perf_counter()
    costs = grid.clearance_costs(bands)
    pen = (gain * np.maximum(costs.astype(np.int64) - 1, 0)).astype(np.uint8)   # (occupied voxels hold cost 0; their bytes are ignored)
    if extra_pen is not None:
        pen = np.minimum(pen.astype(np.int64) + extra_pen, 31).astype(np.uint8)
    t1 = time.perf_counter()
    matrix = grid.chamfer_weighted_matrix(step, pen, point_ids)
    t2 = time.perf_counter()
    dist, lens, ids_all = api.chamfer_weighted_paths(grid, step, pen, [point_ids[pairs[k][0]] for k in mine], [point_ids[pairs[k][1]] for k in mine])
    plan.last_safe_diagonal = dict(step=[int(v) for v in step], gain=int(gain), bands=bands, t_costs_s=t1 - t0, t_matrix_s=t2 - t1,
                                   t_paths_s=time.perf_counter() - t2)
    plan.last_pen, plan.last_costs = pen, costs
    assert all(matrix[pairs[k]] == dist[q] for q, k in enumerate(mine)), "matrix and paths are two routes to the same distances"
    ids_all = [np.zeros(0, np.int64) if p is None else p for p in ids_all]
    wps, lengths = api.shortcut_paths(grid, ids_all, shortcut or 1)
    cost = np.zeros((P, P), np.float64)
    paths = {}
    plan.last_slots, plan.last_create_s, plan.last_batch_s, plan.last_shortcut = 0, 0.0, [], {}
    for q, k in enumerate(mine):
        i, j = pairs[k]
        cost[i, j] = cost[j, i] = lengths[q] if dist[q] >= 0 else np.inf
        paths[(i, j)] = ids_all[q]
        if shortcut:
            plan.last_shortcut[(i, j)] = wps[q]
    return cost, paths, len(mine)


def path_counts(grid, metal, pen, path_list, shortcut):
    """the counts of safe_diagonal_report for one planner's paths of the same pairs: nodes, moves by class, the penalties entered, nodes
    next to the metal (distance field <= 1), segments of the unsmoothed paths that hit the planning grid, the length and, with
    --shortcut, the shortened length and its waypoints"""
    nx, nxy = grid.nx, grid.nx * grid.ny
    d2 = metal.distance_field()
    by_class = np.zeros(4, np.int64)
    n_hit = penalty = near = 0
    for p in path_list:
        p = np.asarray(p, np.int64)
        a, b = p[:-1], p[1:]
        by_class += np.bincount((a % nx != b % nx).astype(np.int64) + ((a // nx) % grid.ny != (b // nx) % grid.ny) + (a // nxy != b // nxy), minlength=4)
        penalty += int(pen[b].astype(np.int64).sum())
        near += int((d2[p] <= 1).sum())
        t = api.Trajectory.stitch(grid, [p])
        n_hit += t.clearance(grid)[3]["n_hit"]
        t.close()
    q = dict(nodes_total=int(sum(len(p) for p in path_list)), moves_by_class=[int(v) for v in by_class[1:]], penalty_total=int(penalty),
             nodes_next_to_metal=int(near), n_hit=int(n_hit), length_total=float(api.shortcut_paths(grid, path_list, 1)[1].sum()))
    if shortcut:
        wps, lengths = api.shortcut_paths(grid, path_list, shortcut)
        q.update(shortened_length_total=float(lengths.sum()), waypoints_total=int(sum(len(w) for w in wps)))
    return q


def safe_diagonal_report(grid, metal, pts, paths, shortcut):
    """what goes into the JSON under safe_diagonal_paths (rank 0, which holds every pair's path): path_counts of the new paths, and of the
    diagonal paths (wa_grid_chamfer_paths, the same steps) and the safe paths (wa_grid_weighted_paths, the same bands) of the same pairs"""
    reach = [ij for ij in sorted(paths) if len(paths[ij])]
    info = plan.last_safe_diagonal
    starts, ends = [pts[i] for i, _ in reach], [pts[j] for _, j in reach]
    q = dict(info, **path_counts(grid, metal, plan.last_pen, [paths[ij] for ij in reach], shortcut))
    q.update(diagonal=path_counts(grid, metal, plan.last_pen, api.chamfer_paths(grid, info["step"], starts, ends)[2], shortcut),
             safe=path_counts(grid, metal, plan.last_pen, api.weighted_paths(grid, plan.last_costs, starts, ends)[2], shortcut))
    return q


def diagonal_report(grid, pts, paths, short, shortcut):
    """what goes into the JSON under diagonal_paths (rank 0, which holds every pair's path): the nodes, the moves by class, the length
    before any shortcut, the segments of the unsmoothed paths that hit the planning grid (none: the box rule is wa_traj_clearance's
    segment test) and, with --shortcut, the shortened total beside the one of the hop-optimal paths of the same pairs"""
    reach = [ij for ij in sorted(paths) if len(paths[ij])]
    nx, nxy = grid.nx, grid.nx * grid.ny
    by_class = np.zeros(4, np.int64)
    n_hit = 0
    for ij in reach:
        p = np.asarray(paths[ij], np.int64)
        a, b = p[:-1], p[1:]
        by_class += np.bincount((a % nx != b % nx).astype(np.int64) + ((a // nx) % grid.ny != (b // nx) % grid.ny) + (a // nxy != b // nxy), minlength=4)
        t = api.Trajectory.stitch(grid, [p])
        n_hit += t.clearance(grid)[3]["n_hit"]
        t.close()
    q = dict(plan.last_diagonal, nodes_total=int(sum(len(paths[ij]) for ij in reach)), moves_by_class=[int(v) for v in by_class[1:]],
             length_total=float(api.shortcut_paths(grid, [paths[ij] for ij in reach], 1)[1].sum()), n_hit=int(n_hit))
    if shortcut:
        _, hop_paths = api.geodesic_paths(grid, [pts[i] for i, _ in reach], [pts[j] for _, j in reach])
        hop_wps, hop_short = api.shortcut_paths(grid, hop_paths, shortcut)
        q.update(shortened_length_total=float(api.shortcut_paths(grid, [short[ij] for ij in reach], 1)[1].sum()),
                 length_total_hop_optimal=float(api.shortcut_paths(grid, hop_paths, 1)[1].sum()),
                 shortened_length_total_hop_optimal=float(hop_short.sum()),
                 waypoints_total=int(sum(len(short[ij]) for ij in reach)),
                 waypoints_total_hop_optimal=int(sum(len(w) for w in hop_wps)))
    return q


def smooth(ctx, grid, segs, wsegs, rev, fit=None, pose_fit=None):
    """main.cpp:283-352 on the device: the tour's segments stitched, then the two smoothing passes; wsegs (--shortcut): the shortened
    segments, whose waypoints are then the coarse points of the cubic fit.  fit = (metal grid, max_level, dump path or None) (--fit):
    the curve is wa_grid_fit_trajectory's instead, control points ON the waypoints' polyline, refined until its samples clear the metal.
    pose_fit = (dirs, tool, hold segments) (--pose-fit): the curve is wa_grid_pose_fit_trajectory's, refined until one of the planned holds
    stays open along every piece of it; the holds are stitched as the waypoints are (a reversed segment's holds reversed, the
    zero-length leg between two segments unheld).  Its summary goes beside the plain fit's; the plain fit's samples and the directions
    per segment are left in smooth.fit_samples and smooth.seg_dir.
    Returns (samples, ok flags, what goes into the JSON)."""
    info = {}
    path = api.Trajectory.stitch(grid, segs, rev)
    ends = path.points()[[0, -1]]
    s2 = None
    if wsegs is not None and fit is not None:
        metal, max_level, dump = fit
        wpath = api.Trajectory.stitch(grid, wsegs, rev)
        _, samples, _, summary = wpath.fit(metal, degree=3, max_level=max_level, n_samples=6001)
        traj = samples.points()
        if dump:
            np.save(dump, wpath.points())
        # today's fit of the same waypoints, for the comparison
        plain, pok, _ = smooth(ctx, grid, segs, wsegs, rev)
        before = api.Trajectory.from_points(ctx, plain[pok.astype(bool)]).clearance(metal)[3]["n_hit"]
        smooth.plain = (plain, pok)
        lens = api.shortcut_paths(grid, wsegs, 1)[1]
        lattice = api.shortcut_paths(grid, segs, 1)[1]
        info.update(shortened_length_total=float(lens.sum()), lattice_length_total=float(lattice.sum()))
        info.update(fit=dict(summary, max_level=max_level, n_hit_plain_fit=int(before)), waypoints=len(wpath), stitched_nodes=len(path),
                    trajectory_samples=len(traj), trajectory_length=float(np.linalg.norm(np.diff(traj, axis=0), axis=1).sum()))
        if pose_fit is not None:
            dirs, tool, hsegs = pose_fit
            parts = []
            for h, r in zip(hsegs, rev):
                parts += [np.asarray(h[::-1] if r else h, np.int32), np.full(1, -1, np.int32)]
            holds = np.concatenate(parts)[:-1]
            t0 = time.perf_counter()
            _, psamples, _, seg_dir, _, psummary = wpath.pose_fit(metal, dirs, tool, holds, degree=3, max_level=max_level, n_samples=6001)
            smooth.fit_samples, smooth.seg_dir = traj, seg_dir
            traj = psamples.points()
            info.update(pose_fit=dict(psummary, max_level=max_level, n_held_legs=int((holds >= 0).sum()), t_s=time.perf_counter() - t0),
                        trajectory_length=float(np.linalg.norm(np.diff(traj, axis=0), axis=1).sum()))
        return traj, np.ones(len(traj), np.uint8), info
    if wsegs is not None:
        # the shortened segments stitched the same way: their waypoints are the coarse points of the cubic fit
        wpath = api.Trajectory.stitch(grid, wsegs, rev)
        # float64 lengths on rank 0 (the gathered costs are fp32): with a span of 1 a path's length is the sum over all its nodes,
        # so over the waypoints it is the shortened length bit for bit, and over the pair paths the unshortened (lattice) one
        lens = api.shortcut_paths(grid, wsegs, 1)[1]
        lattice = api.shortcut_paths(grid, segs, 1)[1]
        info.update(shortened_length_total=float(lens.sum()), lattice_length_total=float(lattice.sum()), waypoints=len(wpath))
        try:
            s2 = api.Bspline(ctx, 3, 3, 2, 2, len(wpath))
            coarse = wpath
        except api.WeldacsError as e:
            if e.code != 1:
                raise
        info.update(shortcut_smoothing=s2 is not None)
    if s2 is None:   # today's coarse points: every 8th node of the stitched path
        s1 = api.Bspline(ctx, 3, 0, 0, 0, len(path))          # BS_Basic<float,3,0,0,0>: time-indexed resampling
        s1.set_param(ends[0], ends[1], path, 150.0)
        n1 = max(16, len(path) // 8)
        _, _, coarse = s1.sample(150.0 / n1, 150.0 / n1, n1, host=False, device=True)
        s2 = api.Bspline(ctx, 3, 3, 2, 2, len(coarse))        # cubic with zero end velocity / acceleration
    z = np.zeros((2, 3), np.float32)
    s2.set_param(np.vstack([ends[:1], z]), np.vstack([ends[1:], z]), coarse, 6000.0)
    traj, ok = s2.sample(0.0, 1.0, 6001)                  # 1 kHz over 6 s
    info.update(stitched_nodes=len(path), coarse_points=len(coarse), trajectory_samples=int(ok.sum()),
                trajectory_length=float(np.linalg.norm(np.diff(traj, axis=0), axis=1).sum()))
    return traj, ok, info


def seam_stage(ctx, cost, seed, n_starts, rules=None):
    """Order and direction of the seams (points 2k, 2k+1 = seam k) from the endpoint costs.  Start 0 of the search is today's order
    stage one level up: ACS-TSP on D[s][t] = the cheapest of the four end combinations, every seam left at the end nearer to its
    successor.  Returns (what goes into the JSON, order, directions)."""
    m = cost.shape[0] // 2
    D = cost.reshape(m, 2, m, 2).min(axis=(1, 3))
    np.fill_diagonal(D, 0.0)
    tour = api.gtsp_solve(ctx, D, mode=api.RNG_DEV, seed=seed)
    order0 = [int(e[0]) for e in tour["edges"][0]]
    dir0 = [int(cost[2 * s:2 * s + 2, 2 * t:2 * t + 2].min(axis=1).argmin() == 0) for s, t in zip(order0, order0[1:] + order0[:1])]
    r = api.seam_tour(ctx, cost, closed=True, or_len=3, n_starts=n_starts, seed=seed, order0=order0, dir0=dir0)
    s = r["summary"]
    info = dict(seams=dict(m=m, acs_tsp=dict(order=order0, dir=dir0, cost=s["start0_cost_q_in"] / api.SEAM_Q, seam_level_cost=float(tour["L"][0])),
                           searched=dict(order=r["order"].tolist(), dir=r["dir"].tolist(), cost=r["cost"], best_start=s["best_start"],
                                         n_starts=s["n_starts"], start0_descent_cost=s["start0_cost_q_out"] / api.SEAM_Q,
                                         passes_total=s["passes_total"], n_capped=s["n_capped"])))
    if m <= 16:
        ex = api.seam_tour_exact(ctx, cost, closed=True)
        info["seams"].update(exact=dict(order=ex["order"].tolist(), dir=ex["dir"].tolist(), cost=ex["cost"]))
    if rules is None:
        return info, r["order"].tolist(), r["dir"].tolist()
    # job rules (--seam-before / --seam-fixed): what the free tour above breaks, then the tour that keeps them (wa_gtsp_seam_tour_rules,
    # started from the repaired identity: the ACS-TSP tour knows no rules) and the exact one beside it; the job is stitched from this tour
    before, after, fixed = rules
    bad_p, bad_d = api.seam_rules_check(r["order"], r["dir"], before, after, fixed, closed=True, ctx=ctx)
    rr = api.seam_tour_rules(ctx, cost, before, after, fixed, closed=True, or_len=3, n_starts=n_starts, seed=seed)
    s = rr["summary"]
    assert api.seam_rules_check(rr["order"], rr["dir"], before, after, fixed, closed=True, ctx=ctx) == (0, 0)
    info["seam_rules"] = dict(before=[int(x) for x in before], after=[int(x) for x in after], fixed=[int(x) for x in fixed],
                              n_prec=s["n_prec"], n_fixed=s["n_fixed"],
                              unconstrained_breaks=dict(precedences=bad_p, directions=bad_d, cost=r["cost"]),
                              searched=dict(order=rr["order"].tolist(), dir=rr["dir"].tolist(), cost=rr["cost"], best_start=s["best_start"],
                                            n_starts=s["n_starts"], passes_total=s["passes_total"], n_capped=s["n_capped"]))
    if m <= 16:
        ex = api.seam_tour_rules_exact(ctx, cost, before, after, fixed, closed=True)
        info["seam_rules"].update(exact=dict(order=ex["order"].tolist(), dir=ex["dir"].tolist(), cost=ex["cost"]))
    return info, rr["order"].tolist(), rr["dir"].tolist()


def parse_seam_rules(ap, args):
    """--seam-before A:B[,A:B...] and --seam-fixed S:D[,...] as (before, after, fixed bytes), or None when neither is given"""
    if args.seam_before is None and args.seam_fixed is None:
        return None
    if not args.seams:
        ap.error("--seam-before / --seam-fixed need the seams of --seams")
    m = args.points // 2

    def pairs(text, what):
        out = []
        for item in (text or "").split(","):
            if not item:
                continue
            try:
                a, b = (int(x) for x in item.split(":"))
            except ValueError:
                ap.error("%s takes N:N[,N:N...], not %r" % (what, item))
            out.append((a, b))
        return out

    before, after, fixed = [], [], [0] * m
    for a, b in pairs(args.seam_before, "--seam-before"):
        if not (0 <= a < m and 0 <= b < m) or a == b or b == 0:
            ap.error("--seam-before %d:%d: two different seams of 0 .. %d, and nothing goes before seam 0 (the tour starts there)" % (a, b, m - 1))
        before.append(a)
        after.append(b)
    for s, d in pairs(args.seam_fixed, "--seam-fixed"):
        if not 0 <= s < m or d not in (0, 1):
            ap.error("--seam-fixed %d:%d: a seam of 0 .. %d and the direction 0 (enter at the even point) or 1" % (s, d, m - 1))
        fixed[s] = d + 1
    return before, after, fixed


def torch_tool_and_cone(metal, K):
    """the torch of --torch and --torch-grid: a 300 mm body of 24 beads and K directions of a cone around +z"""
    length16 = int(min(65536, round(16 * 0.3 / float(metal.precision))))
    tool = api.torch_tool(np.rint(np.linspace(0, length16, 24)).astype(np.int64), np.full(24, 1))
    return tool, api.torch_cone(K, 1.2), length16


def torch_grid_report(base, count, paths, paths_without, shortcut):
    """what --torch-grid costs and buys on the pair paths themselves: nodes, lengths and nodes without any open direction (count:
    Grid.torch_reach of the grid planned on without the flag), beside the same planner's paths on that grid"""
    def totals(table):
        reach = [np.asarray(table[ij], np.int64) for ij in sorted(table) if len(table[ij])]
        q = dict(pairs_reached=len(reach), nodes_total=int(sum(len(p) for p in reach)), nodes_no_dir=int(sum((count[p] == 0).sum() for p in reach)),
                 length_total=float(api.shortcut_paths(base, reach, 1)[1].sum()))
        if shortcut:
            q.update(shortened_length_total=float(api.shortcut_paths(base, reach, shortcut)[1].sum()))
        return q
    return dict(totals(paths), without=totals(paths_without) if paths_without is not None else None)


def torch_stage(ctx, metal, xyz, stops, K, max_turn=-1, want=None):
    """Torch axes along the trajectory's samples (wa_traj_tool_axes): one of K directions of a cone around +z per sample so that a
    300 mm torch body (24 beads) stays clear of the metal.  Legs: the travel moves between the tour's stops, cut at the sample nearest to
    each stop.  Wish: the torch points down the gradient of the distance field (at the nearest metal), so the body -- a direction runs
    from the tip into the body -- is wished along the gradient itself; computed here in numpy.  Beside the plan, the check of the
    linearly interpolated, renormalised axes half-way between consecutive samples: what a controller that interpolates would send.
    want (--pose-fit): the wish per sample instead, the direction the fit found open along the sample's segment (zero rows: none)."""
    curve = api.Trajectory.from_points(ctx, xyz)
    n = len(xyz)
    cuts = [0]
    for p in stops[1:-1]:
        cuts.append(cuts[-1] + int(np.argmin(np.linalg.norm(xyz[cuts[-1]:] - p, axis=1))))
    off = np.asarray(cuts + [n], np.int64)
    ids = curve.clearance(metal)[0]
    d2 = metal.distance_field().astype(np.float64).reshape(metal.nz, metal.ny, metal.nx)
    gz, gy, gx = np.gradient(np.sqrt(d2))
    if want is None:
        want = np.stack([gx.ravel()[ids], gy.ravel()[ids], gz.ravel()[ids]], 1).astype(np.float32)
        want[~np.isfinite(want).all(1)] = 0                      # (a grid without metal: no wish)
    tool, dirs, length16 = torch_tool_and_cone(metal, K)
    r = curve.torch_axes(metal, dirs, tool, w_near=4, w_want=1, w_turn=8, near_add=8, max_turn=max_turn, want=want, off=off, feas=False)
    info = dict(r["summary"], K=K, n_legs=len(off) - 1, directions_used=int(len(set(r["dir"].tolist()))), tool_length16=length16)
    torch_stage.last = (off, r["dir"], dirs, tool)               # (what --tick-poses goes on from)
    if n > 1:
        a = dirs[r["dir"]].astype(np.float64)
        mid = a[:-1] + a[1:]
        norm = np.linalg.norm(mid, axis=1, keepdims=True)
        mid = np.where(norm > 0, mid / np.where(norm > 0, norm, 1), a[:-1])
        half = api.Trajectory.from_points(ctx, ((xyz[:-1].astype(np.float64) + xyz[1:]) / 2).astype(np.float32))
        cs = half.torch_check(metal, mid.astype(np.float32), tool, 8)[2]
        info.update(interpolated=dict(n=cs["n"], n_blocked=cs["n_chosen_blocked"], first_blocked=cs["first_chosen_blocked"],
                                      n_near=cs["n_chosen_near"]))
    return info


def tick_pose_stage(ctx, metal, xyz, limits, tick, omega, h, duration_free):
    """Tool poses at the controller's ticks (--tick-poses), on the device from end to end: the chosen directions of torch_stage as
    quantised axes, smoothed along the path where the body stays clear of the metal (wa_traj_axes_smooth), turned into a per-sample
    speed limit for the turn rate omega (wa_traj_axes_limits), the curve timed again under that limit (wa_traj_retime), and the axis
    at every tick with its check against the metal (wa_traj_tick_axes).  The axes never pass through the host."""
    off, chosen, dirs, tool = torch_stage.last
    v_max, acc, dec, a_lat, v_near, near_d2 = limits
    curve = api.Trajectory.from_points(ctx, xyz)
    sm = curve.smooth_axes(api.quantise_axes(dirs)[chosen], h, 8, metal, tool, off)
    v_limit, ls = curve.axis_limits(sm["q"], omega, v_max, v_max * 1e-3)
    time_q, w_q, _, _, rs = curve.retime(v_max, acc, dec, tick, a_lat=a_lat, grid=metal, v_near=v_near, near_d2=int(near_d2), v_limit=v_limit,
                                         ticks=False)
    info = dict(omega=omega, h=h, smooth=sm["summary"], limits=ls, duration_free=duration_free, duration_turn_limited=rs["time_q"] / api.RETIME_Q,
                ticks=None, max_tick_turn=None, blocked_ticks=None)
    if rs["n_ticks"] <= 1 << 31:
        axes, _, ts = curve.tick_axes(sm["q"], time_q, w_q, acc, dec, tick, metal, tool, near_add=8, blocked=False)
        info.update(ticks=ts, max_tick_turn=ts["max_tick_turn"], blocked_ticks=ts["n_blocked"])
        axes.close()
    return info


def jerk_pose_stage(ctx, metal, xyz, limits, tick, omega, h, jerk):
    """Tool poses at the jerk-limited ticks (--jerk-poses): tick_pose_stage's chain -- the chosen directions smoothed
    (wa_traj_axes_smooth) and turned into a per-sample speed limit for the turn rate omega (wa_traj_axes_limits) -- ending in ONE call
    that times the curve under that limit, filters the ticks over the window of the jerk limit and gives every filtered tick its
    checked axis (wa_traj_retime_jerk_axes).  Neither the filtered arc lengths nor the axes pass through the host."""
    off, chosen, dirs, tool = torch_stage.last
    v_max, acc, dec, a_lat, v_near, near_d2 = limits
    curve = api.Trajectory.from_points(ctx, xyz)
    sm = curve.smooth_axes(api.quantise_axes(dirs)[chosen], h, 8, metal, tool, off)
    v_limit, ls = curve.axis_limits(sm["q"], omega, v_max, v_max * 1e-3)
    window = api.jerk_window(acc, dec, jerk, tick)
    _, _, _, _, _, _, rs, _, sj, axes, _, sa = curve.retime_jerk_axes(sm["q"], v_max, acc, dec, tick, window, grid=metal, tool=tool, near_add=8,
                                                                      a_lat=a_lat, v_near=v_near, near_d2=int(near_d2), v_limit=v_limit,
                                                                      ticks=False, blocked=False)
    if axes is not None:
        axes.close()
    return dict(omega=omega, h=h, jerk_limit=jerk, window=window, smooth=sm["summary"], limits=ls,
                duration_turn_limited=rs["time_q"] / api.RETIME_Q, duration_s=(sj["n_ticks"] - 1) * tick, n_back=sj["n_back"],
                n_short_rests=sj["n_short_rests"], ticks=sa, max_tick_turn=sa["max_tick_turn"], blocked_ticks=sa["n_blocked"])


def jerk_report(ctx, metal, sj, filtered, tick, plain_ticks, plain_time_q, jerk):
    """what --jerk adds to the JSON: the summary of wa_traj_retime_jerk, the filtered duration against the unfiltered one and the
    clearance check of the filtered ticks"""
    return dict(sj, jerk_limit=jerk, jerk_bound=2.0 * sj["in_max_d2"] / sj["window"] / api.RETIME_Q / tick ** 3,
                max_jerk=sj["max_d3"] / api.RETIME_Q / tick ** 3, duration_s=(sj["n_ticks"] - 1) * tick,
                unfiltered_duration_s=plain_time_q / api.RETIME_Q, unfiltered_n_ticks=plain_ticks,
                ticks_clearance=filtered.clearance(metal)[3] if filtered is not None else None)


def weld_pass_stage(ctx, metal, segs, rev, weld_speed, t_start, t_end, limits, tick, jerk=None):
    """Weld passes in the timed trajectory (--seams --weld-passes): the stitched polyline as it stands -- segs alternates seams and the
    travel between them, each walked in its tour direction -- cut into steps of at most half the grid precision, the sample at both
    ends of every seam doubled.  The doubled sample at a seam's entry is a stop of t_start seconds (strike the arc), the one at its
    exit a stop of t_end (crater fill); seam samples are capped at the weld speed and seam segments tagged 1.  wa_traj_retime_stops
    times it, wa_traj_tick_axes_stops tags every controller tick (the axis is held straight up: the torch stage is not part of this).
    Returns what goes into the JSON under weld_passes."""
    v_max, acc, dec, a_lat, v_near, near_d2 = limits
    cx, cy, cz = metal.coords()
    step = 0.5 * float(metal.precision)

    def dense(ids):
        ids = np.asarray(ids, np.int64)
        p = np.stack([cx[ids % metal.nx], cy[(ids // metal.nx) % metal.ny], cz[ids // (metal.nx * metal.ny)]], 1).astype(np.float64)
        out = [p[:1]]
        for a, b in zip(p[:-1], p[1:]):
            m = max(1, int(np.ceil(np.linalg.norm(b - a) / step)))
            out.append(a[None, :] + (b - a)[None, :] * (np.arange(1, m + 1, dtype=np.float64) / m)[:, None])
            out[-1][-1] = b
        return np.concatenate(out).astype(np.float32)

    parts, dwell, tag, vlim, seam_length = [], [], [], [], 0.0
    for k, (seg, r) in enumerate(zip(segs, rev)):
        pts = dense(seg[::-1] if r else seg)
        if k % 2 == 0:   # a seam: entry doubled, the pass, exit doubled
            parts += [pts[:1], pts, pts[-1:]]
            if k:
                dwell.append(-1.0)   # (from the travel's last sample to the entry: no length when they are one voxel)
                tag.append(0)
            dwell += [t_start] + [-1.0] * (len(pts) - 1) + [t_end]
            tag += [0] + [1] * (len(pts) - 1) + [0]
            vlim += [weld_speed] * (len(pts) + 2)
            seam_length += float(np.linalg.norm(np.diff(pts.astype(np.float64), axis=0), axis=1).sum())
        else:            # travel: the seam before ends with its first sample, the seam behind begins with its last
            pts = pts[1:-1]
            if len(pts):
                parts.append(pts)
                dwell += [-1.0] * len(pts)
                tag += [0] * len(pts)
                vlim += [v_max] * len(pts)
    xyz = np.concatenate(parts)
    dwell, tag = np.asarray(dwell, np.float64), np.asarray(tag, np.uint8)
    curve = api.Trajectory.from_points(ctx, xyz)
    kw = dict(dwell=dwell, a_lat=a_lat, grid=metal, v_near=v_near, near_d2=int(near_d2), v_limit=np.asarray(vlim, np.float32))
    if jerk is not None:   # the same passes through the moving average: its ticks, its tags; the timing reported is the underlying profile's
        _, _, _, _, plain, _ = curve.retime_stops(v_max, acc, dec, tick, ticks=False, **kw)
        time_q, w_q, _, ticks, _, tags, rs, ss, sj = curve.retime_jerk(v_max, acc, dec, tick, api.jerk_window(acc, dec, jerk, tick),
                                                                       seg_tag=tag, **kw)
        weld_q = int(np.diff(time_q)[tag != 0].sum())
        return dict(n_stops=ss["n_stops"], dwell_s=ss["dwell_q"] / api.RETIME_Q, weld_s=weld_q / api.RETIME_Q,
                    travel_s=(rs["time_q"] - weld_q - ss["dwell_q"]) / api.RETIME_Q, duration_s=rs["time_q"] / api.RETIME_Q,
                    n_ticks=sj["n_ticks"], weld_ticks=int((tags != 0).sum()) if tags is not None else None,
                    ticks_clearance=ticks.clearance(metal)[3] if ticks is not None else None, samples=len(xyz), seam_length=seam_length,
                    weld_speed=weld_speed, t_start_s=t_start, t_end_s=t_end, tick_s=tick,
                    jerk=jerk_report(ctx, metal, sj, ticks, tick, plain["n_ticks"], plain["time_q"], jerk))
    time_q, w_q, _, ticks, rs, ss = curve.retime_stops(v_max, acc, dec, tick, **kw)
    q = np.tile(np.array([0, 0, 16384], np.int32), (len(xyz), 1))
    _, _, _, _, ts = curve.tick_axes_stops(q, time_q, w_q, acc, dec, tick, seg_tag=tag, axes=False, blocked=False)
    weld_q = int(np.diff(time_q)[tag != 0].sum())
    return dict(n_stops=ss["n_stops"], dwell_s=ss["dwell_q"] / api.RETIME_Q, weld_s=weld_q / api.RETIME_Q,
                travel_s=(rs["time_q"] - weld_q - ss["dwell_q"]) / api.RETIME_Q, duration_s=rs["time_q"] / api.RETIME_Q, n_ticks=rs["n_ticks"],
                weld_ticks=ts["n_tagged"], ticks_clearance=ticks.clearance(metal)[3] if ticks is not None else None,
                samples=len(xyz), seam_length=seam_length, weld_speed=weld_speed, t_start_s=t_start, t_end_s=t_end, tick_s=tick)


def wait_for_device_memory(ctx, want=0.85, timeout_s=30.0):
    """A process that has just exited may still be giving its device memory back; allocations made meanwhile can end up in
    host-visible memory (measured: the whole run 4x slower).  Wait until most of the device memory is free."""
    t0 = time.perf_counter()
    while True:
        free, total = ctx.memory_info()
        if free >= want * total or time.perf_counter() - t0 > timeout_s:
            return time.perf_counter() - t0
        time.sleep(0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=96)
    ap.add_argument("--points", type=int, default=16)
    ap.add_argument("--generations", type=int, default=150)
    ap.add_argument("--slots", type=int, default=0, help="concurrent pair searches per GPU; 0 = sized by rule (memory, whole batches)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--neighbourhood", type=int, default=6, choices=(6, 26), help="26: the variant the reference stubs out (ACSRank_3D.hpp:361-388)")
    ap.add_argument("--lazy", action="store_true",
                    help="wa_acs_create_lazy: never-deposited voxels are not swept (same results, O(deposited voxels) per generation)")
    ap.add_argument("--clearance", type=float, default=None,
                    help="metres of clearance: plan on the grid inflated by it (weld points kept free), then check the final trajectory "
                         "against the original grid (wa_traj_clearance)")
    ap.add_argument("--shortcut", action="store_true",
                    help="shorten every pair path by line of sight on the planning grid (wa_grid_path_shortcut): the shortened lengths are "
                         "the pair costs of the seam order, and the waypoints are the coarse points of the cubic fit")
    ap.add_argument("--max-span", type=int, default=128, help="--shortcut: the farthest node an anchor may see (1..4096)")
    ap.add_argument("--geodesic", action="store_true",
                    help="exact hop matrix of the weld points on the planning grid first (wa_grid_geodesic_matrix): pairs without any path "
                         "are not searched and are listed, and every search is held against the optimum")
    ap.add_argument("--exact-paths", action="store_true",
                    help="take the pair paths from the exact planner (wa_grid_geodesic_paths) instead of the colony")
    ap.add_argument("--safe-paths", type=int, default=0, choices=range(1, 8), metavar="R",
                    help="take the pair paths from the clearance-weighted exact planner (wa_grid_weighted_paths) instead of the colony: "
                         "entering a voxel costs 1 + the number of bands 1^2 .. R^2 (voxels squared) its distance to the metal lies within")
    ap.add_argument("--diagonal-paths", type=int, nargs="*", default=None, metavar="STEP",
                    help="take the pair paths from the exact planner with diagonal moves (wa_grid_chamfer_paths) instead of the colony: "
                         "three step costs for face, edge and corner moves, each 1 .. 16 (default 3 4 5)")
    ap.add_argument("--safe-gain", type=int, default=None, metavar="G",
                    help="--safe-paths R together with --diagonal-paths (wa_grid_chamfer_weighted_paths): entering a voxel adds G per band "
                         "it lies within to the move's step cost (default: the face step); G * R is at most 31")
    ap.add_argument("--fit", type=int, nargs="?", const=6, default=None, choices=range(0, 9), metavar="MAX_LEVEL",
                    help="needs --shortcut: the trajectory is wa_grid_fit_trajectory's (control points on the waypoints' polyline, refined "
                         "leg by leg up to MAX_LEVEL until the sampled curve clears the metal) instead of the cubic through the waypoints")
    ap.add_argument("--retime", action="store_true",
                    help="re-time the trajectory's samples on the device (wa_traj_retime): rest to rest under --retime-limits, slow near the metal "
                         "and round bends, and the positions every --retime-tick seconds, checked against the metal")
    ap.add_argument("--retime-limits", type=float, nargs=6, default=[10.0, 20.0, 20.0, 10.0, 2.0, 4.0],
                    metavar=("V_MAX", "ACC", "DEC", "A_LAT", "V_NEAR", "NEAR_D2"),
                    help="--retime: coordinate units per s, per s^2 (up), per s^2 (down), per s^2 (lateral), per s where the distance field is <= NEAR_D2 (voxels squared)")
    ap.add_argument("--retime-tick", type=float, default=0.001, help="--retime: the controller period in seconds")
    ap.add_argument("--fit-dump", default=None, help="--fit: write the fitted polyline (n x 3 float32) to this .npy file")
    ap.add_argument("--seams", action="store_true",
                    help="points 2k and 2k+1 are the two ends of weld seam k: order AND direction of the seams by wa_gtsp_seam_tour, started from "
                         "the seam-level ACS-TSP tour; the exact tour beside it up to 16 seams")
    ap.add_argument("--jerk", type=float, default=None, metavar="J",
                    help="--retime, or --seams --weld-passes: jerk-limited controller ticks (wa_traj_retime_jerk): a moving average along the arc "
                         "length over the window that bounds the jerk by J (coordinate units per s^3), caps lowered over its reach, dwells "
                         "extended; reported under jerk")
    ap.add_argument("--weld-passes", type=float, nargs=3, default=None, metavar=("V", "T_START", "T_END"),
                    help="--seams: time the stitched polyline with the weld passes in it (wa_traj_retime_stops): the torch stops T_START seconds "
                         "where it enters a seam, welds at no more than V, stops T_END seconds where it leaves; --retime-limits and "
                         "--retime-tick apply; reported under weld_passes")
    ap.add_argument("--seam-before", metavar="A:B[,A:B...]",
                    help="--seams: seam A is welded before seam B (a tack before its seam, a root pass before its fill); the tour then comes "
                         "from wa_gtsp_seam_tour_rules and the JSON gains seam_rules (what the free tour breaks, both costs)")
    ap.add_argument("--seam-fixed", metavar="S:D[,S:D...]",
                    help="--seams: seam S is welded one way only, D = 0 from its even point, D = 1 from its odd point")
    ap.add_argument("--seam-starts", type=int, default=1024, help="--seams: descents of the local search (start 0 is the ACS-TSP tour)")
    ap.add_argument("--torch", type=int, nargs="?", const=64, default=None, metavar="K",
                    help="after --fit or --retime: the torch axis at every sample of the trajectory, one of K directions (1 .. 256) of a cone "
                         "around +z, so that the torch body clears the metal (wa_traj_tool_axes); prints the summary and the check of the "
                         "interpolated axes between samples")
    ap.add_argument("--jerk-poses", action="store_true",
                    help="--jerk J with --tick-poses OMEGA: the torch axes at the jerk-limited ticks (wa_traj_retime_jerk_axes) -- the smoothed "
                         "axes and their speed limit as for --tick-poses, then one call that times, filters and gives every filtered tick "
                         "its checked axis; reported under jerk_poses")
    ap.add_argument("--tick-poses", type=float, nargs="+", default=None, metavar=("OMEGA", "H"),
                    help="--retime --torch K: the torch axis at every controller tick, on the device: the chosen directions smoothed over windows "
                         "of half-width H along the path (default: 8 voxels) where the body stays clear, the timing limited to OMEGA (chord of "
                         "the unit axes per second), the axes interpolated per tick and checked against the metal; reported under tick_poses")
    ap.add_argument("--torch-grid", type=int, nargs="?", const=1, default=None, metavar="MIN_DIRS",
                    help="with --torch K: plan on the torch-fit grid (wa_grid_tool_fit), whose free voxels leave the torch body at least MIN_DIRS "
                         "(default 1) of the K directions; around every weld point the voxels within --torch-keep-r2 (squared voxels) stay as "
                         "they are.  With --safe-paths and --diagonal-paths the penalties of wa_grid_tool_penalties (thresholds K/8, K/4, K/2, "
                         "each worth --safe-gain) are added to the clearance penalties, the sum clamped at 31.  --torch then also runs on the "
                         "plain trajectory (no --fit / --retime needed).  MIN_DIRS 0 is the comparison run: the planning grid and the penalties "
                         "are left as they are, everything else is reported alike")
    ap.add_argument("--pose-paths", type=int, default=None, metavar="MAX_TURN",
                    help="with --torch K: take the pair paths from the exact search over (voxel, torch direction) (wa_grid_pose_paths): every "
                         "node of a path has one of the K directions open, and from node to node the torch turns by at most MAX_TURN (the "
                         "measure U of wa_traj_tool_axes, 0 .. 3145728; -1: no limit).  Pairs without such a path are reported and left out, "
                         "as with --geodesic; --torch then runs on the finished trajectory with the same limit and the line carries its "
                         "n_no_dir and n_over_turn.  --shortcut alone leaves the planned voxels and so drops the guarantee; add --pose-shortcut")
    ap.add_argument("--pose-turn-costs", nargs=2, default=None, metavar=("HOP", "U1=C1[,U2=C2...]"),
                    help="needs --pose-paths: the pair paths come from wa_grid_pose_weighted_paths -- a step costs HOP (1 .. 8), plus C1 when "
                         "it turns the torch by more than U1, C2 by more than U2, ... (at most 4 ascending bands, costs non-decreasing, at most "
                         "15); the pair costs stay what they are.  With it --safe-paths G may be combined with --pose-paths: entering a "
                         "voxel then adds min(15, its clearance cost - 1) with bands at 1^2 .. G^2.  pose_paths.planners reports hops, "
                         "direction changes and the sum of U per planner")
    ap.add_argument("--pose-diagonal", type=int, nargs="*", default=None, metavar="STEP",
                    help="needs --pose-paths: the pair paths come from wa_grid_pose_diag_paths, which moves on the 26-neighbour lattice -- "
                         "a face, edge and corner move cost F E C (three integers 1 .. 16, default 3 4 5), a diagonal move keeps the torch "
                         "direction and needs it open in every voxel of the box it spans.  With --pose-turn-costs HOP must equal F, and the "
                         "bands and costs apply to face moves.  pose_diagonal reports times, nodes, moves by class and lengths beside the "
                         "totals of the staircase planner it replaces")
    ap.add_argument("--pose-shortcut", action="store_true",
                    help="needs --pose-paths and --shortcut: the waypoints and costs of the pair paths come from wa_grid_pose_shortcut, which "
                         "straightens a stretch only where a planned direction stays open along the whole segment and keeps MAX_TURN at the "
                         "waypoints; pose_paths.shortcut reports the held and unheld segments and the length beside the plain shortcut's")
    ap.add_argument("--pose-fit", action="store_true",
                    help="needs --pose-paths, --shortcut, --pose-shortcut and --fit: the trajectory comes from wa_grid_pose_fit_trajectory, "
                         "which refines the spline until one of the holds of --pose-shortcut stays open along every piece of the sampled "
                         "curve; its summary stands beside the plain fit's, and --torch takes the directions it found as wishes")
    ap.add_argument("--torch-keep-r2", type=int, default=16, metavar="R2",
                    help="--torch-grid: the squared radius in voxels of the bubble around every weld point inside which the grid is kept (default 16)")
    args = ap.parse_args()
    if args.torch_grid is not None and args.torch is None:
        ap.error("--torch-grid needs the directions of --torch K")
    if args.torch_grid is not None and not 0 <= args.torch_grid <= (args.torch or 0):
        ap.error("--torch-grid takes 0 .. K directions")
    if args.torch_keep_r2 < 0:
        ap.error("--torch-keep-r2 is at least 0")
    if args.pose_paths is not None:
        if args.torch is None:
            ap.error("--pose-paths needs the directions of --torch K")
        if not -1 <= args.pose_paths <= 3 << 20:
            ap.error("--pose-paths takes -1 or 0 .. 3145728")
        if args.exact_paths or (args.safe_paths and args.pose_turn_costs is None) or args.diagonal_paths is not None or args.geodesic:
            ap.error("--pose-paths is a pair planner of its own: not with --exact-paths, --safe-paths (without --pose-turn-costs), "
                     "--diagonal-paths or --geodesic")
    pose_turn_costs = None
    if args.pose_turn_costs is not None:
        if args.pose_paths is None:
            ap.error("--pose-turn-costs needs --pose-paths")
        try:
            bands = [tuple(int(v) for v in b.split("=")) for b in args.pose_turn_costs[1].split(",")]
            pose_turn_costs = (int(args.pose_turn_costs[0]), [u for u, _ in bands], [0] + [c for _, c in bands])
        except ValueError:
            ap.error("--pose-turn-costs takes HOP and U1=C1[,U2=C2...] in integers")
        if len(bands) > 4:
            ap.error("--pose-turn-costs takes at most 4 bands")
    pose_diagonal = None
    if args.pose_diagonal is not None:
        if args.pose_paths is None:
            ap.error("--pose-diagonal needs --pose-paths")
        if len(args.pose_diagonal) not in (0, 3) or not all(1 <= v <= 16 for v in args.pose_diagonal):
            ap.error("--pose-diagonal takes no values (3 4 5) or the three steps F E C, each 1 .. 16")
        pose_diagonal = list(args.pose_diagonal) or [3, 4, 5]
        if pose_turn_costs is not None and pose_turn_costs[0] != pose_diagonal[0]:
            ap.error("--pose-diagonal with --pose-turn-costs: HOP (%d) must equal the face step F (%d)" % (pose_turn_costs[0], pose_diagonal[0]))
        if pose_turn_costs is not None and not 1 <= pose_turn_costs[0] <= 8:
            ap.error("--pose-turn-costs takes a HOP of 1 .. 8")
    if args.pose_shortcut and (args.pose_paths is None or not args.shortcut):
        ap.error("--pose-shortcut needs --pose-paths and --shortcut")
    if args.pose_fit and (not args.pose_shortcut or args.fit is None):
        ap.error("--pose-fit needs --pose-paths, --shortcut, --pose-shortcut and --fit")
    if args.torch is not None and args.fit is None and not args.retime and args.torch_grid is None and args.pose_paths is None:
        ap.error("--torch works on the samples of --fit or --retime")
    if args.tick_poses is not None and (len(args.tick_poses) > 2 or not args.retime or args.torch is None):
        ap.error("--tick-poses takes OMEGA and optionally H, and needs --retime and --torch K")
    if args.torch is not None and not 1 <= args.torch <= 256:
        ap.error("--torch takes 1 .. 256 directions")
    if args.diagonal_paths is not None:
        args.diagonal_paths = args.diagonal_paths or [3, 4, 5]
        if len(args.diagonal_paths) != 3 or not all(1 <= v <= 16 for v in args.diagonal_paths):
            ap.error("--diagonal-paths takes three step costs in 1 .. 16")
    both = bool(args.safe_paths) and args.diagonal_paths is not None
    if both:
        if args.safe_gain is None:
            args.safe_gain = args.diagonal_paths[0]
        if args.safe_gain < 0 or args.safe_gain * args.safe_paths > 31:
            ap.error("--safe-gain times --safe-paths is at most 31 (WA_PEN_MAX)")
    if args.fit is not None and not args.shortcut:
        ap.error("--fit needs the waypoints of --shortcut")
    if args.seams and (args.points % 2 or args.points < 2):
        ap.error("--seams needs an even number of --points (two per seam)")
    if args.jerk_poses and (args.jerk is None or args.tick_poses is None):
        ap.error("--jerk-poses needs --jerk J and --tick-poses OMEGA")
    if args.jerk is not None:
        if args.tick_poses is not None and not args.jerk_poses:
            ap.error("--jerk with --tick-poses needs --jerk-poses: the ticks of --tick-poses are the unfiltered ones, the torch axes at "
                     "the jerk-limited ticks are --jerk-poses'")
        if not args.retime and args.weld_passes is None:
            ap.error("--jerk needs --retime, or --seams --weld-passes")
        if not (args.jerk > 0 and np.isfinite(args.jerk)):
            ap.error("--jerk takes a jerk limit > 0")
    if args.seams and (args.fit is not None or args.retime):
        ap.error("--seams does not go together with --fit / --retime yet (--weld-passes times a tour of seams)")
    seam_rules = parse_seam_rules(ap, args)
    if args.weld_passes is not None:
        if not args.seams:
            ap.error("--weld-passes needs the seams of --seams")
        v, ts, te = args.weld_passes
        if not (np.isfinite([v, ts, te]).all() and v > 0 and ts >= 0 and te >= 0):
            ap.error("--weld-passes takes a weld speed > 0 and two dwells >= 0")
    rank, local_rank, world = wd.env_rank()
    ctx = api.Context(local_rank)
    comm = None
    if world > 1 or os.environ.get("WA_FORCE_DIST") == "1":
        uid = wd.ship_unique_id(rank, world, api.Comm.unique_id)      # 128 bytes from rank 0 over a socket: no torch, no MPI
        comm = api.Comm(ctx, rank, world, np.frombuffer(uid, np.uint8))
        comm.barrier()
    wait_for_device_memory(ctx)
    n = args.grid
    if comm is None or rank == 0:
        free, cx, cy, cz, prec, wall = synth.synth_grid(n, seed=2024, occ_prob=0.10)
        grid = api.Grid.from_occupancy(ctx, free, cx, cy, cz, prec, wall)
    else:
        grid = None
    if comm is not None:
        # ONE rank builds the grid (with a mesh that is the O(triangles x voxels) voxelisation, model_grid_map.hpp:223-268), the others
        # receive a replica: occupancy + axis tables by ncclBroadcast (wa_comm_broadcast_grid)
        grid = comm.broadcast_grid(grid, root=0)
        if rank != 0:
            free = grid.occupancy()
    pts = synth.synth_weld_points(free, n, args.points, seed=args.seed)
    predict = float(0.35 ** -1 * 24)  # 24 ants per search at precision 1 (ACSRank_3D.hpp:247)
    metal = grid
    if args.clearance is not None:
        # plan with a safety margin: every voxel nearer the metal than the radius becomes an obstacle, except around the weld points
        grid = metal.inflate(metal.clearance_radius(args.clearance), pts)
    torch_grid, extra_pen = None, None
    if args.torch_grid is not None:
        # plan where the torch body fits: the bead rule of --torch for every voxel, before any path is planned
        t_tg = time.perf_counter()
        base = grid
        tool, dirs, _ = torch_tool_and_cone(metal, args.torch)
        _, count, reach_summary = base.torch_reach(dirs, tool, masks=False)
        torch_grid = dict(min_dirs=args.torch_grid, keep_r2=args.torch_keep_r2, reach=reach_summary, free_voxels=base.n_free)
        if args.torch_grid > 0:
            grid = base.torch_fit(dirs, tool, args.torch_grid, pts, args.torch_keep_r2)
            torch_grid.update(free_voxels_fit=grid.n_free)
            if both:
                K, rep = args.torch, max(1, min(args.safe_gain, 10))
                thr = [t for t in (max(1, K // 8), max(1, K // 4), max(1, K // 2)) for _ in range(rep)]
                extra_pen = base.torch_penalties(dirs, tool, thr).astype(np.int64)
                torch_grid.update(penalty_thresholds=thr)
        torch_grid.update(t_grid_s=time.perf_counter() - t_tg)
    hop_matrix, unreachable = None, []
    if args.geodesic:
        t_geo = time.perf_counter()
        hop_matrix = grid.geodesic_matrix(pts)
        t_geo = time.perf_counter() - t_geo
        unreachable = [(i, j) for i in range(args.points) for j in range(i + 1, args.points) if hop_matrix[i, j] == api.WA_HOPS_NONE]
    paths_without = None
    if torch_grid is not None and args.torch_grid > 0 and comm is None:
        # the same exact planner on the grid as it was, for the cost of the detour (the colony is not run twice)
        if both:
            paths_without = plan_safe_diagonal(base, pts, args.safe_paths, args.diagonal_paths, args.safe_gain)[1]
        elif args.safe_paths and args.pose_paths is None:
            paths_without = plan_safe(base, pts, args.safe_paths)[1]
        elif args.diagonal_paths is not None:
            paths_without = plan_diagonal(base, pts, args.diagonal_paths)[1]
        elif args.exact_paths:
            paths_without = plan_exact(base, pts)[1]
    t0 = time.perf_counter()
    if args.pose_paths is not None:
        pose_tool, pose_dirs, _ = torch_tool_and_cone(metal, args.torch)
        pose_costs, pose_diag = None, None
        if pose_turn_costs is not None:
            pen = None
            if args.safe_paths:
                pen = np.clip(grid.clearance_costs([k * k for k in range(1, args.safe_paths + 1)]).astype(np.int32) - 1, 0, 15).astype(np.uint8)
            pose_costs = api.pose_costs(*pose_turn_costs, pen)
            if pose_diagonal is not None:
                pose_diag = api.pose_diag_costs(pose_diagonal, pose_turn_costs[1], pose_turn_costs[2], pen)
        elif pose_diagonal is not None:
            pose_diag = api.pose_diag_costs(pose_diagonal, [], [0])
        cost, paths, n_mine = plan_pose(grid, pts, pose_dirs, pose_tool, args.pose_paths, rank, world, shortcut=args.max_span if args.shortcut else 0,
                                        pose_shortcut=args.pose_shortcut, costs=pose_costs, diag=pose_diag)
    elif both:
        cost, paths, n_mine = plan_safe_diagonal(grid, pts, args.safe_paths, args.diagonal_paths, args.safe_gain, rank, world,
                                                 shortcut=args.max_span if args.shortcut else 0, extra_pen=extra_pen)
    elif args.safe_paths:
        cost, paths, n_mine = plan_safe(grid, pts, args.safe_paths, rank, world, shortcut=args.max_span if args.shortcut else 0)
    elif args.diagonal_paths is not None:
        cost, paths, n_mine = plan_diagonal(grid, pts, args.diagonal_paths, rank, world, shortcut=args.max_span if args.shortcut else 0)
    elif args.exact_paths:
        cost, paths, n_mine = plan_exact(grid, pts, rank, world, shortcut=args.max_span if args.shortcut else 0)
    elif args.geodesic:
        cost, paths, n_mine = plan(ctx, grid, pts, args.generations, predict, args.seed, args.slots, rank, world, lazy=args.lazy, neighbourhood=args.neighbourhood,
                                   shortcut=args.max_span if args.shortcut else 0, skip=unreachable)
    else:
        cost, paths, n_mine = plan(ctx, grid, pts, args.generations, predict, args.seed, args.slots, rank, world, lazy=args.lazy, neighbourhood=args.neighbourhood,
                                   shortcut=args.max_span if args.shortcut else 0)
    short = plan.last_shortcut
    if args.pose_fit and comm is not None:
        raise SystemExit("--pose-fit runs on one GPU: the holds are not gathered")
    if comm is not None:
        # every pair is owned by exactly one rank: its cost goes to every rank, its path to rank 0 (the library's own collectives)
        P = args.points
        pair_list = [(i, j) for i in range(P) for j in range(i + 1, P)]
        index_of = {ij: k for k, ij in enumerate(pair_list)}
        mine = sorted(index_of[ij] for ij in paths)
        vec = comm.allgather_costs(mine, [cost[pair_list[k]] for k in mine], len(pair_list))
        cost = np.zeros((P, P), np.float64)
        for k, (i, j) in enumerate(pair_list):
            cost[i, j] = cost[j, i] = vec[k]
        gathered = comm.gather_paths({k: paths[pair_list[k]] for k in mine}, root=0)
        paths = {pair_list[k]: ids for k, ids in gathered.items()}    # rank 0: all of them; elsewhere empty
        if args.shortcut:
            gathered = comm.gather_paths({k: short[pair_list[k]] for k in mine}, root=0)
            short = {pair_list[k]: ids for k, ids in gathered.items()}
    t_pairs = time.perf_counter() - t0
    finite = np.isfinite(cost).all()
    t_pairs -= plan.last_create_s
    out = dict(grid=n, points=args.points, neighbourhood=args.neighbourhood, slots=plan.last_slots, lazy_evaporation=bool(args.lazy), t_solver_create_s=plan.last_create_s, pairs=args.points * (args.points - 1) // 2, world=world,
               pairs_this_rank=n_mine, t_pairs_s=t_pairs, all_reached=bool(finite))
    if args.exact_paths:
        out.update(exact_paths=True)
    if args.pose_paths is not None and rank == 0:
        gone = [[i, j] for i in range(args.points) for j in range(i + 1, args.points) if not np.isfinite(cost[i, j])]
        out.update(pose_paths=dict(max_turn=args.pose_paths, K=args.torch, unreachable_pairs=gone, reachable_pairs=out["pairs"] - len(gone),
                                   nodes_total=int(sum(len(p) for p in paths.values())), planners=plan_pose.last_totals))
        if pose_turn_costs is not None:
            out["pose_paths"].update(turn_costs=dict(hop=pose_turn_costs[0], bands=pose_turn_costs[1], costs=pose_turn_costs[2],
                                                     safe_paths=args.safe_paths or 0))
        if plan_pose.last_pose_shortcut is not None:
            out["pose_paths"].update(shortcut=plan_pose.last_pose_shortcut)
        if plan_pose.last_diagonal is not None:
            out.update(pose_diagonal=plan_pose.last_diagonal)
    if torch_grid is not None and rank == 0:
        out.update(torch_grid=dict(torch_grid, paths=torch_grid_report(base, count, paths, paths_without, args.max_span if args.shortcut else 0)))
    if rank == 0 and args.geodesic:
        # every search against the optimum: a lattice path of len nodes has len - 1 steps, never fewer than the hop count
        gone = set(unreachable)
        ratios, at_opt, left = [], 0, []
        for (i, j), ids in sorted(paths.items()):
            if (i, j) in gone:
                continue
            if not np.isfinite(cost[i, j]):
                left.append([i, j])
                continue
            steps, h = len(ids) - 1, int(hop_matrix[i, j])
            at_opt += steps == h
            ratios.append(steps / h if h else 1.0)
        out.update(geodesic=dict(t_matrix_s=t_geo, unreachable_pairs=[list(ij) for ij in unreachable], reachable_pairs=out["pairs"] - len(unreachable),
                                 searches_at_optimum=int(at_opt), ratio_mean=float(np.mean(ratios)) if ratios else None,
                                 ratio_max=float(np.max(ratios)) if ratios else None, left_at_inf=left))
    if rank == 0 and finite:
        t1 = time.perf_counter()
        if args.seams:
            info, order, dirs = seam_stage(ctx, cost, args.seed, args.seam_starts, seam_rules)
            out.update(info, t_seams_s=time.perf_counter() - t1, pair_generations_per_s=out["pairs"] * args.generations / t_pairs)
            # every seam is a two-node segment walked in its chosen direction; between two seams the pair path from where the torch
            # leaves one to where it enters the next (the way back to the first seam is not stitched, as without --seams)
            ins = [2 * s + x for s, x in zip(order, dirs)]
            edges = [(a ^ 1, b) for a, b in zip(ins[:-1], ins[1:])]
            rev = []
            for k, d in enumerate(dirs):
                rev.append(int(d))                            # a seam is stored even end first
                if k < len(edges):
                    rev.append(1 if edges[k][0] > edges[k][1] else 0)   # pair paths are stored i<j

            def seg_list(table):
                segs = []
                for k, s in enumerate(order):
                    segs.append(np.array([pts[2 * s], pts[2 * s + 1]], np.int64))
                    if k < len(edges):
                        a, b = edges[k]
                        segs.append(table[(min(a, b), max(a, b))])
                return segs
        else:
            tour = api.gtsp_solve(ctx, cost, mode=api.RNG_DEV, seed=args.seed)
            out.update(tour_cost=float(tour["L"][0]), tour_iterations=int(tour["iters"][0]),
                       order=[int(e[0]) for e in tour["edges"][0]], t_gtsp_s=time.perf_counter() - t1,
                       pair_generations_per_s=out["pairs"] * args.generations / t_pairs)
            edges = tour["edges"][0][:-1]
            rev = [1 if a > b else 0 for a, b in edges]          # stored i<j; walk them in tour direction

            def seg_list(table):
                return [table[(min(a, b), max(a, b))] for a, b in edges]
        # main.cpp:283-352: stitch the tour's segments (rank 0 holds every path), then the two smoothing passes, all on the device
        t2 = time.perf_counter()
        segs = seg_list(paths)
        wsegs = seg_list(short) if args.shortcut else None
        traj, ok, info = smooth(ctx, grid, segs, wsegs, rev, fit=(metal, args.fit, args.fit_dump) if args.fit is not None else None,
                                pose_fit=(pose_dirs, pose_tool, seg_list(plan_pose.last_holds)) if args.pose_fit else None)
        out.update(info, t_trajectory_s=time.perf_counter() - t2)
        if args.weld_passes is not None:
            t6 = time.perf_counter()
            out.update(weld_passes=weld_pass_stage(ctx, metal, wsegs if args.shortcut else segs, rev, *args.weld_passes, args.retime_limits,
                                                   args.retime_tick, args.jerk),
                       t_weld_passes_s=time.perf_counter() - t6)
        if args.retime:
            # what the controller is sent: the same curve at a fixed period, as fast as the limits allow
            t3 = time.perf_counter()
            v_max, acc, dec, a_lat, v_near, near_d2 = args.retime_limits
            curve = api.Trajectory.from_points(ctx, traj[ok.astype(bool)])
            kw = dict(a_lat=a_lat, grid=metal, v_near=v_near, near_d2=int(near_d2))
            if args.jerk is not None:   # (the retime entry describes the underlying profile, the jerk entry the ticks)
                _, _, _, _, plain = curve.retime(v_max, acc, dec, args.retime_tick, ticks=False, **kw)
                _, _, _, ticks, _, _, rs, _, sj = curve.retime_jerk(v_max, acc, dec, args.retime_tick,
                                                                    api.jerk_window(acc, dec, args.jerk, args.retime_tick), **kw)
                out.update(jerk=jerk_report(ctx, metal, sj, ticks, args.retime_tick, plain["n_ticks"], plain["time_q"], args.jerk))
            else:
                _, _, _, ticks, rs = curve.retime(v_max, acc, dec, args.retime_tick, **kw)
            out.update(retime=dict(duration_s=rs["time_q"] / api.RETIME_Q, length=rs["length_q"] / api.RETIME_Q, n_ticks=rs["n_ticks"],
                                   tick_s=args.retime_tick, peak_speed=float(np.sqrt(rs["peak_w_q"] / api.RETIME_Q)),
                                   n_bound=dict(zip(("end", "v_max", "curvature", "clearance"), rs["n_bound"])),
                                   n_on_cap=rs["n_on_cap"], n_on_ramp=rs["n_on_ramp"], n_triangle=rs["n_triangle"],
                                   samples_clearance=curve.clearance(metal)[3],
                                   ticks_clearance=ticks.clearance(metal)[3] if ticks is not None else None,   # (None: more than 2^31 ticks)
                                   limits=dict(v_max=v_max, acc=acc, dec=dec, a_lat=a_lat, v_near=v_near, near_d2=int(near_d2))),
                       t_retime_s=time.perf_counter() - t3)
        if args.torch is not None:
            t4 = time.perf_counter()
            cx, cy, cz = metal.coords()
            first = np.asarray([(seg[-1] if r else seg[0]) for seg, r in zip(segs, rev)] + [segs[-1][0] if rev[-1] else segs[-1][-1]], np.int64)
            stops = np.stack([cx[first % metal.nx], cy[(first // metal.nx) % metal.ny], cz[first // (metal.nx * metal.ny)]], 1)
            turn = args.pose_paths if args.pose_paths is not None else -1
            want = None
            if args.pose_fit:
                # the same stage on the plain fit's samples first, then on the pose fit's with the directions it found as wishes
                before = torch_stage(ctx, metal, np.ascontiguousarray(smooth.fit_samples, np.float32), stops, args.torch, turn)
                out["pose_fit"].update(n_no_dir_plain_fit=before["n_no_dir"], n_over_turn_plain_fit=before["n_over_turn"])
                per_sample = np.concatenate([smooth.seg_dir, smooth.seg_dir[-1:]])
                want = np.where(per_sample[:, None] >= 0, pose_dirs[np.maximum(per_sample, 0)], 0).astype(np.float32)
            out.update(torch=torch_stage(ctx, metal, np.ascontiguousarray(traj[ok.astype(bool)], np.float32), stops, args.torch, turn, want),
                       t_torch_s=time.perf_counter() - t4)
            if args.pose_paths is not None:
                out.update(n_no_dir=out["torch"]["n_no_dir"], n_over_turn=out["torch"]["n_over_turn"])
            if args.jerk_poses:
                t5 = time.perf_counter()
                h = args.tick_poses[1] if len(args.tick_poses) > 1 else 8.0 * float(metal.precision)
                out.update(jerk_poses=jerk_pose_stage(ctx, metal, np.ascontiguousarray(traj[ok.astype(bool)], np.float32), args.retime_limits,
                                                      args.retime_tick, args.tick_poses[0], h, args.jerk),
                           t_jerk_poses_s=time.perf_counter() - t5)
            elif args.tick_poses is not None:
                t5 = time.perf_counter()
                h = args.tick_poses[1] if len(args.tick_poses) > 1 else 8.0 * float(metal.precision)
                out.update(tick_poses=tick_pose_stage(ctx, metal, np.ascontiguousarray(traj[ok.astype(bool)], np.float32), args.retime_limits,
                                                      args.retime_tick, args.tick_poses[0], h, out["retime"]["duration_s"]),
                           t_tick_poses_s=time.perf_counter() - t5)
        if both:
            q = safe_diagonal_report(grid, metal, pts, paths, args.max_span if args.shortcut else 0)
            if args.shortcut:
                # as safe_paths' n_hit: segments of the cubic through the tour's waypoints that cut the metal (without --fit's refinement)
                ptraj, pok = smooth.plain if args.fit is not None else (traj, ok)
                q.update(n_hit_cubic=int(api.Trajectory.from_points(ctx, ptraj[pok.astype(bool)]).clearance(metal)[3]["n_hit"]))
            out.update(safe_diagonal_paths=q)
        if args.safe_paths and not both and args.pose_paths is None:   # (with --pose-paths the penalties feed --pose-turn-costs)
            # what the soft margin buys and costs, against the hop-optimal paths of the same pairs in the same seam order: steps over
            # the optimum, path nodes inside the outermost band, and (--shortcut) segments of the smoothed curve that cut the metal
            P = args.points
            ii, jj = np.triu_indices(P, 1)
            hop_matrix_all = grid.geodesic_matrix(pts)
            _, hop_paths = api.geodesic_paths(grid, pts[ii], pts[jj])
            hop_paths = {(int(i), int(j)): (np.zeros(0, np.int64) if p is None else p) for i, j, p in zip(ii, jj, hop_paths)}
            d2 = metal.distance_field()
            r2 = args.safe_paths ** 2
            within = lambda ps, lim=r2: int(sum((d2[np.asarray(p, np.int64)] <= lim).sum() for p in ps))
            reach = [ij for ij in sorted(paths) if len(paths[ij])]
            q = dict(plan.last_safe, nodes_total=int(sum(len(paths[ij]) for ij in reach)),
                     extra_steps_total=int(sum(len(paths[ij]) - 1 - int(hop_matrix_all[ij]) for ij in reach)),
                     nodes_within_bands=within(paths[ij] for ij in reach), nodes_within_bands_hop_optimal=within(hop_paths[ij] for ij in reach),
                     nodes_next_to_metal=within((paths[ij] for ij in reach), 1), nodes_next_to_metal_hop_optimal=within((hop_paths[ij] for ij in reach), 1))
            if args.shortcut:
                hsegs = seg_list(hop_paths)
                hw = api.shortcut_paths(grid, hsegs, args.max_span)[0]
                htraj, hok, _ = smooth(ctx, grid, hsegs, hw, rev)
                n_hit = lambda t, k: int(api.Trajectory.from_points(ctx, t[k.astype(bool)]).clearance(metal)[3]["n_hit"])
                # (n_hit stays what it is without --fit, the cubic through the waypoints; the fit's own figure is under "fit")
                ptraj, pok = smooth.plain if args.fit is not None else (traj, ok)
                q.update(n_hit=n_hit(ptraj, pok), n_hit_hop_optimal=n_hit(htraj, hok))
            out.update(safe_paths=q)
        if args.diagonal_paths is not None and not args.safe_paths:
            out.update(diagonal_paths=diagonal_report(grid, pts, paths, short, args.max_span if args.shortcut else 0))
        if args.clearance is not None:
            # the curve the robot follows, against the real obstacles: how close it comes, and whether it cuts through any
            final = api.Trajectory.from_points(ctx, traj[ok.astype(bool)])
            summary = final.clearance(metal)[3]
            summary["min_distance"] = float(np.sqrt(summary["min_d2"]) * metal.precision) if summary["min_d2"] != api.WA_D2_NONE else None
            out.update(clearance=args.clearance, clearance_radius_voxels=metal.clearance_radius(args.clearance),
                       free_voxels_inflated=grid.n_free, free_voxels=metal.n_free, trajectory_clearance=summary)
    if rank == 0:
        print(json.dumps(out))
    if comm is not None:
        comm.barrier()
        comm.close()


if __name__ == "__main__":
    main()
