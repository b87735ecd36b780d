"""The torch-axis rules of include/weldacs.h on the CPU: tests/torch_ref.py (the restatement the GPU tests compare with, a dynamic
programme) against the exhaustive enumeration of every sequence, and hand cases whose answer is known without either."""
import numpy as np
import pytest

import torch_ref as T

X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def wall_grid():
    """16^3, unit axes, metal = the slab x in 10..11"""
    free = np.ones((16, 16, 16), np.uint8)
    free[:, :, 10:12] = 0
    return T.make_grid(free, (16, 16, 16))


@pytest.mark.parametrize("seed", range(40))
def test_dynamic_programme_against_every_sequence(seed):
    rs = np.random.RandomState(seed)
    K, n = int(rs.randint(1, 4)), int(rs.randint(1, 6))
    grid = T.boxes_grid(rs, 12, 6)
    xyz = rs.uniform(1, 10, (n, 3)).astype(np.float32)
    dirs = rs.normal(size=(K, 3)).astype(np.float32)
    w = T.weights(int(rs.randint(0, 1025)), int(rs.randint(0, 1025)), int(rs.randint(0, 1025)), int(rs.choice([-1, 2, 9])),
                  int(rs.choice([-1, 1 << 12, 1 << 16])))
    want = rs.normal(size=(n, 3)).astype(np.float32) if seed % 2 else None
    pf, pl = (int(rs.randint(-1, K)), int(rs.randint(-1, K))) if seed % 3 else (-1, -1)
    r = T.plan(grid, xyz, dirs, T.rod(4, 16 * 5, 2), w, want, None, [pf], [pl])
    best, arg = T.brute_force(r["N"], r["T"], pf, pl)
    assert int(r["leg_cost"][0]) == best
    assert T.sequence_cost(r["N"], r["T"], r["dir"], pf, pl) == best and tuple(r["dir"]) in arg
    assert r["summary"]["cost"] == (best if best < T.INF else 0)


def test_one_sample_with_two_different_pins_is_the_only_infinite_leg():
    grid = wall_grid()
    r = T.plan(grid, [[3, 3, 3]], [X, Y, Z], T.rod(2), T.weights(), pin_first=[0], pin_last=[2])
    assert r["leg_cost"][0] == T.INF and r["dir"][0] == 2 and r["summary"]["cost"] == 0
    r = T.plan(grid, [[3, 3, 3], [3, 3, 3]], [X, Y, Z], T.rod(2), T.weights(), pin_first=[0], pin_last=[2])
    assert r["leg_cost"][0] < T.INF and list(r["dir"]) == [0, 2]


def test_next_to_a_wall_the_body_tilts_away():
    grid = wall_grid()
    xyz = T.densify([[8, 2, 8], [8, 13, 8]], 20)
    tool = T.rod(6, 16 * 6, 1)
    r = T.plan(grid, xyz, [X, (-1, 0, 0), Z], tool, T.weights(1, 0, 1, 4))
    assert (r["feas"][:, 0] == 255).all() and (r["feas"][:, 1:] != 255).all()
    assert (r["dir"] != 0).all() and r["summary"]["n_chosen_blocked"] == 0 and r["summary"]["n_blocked_pairs"] == len(xyz)
    # the same axis given to the check: blocked everywhere; the one pointing away: nowhere
    b, _, s = T.check(grid, xyz, np.tile(np.float32(X), (len(xyz), 1)), tool, 4)
    assert b.all() and s["n_chosen_blocked"] == len(xyz) and s["first_chosen_blocked"] == 0
    b, _, s = T.check(grid, xyz, np.tile(np.float32([-1, 0, 0]), (len(xyz), 1)), tool, 4)
    assert not b.any() and s["first_chosen_blocked"] == -1


def test_weights_zero_and_equal_directions_give_index_zero():
    grid = wall_grid()
    xyz = T.densify([[2, 2, 2], [5, 12, 9]], 15)
    r = T.plan(grid, xyz, [(-1, 0, 0), Y, Z], T.rod(3, 16 * 3), T.weights(0, 0, 0), want=np.tile(np.float32(Z), (len(xyz), 1)))
    assert r["summary"]["n_blocked_pairs"] == 0 and (r["dir"] == 0).all() and r["leg_cost"][0] == 0
    r = T.plan(grid, xyz, [Z] * 7, T.rod(3, 16 * 3), T.weights(5, 7, 9, 50))       # the tie rule: the lowest index
    assert (r["dir"] == 0).all()


def test_wish_is_followed_and_a_zero_wish_costs_nothing():
    grid = T.make_grid(np.ones((8, 8, 8), np.uint8), (8, 8, 8))                      # no metal: WA_D2_NONE everywhere
    assert (grid[1] == T.D2_NONE).all()
    xyz = T.densify([[1, 1, 1], [6, 6, 6]], 9)
    want = np.zeros((10, 3), np.float32)
    want[5:] = Y
    r = T.plan(grid, xyz, [X, Y, Z], T.rod(64, 65536, 1 << 30), T.weights(1, 10, 0, 1 << 30), want=want)
    assert list(r["dir"]) == [0] * 5 + [1] * 5 and r["summary"]["n_blocked_pairs"] == 0
    # near: r2 + near_add = 2^31 is above WA_D2_NONE, so every bead inside the grid counts, by the letter of rule 2
    assert r["summary"]["n_chosen_near"] == 10


def test_pins_at_both_ends():
    grid = wall_grid()
    xyz = T.densify([[2, 2, 2], [2, 12, 2]], 11)
    r = T.plan(grid, xyz, [X, Y, Z], T.rod(2, 32), T.weights(0, 0, 3), pin_first=[2], pin_last=[1])
    assert r["dir"][0] == 2 and r["dir"][-1] == 1 and (np.diff(r["dir"]) != 0).sum() == 1      # one turn, as late or early as the tie rule says
    assert r["leg_cost"][0] == 3 * int(T.turn(T.quantise(Z), T.quantise(Y)))


def test_max_turn_forces_intermediate_directions():
    arc = [(np.cos(a), np.sin(a), 0) for a in np.linspace(0, np.pi, 5)]
    step = int(T.turn(T.quantise(arc[0]), T.quantise(arc[1])))
    grid = wall_grid()
    xyz5, xyz3 = T.densify([[2, 2, 2], [2, 6, 2]], 4), T.densify([[2, 2, 2], [2, 6, 2]], 2)
    w = T.weights(0, 0, 0, -1, step + 8)
    r = T.plan(grid, xyz5, arc, T.rod(1, 0, 0), w, pin_first=[0], pin_last=[4])
    assert list(r["dir"]) == [0, 1, 2, 3, 4] and r["summary"]["n_over_turn"] == 0 and r["leg_cost"][0] == 0
    r = T.plan(grid, xyz3, arc, T.rod(1, 0, 0), w, pin_first=[0], pin_last=[4])       # too few samples: the limit is paid for, not refused
    assert r["summary"]["n_over_turn"] >= 1 and r["leg_cost"][0] >= T.BLOCK and r["summary"]["max_turn_taken"] > step + 8
    r = T.plan(grid, xyz5, arc, T.rod(1, 0, 0), T.weights(0, 0, 0), pin_first=[0], pin_last=[4])
    assert r["summary"]["n_over_turn"] == 0 and r["leg_cost"][0] == 0                 # the limit off


def test_a_bead_that_leaves_the_grid_passes():
    free = np.ones((16, 16, 16), np.uint8)
    free[:, :, 15] = 0                                                               # metal = the last layer in x
    grid = T.make_grid(free, (16, 16, 16))
    xyz = np.float32([[13, 8, 8]])
    inside = (np.array([32]), np.array([0]))                                         # 2 voxels behind the tip: x = 15, on the metal
    outside = (np.array([64]), np.array([0]))                                        # 4 voxels: x = 17, outside
    assert T.plan(grid, xyz, [X], inside, T.weights())["feas"][0, 0] == 255
    assert T.plan(grid, xyz, [X], outside, T.weights())["feas"][0, 0] == 0
    # a sample outside the grid is clamped onto it and counted
    r = T.plan(grid, np.float32([[-3, 8, 8], [13, 20, 8]]), [X], outside, T.weights())
    assert r["summary"]["n_outside"] == 2


def test_floor_rule_for_negative_offsets():
    q = np.array([[-16384, 0, 16384]])
    o = T.offsets(q, [8, 9, 24, 25])
    assert o[0, :, 0].tolist() == [0, -1, -1, -2] and o[0, :, 2].tolist() == [1, 1, 2, 2]   # -0.5 -> 0 (floor(-0.5 + 0.5)), -0.5625 -> -1
    assert o[0, :, 0].tolist() == [(-16384 * d + (1 << 17)) // (1 << 18) for d in (8, 9, 24, 25)]
    free = np.ones((16, 16, 16), np.uint8)
    free[:, :, 4] = 0
    grid = T.make_grid(free, (16, 16, 16))
    xyz = np.float32([[5, 8, 8]])
    assert T.plan(grid, xyz, [(-1, 0, 0)], (np.array([8]), np.array([0])), T.weights())["feas"][0, 0] == 0     # offset 0: the tip's own voxel, free
    assert T.plan(grid, xyz, [(-1, 0, 0)], (np.array([9]), np.array([0])), T.weights())["feas"][0, 0] == 255         # offset -1: the metal


def test_quantisation():
    assert T.quantise((0, 0, 2)) == (0, 0, 16384) and T.quantise((3, 4, 0)) == (9830, 13107, 0)
    assert T.quantise((0, 0, 0)) is None and T.quantise((np.inf, 0, 1)) is None and T.quantise((np.nan, 0, 1)) is None
    assert T.quantise((1e30, 0, 0)) == (16384, 0, 0) and T.quantise((1e-45, 0, 0)) == (16384, 0, 0)
    assert int(T.turn((16384, 0, 0), (-16384, 0, 0))) == 1 << 20


def test_random_cases_cover_what_the_gpu_tests_need():
    """the seeded cases of the GPU suite, looked at on the CPU: each thing the GPU comparison is meant to meet is met by at least one
    of them -- blocked pairs, a sample with no direction left, chosen near and blocked directions, turns above the limit, samples
    outside, empty legs, pins on and off, and every kind of wish (none, partly zero, dense)"""
    seen = dict(blocked=0, no_dir=0, chosen_blocked=0, near=0, over=0, outside=0, empty=0, pins=0, no_pins=0, no_wish=0, part_wish=0,
                dense_wish=0)
    ks = set()
    for seed in T.RANDOM_SEEDS[:14]:
        c = T.random_case(seed)
        ks.add(len(c["dirs"]))
        if len(c["dirs"]) > 64 and len(c["xyz"]) > 60:
            continue                                                                 # (kept quick: the large ones run in the GPU suite)
        s = T.plan(**c)["summary"]
        zero_rows = 0 if c["want"] is None else int((c["want"] == 0).all(1).sum())
        seen["blocked"] += s["n_blocked_pairs"] > 0
        seen["no_dir"] += s["n_no_dir"] > 0
        seen["chosen_blocked"] += s["n_chosen_blocked"] > 0
        seen["near"] += s["n_chosen_near"] > 0
        seen["over"] += s["n_over_turn"] > 0
        seen["outside"] += s["n_outside"] > 0
        seen["empty"] += bool((np.diff(c["off"]) == 0).any())
        seen["pins"] += c["pin_first"] is not None
        seen["no_pins"] += c["pin_first"] is None
        seen["no_wish"] += c["want"] is None
        seen["part_wish"] += c["want"] is not None and zero_rows > 0
        seen["dense_wish"] += c["want"] is not None and zero_rows == 0
    assert all(v >= 1 for v in seen.values()) and seen["blocked"] >= 2 and len(ks) >= 4, (seen, ks)
