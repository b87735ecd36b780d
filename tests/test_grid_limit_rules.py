"""The largest grids the library accepts, mirrored from welding_robot_amd/csrc and include/weldacs.h.  tests/test_gpu_grid_limits.py
creates grids and solvers at every limit and one voxel past it, and compares walks near the top of each size range with the oracle; it
takes its sizes from this table.  If a constant or a comparison moves in the source, this test fails, and the GPU cases must move with it.

  nb6_bound     wa_acs_create, 6 neighbours: the walk addresses a slot's field with signed 32-bit byte offsets (24 B per voxel)
  nb26_ids      WaNbT<26>: a path word is a 27-bit voxel id + the 5-bit edge index
  nb26_bound    wa_acs_create, 26 neighbours: ids 0 .. IDM fit the id field
  nb26_fast     k_walk_dev26's fast loop: 32-bit byte offsets into 104-byte records, only while the field is below 2^31 bytes
  nb26_record   ... the offsets it forms (cur * 104 + the lane's edge)
  id_mask       WA_ID_MASK: a 6-neighbour path word's voxel id field (ids of every grid)
  grid_bound    grid_alloc: ids 0 .. WA_ID_MASK
  tab16_ids     16-bit tabu entries exist for grids of up to 2^27 voxels ...
  tab16_quot    ... and are used where hash_log2 + 12 >= the id bits (12-bit quotient)
  hash_log2_max WA_HASH_LOG2 is clamped to 2^15 slots"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "welding_robot_amd", "csrc")
SRC = {k: os.path.join(CSRC, f) for k, f in (("acs", "host_acs.inc"), ("grid", "host_grid.inc"), ("dev", "acs_dev.hpp"),
                                               ("nb26", "acs_nb26.hpp"), ("wa", "wa_device.h"))}
HEADER = os.path.join(ROOT, "include", "weldacs.h")

# ------------------------------------------------------------------ the table
# rule -> (source, regex over whitespace-collapsed text, its constants in order of appearance; hex groups are read as hex)
TABLE = {
    "nb6_bound": ("acs", r"if \(nb == 6 && (\d+) \* n >= \(int64_t\)(\d+) << (\d+)\) \{", (24, 1, 31)),
    "nb26_ids": ("dev", r"template <> struct WaNbT<26> \{ static constexpr int SHIFT = (\d+); static constexpr int32_t IDM = \((\d+) << (\d+)\) - (\d+); \};",
                 (27, 1, 27, 1)),
    "nb26_bound": ("acs", r"if \(nb == 26 && n > \(int64_t\)WaNbT<26>::IDM \+ (\d+)\) \{", (1,)),
    "nb26_fast": ("nb26", r"if \(MODE == 1 && R\.alpha == 1 && len <= spill_at && len < \(int32_t\)D\.path_cap && (\d+)LL \* D\.d\.n < \((\d+)LL << (\d+)\)\) \{",
                  (104, 1, 31)),
    "nb26_record": ("nb26", r"const uint32_t off = \(uint32_t\)cur \* (\d+)u \+ lane_off;", (104,)),
    "id_mask": ("wa", r"#define WA_ID_MASK 0x([0-9A-Fa-f]+)u", (0x1FFFFFFF,)),
    "grid_bound": ("grid", r"if \(n > \(int64_t\)WA_ID_MASK \+ (\d+)\) return fail\(ctx, WA_ERR_ARG,", (1,)),
    "tab16_ids": ("acs", r"if \(nb == 6 && id_bits <= (\d+) && s->tab16_env != 0\) \{", (27,)),
    "tab16_quot": ("acs", r"s->D\.tab16_kmul != 0 && s->id_bits <= s->hash_log2 \+ (\d+)\) \{", (12,)),
    "hash_log2_max": ("acs", r"if \(s->hash_log2 > (\d+)\) s->hash_log2 = (\d+);", (15, 15)),
}
HEX = {"id_mask"}
# rules without a constant of their own: the 6-neighbour ids are WA_ID_MASK's, the error messages name the limits
RULES = (
    ("dev", r"template <> struct WaNbT<6> \{ static constexpr int SHIFT = WA_K_SHIFT; static constexpr int32_t IDM = \(int32_t\)WA_ID_MASK; \};"),
    ("acs", r"\"wa_acs_create: grids above 89,478,485 voxels \(~447\^3\) are not supported\""),
    ("acs", r"\"wa_acs_create: 26-neighbour grids above 2\^27 voxels \(512\^3\) are not supported\""),
    ("grid", r"\"grid larger than 2\^29 voxels\""),
)


def _c(name):
    return TABLE[name][2]


# ------------------------------------------------------------------ the limits, derived from the table
def max_voxels_nb6():
    """largest n with rec * n < 2^k"""
    rec, one, k = _c("nb6_bound")
    return ((one << k) - 1) // rec


def max_voxels_nb26():
    return ((_c("nb26_ids")[1] << _c("nb26_ids")[2]) - _c("nb26_ids")[3]) + _c("nb26_bound")[0]


def nb26_fast_loop(n):
    """does a 26-neighbour DEV walk on n voxels take the fast loop (32-bit offsets) at all?"""
    rec, one, k = _c("nb26_fast")
    return rec * n < (one << k)


def max_voxels_grid():
    return _c("id_mask")[0] + _c("grid_bound")[0]


def id_bits(n):
    """bits of the largest voxel id (host_acs.inc: smallest b with 2^b >= n)"""
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def entries16(n, hash_log2):
    """can WA_TAB16=1 give a 6-neighbour walk on n voxels 16-bit entries at this table size?"""
    b = id_bits(n)
    return b <= _c("tab16_ids")[0] and b <= min(hash_log2, _c("hash_log2_max")[0]) + _c("tab16_quot")[0]


def smallest_table16(n):
    """the smallest tabu table (log2 of its slots) whose 16-bit entries can name n voxels' ids"""
    return id_bits(n) - _c("tab16_quot")[0]


# the sizes the GPU file runs, each with a dims triple (nx, ny, nz) whose product it is
NB6_MAX = max_voxels_nb6()
NB26_MAX = max_voxels_nb26()
NB26_FAST_EDGE = ((_c("nb26_fast")[1] << _c("nb26_fast")[2]) - 1) // _c("nb26_fast")[0]     # the last size with the fast loop
GRID_MAX = max_voxels_grid()
DIMS = {
    "nb6_max": (565, 1247, 127),
    "nb6_over": (87211, 38, 27),
    "nb26_fast": (560, 153, 241),              # NB26_FAST_EDGE - 1
    "nb26_general": (211, 293, 334),           # NB26_FAST_EDGE + 1
    "nb26_max": (512, 512, 512),
    "nb26_over": (87211, 57, 27),
    "grid_max": (1024, 1024, 512),
    "grid_over": (3033169, 59, 3),
}
SIZES = {"nb6_max": NB6_MAX, "nb6_over": NB6_MAX + 1, "nb26_fast": NB26_FAST_EDGE - 1, "nb26_general": NB26_FAST_EDGE + 1,
         "nb26_max": NB26_MAX, "nb26_over": NB26_MAX + 1, "grid_max": GRID_MAX, "grid_over": GRID_MAX + 1}


# ------------------------------------------------------------------ the source, read back
def _text(src):
    return {k: re.sub(r"\s+", " ", v) for k, v in src.items()}


def mirrored(src):
    """rule -> its constants as the sources state them (None: the statement is not there, or not once); RULES -> found"""
    text = _text(src)
    out = {}
    for name, (where, pat, _) in TABLE.items():
        found = set(re.findall(pat, text[where]))
        f = found.pop() if len(found) == 1 else None
        if f is not None:
            f = f if isinstance(f, tuple) else (f,)
            f = tuple(int(x, 16 if name in HEX else 10) for x in f)
        out[name] = f
    for where, pat in RULES:
        out[pat] = bool(re.search(pat, text[where]))
    return out


def _sources():
    out = {}
    for k, p in SRC.items():
        with open(p) as f:
            out[k] = f.read()
    return out


def _want():
    w = {name: c for name, (_, _, c) in TABLE.items()}
    w.update({pat: True for _, pat in RULES})
    return w


def test_the_table_is_what_the_source_states():
    got, want = mirrored(_sources()), _want()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_moving_any_constant_of_a_rule_is_noticed(name):
    """each constant of the rule, changed by one in a copy of the source text, makes the mirror differ -- in that rule"""
    src = _sources()
    where, pat, consts = TABLE[name]
    text = _text(src)
    m = re.search(pat, text[where])
    assert m is not None
    for k in range(1, len(consts) + 1):
        base = 16 if name in HEX else 10
        v = int(m.group(k), base)
        new = format(v + 1, "X") if base == 16 else str(v + 1)
        mutated = dict(text, **{where: text[where][:m.start(k)] + new + text[where][m.end(k):]})
        got = mirrored(mutated)
        assert got[name] != consts, (name, k)
        assert all(got[o] == w for o, w in _want().items() if o != name), (name, k)


@pytest.mark.parametrize("name,old,new", [
    ("nb6_bound", "24 * n >= (int64_t)1 << 31", "24 * n > (int64_t)1 << 31"),
    ("nb26_bound", "n > (int64_t)WaNbT<26>::IDM + 1", "n >= (int64_t)WaNbT<26>::IDM + 1"),
    ("nb26_fast", "104LL * D.d.n < (1LL << 31)", "104LL * D.d.n <= (1LL << 31)"),
    ("grid_bound", "n > (int64_t)WA_ID_MASK + 1", "n >= (int64_t)WA_ID_MASK + 1"),
    ("tab16_quot", "s->id_bits <= s->hash_log2 + 12", "s->id_bits < s->hash_log2 + 12"),
])
def test_changing_a_comparison_is_noticed(name, old, new):
    src = _text(_sources())
    where = TABLE[name][0]
    assert src[where].count(old) == 1, old
    got = mirrored(dict(src, **{where: src[where].replace(old, new)}))
    assert got[name] is None


def test_removing_the_fast_loop_size_condition_is_noticed():
    src = _text(_sources())
    cond = " && 104LL * D.d.n < (1LL << 31)"
    assert src["nb26"].count(cond) == 1
    assert mirrored(dict(src, nb26=src["nb26"].replace(cond, "")))["nb26_fast"] is None


# ------------------------------------------------------------------ the limits
def test_the_limits():
    assert NB6_MAX == 89_478_485 and 24 * NB6_MAX < 2 ** 31 <= 24 * (NB6_MAX + 1)
    assert NB26_MAX == 2 ** 27 == 1 << _c("nb26_ids")[0]            # every id of the 27-bit field, no more
    assert NB26_FAST_EDGE == 20_648_881 and nb26_fast_loop(NB26_FAST_EDGE) and not nb26_fast_loop(NB26_FAST_EDGE + 1)
    assert GRID_MAX == 2 ** 29 and GRID_MAX - 1 == _c("id_mask")[0]
    assert nb26_fast_loop(SIZES["nb26_fast"]) and not nb26_fast_loop(SIZES["nb26_general"]) and not nb26_fast_loop(NB26_MAX)
    # (the 6-neighbour bound keeps every id below the 26-neighbour one, and both below the grid's)
    assert NB6_MAX < NB26_MAX < GRID_MAX


@pytest.mark.parametrize("name", sorted(DIMS))
def test_every_size_has_its_dims(name):
    nx, ny, nz = DIMS[name]
    assert nx * ny * nz == SIZES[name], (name, nx * ny * nz, SIZES[name])
    assert max(DIMS[name]) < 2 ** 31 and nx * ny < 2 ** 31          # (nxy is an int32)


def test_16_bit_entries_at_the_widest_ids():
    assert id_bits(NB6_MAX) == 27 and id_bits(2 ** 24 + 1) == 25 and id_bits(2 ** 25 + 1) == 26 and id_bits(2 ** 21) == 21
    assert smallest_table16(NB6_MAX) == 15 == _c("hash_log2_max")[0]       # the 6-neighbour top needs the full 12-bit quotient
    assert entries16(NB6_MAX, 15) and not entries16(NB6_MAX, 14)
    for n in (2 ** 24 + 1, 2 ** 25 + 1):
        lg = smallest_table16(n)
        assert entries16(n, lg) and not entries16(n, lg - 1), n
    assert not entries16(2 ** 27 + 1, 15)


# ------------------------------------------------------------------ the header says what the code does
def test_the_header_states_each_limit():
    with open(HEADER) as f:
        h = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", f.read()))

    def comment_before(decl):
        i = h.index(decl)
        j = h.rindex("/*", 0, i)
        return h[j:i]
    c6 = comment_before("int wa_acs_create(wa_ctx *ctx,")
    assert "Grids up to {:,} voxels".format(NB6_MAX) in c6, c6
    assert "24 B * voxels < 2^31" in c6
    c26 = comment_before("int wa_acs_create_nb(")
    assert "grids up to 2^%d voxels" % (NB26_MAX.bit_length() - 1) in c26, c26
    cg = comment_before("int wa_grid_from_occupancy(")
    assert "Grids up to 2^%d voxels (ids 0 .. 2^%d - 1)" % ((GRID_MAX.bit_length() - 1,) * 2) in cg, cg
