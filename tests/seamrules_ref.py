"""numpy restatement of seam tours under job rules: precedences between seams and one-way seams, on top of seamtour_ref.

No product code here.  admissible / best_move_scalar state the rules one move at a time (apply the move, test the state); best_move
evaluates a whole pass with array arithmetic and the position limits the device uses (tests/test_seamrules_rules.py holds the two
against each other); seam_tour_rules and seam_tour_rules_exact are what the library's results are compared with, byte for byte."""
import itertools

import numpy as np

import seamtour_ref as R

INF = R.INF
MAX_PREC = 1 << 16


class Rules:
    """the checked inputs: M, the anchor seam, the distinct pairs, every seam's direct predecessors / successors, fixed per seam (M entries)"""

    def __init__(self, m, closed, before=(), after=(), fixed=None):
        before, after = [int(x) for x in before], [int(x) for x in after]
        if not 1 <= m <= 1024 or len(before) != len(after) or len(before) > MAX_PREC:
            raise ValueError("m or n_prec")
        self.m, self.closed = m, bool(closed)
        self.M = m if closed else m + 1
        self.anchor = 0 if closed else m
        fixed = [0] * m if fixed is None else [int(x) for x in fixed]
        if len(fixed) != m or any(not 0 <= x <= 2 for x in fixed):
            raise ValueError("fixed")
        self.fixed = np.array(fixed + [0] * (self.M - m), np.int64)
        for a, b in zip(before, after):
            if not (0 <= a < m and 0 <= b < m) or a == b or (closed and b == 0):
                raise ValueError("pair")
        self.pairs = sorted(set(zip(before, after)))
        self.preds = [[] for _ in range(self.M)]
        self.succs = [[] for _ in range(self.M)]
        for a, b in self.pairs:
            self.preds[b].append(a)
            self.succs[a].append(b)
        left = [len(p) for p in self.preds]   # a cycle leaves seams that never become ready
        ready = [s for s in range(self.M) if not left[s]]
        done = 0
        while ready:
            s = ready.pop()
            done += 1
            for u in self.succs[s]:
                left[u] -= 1
                if not left[u]:
                    ready.append(u)
        if done != self.M:
            raise ValueError("cycle")
        self.n_prec, self.n_fixed = len(self.pairs), int((self.fixed != 0).sum())


def violations(E, ru):
    """(pairs whose order is broken, fixed seams entered at the wrong end) of a state read from position 0"""
    pos = {e >> 1: k for k, e in enumerate(E)}
    bad_p = sum(1 for a, b in ru.pairs if pos[a] >= pos[b])
    bad_d = sum(1 for e in E if ru.fixed[e >> 1] and (e & 1) != ru.fixed[e >> 1] - 1)
    return bad_p, bad_d


def admissible(E, ru):
    return (E[0] >> 1) == ru.anchor and violations(E, ru) == (0, 0)


def check(m, closed, before, after, fixed, order, dirs):
    """what wa_gtsp_seam_rules_check counts: the tour as the caller holds it, read from its anchor; every given pair counts, duplicates too"""
    ru = Rules(m, closed, before, after, fixed)
    order, dirs = [int(x) for x in order], [int(x) for x in dirs]
    if sorted(order) != list(range(m)) or any(x not in (0, 1) for x in dirs):
        raise ValueError("order / dir")
    at = order.index(0) if closed else 0
    pos = {order[(at + k) % m]: k for k in range(m)}
    bad_p = sum(1 for a, b in zip(before, after) if pos[int(a)] >= pos[int(b)])
    bad_d = sum(1 for s, d in zip(order, dirs) if ru.fixed[s] and d != ru.fixed[s] - 1)
    return bad_p, bad_d


# ---------------------------------------------------------------- the moves, one at a time
def moves(M, or_len):
    """rule 4's moves with rule 4's numbers: i >= 1, and Reverse(0, 0)"""
    return [(num, kind, args) for num, kind, args in R.moves(M, or_len) if args[0] >= 1 or (kind == "A" and args == (0, 0))]


def best_move_scalar(E, W, or_len, ru):
    best = None
    for num, kind, args in moves(len(E), or_len):
        if not admissible(R.move_apply(E, kind, args), ru):
            continue
        d = R.move_delta(E, W, kind, args)
        if best is None or (d, num) < best:
            best = (d, num)
    return best


# ---------------------------------------------------------------- a pass with array arithmetic
def limits(E, ru):
    """per position p of an admissible state: fixp (the seam there is one-way), near[k][p] = the last position before p - k of a direct
    predecessor (-1: none), far[k][p] = the first position behind p + k of a direct successor (M: none), k = 0, 1, 2; and per i
    rmax[i] = the last j such that no position in i .. j is one-way or has near[0] >= i (i - 1: not even i)"""
    M = len(E)
    pos = np.zeros(M, np.int64)
    pos[[e >> 1 for e in E]] = np.arange(M)
    fixp = np.array([ru.fixed[e >> 1] != 0 for e in E])
    near = np.full((3, M), -1, np.int64)
    far = np.full((3, M), M, np.int64)
    for p, e in enumerate(E):
        pp = pos[ru.preds[e >> 1]]
        sp = pos[ru.succs[e >> 1]]
        for k in range(3):
            near[k, p] = pp[pp < p - k].max(initial=-1)
            far[k, p] = sp[sp > p + k].min(initial=M)
    rmax = np.zeros(M, np.int64)
    for i in range(M):
        j = i
        while j < M and not fixp[j] and near[0, j] < i:
            j += 1
        rmax[i] = j - 1
    return fixp, near, far, rmax


def best_move(E, W, or_len, ru):
    """(smallest delta, its lowest move number) over every admissible move, or None when there is none"""
    M = len(E)
    e = np.asarray(E, np.int64)
    o = e ^ 1
    pos = np.arange(M)
    _, near, far, rmax = limits(E, ru)
    found = []
    if M >= 2:
        i, j = pos[:, None], pos[None, :]
        ok = (j >= i) & (j - i <= M - 2) & (j <= rmax[:, None]) & ((i >= 1) | (j == 0))
        a, jn = (i - 1) % M, (j + 1) % M
        d = W[o[a], o[j]] + W[e[i], e[jn]] - W[o[a], e[i]] - W[o[j], e[jn]]
        found.append((d, i * M + j + 0 * d, ok))
    for L in range(1, min(or_len, M - 2) + 1):
        first = pos[:M - L + 1]
        i = first[:, None]
        g = pos[None, :]
        a, b, l, h = (i - 1) % M, (i + L) % M, i + L - 1, (g + 1) % M
        fwd = np.min([far[L - 1 - q][first + q] for q in range(L)], axis=0)[:, None]     # the block may go behind g < fwd
        back = np.max([near[q][first + q] for q in range(L)], axis=0)[:, None]           # ... or behind g >= back
        ok = ~((g >= i) & (g <= l)) & (g != a) & (i >= 1) & np.where(g > l, g < fwd, g >= back)
        base = W[o[a], e[b]] - W[o[a], e[i]] - W[o[l], e[b]] - W[o[g], e[h]]
        for r in (0, 1):
            x = W[o[g], o[l]] + W[e[i], e[h]] if r else W[o[g], e[i]] + W[o[l], e[h]]
            d = base + x
            found.append((d, M * M + (((i * 3 + L - 1) * M + g) * 2 + r) + 0 * d, ok & (rmax[first][:, None] >= l) if r else ok))
    if not found:
        return None
    d = np.concatenate([np.where(ok, d, INF).ravel() for d, _, ok in found])
    num = np.concatenate([n.ravel() for _, n, _ in found])
    if d.min() == INF:
        return None
    lo = d.min()
    return int(lo), int(num[d == lo].min())


def descend(E, W, or_len, max_passes, ru, trace=None):
    """(final E, passes, capped); trace collects every state"""
    E = list(E)
    passes = 0
    while True:
        if trace is not None:
            trace.append(list(E))
        if passes == max_passes:
            return E, passes, 1
        passes += 1
        best = best_move(E, W, or_len, ru)
        if best is None or best[0] >= 0:
            return E, passes, 0
        kind, args = R.decode(best[1], len(E))
        E = R.move_apply(E, kind, args)


# ---------------------------------------------------------------- starts
def repair(E, ru):
    """the anchor first, then step by step the seam that stands earliest in E among those whose predecessors are all placed; the drawn
    direction stays unless fixed forces the other"""
    left = [len(p) for p in ru.preds]
    placed = [False] * ru.M
    out = []
    for step in range(ru.M):
        for e in E:
            s = e >> 1
            if not placed[s] and (s == ru.anchor if step == 0 else left[s] == 0):
                break
        placed[s] = True
        for u in ru.succs[s]:
            left[u] -= 1
        out.append(2 * s + (ru.fixed[s] - 1 if ru.fixed[s] else e & 1))
    return [int(x) for x in out]


def start0(ru, order0=None, dir0=None):
    m = ru.m
    if order0 is None:
        order = [e >> 1 for e in repair([2 * s for s in range(ru.M)], ru) if (e >> 1) < m]
    else:
        order = [int(x) for x in order0]
    if sorted(order) != list(range(m)):
        raise ValueError("order0")
    if dir0 is None:
        dirs = [max(int(ru.fixed[s]) - 1, 0) for s in order]
    else:
        dirs = [int(x) for x in dir0]
    if len(dirs) != m or any(x not in (0, 1) for x in dirs):
        raise ValueError("dir0")
    E = ([] if ru.closed else [2 * m]) + [2 * s + x for s, x in zip(order, dirs)]
    if not admissible(E, ru):
        raise ValueError("start 0 is not admissible")
    return E


def seam_tour_rules(dist, m, before=(), after=(), fixed=None, closed=True, or_len=3, n_starts=1, max_passes=1 << 20, seed=1, order0=None,
                    dir0=None, trace=None):
    if not (1 <= m <= 1024 and 0 <= or_len <= 3 and 1 <= n_starts <= 1 << 20 and 1 <= max_passes <= 1 << 20):
        raise ValueError("parameters")
    ru = Rules(m, closed, before, after, fixed)
    first = start0(ru, order0, dir0)
    W = R.quantise(dist, m, closed)
    M = ru.M
    costs, passes, capped, finals = [], [], [], []
    for r in range(n_starts):
        E, p, c = descend(first if r == 0 else repair(R.random_start(M, seed, r), ru), W, or_len, max_passes, ru, trace)
        finals.append(E)
        costs.append(R.tour_cost(E, W))
        passes.append(p)
        capped.append(c)
    best = int(np.argmin(costs))
    order, dirs = R.emit(finals[best], m, closed)
    summary = dict(m=m, M=M, n_starts=n_starts, best_start=best, n_capped=int(sum(capped)), cost_q=int(costs[best]),
                   start0_cost_q_in=R.tour_cost(first, W), start0_cost_q_out=int(costs[0]), passes_total=int(sum(passes)),
                   n_prec=ru.n_prec, n_fixed=ru.n_fixed)
    return dict(order=order, dir=dirs, cost_q=int(costs[best]), start_cost_q=np.array(costs, np.int64),
                start_passes=np.array(passes, np.int32), summary=summary, E=finals[best], W=W, rules=ru)


# ---------------------------------------------------------------- the exact tour
def _table(W, n, predmask, fix):
    """the subset programme with seam 0 of W first, entered at endpoint 0: f[S][e], e the endpoint (less 2) at which the last seam is left;
    INF where a predecessor of that seam is missing from S or fixed forbids the entry at e ^ 1.  (best cost, E) or (INF, None)"""
    ne = 2 * n
    f = np.full((1 << n, ne), INF, np.int64)
    Wn = W[2:, 2:]
    S_all = np.arange(1 << n)
    pop = np.array([bin(s).count("1") for s in S_all])
    for level in range(1, n + 1):
        for t in range(n):
            S = S_all[(pop == level) & ((S_all >> t) & 1 == 1)]
            S = S[((S ^ (1 << t)) & predmask[t]) == predmask[t]]
            for e in (2 * t, 2 * t + 1):
                if fix[t] and ((e ^ 1) & 1) != fix[t] - 1:
                    continue
                if level == 1:
                    f[S, e] = W[1, (e ^ 1) + 2]
                else:
                    f[S, e] = np.minimum((f[S ^ (1 << t)] + Wn[:, e ^ 1][None, :]).min(1), INF)
    S = (1 << n) - 1
    last = np.where(f[S] < INF, f[S] + W[2:, 0], INF)
    cur = int(np.argmin(last))
    if last[cur] >= INF:
        return INF, None
    opt = int(last[cur])
    rev = []
    while True:
        rev.append((cur ^ 1) + 2)
        here = int(f[S, cur])
        S ^= 1 << (cur >> 1)
        if S == 0:
            break
        cand = np.where(f[S] < INF, f[S] + Wn[:, cur ^ 1], INF)
        cur = int(np.flatnonzero(cand == here)[0])
    return opt, [0] + rev[::-1]


def seam_tour_rules_exact(dist, m, before=(), after=(), fixed=None, closed=True):
    ru = Rules(m, closed, before, after, fixed)
    M = ru.M
    if M > 16:
        raise OverflowError("more than 16 seams")
    W = R.quantise(dist, m, closed)
    n = M - 1
    # the anchor becomes seam 0 of the programme: an open tour's dummy moves to the front, seam s becomes s + 1
    seam_of = list(range(M)) if closed else [m] + list(range(m))
    idx = np.array([2 * s + b for s in seam_of for b in (0, 1)])
    Wa = W[np.ix_(idx, idx)]
    label = {s: t for t, s in enumerate(seam_of)}
    predmask = [sum(1 << (label[a] - 1) for a in ru.preds[seam_of[t + 1]] if label[a] >= 1) for t in range(n)]
    fix = [int(ru.fixed[seam_of[t + 1]]) for t in range(n)]
    best = None
    for d in ((0, 1) if closed else (0,)):
        if closed and ru.fixed[0] and ru.fixed[0] - 1 != d:
            continue
        if n == 0:
            cand = (0, [d])
        else:
            swap = np.arange(2 * M)
            if d:
                swap[0], swap[1] = 1, 0
            c, E = _table(Wa[np.ix_(swap, swap)], n, predmask, fix)
            cand = (c, [d] + E[1:])
        if best is None or cand[0] < best[0]:
            best = cand
    opt, Ea = best
    E = [2 * seam_of[e >> 1] + (e & 1) for e in Ea]
    order, dirs = R.emit(E, m, closed)
    return dict(order=order, dir=dirs, cost_q=int(opt), E=E, W=W, rules=ru)


def brute_force_rules(dist, m, before=(), after=(), fixed=None, closed=True):
    """the optimum over every admissible order and every admissible choice of directions, the anchor first"""
    ru = Rules(m, closed, before, after, fixed)
    W = R.quantise(dist, m, closed)
    M = ru.M
    bits = (np.arange(1 << M)[:, None] >> np.arange(M)[None, :]) & 1
    best = None
    for perm in itertools.permutations([s for s in range(M) if s != ru.anchor]):
        seams = (ru.anchor,) + perm
        pos = {s: k for k, s in enumerate(seams)}
        if any(pos[a] >= pos[b] for a, b in ru.pairs):
            continue
        fx = ru.fixed[list(seams)]
        ok = ((fx[None, :] == 0) | (bits == fx[None, :] - 1)).all(1)
        E = (2 * np.array(seams)[None, :] + bits)[ok]
        c = int(W[E ^ 1, np.roll(E, -1, axis=1)].sum(1).min())
        best = c if best is None or c < best else best
    return best


def random_rules(m, seed, closed):
    """the recipe of the GPU tests: m pairs oriented by a hidden order (seam 0 first in it when the tour is closed), a quarter of the
    seams one-way"""
    rs = np.random.RandomState(seed)
    hidden = rs.permutation(m)
    if closed:
        hidden = np.concatenate([[0], hidden[hidden != 0]])
    rank = np.empty(m, np.int64)
    rank[hidden] = np.arange(m)
    before, after = [], []
    while len(before) < m and m >= 2:
        a, b = rs.randint(0, m, 2)
        if a == b:
            continue
        if rank[a] > rank[b]:
            a, b = b, a
        before.append(int(a))
        after.append(int(b))
    fixed = np.zeros(m, np.uint8)
    pick = rs.permutation(m)[:(m + 3) // 4]
    fixed[pick] = rs.randint(1, 3, len(pick))
    return np.array(before, np.int32), np.array(after, np.int32), fixed
