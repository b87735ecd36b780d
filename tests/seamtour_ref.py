"""numpy restatement of the seam-tour definition: order and direction of two-ended weld seams.

No product code here.  The scalar functions (delta_reverse, delta_move, apply_reverse, apply_move, moves) state the rules one move at a
time on Python lists; best_move evaluates a whole pass with array arithmetic (tests/test_seamtour_rules.py holds the two against each
other); seam_tour and seam_tour_exact are what the library's results are compared with, byte for byte."""
import itertools

import numpy as np

Q = 1 << 20
W_LIMIT = 1 << 40
INF = 1 << 62
_MASK = (1 << 64) - 1


def quantise(dist, m, closed=True):
    """W (2M x 2M int64, symmetric) from the upper triangle of dist (2m x 2m); ValueError where the library answers WA_ERR_ARG"""
    dist = np.asarray(dist, np.float64).reshape(2 * m, 2 * m)
    M = m if closed else m + 1
    W = np.zeros((2 * M, 2 * M), np.int64)
    i, j = np.triu_indices(2 * m, 1)
    keep = (i >> 1) != (j >> 1)
    i, j = i[keep], j[keep]
    with np.errstate(over="ignore", invalid="ignore"):
        d = dist[i, j] * float(Q)
    if not np.all(np.isfinite(d) & (d >= 0)):
        raise ValueError("a cost is negative or not finite")
    r = np.rint(d)
    if not np.all(r < float(W_LIMIT)):
        raise ValueError("a cost reaches 2^40 quanta")
    W[i, j] = r.astype(np.int64)
    W[j, i] = W[i, j]
    return W


def tour_cost(E, W):
    M = len(E)
    return sum(int(W[E[k] ^ 1, E[(k + 1) % M]]) for k in range(M))


# ---------------------------------------------------------------- the moves, one at a time
def delta_reverse(E, W, i, j):
    M = len(E)
    oa, ii, oj, inx = E[(i - 1) % M] ^ 1, E[i], E[j] ^ 1, E[(j + 1) % M]
    return int(W[oa, oj]) + int(W[ii, inx]) - int(W[oa, ii]) - int(W[oj, inx])


def delta_move(E, W, i, L, g, r):
    M = len(E)
    a, b, f, l, h = (i - 1) % M, (i + L) % M, i, i + L - 1, (g + 1) % M
    oa, ib, i_f, ol, og, ih = E[a] ^ 1, E[b], E[f], E[l] ^ 1, E[g] ^ 1, E[h]
    x = int(W[og, ol]) + int(W[i_f, ih]) if r else int(W[og, i_f]) + int(W[ol, ih])
    return int(W[oa, ib]) - int(W[oa, i_f]) - int(W[ol, ib]) - int(W[og, ih]) + x


def apply_reverse(E, i, j):
    return E[:i] + [e ^ 1 for e in reversed(E[i:j + 1])] + E[j + 1:]


def apply_move(E, i, L, g, r):
    block = E[i:i + L]
    if r:
        block = [e ^ 1 for e in reversed(block)]
    anchor = E[g]
    rest = E[:i] + E[i + L:]
    at = rest.index(anchor) + 1
    return rest[:at] + block + rest[at:]


def moves(M, or_len):
    """every move of a pass: (number, kind, arguments)"""
    out = []
    for i in range(M):
        for j in range(i, M):
            if j - i <= M - 2:
                out.append((i * M + j, "A", (i, j)))
    for i in range(M):
        for L in range(1, min(or_len, M - 2) + 1):
            if i + L - 1 > M - 1:
                continue
            for g in range(M):
                if i <= g <= i + L - 1 or g == (i - 1) % M:
                    continue
                for r in (0, 1):
                    out.append((M * M + (((i * 3 + L - 1) * M + g) * 2 + r), "B", (i, L, g, r)))
    return out


def move_delta(E, W, kind, args):
    return delta_reverse(E, W, *args) if kind == "A" else delta_move(E, W, *args)


def move_apply(E, kind, args):
    return apply_reverse(E, *args) if kind == "A" else apply_move(E, *args)


def decode(num, M):
    if num < M * M:
        return "A", (num // M, num % M)
    v = num - M * M
    r, v = v & 1, v >> 1
    g, v = v % M, v // M
    return "B", (v // 3, v % 3 + 1, g, r)


def best_move_scalar(E, W, or_len):
    best = None
    for num, kind, args in moves(len(E), or_len):
        d = move_delta(E, W, kind, args)
        if best is None or (d, num) < best:
            best = (d, num)
    return best


# ---------------------------------------------------------------- a pass with array arithmetic
def best_move(E, W, or_len):
    """(smallest delta, its lowest move number) over every move, or None when there is no move at all"""
    M = len(E)
    e = np.asarray(E, np.int64)
    o = e ^ 1
    pos = np.arange(M)
    found = []
    if M >= 2:
        i, j = pos[:, None], pos[None, :]
        ok = (j >= i) & (j - i <= M - 2)
        a, jn = (i - 1) % M, (j + 1) % M
        d = W[o[a], o[j]] + W[e[i], e[jn]] - W[o[a], e[i]] - W[o[j], e[jn]]
        found.append((d, i * M + j + 0 * d, ok))
    for L in range(1, min(or_len, M - 2) + 1):
        i = pos[:M - L + 1][:, None]
        g = pos[None, :]
        a, b, l, h = (i - 1) % M, (i + L) % M, i + L - 1, (g + 1) % M
        ok = ~((g >= i) & (g <= l)) & (g != a)
        base = W[o[a], e[b]] - W[o[a], e[i]] - W[o[l], e[b]] - W[o[g], e[h]]
        for r in (0, 1):
            x = W[o[g], o[l]] + W[e[i], e[h]] if r else W[o[g], e[i]] + W[o[l], e[h]]
            d = base + x
            found.append((d, M * M + (((i * 3 + L - 1) * M + g) * 2 + r) + 0 * d, ok))
    if not found:
        return None
    d = np.concatenate([np.where(ok, d, INF).ravel() for d, _, ok in found])
    num = np.concatenate([n.ravel() for _, n, _ in found])
    if d.min() == INF:
        return None
    lo = d.min()
    return int(lo), int(num[d == lo].min())


def descend(E, W, or_len, max_passes):
    """(final E, passes, capped)"""
    E = list(E)
    passes = 0
    while True:
        if passes == max_passes:
            return E, passes, 1
        passes += 1
        best = best_move(E, W, or_len)
        if best is None or best[0] >= 0:
            return E, passes, 0
        kind, args = decode(best[1], len(E))
        E = move_apply(E, kind, args)


# ---------------------------------------------------------------- starts
def _draw(s):
    s = (s + 0x9E3779B97F4A7C15) & _MASK
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return s, z ^ (z >> 31)


def random_start(M, seed, r):
    s = (seed ^ (r * 0xD1B54A32D192ED03)) & _MASK
    P = list(range(M))
    for k in range(M - 1, 0, -1):
        s, d = _draw(s)
        j = ((d >> 32) * (k + 1)) >> 32
        P[k], P[j] = P[j], P[k]
    E = []
    for k in range(M):
        s, d = _draw(s)
        E.append(2 * P[k] + (d >> 63))
    return E


def start0(m, closed, order0=None, dir0=None):
    order0 = list(range(m)) if order0 is None else [int(x) for x in order0]
    dir0 = [0] * m if dir0 is None else [int(x) for x in dir0]
    if sorted(order0) != list(range(m)) or any(x not in (0, 1) for x in dir0):
        raise ValueError("order0 / dir0")
    return [2 * s + x for s, x in zip(order0, dir0)] + ([] if closed else [2 * m])


def emit(E, m, closed):
    """(order, dir) as the caller sees them: seam 0 first, or the seam behind the dummy first and the dummy dropped"""
    M = len(E)
    seams = [x >> 1 for x in E]
    at = seams.index(0) if closed else seams.index(m) + 1
    rot = [E[(at + k) % M] for k in range(m)]
    return np.array([x >> 1 for x in rot], np.int32), np.array([x & 1 for x in rot], np.uint8)


def seam_tour(dist, m, closed=True, or_len=3, n_starts=1, max_passes=1 << 20, seed=1, order0=None, dir0=None):
    if not (1 <= m <= 1024 and 0 <= or_len <= 3 and 1 <= n_starts <= 1 << 20 and 1 <= max_passes <= 1 << 20):
        raise ValueError("parameters")
    first = start0(m, closed, order0, dir0)
    W = quantise(dist, m, closed)
    M = len(first)
    costs, passes, capped, finals = [], [], [], []
    for r in range(n_starts):
        E, p, c = descend(first if r == 0 else random_start(M, seed, r), W, or_len, max_passes)
        finals.append(E)
        costs.append(tour_cost(E, W))
        passes.append(p)
        capped.append(c)
    best = int(np.argmin(costs))   # (the first among equals)
    order, dirs = emit(finals[best], m, closed)
    summary = dict(m=m, M=M, n_starts=n_starts, best_start=best, n_capped=int(sum(capped)), cost_q=int(costs[best]),
                   start0_cost_q_in=tour_cost(first, W), start0_cost_q_out=int(costs[0]), passes_total=int(sum(passes)))
    return dict(order=order, dir=dirs, cost_q=int(costs[best]), start_cost_q=np.array(costs, np.int64),
                start_passes=np.array(passes, np.int32), summary=summary, E=finals[best], W=W)


# ---------------------------------------------------------------- the exact tour
def seam_tour_exact(dist, m, closed=True):
    M = m if closed else m + 1
    if M > 16:
        raise OverflowError("more than 16 seams")
    W = quantise(dist, m, closed)
    n, ne = M - 1, 2 * (M - 1)
    E = [0]
    opt = 0
    if n:
        f = np.full((1 << n, ne), INF, np.int64)
        Wn = W[2:, 2:]
        S_all = np.arange(1 << n)
        pop = np.array([bin(s).count("1") for s in S_all])
        for level in range(1, n + 1):
            for t in range(n):
                S = S_all[(pop == level) & ((S_all >> t) & 1 == 1)]
                for e in (2 * t, 2 * t + 1):
                    if level == 1:
                        f[S, e] = W[1, (e ^ 1) + 2]
                    else:
                        f[S, e] = (f[S ^ (1 << t)] + Wn[:, e ^ 1][None, :]).min(1)
        S = (1 << n) - 1
        last = f[S] + W[2:, 0]
        cur = int(np.argmin(last))   # (the lowest endpoint among equals)
        opt = int(last[cur])
        rev = []
        while True:
            rev.append((cur ^ 1) + 2)
            here = int(f[S, cur])
            S ^= 1 << (cur >> 1)
            if S == 0:
                break
            cand = f[S] + Wn[:, cur ^ 1]
            cur = int(np.flatnonzero(cand == here)[0])
        E += rev[::-1]
    order, dirs = emit(E, m, closed)
    return dict(order=order, dir=dirs, cost_q=opt, E=E, W=W)


def brute_force(dist, m, closed=True):
    """the optimum over every order and every direction (seam 0 first: a rotation costs nothing)"""
    W = quantise(dist, m, closed)
    M = W.shape[0] // 2
    bits = (np.arange(1 << M)[:, None] >> np.arange(M)[None, :]) & 1   # every choice of directions
    best = None
    for perm in itertools.permutations(range(1, M)):
        E = 2 * np.array((0,) + perm)[None, :] + bits
        c = int(W[E ^ 1, np.roll(E, -1, axis=1)].sum(1).min())
        best = c if best is None or c < best else best
    return best
