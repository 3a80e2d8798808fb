"""The numbering of kernels/csr_order.hpp as a plain model: numpy and plain Python, no schedule and no tiles of the kernels.

Written from the header comment of csr_order.hpp and the contract of liship_csr_order (include/liship.h); nothing here calls the
library.  The numbering is a function of its inputs alone, so the model predicts it index by index:

(a) component 0 is seeded at vertex 0, even when vertex 0 has no neighbour; each later component at the smallest unowned index
    that has a neighbour in [0, n) other than itself; at most 8 components;
(b) landmark 0 of a component is its vertex farthest from the seed, landmark f the vertex that maximises the smallest distance
    to landmarks 0 .. f-1; ties go to the smallest index;
(c) bits = min(15, 56 // fields) per distance; shift = the smallest value for which the deepest landmark search (its number of
    levels, eccentricity + 1) still fits: (deepest >> shift) < 2 ** bits;
(d) key = component in the top byte | the bit-interleaved clamped distances, bit b of field f at bit fields * b + f | bit 62 for a
    row that reads a column >= n when ncols > n; 0xff << 56 for a vertex without a component;
(e) order = the stable argsort of the keys; inner_rows = the rows that have a component and read no ghost column;
(f) a search of eccentricity D costs D // 32 + 1 batches, 512 batches in all: the 513th declines.

The model is specified for structurally symmetric patterns (every search of a component then stays inside it).  components()
and inner_rows() alone hold for any pattern: a vertex belongs to the first seed that reaches it along the stored entries."""
from types import SimpleNamespace

import numpy as np

MAX_COMPONENTS = 8
LEVELS_PER_BATCH = 32
BATCHES = 512
NO_COMPONENT = np.uint64(0xFF) << np.uint64(56)
GHOST_BIT = np.uint64(1) << np.uint64(62)


class Graph:
    """the edges the searches follow: entry (r, c) with 0 <= c < n and c != r (negative and ghost columns are no vertices)"""

    def __init__(self, n, ptr, idx):
        ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
        keep = (idx >= 0) & (idx < n) & (idx != rows)
        self.n = n
        self.adj = idx[keep]
        self.start = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64)
        self.has_neighbour = np.diff(self.start) > 0

    def neighbours(self, front):
        s, lens = self.start[front], self.start[front + 1] - self.start[front]
        total = int(lens.sum())
        if total == 0:
            return np.empty(0, np.int64)
        return self.adj[np.repeat(s - (np.cumsum(lens) - lens), lens) + np.arange(total)]


def bfs(g, src, blocked=None):
    """distances from src (-1: not reached) and the eccentricity of src; `blocked` vertices are never entered"""
    dist = np.full(g.n, -1, np.int64)
    seen = np.zeros(g.n, bool) if blocked is None else blocked.copy()
    dist[src], seen[src] = 0, True
    front, d = np.array([src], np.int64), 0
    while True:
        nb = g.neighbours(front)
        nb = np.unique(nb[~seen[nb]])
        if nb.size == 0:
            return dist, d
        d += 1
        dist[nb], seen[nb] = d, True
        front = nb


def batches_of(ecc):
    return ecc // LEVELS_PER_BATCH + 1


def spread(v, fields, bits):
    """bit b of v -> bit fields * b (numpy, uint64)"""
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.uint64)
    for b in range(bits):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(fields * b)
    return out


def morton(dist, bits, shift):
    """dist: (fields, m) distances -> the interleaved code, field f at bit fields * b + f"""
    dist = np.asarray(dist, np.int64)
    fields = dist.shape[0]
    code = np.zeros(dist.shape[1], np.uint64)
    for f in range(fields):
        d = np.minimum(np.maximum(dist[f], 0) >> shift, (1 << bits) - 1)
        code |= spread(d, fields, bits) << np.uint64(f)
    return code


def key_width(fields, deepest):
    bits = min(15, 56 // fields)
    shift = 0
    while (deepest >> shift) >= (1 << bits):
        shift += 1
    return bits, shift


def _first_max(score, members):
    """the smallest index among `members` that maximises score (score >= 0 only)"""
    ok = members & (score >= 0)
    best = score[ok].max()
    return int(np.flatnonzero(ok & (score == best))[0])


def reads_ghost(n, ncols, ptr, idx):
    idx = np.asarray(idx, np.int64)
    if ncols <= n:
        return np.zeros(n, bool)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(ptr, np.int64)))
    return np.bincount(rows[idx >= n], minlength=n) > 0


def components(n, ptr, idx, g=None):
    """(a) alone, for any pattern: comp[v] = the first seed's number that reaches v, -1 for none; and the seeds"""
    g = g or Graph(n, ptr, idx)
    comp, seeds = np.full(n, -1, np.int64), []
    for c in range(MAX_COMPONENTS):
        if c == 0:
            seed = 0
        else:
            cand = np.flatnonzero((comp < 0) & g.has_neighbour)
            if cand.size == 0:
                break
            seed = int(cand[0])
        dist, _ = bfs(g, seed, blocked=comp >= 0)
        comp[dist >= 0] = c
        seeds.append(seed)
    return comp, seeds


def inner_rows(n, ncols, ptr, idx):
    """(e)'s count, for any pattern"""
    if n == 0:
        return 0
    comp, _ = components(n, ptr, idx)
    return int(((comp >= 0) & ~reads_ghost(n, ncols, ptr, idx)).sum())


def order(n, ncols, ptr, idx, landmarks):
    """the whole model.  Returns a namespace: found, order, inner_rows, and what a case proves its edge by -- fields, bits, shift,
    deepest, batches (used, or the count at which it declined), components, declined_in (component whose search broke the budget,
    or None), seeds, landmarks (per component), loose (size of the no-component bucket), keys"""
    fields = min(max(landmarks, 3), 6)
    out = SimpleNamespace(found=True, order=np.empty(0, np.int64), inner_rows=0, fields=fields, bits=min(15, 56 // fields), shift=0, deepest=0,
                          batches=0, components=0, declined_in=None, seeds=[], landmarks=[], loose=0, keys=np.empty(0, np.uint64))
    if n <= 0:
        return out
    g = Graph(n, ptr, idx)
    comp = np.full(n, -1, np.int64)
    field = np.full((fields, n), -1, np.int64)

    def spend(ecc, c):
        out.batches += batches_of(ecc)
        if out.batches > BATCHES:
            out.found, out.declined_in = False, c
        return out.found

    for c in range(MAX_COMPONENTS):
        if c == 0:
            seed = 0
        else:
            cand = np.flatnonzero((comp < 0) & g.has_neighbour)
            if cand.size == 0:
                break
            seed = int(cand[0])
        from_seed, ecc = bfs(g, seed, blocked=comp >= 0)
        if not spend(ecc, c):
            return out
        members = from_seed >= 0
        comp[members] = c
        out.components += 1
        out.seeds.append(seed)
        marks = []
        for f in range(fields):
            at = _first_max(from_seed if f == 0 else field[:f].min(axis=0), members)
            dist, ecc = bfs(g, at)
            if not spend(ecc, c):
                return out
            field[f][dist >= 0] = dist[dist >= 0]
            out.deepest = max(out.deepest, ecc + 1)
            marks.append(at)
        out.landmarks.append(marks)
    out.bits, out.shift = key_width(fields, out.deepest)
    ghost = reads_ghost(n, ncols, ptr, idx)
    has = comp >= 0
    keys = (np.maximum(comp, 0).astype(np.uint64) << np.uint64(56)) | morton(field, out.bits, out.shift) | np.where(ghost, GHOST_BIT, np.uint64(0))
    keys[~has] = NO_COMPONENT
    out.keys = keys
    out.order = np.argsort(keys, kind="stable")
    out.inner_rows = int((has & ~ghost).sum())
    out.loose = int((~has).sum())
    return out
