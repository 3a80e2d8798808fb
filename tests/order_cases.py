"""The matrices liship_csr_order is held to tests/order_model.py on (tests/test_order_gpu.py), each built to ONE edge of
kernels/csr_order.hpp and kept small, and what the model must report for the case to have reached that edge (`expect`: asserted
for every case by tests/test_order_model_cpu.py, so a case cannot quietly stop covering its edge).

A case is a namespace: name, n, ncols, ptr, idx (int32 CSR pattern: the ordering reads no values), landmarks, symmetric, expect.
expect keys: found, shift / shift_min, batches, components, loose, declined_in, deepest, landmarks0 (component 0's), head (the first
entries of the order).  The edges: 256-thread grids, 2048-element sort tiles and their 256-element rounds, batches of 32 levels under a
budget of 512 batches, 8 components, the key's bit budget, the ghost-row bit."""
from types import SimpleNamespace

import numpy as np

import order_model as om

SIZES = [1, 2, 3, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 1]


def csr_of_edges(n, u, v, diagonal=None, extra=None):
    """the symmetric pattern of the undirected edges (u[k], v[k]); diagonal: a mask of rows that store their own column too;
    extra: (rows, columns) entries appended as they are (ghost and negative columns: no vertices, no symmetry asked)"""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    rows, cols = np.concatenate([u, v]), np.concatenate([v, u])
    if diagonal is not None:
        d = np.flatnonzero(diagonal)
        rows, cols = np.concatenate([rows, d]), np.concatenate([cols, d])
    if extra is not None:
        rows, cols = np.concatenate([rows, np.asarray(extra[0], np.int64)]), np.concatenate([cols, np.asarray(extra[1], np.int64)])
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return ptr, cols.astype(np.int32)


def grid_edges(n):
    """a 5-point grid of width ~sqrt(n), row by row, cut to its first n vertices"""
    w = max(2, int(np.sqrt(n)))
    i = np.arange(n, dtype=np.int64)
    right = i[((i + 1) % w != 0) & (i + 1 < n)]
    down = i[i + w < n]
    return np.concatenate([right, down]), np.concatenate([right + 1, down + w])


def case(name, n, ptr, idx, landmarks, ncols=None, symmetric=True, **expect):
    expect.setdefault("found", True)
    return SimpleNamespace(name=name, n=n, ncols=n if ncols is None else ncols, ptr=ptr, idx=idx, landmarks=landmarks, symmetric=symmetric, expect=expect)


def grid(n, landmarks, scramble):
    u, v = grid_edges(n)
    if scramble:
        p = np.random.default_rng(1000 + n).permutation(n)
        u, v = p[u], p[v]
    diag = np.arange(n) % 3 != 1                                      # most rows store their diagonal, as matrices do: it is no neighbour
    ptr, idx = csr_of_edges(n, u, v, diagonal=diag)
    return case(f"grid_{n}_{'random' if scramble else 'natural'}_L{landmarks}", n, ptr, idx, landmarks, components=1, loose=0, shift=0)


def path(n, landmarks=3, **expect):
    i = np.arange(n - 1)
    ptr, idx = csr_of_edges(n, i, i + 1, diagonal=np.ones(n, bool))
    return case(f"path_{n}", n, ptr, idx, landmarks, **expect)


def ladder(k, landmarks, scramble=False, **expect):
    """2 x k: vertex (i, j) is 2 i + j; scramble: numbered at random but for vertex 0 (in index order, distances that share a shifted cell stay sorted: a lost shift would not show)"""
    i = np.arange(k - 1)
    u = np.concatenate([2 * i, 2 * i + 1, 2 * np.arange(k)])
    v = np.concatenate([2 * i + 2, 2 * i + 3, 2 * np.arange(k) + 1])
    if scramble:
        p = np.concatenate([[0], 1 + np.random.default_rng(k).permutation(2 * k - 1)])
        u, v = p[u], p[v]
    ptr, idx = csr_of_edges(2 * k, u, v)
    return case(f"ladder_{k}_L{landmarks}{'_random' if scramble else ''}", 2 * k, ptr, idx, landmarks, components=1, loose=0, **expect)


def star(n=5000):
    ptr, idx = csr_of_edges(n, np.zeros(n - 1, np.int64), np.arange(1, n))
    return case(f"star_{n}", n, ptr, idx, 3, components=1, loose=0, shift=0, landmarks0=[1, 2, 3], head=[0, 3, 2, 1, 4, 5])


def bipartite(a=40, b=3000):
    """complete K(a, b): two keys carry all vertices but the landmarks -- whole rounds and tiles of one digit"""
    u = np.repeat(np.arange(a), b)
    v = np.tile(np.arange(a, a + b), a)
    ptr, idx = csr_of_edges(a + b, u, v)
    return case(f"bipartite_{a}_{b}", a + b, ptr, idx, 3, components=1, loose=0, shift=0)


def all_loose(n=5000):
    """empty and diagonal-only rows: vertex 0 is component 0 on its own, everybody else the last bucket, in index order"""
    ptr, idx = csr_of_edges(n, [], [], diagonal=np.arange(n) % 2 == 0)
    return case(f"all_loose_{n}", n, ptr, idx, 3, components=1, loose=n - 1, shift=0, batches=4, head=[0, 1, 2, 3])


def tree_plus(m, rng):
    """a connected graph on m vertices: a random tree and a few chords"""
    u = np.arange(1, m)
    v = (rng.random(m - 1) * u).astype(np.int64)                       # parent of k: somebody before it
    cu, cv = rng.integers(0, m, m // 3), rng.integers(0, m, m // 3)
    keep = cu != cv
    return np.concatenate([u, cu[keep]]), np.concatenate([v, cv[keep]])


def interleaved_components(k, zero_alone, seed, ghosts=0):
    """k connected components of unequal sizes, their vertices spread over the index space, with empty rows and diagonal-only rows in
    between; zero_alone: vertex 0 has no neighbour (it is component 0 all the same).  Components are numbered by their smallest
    index; those past the eighth, and the loose rows, come last in index order.  ghosts: that many entries in ghost columns [n, n + 8),
    declared: the rows of EVERY component that read one come behind the rows of every component that read none."""
    rng = np.random.default_rng(seed)
    sizes = [23 + 41 * ((5 * j) % 7) + 3 * j for j in range(k)]
    loose = 150 + (1 if zero_alone else 0)
    n = sum(sizes) + loose
    where = rng.permutation(np.arange(1, n)) if zero_alone else rng.permutation(n)
    if not zero_alone:                                                 # vertex 0 belongs to a component (a loose vertex 0 would take a slot of its own)
        j = int(np.flatnonzero(where == 0)[0])
        where[0], where[j] = where[j], where[0]
    us, vs, at, firsts = [], [], 0, []
    for m in sizes:
        lab = where[at:at + m]
        at += m
        u, v = tree_plus(m, rng)
        us.append(lab[u]); vs.append(lab[v]); firsts.append(int(lab.min()))
    loose_rows = np.concatenate([where[at:], [0]]) if zero_alone else where[at:]
    diag = np.zeros(n, bool)
    diag[loose_rows[::2]] = True                                       # half of the loose rows hold their diagonal, half nothing
    diag[where[:at:5]] = True
    extra = (rng.integers(0, n, ghosts), n + rng.integers(0, 8, ghosts)) if ghosts else None
    ptr, idx = csr_of_edges(n, np.concatenate(us), np.concatenate(vs), diagonal=diag, extra=extra)
    slots = om.MAX_COMPONENTS - (1 if zero_alone else 0)
    by_first = np.argsort(firsts)                                     # the order the seeds are found in
    left_out = sum(sizes[j] for j in by_first[slots:])
    return case(f"components_{k}{'_zero_alone' if zero_alone else ''}{'_ghosts' if ghosts else ''}", n, ptr, idx, 3, ncols=n + 8 if ghosts else n, components=min(k + (1 if zero_alone else 0), om.MAX_COMPONENTS),
                loose=loose - (1 if zero_alone else 0) + left_out, shift=0)


def ghost_grid(declared):
    """a randomly numbered grid whose rows also read 300 ghost columns [n, n + 8), a few columns < 0, and one row that reads a ghost
    column and nothing else (no component: it reads a ghost and is not inner).  declared: ncols = n + 8; else ncols = n and the
    same entries are nobody's business."""
    n = 3001
    rng = np.random.default_rng(77)
    u, v = grid_edges(n - 1)
    p = rng.permutation(np.delete(np.arange(n), 1234))                 # the grid's vertices: everybody but 1234, the lone ghost reader
    u, v = p[u], p[v]
    rows = np.concatenate([rng.integers(0, n, 300), [1234], rng.integers(0, n, 6)])
    cols = np.concatenate([n + rng.integers(0, 8, 300), [n + 5], np.full(6, -1)])
    ptr, idx = csr_of_edges(n, u, v, diagonal=np.arange(n) != 1234, extra=(rows, cols))
    return case(f"ghost_grid_{'declared' if declared else 'undeclared'}", n, ptr, idx, 3, ncols=n + 8 if declared else n, components=1, loose=1, shift=0)


def budget_second_component():
    """a triangle {0, 1, 2} (4 batches), then a path whose four searches need 512 on their own"""
    n = 3 + 4672
    i = 3 + np.arange(4671)
    ptr, idx = csr_of_edges(n, np.concatenate([[0, 1, 2], i]), np.concatenate([[1, 2, 0], i + 1]))
    return case("budget_second_component", n, ptr, idx, 3, found=False, declined_in=1, batches=516)


def random_directed(n=3000):
    rng = np.random.default_rng(5)
    rows, cols = np.repeat(np.arange(n), 3), rng.integers(0, n, 3 * n)
    keep = rng.random(3 * n) < 0.8
    o = np.lexsort((cols[keep], rows[keep]))
    rows, cols = rows[keep][o], cols[keep][o]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return case("random_directed", n, ptr, cols.astype(np.int32), 3, symmetric=False)


def upper_triangular(n=3000):
    rng = np.random.default_rng(6)
    rows = np.repeat(np.arange(n), 3)
    cols = rows + rng.integers(0, 40, 3 * n)                          # the diagonal now and then, else up to 39 to the right
    keep = cols < n
    rows, cols = rows[keep], cols[keep]
    o = np.lexsort((cols, rows))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return case("upper_triangular", n, ptr, cols[o].astype(np.int32), 4, symmetric=False)


def _build():
    cases = []
    for n in SIZES:
        for scramble in (False, True):
            for landmarks in (3, 6):
                cases.append(grid(n, landmarks, scramble))
    cases += [grid(2049, 4, True), grid(4097, 5, True)]
    cases += [star(), bipartite(), all_loose()]
    cases += [ladder(510, 6, deepest=511, shift=0), ladder(511, 6, deepest=512, shift=1), ladder(1100, 6, shift=2, batches=197),
              ladder(2100, 5, shift_min=1), ladder(511, 6, scramble=True, deepest=512, shift=1)]
    cases += [path(4672, found=True, batches=512, components=1, loose=0, landmarks0=[4671, 0, 2335]),
              path(4673, found=False, declined_in=0), budget_second_component()]
    cases += [interleaved_components(1, False, 11), interleaved_components(2, True, 12), interleaved_components(8, False, 13),
              interleaved_components(8, True, 14), interleaved_components(9, False, 15), interleaved_components(12, True, 16)]
    cases += [ghost_grid(True), ghost_grid(False), interleaved_components(3, False, 17, ghosts=120), interleaved_components(10, True, 18, ghosts=300)]
    cases += [random_directed(), upper_triangular()]
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_MODEL = {}


def model_of(case):
    """the model's answer for a case, computed once and shared by the tests that need it"""
    if case.name not in _MODEL:
        _MODEL[case.name] = om.order(case.n, case.ncols, case.ptr, case.idx, case.landmarks)
    return _MODEL[case.name]
