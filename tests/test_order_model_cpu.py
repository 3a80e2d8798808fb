"""tests/order_model.py held to something independent of it, and every matrix of tests/order_cases.py held to the edge it was built
for -- through the model's own outputs (shift, batches used, components found, size of the no-component bucket), so a case cannot
quietly stop covering its edge.  No GPU here: tests/test_order_gpu.py holds the kernels of kernels/csr_order.hpp to the model."""
from collections import deque

import numpy as np
import pytest

import order_cases as oc
import order_model as om

model_of = oc.model_of


def queue_bfs(n, ptr, idx, src):
    dist = [-1] * n
    dist[src] = 0
    q = deque([src])
    ptr, idx = ptr.tolist(), idx.tolist()
    while q:
        v = q.popleft()
        for k in range(ptr[v], ptr[v + 1]):
            c = idx[k]
            if 0 <= c < n and c != v and dist[c] < 0:
                dist[c] = dist[v] + 1
                q.append(c)
    return np.array(dist, np.int64)


@pytest.mark.parametrize("name", [c.name for c in oc.CASES])
def test_distances_against_a_queue(name):
    """the level-synchronous numpy search against a plain-Python queue, from vertex 0, the last vertex and a landmark"""
    c = oc.BY_NAME[name]
    g = om.Graph(c.n, c.ptr, c.idx)
    m = model_of(c)
    sources = {0, c.n - 1, c.n // 2} | ({m.landmarks[-1][-1]} if m.landmarks else set())
    for src in sorted(sources):
        want = queue_bfs(c.n, c.ptr, c.idx, src)
        dist, ecc = om.bfs(g, src)
        assert np.array_equal(dist, want), src
        assert ecc == want.max()


def test_morton_against_a_bit_loop():
    rng = np.random.default_rng(2)
    for fields in (3, 4, 5, 6):
        bits = min(15, 56 // fields)
        for shift in (0, 1, 3):
            dist = rng.integers(-1, 1 << (bits + shift + 1), (fields, 200))          # -1 and values past the clamp among them
            dist[:, 0] = (1 << bits) - 1
            dist[:, 1] = ((1 << bits) << shift) - 1
            got = om.morton(dist, bits, shift)
            for j in range(dist.shape[1]):
                code = 0
                for f in range(fields):
                    d = min(max(int(dist[f, j]), 0) >> shift, (1 << bits) - 1)
                    for b in range(bits):
                        if (d >> b) & 1:
                            code |= 1 << (fields * b + f)
                assert int(got[j]) == code, (fields, shift, j)
                assert code < 1 << 56                                               # the top byte is the component's
    assert [om.key_width(f, 1)[0] for f in (3, 4, 5, 6)] == [15, 14, 11, 9]
    assert om.key_width(6, 511) == (9, 0) and om.key_width(6, 512) == (9, 1) and om.key_width(3, 32767) == (15, 0) and om.key_width(3, 32768) == (15, 1)


@pytest.mark.parametrize("dims", [(5, 4, 3), (7, 7, 2), (1, 9, 6)])
def test_grid_keys_are_the_distance_triples(dims):
    """a x b x c 7-point grid, 3 landmarks: equal keys <=> equal distance triples (no field dropped, none shifted onto another), and a permutation"""
    a, b, c = dims
    n = a * b * c
    v = np.arange(n).reshape(c, b, a)
    u_, v_ = [], []
    for ax in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        u_.append(v[tuple(lo)].ravel()); v_.append(v[tuple(hi)].ravel())
    ptr, idx = oc.csr_of_edges(n, np.concatenate(u_), np.concatenate(v_), diagonal=np.ones(n, bool))
    m = om.order(n, n, ptr, idx, 3)
    assert m.found and m.components == 1 and m.shift == 0 and m.loose == 0 and m.inner_rows == n
    assert np.array_equal(np.sort(m.order), np.arange(n))
    g = om.Graph(n, ptr, idx)
    triples = np.stack([om.bfs(g, at)[0] for at in m.landmarks[0]], axis=1)
    # landmark 0 is the corner opposite vertex 0 (the only vertex at the largest distance)
    assert m.landmarks[0][0] == n - 1
    for i in range(n):
        same_key = m.keys == m.keys[i]
        same_triple = (triples == triples[i]).all(axis=1)
        assert np.array_equal(same_key, same_triple), i
    assert np.all(np.diff(m.keys[m.order].astype(np.uint64)) >= 0)


def test_star_is_stable():
    """all leaves but the landmarks share one key: they come out in index order"""
    c = oc.BY_NAME["star_5000"]
    m = model_of(c)
    assert m.landmarks[0] == [1, 2, 3]
    assert m.order[:6].tolist() == [0, 3, 2, 1, 4, 5]
    assert np.array_equal(m.order[4:], np.arange(4, c.n))
    assert len(np.unique(m.keys[4:])) == 1


def test_path_landmarks_and_budget():
    for n in (10, 11, 4672):
        p = oc.path(n)
        m = om.order(n, n, p.ptr, p.idx, 3)
        assert m.landmarks[0] == [n - 1, 0, (n - 1) // 2], n
    assert model_of(oc.BY_NAME["path_4672"]).batches == om.BATCHES
    m = model_of(oc.BY_NAME["path_4673"])
    assert not m.found and m.batches > om.BATCHES
    assert [om.batches_of(d) for d in (0, 31, 32, 63, 64)] == [1, 1, 2, 2, 3]


def test_ladders_cross_the_key_width():
    got = {k: model_of(oc.BY_NAME[f"ladder_{k}_L6"]) for k in (510, 511, 1100)}
    assert (got[510].deepest, got[510].shift) == (511, 0)
    assert (got[511].deepest, got[511].shift) == (512, 1)
    assert (got[1100].shift, got[1100].batches) == (2, 197)
    deep = model_of(oc.BY_NAME["ladder_2100_L5"])
    assert deep.bits == 11 and deep.deepest > 2048 and deep.shift >= 1


@pytest.mark.parametrize("name", [c.name for c in oc.CASES])
def test_case_reaches_its_edge(name):
    """what the catalogue promises for the case, from the model's own outputs; a found order is a permutation sorted by key"""
    c = oc.BY_NAME[name]
    m = model_of(c)
    e = dict(c.expect)
    assert m.found == e.pop("found")
    if "shift" in e:
        assert m.shift == e.pop("shift")
    if "shift_min" in e:
        assert m.shift >= e.pop("shift_min") > 0
    for what in ("batches", "components", "loose", "declined_in", "deepest"):
        if what in e:
            assert getattr(m, what) == e.pop(what), what
    if "landmarks0" in e:
        assert m.landmarks[0] == e.pop("landmarks0")
    if "head" in e:
        head = e.pop("head")
        assert m.order[:len(head)].tolist() == head
    assert not e, e                                                     # nothing promised that nobody checks
    if not m.found:
        return
    assert np.array_equal(np.sort(m.order), np.arange(c.n))
    assert m.batches <= om.BATCHES
    assert m.inner_rows == om.inner_rows(c.n, c.ncols, c.ptr, c.idx)
    if m.loose:                                                         # components past the eighth and loose rows: last, in index order
        tail = m.order[c.n - m.loose:]
        assert np.all(np.diff(tail) > 0) and np.all(m.keys[tail] == om.NO_COMPONENT)
    if c.symmetric:
        rows = np.repeat(np.arange(c.n), np.diff(c.ptr))
        own = (c.idx >= 0) & (c.idx < c.n)
        a = set(zip(rows[own].tolist(), c.idx[own].tolist()))
        assert all((j, i) in a for i, j in a)                           # the pattern the model is specified for


def test_catalogue_covers_the_edges():
    names = set(oc.BY_NAME)
    for n in oc.SIZES:
        for kind in ("natural", "random"):
            for lm in (3, 6):
                assert f"grid_{n}_{kind}_L{lm}" in names
    landmarks = [c.landmarks for c in oc.CASES]
    assert landmarks.count(4) >= 1 and landmarks.count(5) >= 2
    comps = {model_of(oc.BY_NAME[k]).components for k in names if k.startswith("components_") and not k.endswith("_ghosts")}
    assert comps == {1, 3, 8}                                           # 1; vertex 0 alone + 2; 8 reached from below, exactly and from above
    g = model_of(oc.BY_NAME["ghost_grid_declared"])
    u = model_of(oc.BY_NAME["ghost_grid_undeclared"])
    c = oc.BY_NAME["ghost_grid_declared"]
    ghosts = int(om.reads_ghost(c.n, c.ncols, c.ptr, c.idx).sum())
    assert 200 < ghosts < 320 and g.inner_rows == c.n - ghosts and u.inner_rows == c.n - 1
    assert om.reads_ghost(c.n, c.ncols, c.ptr, c.idx)[1234] and g.keys[1234] == om.NO_COMPONENT          # the lone ghost reader: no component, not inner
    assert not np.array_equal(g.order, u.order) and (c.idx < 0).sum() == 6
    assert np.all(om.reads_ghost(c.n, c.ncols, c.ptr, c.idx)[g.order[g.inner_rows:c.n - 1]])             # the rows that read a ghost: behind all that read none
    for name in ("components_3_ghosts", "components_10_zero_alone_ghosts"):                               # ghost readers in several components: behind ALL rows that read none
        c, m = oc.BY_NAME[name], model_of(oc.BY_NAME[name])
        ghost, comp = om.reads_ghost(c.n, c.ncols, c.ptr, c.idx), (m.keys >> np.uint64(56)) & np.uint64(7)
        front, back = m.order[:m.inner_rows], m.order[m.inner_rows:c.n - m.loose]
        assert not ghost[front].any() and ghost[back].all() and ghost[m.order[c.n - m.loose:]].any()
        assert len(np.unique(comp[front])) == m.components and len(np.unique(comp[back])) >= 3
        assert np.all(np.diff(comp[front].astype(np.int64)) >= 0) and np.all(np.diff(comp[back].astype(np.int64)) >= 0)
    k = model_of(oc.BY_NAME["bipartite_40_3000"])
    _, counts = np.unique(k.keys, return_counts=True)
    assert counts.max() == 3000 > 2048                                                                    # one key fills whole sort tiles
