"""liship_csr_order -- the numbering of kernels/csr_order.hpp (breadth-first searches from landmarks, Morton keys, the stable radix sort)
without the size gate and the keep rule of liship_csr_plan_reorder -- against tests/order_model.py, index by index, on the matrices of
tests/order_cases.py: each built to one edge of the kernels (256-thread grids, 2048-element sort tiles and their 256-element rounds,
batches of 32 levels under the budget, 8 components, the key's bit budget, the ghost-row bit).  tests/test_order_model_cpu.py holds
the model to independent statements and every case to its edge.

There is no tolerance here: order, inner_rows and found equal the model's, and a second call returns the same array."""
import ctypes as C

import numpy as np
import pytest

import lis_amd
import order_cases as oc
import order_model as om
from lis_amd import DeviceArray as DA

pytestmark = pytest.mark.gpu
model_of = oc.model_of
ERR_ARG = -1
UNWRITTEN = -7


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the ordering has no CPU fallback"
    assert not lib.liship_missing
    return lib


def run_order(lib, n, ncols, ptr, idx, landmarks):
    """one call of the door: (return code, found, order, inner_rows); order is filled with UNWRITTEN beforehand"""
    dptr, didx = DA.from_host(ptr, np.int32), DA.from_host(idx, np.int32)
    order = np.full(max(n, 1), UNWRITTEN, np.int32)
    inner, found = C.c_int(UNWRITTEN), C.c_int(UNWRITTEN)
    rc = lib.liship_csr_order(n, ncols, dptr.ptr, didx.ptr, landmarks, order.ctypes.data, C.addressof(inner), C.addressof(found), None)
    return rc, found.value, order[:n], inner.value


def assert_matches_model(lib, case):
    m = model_of(case)
    runs = [run_order(lib, case.n, case.ncols, case.ptr, case.idx, case.landmarks) for _ in range(2)]
    for rc, found, order, inner in runs:
        assert rc == 0
        assert found == (1 if m.found else 0)
        if m.found:
            assert inner == m.inner_rows
            bad = np.flatnonzero(order != m.order)
            assert bad.size == 0, (case.name, "first difference at", int(bad[0]), order[bad[:8]], m.order[bad[:8]], "shift", m.shift, "batches", m.batches)
    assert np.array_equal(runs[0][2], runs[1][2])


SYMMETRIC = [c.name for c in oc.CASES if c.symmetric and c.expect["found"]]


@pytest.mark.parametrize("name", SYMMETRIC)
def test_order_equals_the_model(lib, name):
    case = oc.BY_NAME[name]
    m = model_of(case)
    print(name, "n", case.n, "fields", m.fields, "shift", m.shift, "batches", m.batches, "components", m.components, "loose", m.loose)
    if "shift" in case.expect and case.expect["shift"] > 0 or "shift_min" in case.expect:
        assert m.shift > 0                                              # the case is for a key that loses low distance bits
    assert_matches_model(lib, case)


def test_order_declines_at_the_level_budget_and_recovers(lib):
    """512 batches are served, the 513th declines -- found = 0, no error -- in the first component or in the second; the next ordering in
    the same process is not affected"""
    assert model_of(oc.BY_NAME["path_4672"]).batches == om.BATCHES
    assert_matches_model(lib, oc.BY_NAME["path_4672"])
    for name in ("path_4673", "budget_second_component"):
        case = oc.BY_NAME[name]
        assert not model_of(case).found
        rc, found, order, inner = run_order(lib, case.n, case.ncols, case.ptr, case.idx, case.landmarks)
        assert (rc, found) == (0, 0), name
        assert_matches_model(lib, oc.BY_NAME["grid_2049_random_L3"])


@pytest.mark.parametrize("name", [c.name for c in oc.CASES if not c.symmetric])
def test_order_of_a_nonsymmetric_pattern(lib, name):
    """the model is not defined here; the contract is: a permutation, the same on two runs, inner_rows = rows with a component"""
    case = oc.BY_NAME[name]
    for ncols in (case.n, case.n + 3):                                  # (no column reaches [n, n + 3): declaring them changes nothing)
        a, b = (run_order(lib, case.n, ncols, case.ptr, case.idx, case.landmarks) for _ in range(2))
        assert a[:2] == (0, 1) and b[:2] == (0, 1)
        assert np.array_equal(np.sort(a[2]), np.arange(case.n))
        assert np.array_equal(a[2], b[2])
        assert a[3] == b[3] == om.inner_rows(case.n, ncols, case.ptr, case.idx)


def test_order_argument_edges(lib):
    case = oc.BY_NAME["grid_513_random_L3"]
    dptr, didx = DA.from_host(case.ptr, np.int32), DA.from_host(case.idx, np.int32)
    order, inner, found = np.full(case.n, UNWRITTEN, np.int32), C.c_int(UNWRITTEN), C.c_int(UNWRITTEN)
    # n = 0: nothing to order, null pointers and all
    assert lib.liship_csr_order(0, 0, None, None, 3, None, None, C.addressof(found), None) == 0 and found.value == 1
    assert lib.liship_csr_order(0, 0, dptr.ptr, didx.ptr, 3, order.ctypes.data, C.addressof(inner), C.addressof(found), None) == 0
    assert found.value == 1 and inner.value == 0 and np.all(order == UNWRITTEN)
    # null pointers with n > 0, a negative n
    args = [dptr.ptr, didx.ptr, order.ctypes.data, C.addressof(inner), C.addressof(found)]
    for k in range(5):
        a = list(args); a[k] = None
        assert lib.liship_csr_order(case.n, case.n, a[0], a[1], 3, a[2], a[3], a[4], None) == ERR_ARG, k
    assert lib.liship_csr_order(-1, 0, *args[:2], 3, *args[2:], None) == ERR_ARG
    assert np.all(order == UNWRITTEN)
    # landmarks are clamped to 3 .. 6; ncols < n means no ghost columns
    want3, want6 = (om.order(case.n, case.n, case.ptr, case.idx, k).order for k in (3, 6))
    assert not np.array_equal(want3, want6)
    for landmarks, want in ((0, want3), (-5, want3), (3, want3), (99, want6), (7, want6)):
        rc, found_, got, _ = run_order(lib, case.n, case.n if landmarks else 0, case.ptr, case.idx, landmarks)
        assert (rc, found_) == (0, 1) and np.array_equal(got, want), landmarks
