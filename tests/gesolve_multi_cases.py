"""The cases and the driver that the goldens (tests/golden/make_golden_gesolve_multi.py), the CPU and the GPU tests of several pairs of the generalized problem
(-e gsi | gli | gai through lis_gesolve) share, on the pencils of tests/gesolve_cases.py.

The calls are those of the reference's test/getest5.c: lis_esolver_create -> lis_esolver_set_option -> lis_gesolve, then everything the solve left is read from
LIS_ESOLVER_STRUCT itself before lis_esolver_destroy (evalue[], resid[], iter[] of ss entries, evector[], rhistory), so that the reference's bits and this
library's come through one path."""
import ctypes as C
import math

import numpy as np

import gesolve_cases as gc
import lisdrv
from lis_amd import _capi as capi

ETOL = 1e-10
BIT_COMMON = " -etol 1e-10 -emaxiter 60 -eprint mem"
TREE_MAXITER = 150
TREE_COMMON = " -etol 1e-10 -emaxiter %d" % TREE_MAXITER
THREADS_BITS = (1, 8)
THREADS_TREE = (1, 2, 4, 8)
# (pencil, options): compared in every bit at T = 1 and 8
BIT_CASES = [
    ("P1", "-e gsi -ss 3 -ige gpi"),
    ("P1", "-e gsi -ss 3 -ige gii"),
    ("P1", "-e gsi -ss 2 -ige gii -shift 0.005"),
    ("P3v", "-e gsi -ss 3 -ige gii"),
    ("P3", "-e gli -ss 4"),
    ("P2", "-e gli -ss 4 -ige gcr"),
    ("P1", "-e gli -ss 3 -rval true"),
    ("P4", "-e gli -ss 4"),
    ("P3", "-e gai -ss 4"),
    ("P1", "-e gai -ss 3 -ige grqi"),
    ("P3v", "-e gai -ss 3 -rval true"),
]
# compared in the tree mode, mode by mode: (pencil, options, the modes that the reference must carry at T = 1, 2, 4 and 8)
TREE_CASES = [
    ("P3", "-e gli -ss 4", (0, 1, 2, 3)),
    ("P2", "-e gai -ss 4", (0, 1, 2, 3)),
    ("P3", "-e gsi -ss 2 -ige gii", (0,)),
]


def subspace(options):
    words = options.split()
    return int(words[words.index("-ss") + 1])


def key(kind, pencil, options, T):
    return "%s|%s|%s|T%d" % (kind, pencil, options, T)


def admitted(per_T, mode):
    """The admission rule of a tree case: per_T maps "T1", "T2", "T4", "T8" to {"iter": [...], "evalue_hex": [...]}.  The reference ends `mode` below -emaxiter
    at every T, at one finite eigenvalue: every T's within 2 etol of T = 1's."""
    ref = float.fromhex(per_T["T1"]["evalue_hex"][mode])
    for T in THREADS_TREE:
        v = per_T["T%d" % T]
        ev = float.fromhex(v["evalue_hex"][mode])
        if not (v["iter"][mode] < TREE_MAXITER and math.isfinite(ev) and abs(ev - ref) <= 2.0 * ETOL * abs(ref)):
            return False
    return True


def gesolve(lib, A, B, options):
    """lis_gesolve with `options` -> dict(err, status, evalue0, ss, x, evalue[ss]) and, unless the options hold -rval true (the reference leaves heap contents in
    them then), resid[ss], iter[ss], rhistory, evector[ss]; E and vx stay alive for the getters until release()."""
    n = A.contents.n
    ss = subspace(options)
    rval = "-rval true" in options
    vx = lisdrv.new_vector(lib, A)
    E = capi.PE()
    assert lib.lis_esolver_create(C.byref(E)) == 0
    assert lib.lis_esolver_set_option(options.encode(), E) == 0
    ev = C.c_double(-7.0)
    err = lib.lis_gesolve(A, B, vx, C.byref(ev), E)
    e = E.contents
    out = dict(err=err, status=e.retcode, evalue0=ev.value, ss=ss, rval=rval, E=E, vx=vx)
    if err == 0:
        out.update(x=lisdrv.get_vector(lib, vx, n), evalue=lisdrv._arr(e.evalue, ss, np.float64))
    if err == 0 and not rval:
        count = e.iter[0] + 1 - (1 if e.retcode != 0 else 0)
        vecs = C.cast(e.evector, C.POINTER(capi.PV))
        out.update(resid=lisdrv._arr(e.resid, ss, np.float64), iter=lisdrv._arr(e.iter, ss, np.int32), rhistory=lisdrv._arr(e.rhistory, count, np.float64),
                   evector=[lisdrv.get_vector(lib, vecs[i], n) for i in range(ss)])
    return out


def release(lib, res):
    lib.lis_esolver_destroy(res.pop("E"))
    lib.lis_vector_destroy(res.pop("vx"))


def make_pencil(lib, name):
    a, b = gc.PENCILS[name]()
    return lisdrv.make_csr(lib, *a), lisdrv.make_csr(lib, *b)
