"""X -> CSR: numpy models of the seven conversions the library serves in HBM, and the matrices they are tested on.

A source is a dict: fmt ("ell", "dia", "bsr", "dns", "vbr", "csc", "jad"), n, and the format's arrays under the names lisdrv.matrix_arrays / vbr_cases give
them.  model(src) -> (ptr, index, value): for every row the kept entries in the order of lis_matrix_convert_<fmt>2csr (lis_convert.c lisi_convert_to_csr
restates those routines), one loop nest per format.  "Kept" is the C comparison value != 0.0: +0.0 and -0.0 go, NaN, infinities and subnormals stay; CSC and
JAD keep everything.  tests/test_tocsr_cpu.py holds the models to the reference and to the library's host routine, tests/test_tocsr_gpu.py holds the kernels
and the library's HBM path to the models.

The sources: every CSR matrix of tests/convert_cases.py that has edges worth keeping (EDGES, empties, unsorted, duplicates, specials) in every format -- X from
the oracle's csr2<fmt>, csr2dns of coo_dns_cases, csr2vbr of vbr_cases -- plus sources written down as arrays (HAND) for what no conversion from CSR produces:
stored zeros of either sign next to NaN / inf / subnormals in one row, a row that loses every entry and one that loses none, maxnzr = 1 and nnd = 1, the DIA
offsets -(n-1) and n-1, BSR blocks out of column order with n % bnr != 0, VBR blocks of 1 .. 3 rows holding zeros, one-row matrices.  random_source makes the
kernel-level inputs: any n and width, values with zeros of both signs and the special values mixed in."""
import numpy as np

import convert_cases as cc
import coo_dns_cases as dc
import vbr_cases as vc

I32, F64 = np.int32, np.float64
FORMATS = ("ell", "dia", "bsr", "dns", "vbr", "csc", "jad")
KERNEL_FORMATS = ("ell", "dia", "bsr", "dns", "vbr")          # the others are a copy of the source's row-form HBM copy
BSR_SHAPES = ((2, 2), (3, 2), (1, 1))
CSR_CASES = cc.EDGES + ["empties", "unsorted", "duplicates", "specials"]
SUBNORMAL = 5e-324
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], np.uint64).view(F64)[0]
SPECIAL_ROW = [0.0, -0.0, np.nan, np.inf, -np.inf, SUBNORMAL, NAN_PAYLOAD, -0.0]      # one row's stored values: three go, five stay


# ---------------------------------------------------------------- the models
def _csr(rows):
    """rows: per row a list of (column, value)"""
    ptr = np.zeros(len(rows) + 1, I32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([c for r in rows for c, _ in r], I32), np.array([v for r in rows for _, v in r], F64)


def ell2csr(s):
    n, mx = s["n"], s["maxnzr"]
    rows = [[] for _ in range(n)]
    for j in range(mx):
        for i in range(n):
            if s["value"][j * n + i] != 0.0:
                rows[i].append((s["index"][j * n + i], s["value"][j * n + i]))
    return _csr(rows)


def dia2csr(s):
    n, np_ = s["n"], s.get("np", s["n"])
    rows = [[] for _ in range(n)]
    for d in range(s["nnd"]):
        for i in range(n):
            col = i + int(s["index"][d])
            if 0 <= col < np_ and s["value"][d * n + i] != 0.0:
                rows[i].append((col, s["value"][d * n + i]))
    return _csr(rows)


def bsr2csr(s):
    n, bnr, bnc = s["n"], s["bnr"], s["bnc"]
    bs, pad = bnr * bnc, (bnc - n % bnc) % bnc
    rows = [[] for _ in range(n)]
    for br in range(s["nr"]):
        for b in range(s["bptr"][br], s["bptr"][br + 1]):
            for jc in range(bnc):
                for ii in range(bnr):
                    r, v = br * bnr + ii, s["value"][b * bs + jc * bnr + ii]
                    if r >= n or not (v != 0.0):
                        continue
                    col = int(s["bindex"][b]) * bnc + jc
                    if col >= n + pad:
                        col -= pad
                    elif col >= n:
                        continue
                    rows[r].append((col, v))
    return _csr(rows)


def dns2csr(s):
    n, np_ = s["n"], s.get("np", s["n"])
    rows = [[] for _ in range(n)]
    for i in range(n):
        for j in range(np_):
            if s["value"][j * n + i] != 0.0:
                rows[i].append((j, s["value"][j * n + i]))
    return _csr(rows)


def vbr2csr(s):
    rows = [[] for _ in range(s["n"])]
    for bi in range(s["nr"]):
        l, bnr = int(s["row"][bi]), int(s["row"][bi + 1] - s["row"][bi])
        for i in range(bnr):
            for bj in range(s["bptr"][bi], s["bptr"][bi + 1]):
                c0 = int(s["col"][s["bindex"][bj]])
                bnc = int(s["col"][s["bindex"][bj] + 1]) - c0
                for j in range(bnc):
                    v = s["value"][int(s["ptr"][bj]) + j * bnr + i]
                    if v != 0.0:
                        rows[l + i].append((c0 + j, v))
    return _csr(rows)


def csc2csr(s):
    rows = [[] for _ in range(s["n"])]
    for col in range(s.get("np", s["n"])):
        for k in range(s["ptr"][col], s["ptr"][col + 1]):
            rows[s["index"][k]].append((col, s["value"][k]))
    return _csr(rows)


def jad2csr(s):
    rows = [[] for _ in range(s["n"])]
    for j in range(s["maxnzr"]):
        for k in range(s["ptr"][j + 1] - s["ptr"][j]):
            rows[s["row"][k]].append((s["index"][s["ptr"][j] + k], s["value"][s["ptr"][j] + k]))
    return _csr(rows)


# what the upload of a CSC / JAD matrix lays out in HBM (lis_upload.c upload_csc_as_csr / upload_jad_as_csr, restated loop for loop: a count per row, its
# prefix sum, then a cursor per row that the entries advance in the order the reference's product adds them).  lis_convert_tocsr.c copies these rows as the
# conversion, so they must BE the models above
def csc_upload_rows(s):
    n, np_, nnz = s["n"], s.get("np", s["n"]), len(s["index"])
    tptr = np.zeros(n + 2, I32)
    for k in range(nnz):
        tptr[s["index"][k] + 1] += 1
    for r in range(n):
        tptr[r + 1] += tptr[r]
    fill, tidx, tval = tptr[:n].copy(), np.zeros(nnz, I32), np.zeros(nnz, F64)
    for c in range(np_):
        for k in range(s["ptr"][c], s["ptr"][c + 1]):
            dst = fill[s["index"][k]]
            fill[s["index"][k]] += 1
            tidx[dst], tval[dst] = c, s["value"][k]
    return tptr[:n + 1].copy(), tidx, tval


def jad_upload_rows(s):
    n, nnz, mx = s["n"], len(s["index"]), s["maxnzr"]
    cptr = np.zeros(n + 2, I32)
    for j in range(mx):
        for k in range(s["ptr"][j + 1] - s["ptr"][j]):
            cptr[s["row"][k] + 1] += 1
    for r in range(n):
        cptr[r + 1] += cptr[r]
    fill, cidx, cval = cptr[:n].copy(), np.zeros(nnz, I32), np.zeros(nnz, F64)
    for j in range(mx):
        b = int(s["ptr"][j])
        for k in range(s["ptr"][j + 1] - b):
            dst = fill[s["row"][k]]
            fill[s["row"][k]] += 1
            cidx[dst], cval[dst] = s["index"][b + k], s["value"][b + k]
    return cptr[:n + 1].copy(), cidx, cval


MODELS = dict(ell=ell2csr, dia=dia2csr, bsr=bsr2csr, dns=dns2csr, vbr=vbr2csr, csc=csc2csr, jad=jad2csr)


def model(src):
    return MODELS[src["fmt"]](src)


def counts(src):
    """what the count kernels leave per row"""
    return np.diff(model(src)[0]).astype(I32)


def dns_slab_counts(src, slab):
    """count[i * nslab + s]: kept entries of row i on the columns s * slab .. of the DNS count kernel"""
    n, np_ = src["n"], src.get("np", src["n"])
    keep = src["value"].reshape(np_, n).T != 0.0
    nslab = (np_ + slab - 1) // slab
    out = np.zeros((n, nslab), I32)
    for s in range(nslab):
        out[:, s] = keep[:, s * slab:(s + 1) * slab].sum(axis=1)
    return out.ravel()


def same_csr(got, want):
    """(ok, which array differs): integers equal, every bit of every value"""
    for k, g, w in zip(("ptr", "index", "value"), got, want):
        if k == "value":
            if not cc.same_bits(g, w):
                return False, k
        elif not np.array_equal(np.asarray(g), np.asarray(w)):
            return False, k
    return True, None


# ---------------------------------------------------------------- sources made from the CSR cases
def from_csr(fmt, csr, bnr=2, bnc=2):
    ptr, idx, val = csr
    n = len(ptr) - 1
    if fmt == "dns":
        return dict(fmt=fmt, n=n, value=dc.csr2dns(ptr, idx, val))
    if fmt == "vbr":
        v, _ = vc.csr2vbr(ptr, idx, val)
        return dict(v, fmt=fmt)
    a = cc.oracle_arrays(fmt, ptr, idx, val, bnr, bnc)
    if fmt == "bsr":
        a.update(bnr=bnr, bnc=bnc)
    return dict(a, fmt=fmt, n=n)


def _specials_in_one_row(n=5, width=len(SPECIAL_ROW)):
    """ELL / DIA / DNS / BSR / VBR arrays of one small matrix pattern: row 1 stores SPECIAL_ROW, row 2 only zeros (every entry dropped), row 3 no zero (none dropped),
    rows 0 and 4 a mix"""
    v = np.empty((n, width))
    for i in range(n):
        v[i] = [(-1) ** k * (1.5 + i + k / 8.0) if (i + k) % 3 else 0.0 for k in range(width)]
    v[1] = SPECIAL_ROW
    v[2] = [0.0, -0.0] * (width // 2)
    v[3] = np.arange(1, width + 1) * -0.375
    return v


def _bsr_padding_zeroed(s):
    """value[] with +0.0 wherever a block reaches beyond the n rows or the n columns: what csr2bsr leaves there"""
    n, bnr, bnc = s["n"], s["bnr"], s["bnc"]
    v = s["value"].copy().reshape(-1, bnc, bnr)
    for br in range(s["nr"]):
        for b in range(s["bptr"][br], s["bptr"][br + 1]):
            for jc in range(bnc):
                for ii in range(bnr):
                    if br * bnr + ii >= n or s["bindex"][b] * bnc + jc >= n:
                        v[b, jc, ii] = 0.0
    return v.ravel()


# Where the reference defines nothing: lis_matrix_convert_bsr2csr counts EVERY non-zero of a block, so one in a padding row is counted past the end of ptr[]
# (a write behind the allocation) and one in a padding column comes out as a column >= n.  csr2bsr never stores such a value and the host routine skips them, as do
# the kernels; these sources are held to the host routine alone.
NO_REFERENCE = {"bsr_2x2_n7_padding": "non-zeros in the padding row and column", "bsr_3x2_n7_padding": "non-zeros in the padding rows and column",
                "bsr_2x2_n1": "non-zeros in the padding row and column"}


def hand():
    out = {}
    v = _specials_in_one_row()
    n, w = v.shape
    # ELL: slot j of row i on column (i + 2 j) % n -- out of order and repeating, as the format allows
    out["ell_specials"] = dict(fmt="ell", n=n, maxnzr=w, index=np.array([(i + 2 * j) % n for j in range(w) for i in range(n)], I32), value=v.T.ravel().copy())
    out["ell_maxnzr1"] = dict(fmt="ell", n=7, maxnzr=1, index=np.arange(6, -1, -1).astype(I32), value=np.array([1.0, 0.0, -2.0, -0.0, np.nan, 3.0, SUBNORMAL]))
    out["ell_n1"] = dict(fmt="ell", n=1, maxnzr=3, index=np.zeros(3, I32), value=np.array([0.0, -4.0, 4.0]))
    # DIA: 8 diagonals of an 8 x 8 matrix, offsets out of order, the two corners among them
    m = 8
    offs = np.array([0, -(m - 1), m - 1, 3, -2, 1, -5, 6], I32)
    dv = np.empty((8, m))
    for d in range(8):
        dv[d] = [SPECIAL_ROW[(i + d) % len(SPECIAL_ROW)] if (i * 3 + d) % 4 else 2.0 + i - d for i in range(m)]
    dv[:, 2] = [0.0, -0.0] * 4                                   # row 2: every entry dropped
    dv[:, 3] = np.arange(1, 9) * 0.5                             # row 3: none of those that reach it
    dv[1, m - 1], dv[2, 0] = 11.0, -11.0                         # the two corners of the matrix hold entries
    out["dia_corners"] = dict(fmt="dia", n=m, nnd=8, index=offs, value=dv.ravel().copy())
    out["dia_nnd1"] = dict(fmt="dia", n=6, nnd=1, index=np.array([-(6 - 1)], I32), value=np.array([9.0, 9.0, 9.0, 9.0, 9.0, -1.25]))
    out["dia_nnd1_top"] = dict(fmt="dia", n=6, nnd=1, index=np.array([6 - 1], I32), value=np.array([0.75, 9.0, 9.0, 9.0, 9.0, 9.0]))
    out["dia_n1"] = dict(fmt="dia", n=1, nnd=1, index=np.zeros(1, I32), value=np.array([-0.5]))
    # DNS
    dn = np.zeros((n, n))
    dn[:, :] = v[:, :n]
    dn[1, :] = SPECIAL_ROW[:n]
    out["dns_specials"] = dict(fmt="dns", n=n, value=dn.T.ravel().copy())
    out["dns_n1"] = dict(fmt="dns", n=1, value=np.array([np.inf]))
    # BSR: n % bnr != 0, the blocks of a block row out of column order, explicit zeros and specials inside the blocks, values in the padding rows / columns
    for bnr, bnc in BSR_SHAPES:
        nb = 7
        nr, nc = 1 + (nb - 1) // bnr, 1 + (nb - 1) // bnc
        rng = np.random.default_rng(100 * bnr + bnc)
        bptr, bindex = [0], []
        for br in range(nr):
            take = rng.permutation(nc)[:1 + br % 3].tolist()
            bindex += sorted(take, reverse=True) if br % 2 == 0 else take
            bptr.append(len(bindex))
        val = rng.uniform(-2, 2, len(bindex) * bnr * bnc)
        val[rng.uniform(size=len(val)) < 0.3] = 0.0
        val[1::5] = -0.0
        val[:len(SPECIAL_ROW)] = SPECIAL_ROW[:len(val)]
        s = dict(fmt="bsr", n=nb, bnr=bnr, bnc=bnc, nr=nr, nc=nc, bnnz=len(bindex), bptr=np.array(bptr, I32), bindex=np.array(bindex, I32), value=val)
        out["bsr_%dx%d_n7" % (bnr, bnc)] = dict(s, value=_bsr_padding_zeroed(s))
        if (nb % bnr or nb % bnc) and not np.array_equal(s["value"].view(np.uint64), out["bsr_%dx%d_n7" % (bnr, bnc)]["value"].view(np.uint64)):
            out["bsr_%dx%d_n7_padding" % (bnr, bnc)] = s              # values where no row / column of the matrix is: NO_REFERENCE
    out["bsr_2x2_n1"] = dict(fmt="bsr", n=1, bnr=2, bnc=2, nr=1, nc=1, bnnz=1, bptr=np.array([0, 1], I32), bindex=np.zeros(1, I32),
                             value=np.array([3.5, 7.0, 7.0, 7.0]))
    out["bsr_2x2_n1_clean"] = dict(out["bsr_2x2_n1"], value=np.array([3.5, 0.0, 0.0, 0.0]))
    # VBR: block rows and columns of 1 .. 3, blocks out of column order, zeros and the special values inside them
    heights = [1, 2, 3, 1, 3, 2]
    row = np.concatenate([[0], np.cumsum(heights)]).astype(I32)
    nv = int(row[-1])
    col = row.copy()
    rng = np.random.default_rng(17)
    bptr, bindex, vptr, chunks = [0], [], [0], []
    for bi, h in enumerate(heights):
        for bj in rng.permutation(len(heights))[:1 + bi % 3]:
            bindex.append(int(bj))
            blk = rng.uniform(-2, 2, (int(col[bj + 1] - col[bj]), h))
            blk[rng.uniform(size=blk.shape) < 0.35] = 0.0
            chunks.append(blk.ravel())
            vptr.append(vptr[-1] + blk.size)
        bptr.append(len(bindex))
    value = np.concatenate(chunks)
    value[2::7] = -0.0
    value[:len(SPECIAL_ROW)] = SPECIAL_ROW
    out["vbr_1to3"] = dict(fmt="vbr", n=nv, nr=len(heights), nc=len(heights), bnnz=len(bindex), nnz=len(value), row=row, col=col, ptr=np.array(vptr, I32),
                           bptr=np.array(bptr, I32), bindex=np.array(bindex, I32), value=value)
    out["vbr_n1"] = dict(fmt="vbr", n=1, nr=1, nc=1, bnnz=1, nnz=1, row=np.array([0, 1], I32), col=np.array([0, 1], I32), ptr=np.array([0, 1], I32),
                         bptr=np.array([0, 1], I32), bindex=np.zeros(1, I32), value=np.array([-6.0]))
    return out


HAND = hand()


def _sources():
    out = {}
    for name in CSR_CASES:
        for fmt in FORMATS:
            for bnr, bnc in (BSR_SHAPES if fmt == "bsr" else ((0, 0),)):
                out["%s-%s%s" % (name, fmt, "%dx%d" % (bnr, bnc) if fmt == "bsr" else "")] = (name, fmt, bnr, bnc)
    return out


FROM_CSR = _sources()                  # id -> (CSR case, fmt, bnr, bnc); the arrays are made when asked for (source)
_made = {}


def source(key):
    """the source dict of a FROM_CSR or HAND id; built once, never written to"""
    if key in HAND:
        return HAND[key]
    if key not in _made:
        name, fmt, bnr, bnc = FROM_CSR[key]
        _made[key] = from_csr(fmt, cc.CASES[name], bnr or 2, bnc or 2)
    return _made[key]


ALL = list(FROM_CSR) + list(HAND)


# ---------------------------------------------------------------- kernel-level inputs of any size
def _values(rng, count, zeros=0.3):
    v = rng.uniform(-2, 2, count)
    z = rng.uniform(size=count)
    v[z < zeros] = 0.0
    v[z < zeros / 2] = -0.0
    for k, s in enumerate(SPECIAL_ROW):
        if count > 3 * k + 1:
            v[3 * k + 1] = s
    return v


def random_source(fmt, n, width, seed=0):
    """fmt with n rows and `width` slots / diagonals / columns (DNS: np = width is not served by the library, which wants np = n: kernel level only) / blocks per block row"""
    rng = np.random.default_rng(1000003 * seed + 1009 * n + width + len(fmt))
    if fmt == "ell":
        return dict(fmt=fmt, n=n, maxnzr=width, index=rng.integers(0, n, n * width).astype(I32), value=_values(rng, n * width))
    if fmt == "dia":
        span = np.arange(-(n - 1), n)
        offs = [o for o in (-(n - 1), n - 1, 0) if o in span]
        offs = list(dict.fromkeys(offs))[:width]
        rest = [o for o in rng.permutation(span).tolist() if o not in offs]
        offs = (offs + rest)[:min(width, len(span))]
        offs = rng.permutation(np.array(offs)).astype(I32)
        return dict(fmt=fmt, n=n, nnd=len(offs), index=offs, value=_values(rng, n * len(offs)))
    if fmt == "dns":
        return dict(fmt=fmt, n=n, np=width, value=_values(rng, n * width))
    if fmt == "bsr":
        bnr, bnc = ((2, 2), (3, 2), (1, 1), (2, 3))[(n + width) % 4]
        nr, nc = 1 + (n - 1) // bnr, 1 + (n - 1) // bnc
        per = rng.integers(0, min(width, nc) + 1, nr)
        bptr = np.concatenate([[0], np.cumsum(per)]).astype(I32)
        bindex = np.concatenate([rng.permutation(nc)[:k] for k in per] + [np.zeros(0, np.int64)]).astype(I32)
        return dict(fmt=fmt, n=n, bnr=bnr, bnc=bnc, nr=nr, nc=nc, bnnz=len(bindex), bptr=bptr, bindex=bindex, value=_values(rng, len(bindex) * bnr * bnc))
    assert fmt == "vbr"
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(rng.integers(1, 4))))
    row = np.array(cuts, I32)
    col = row
    nr = len(row) - 1
    per = rng.integers(0, min(width, nr) + 1, nr)
    bptr = np.concatenate([[0], np.cumsum(per)]).astype(I32)
    bindex = np.concatenate([rng.permutation(nr)[:k] for k in per] + [np.zeros(0, np.int64)]).astype(I32)
    heights, widths = np.repeat(np.diff(row), per), np.diff(col)[bindex]
    ptr = np.concatenate([[0], np.cumsum(heights * widths)]).astype(I32)
    return dict(fmt=fmt, n=n, nr=nr, nc=nr, bnnz=len(bindex), nnz=int(ptr[-1]), row=row, col=col, ptr=ptr, bptr=bptr, bindex=bindex, value=_values(rng, int(ptr[-1])))
