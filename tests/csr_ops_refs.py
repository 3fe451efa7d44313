'''Plain numpy restatements of the matrix algebra of nh_csr_ops.hip -- transpose, selection, the sum of two patterns -- and the matrices the tests feed them.
No device, no library.  A matrix is a `Csr`: (values float64, rowptr int64, colidx int64, ncols), rows sorted and unique.  Index arrays are compared with
numpy.array_equal, values as int64 views (`bits`), so that NaN, -0.0 and the infinities count.  test_csr_ops_refs_host.py pins every function here to what
scipy computes for the same input, which is what the host path of HipMatrix returns.'''
import collections
import functools

import numpy

from pattern_refs import I64, ref_union, ref_pattern, random_csr, hub, fan, chain, empty_mesh

Csr = collections.namedtuple('Csr', 'values rowptr colidx ncols')


def bits(values):
    return numpy.ascontiguousarray(values, dtype=float).view(I64)


def same(a, b, computed=False):
    '''Two triplets are the same matrix, bit for bit.  `computed`: the values come out of an addition (a sum of matrices), and there a NaN equals any NaN.
    Which sign and payload the NaN of NaN + (-NaN) or of inf - inf carries is left open by IEEE 754, and implementations do differ: x86 returns the NaN of its
    first operand, so the answer depends on the order in which a compiler feeds a commutative addition (numpy's a + b and scipy's differ on this very input),
    and its inf - inf has the sign bit set where other hardware's has not.  Everything else -- that the entry is kept, that it is a NaN, every bit of every
    number, the sign of zero -- is compared.  A transpose or a submatrix copies, and is compared without this allowance.'''
    va, vb = bits(a[0]), bits(b[0])
    if computed and va.shape == vb.shape:
        both = numpy.isnan(a[0]) & numpy.isnan(b[0])
        va, vb = numpy.where(both, 0, va), numpy.where(both, 0, vb)
    return a[3] == b[3] and numpy.array_equal(a[1], b[1]) and numpy.array_equal(a[2], b[2]) and numpy.array_equal(va, vb)


def rows_of(rowptr):
    return numpy.repeat(numpy.arange(len(rowptr) - 1, dtype=I64), numpy.diff(rowptr))


# ---- references -------------------------------------------------------------------------------------------------------------------------------------

def ref_transpose(rowptr, colidx, ncols):
    '''(rowptr_t, colidx_t, pos) of nh_csr_transpose: pos[k'] is where entry k' of the transpose lies in the operand; rows of the transpose ascend'''
    colidx = numpy.asarray(colidx, dtype=I64)
    pos = numpy.argsort(colidx, kind='stable').astype(I64)  # (stable: within a column by position, that is by row)
    rowptr_t = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(colidx, minlength=ncols))]).astype(I64)
    return rowptr_t, rows_of(rowptr)[pos], pos


def ref_select(values, rowptr, colidx, ncols, rowkeep=None, colkeep=None, drop_zeros=False):
    '''(rowptr_s, colidx_s, pos, ncols_s) of nh_csr_select_*: entry k of row i stays iff rowkeep[i] and colkeep[colidx[k]] (None: all) and, with drop_zeros,
    values[k] != 0; kept rows and columns are numbered anew in ascending order'''
    nrows = len(rowptr) - 1
    rowkeep = numpy.ones(nrows, dtype=bool) if rowkeep is None else numpy.asarray(rowkeep) != 0
    colkeep = numpy.ones(ncols, dtype=bool) if colkeep is None else numpy.asarray(colkeep) != 0
    row = rows_of(rowptr)
    keep = rowkeep[row] & colkeep[colidx]
    if drop_zeros:
        keep &= numpy.asarray(values) != 0
    pos = numpy.flatnonzero(keep).astype(I64)
    newrow, newcol = numpy.cumsum(rowkeep) - 1, numpy.cumsum(colkeep) - 1
    rowptr_s = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(newrow[row[pos]], minlength=int(rowkeep.sum())))]).astype(I64)
    return rowptr_s, newcol[colidx[pos]].astype(I64), pos, int(colkeep.sum())


def ref_add(a, b, sign):
    '''the Csr of a + sign b as the device forms it: the union of the patterns, zero, a placed, sign b added, the entries that are exactly zero dropped'''
    assert a.ncols == b.ncols and sign in (1., -1.)
    rowptr, colidx, (pa, pb) = ref_union([(a.rowptr, a.colidx), (b.rowptr, b.colidx)])
    values = numpy.zeros(len(colidx))
    values[pa] = a.values
    with numpy.errstate(invalid='ignore'):
        values[pb] += sign * b.values
    rowptr_s, colidx_s, pos, _ = ref_select(values, rowptr, colidx, a.ncols, drop_zeros=True)
    return Csr(values[pos], rowptr_s, colidx_s, a.ncols)


def transposed(m):
    rowptr_t, colidx_t, pos = ref_transpose(m.rowptr, m.colidx, m.ncols)
    return Csr(m.values[pos], rowptr_t, colidx_t, len(m.rowptr) - 1)


def selected(m, rowkeep=None, colkeep=None):
    rowptr_s, colidx_s, pos, ncols_s = ref_select(m.values, m.rowptr, m.colidx, m.ncols, rowkeep, colkeep)
    return Csr(m.values[pos], rowptr_s, colidx_s, ncols_s)


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------------------

SPECIAL = numpy.array([numpy.nan, -numpy.nan, numpy.inf, -numpy.inf, -0., 0., 5e-324, -1.])  # stored zeros, both NaN signs: a transpose or a submatrix keeps them all

# row lengths below, at and above every lane count 1 .. 64 and twice that (a row of n entries at L lanes: n < L idle lanes, n = L one full vote, n > L strides)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 1)


def _with_values(rng, rowptr, colidx, ncols, special=True):
    values = rng.normal(size=len(colidx))
    if special and len(values):
        at = rng.permutation(len(values))[:len(SPECIAL)]
        values[at] = SPECIAL[:len(at)]
    return Csr(values, numpy.asarray(rowptr, dtype=I64), numpy.asarray(colidx, dtype=I64), int(ncols))


def _random(seed, nrows, ncols, density, empty_rows=(), empty_cols=()):
    rng = numpy.random.default_rng(seed)
    mask = rng.random((nrows, ncols)) < density
    mask[list(empty_rows)] = False
    mask[:, list(empty_cols)] = False
    return _with_values(rng, numpy.concatenate([[0], numpy.cumsum(mask.sum(1))]), numpy.nonzero(mask)[1], ncols)


def _rowlens():
    rng = numpy.random.default_rng(11)
    ncols = 140
    cols = [numpy.sort(rng.permutation(ncols)[:n]) for n in LENGTHS]
    return _with_values(rng, numpy.concatenate([[0], numpy.cumsum(LENGTHS)]), numpy.concatenate(cols), ncols)


def _from_conn(conn, seed):
    srowptr, scol, *_ = ref_pattern(*conn.args)
    return _with_values(numpy.random.default_rng(seed), srowptr, scol.astype(I64), conn.ncols)


def _dense_cross(n=3000, row=1500, col=1700):
    '''tridiagonal with one dense row and one dense column: an output row of the transpose longer than a workgroup sorts in LDS (2048), and a row longer than
    any number of lanes'''
    mask_rows = numpy.concatenate([numpy.arange(n), numpy.arange(n - 1), numpy.arange(1, n), numpy.full(n, row), numpy.arange(n)])
    mask_cols = numpy.concatenate([numpy.arange(n), numpy.arange(1, n), numpy.arange(n - 1), numpy.arange(n), numpy.full(n, col)])
    key = numpy.unique(mask_rows.astype(I64) * n + mask_cols)
    rowptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(key // n, minlength=n))])
    return _with_values(numpy.random.default_rng(5), rowptr, key % n, n)


def tridiagonal(n=262444):
    '''n rows of at most three entries.  Every grid of nh_csr_ops.hip strides: the kernels with one thread per entry (k_tr_count, k_tr_place, k_place, k_add_at)
    launch at most 1024 workgroups of 256, 262 144 threads for 3 n - 2 = 787 330 entries; k_mask_i32 the same for n = 262 444 rows and columns; k_tr_sort takes
    four output rows per workgroup and at most 2048 workgroups, 8192 rows a step; k_select at L lanes per row takes 256 / L rows per workgroup and at most 2048
    workgroups: 262 144 rows a step at L = 2, fewer at every larger L.  At the L = 1 that the lane rule gives this matrix (524 288 rows a step) it does not
    stride: the tests force L = 2 and 64.'''
    rows = numpy.concatenate([numpy.arange(1, n), numpy.arange(n), numpy.arange(n - 1)])
    cols = numpy.concatenate([numpy.arange(n - 1), numpy.arange(n), numpy.arange(1, n)])
    key = numpy.sort(rows.astype(I64) * n + cols)
    rowptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(key // n, minlength=n))])
    return _with_values(numpy.random.default_rng(6), rowptr, key % n, n, special=False)


SMALL = ('empty34', 'holes', 'wide', 'tall', 'rowlens', 'collens', 'random', 'hub', 'fan', 'chain', 'nomesh')
CASES = SMALL + ('cross',)


@functools.lru_cache(maxsize=None)
def case(name):
    '''a Csr, made once per session and never written'''
    if name == 'empty34':
        return Csr(numpy.zeros(0), numpy.zeros(4, dtype=I64), numpy.zeros(0, dtype=I64), 4)
    if name == 'holes':  # empty first, middle and last row, empty first, middle and last column
        return _random(1, 7, 9, .6, empty_rows=(0, 3, 6), empty_cols=(0, 4, 8))
    if name == 'wide':
        return _random(2, 5, 70, .4)
    if name == 'tall':
        return _random(3, 70, 5, .4)
    if name == 'rowlens':
        return _rowlens()
    if name == 'collens':  # the transpose of it: the COLUMNS have those lengths, which are the lengths of the rows that a transpose sorts
        return transposed(_rowlens())
    if name == 'random':
        rng = numpy.random.default_rng(4)
        return _with_values(rng, *random_csr(rng, 37, 41, .2, empty_row=5), 41)
    if name == 'hub':
        return _from_conn(hub(9, 4), 7)
    if name == 'fan':
        return _from_conn(fan(30, 5), 8)
    if name == 'chain':
        return _from_conn(chain(130), 9)
    if name == 'nomesh':
        return _from_conn(empty_mesh(6, 3), 10)
    if name == 'cross':
        return _dense_cross()
    if name == 'tridiagonal':
        return tridiagonal()
    raise KeyError(name)


def masks(m, seed=0):
    '''the selections every matrix is put through: name -> (rowkeep, colkeep), None for all'''
    nrows, ncols = len(m.rowptr) - 1, m.ncols
    rng = numpy.random.default_rng(1000 + seed)
    r, c = rng.random(nrows) < .6, rng.random(ncols) < .5
    if nrows > 1:
        r[[0, -1]] = [False, True]
    return {'rows': (r, None), 'cols': (None, c), 'both': (r, c), 'other': (~r, c), 'norows': (numpy.zeros(nrows, dtype=bool), c),
            'nocols': (r, numpy.zeros(ncols, dtype=bool)), 'nothing': (numpy.zeros(nrows, dtype=bool), numpy.zeros(ncols, dtype=bool))}


def _pair(name):
    rng = numpy.random.default_rng(21)
    nrows, ncols = 9, 11
    full = rng.random((nrows, ncols)) < .5
    if name == 'disjoint':
        split = rng.random((nrows, ncols)) < .5
        ma, mb = full & split, full & ~split
    elif name == 'nested':
        ma, mb = full, full & (rng.random((nrows, ncols)) < .5)
    elif name == 'overlap':
        ma, mb = full, rng.random((nrows, ncols)) < .5
    elif name == 'one_empty':
        ma, mb = full, numpy.zeros_like(full)
    else:
        raise KeyError(name)
    csr = lambda mask: _with_values(rng, numpy.concatenate([[0], numpy.cumsum(mask.sum(1))]), numpy.nonzero(mask)[1], ncols, special=False)
    return csr(ma), csr(mb)


def _cancel():
    '''one row per situation, A and B on the patterns [0, 1, 2] and [1, 2, 3] (partial overlap); in column 1 and 2:
    row 0: 2 + -2 (cancels: no entry) and .1 + .2 against -.3 (cancels to a rounding: kept)
    row 1: NaN against -NaN (kept) and inf against -inf (NaN: kept)
    row 2: -0. + 0. and 0. + 0. (stored zeros cancel like any others: no entry); its columns 0 and 3, held by one part only, are a stored 0. and a -0. (dropped too)
    row 3: 1 + 1 twice (nothing cancels)
    row 4: no entries in either'''
    A = Csr(numpy.array([1., 2., .1 + .2, 2., numpy.nan, numpy.inf, 0., -0., 0., 3., 1., 1.]), numpy.array([0, 3, 6, 9, 12, 12], dtype=I64),
            numpy.tile(numpy.arange(3, dtype=I64), 4), 5)
    B = Csr(numpy.array([-2., -.3, 4., -numpy.nan, -numpy.inf, 5., 0., 0., -0., 1., 1., 6.]), numpy.array([0, 3, 6, 9, 12, 12], dtype=I64),
            numpy.tile(numpy.arange(1, 4, dtype=I64), 4), 5)
    return A, B


PAIRS = ('disjoint', 'nested', 'overlap', 'one_empty', 'cancel', 'all_cancel')


@functools.lru_cache(maxsize=None)
def pair(name):
    '''(A, B): two Csr of one shape on different patterns, for A + B and A - B'''
    if name == 'cancel':
        return _cancel()
    if name == 'all_cancel':  # B = -A on a copy of the pattern: the sum has no entries at all
        A = case('random')
        values = numpy.where(numpy.isfinite(A.values), A.values, 1.)
        return Csr(values, A.rowptr, A.colidx, A.ncols), Csr(-values, A.rowptr.copy(), A.colidx.copy(), A.ncols)
    return _pair(name)
