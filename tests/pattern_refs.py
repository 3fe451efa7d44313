'''Plain numpy restatements of the sparsity-pattern kernels of nh_pattern.hip (stage K6) and the connectivities the pattern tests feed them.  No device, no
library.  Everything here is an integer: the tests compare with numpy.array_equal.

A connectivity is a `Conn`: concatenated per-element dof lists of the test side (rows) and of the trial side (columns), each with its offsets `off` of
nelems + 1 entries.  A fixed number of functions per element nb is the special case off = arange(nelems + 1) * nb; `Conn.nbt` / `Conn.nbr` give that number,
or 0 where the side is ragged.'''
import collections

import numpy

I64 = numpy.int64


class Conn(collections.namedtuple('Conn', 'nrows ncols tdofs toff rdofs roff')):
    @property
    def nelems(self):
        return len(self.toff) - 1

    @property
    def nbt(self):
        return _fixed(self.toff)

    @property
    def nbr(self):
        return _fixed(self.roff)

    @property
    def args(self):
        '''the argument list of ref_pattern'''
        return self.nrows, self.tdofs, self.toff, self.rdofs, self.roff


def _fixed(off):
    '''nb if off is arange(ne + 1) * nb with nb >= 1 and ne >= 1, else 0'''
    d = numpy.diff(off)
    return int(d[0]) if len(d) and d[0] > 0 and (d == d[0]).all() else 0


def _conn(nrows, ncols, tdofs, toff, rdofs, roff):
    return Conn(int(nrows), int(ncols), numpy.asarray(tdofs, dtype=numpy.int32), numpy.asarray(toff, dtype=I64), numpy.asarray(rdofs, dtype=numpy.int32),
                numpy.asarray(roff, dtype=I64))


# ---- references -------------------------------------------------------------------------------------------------------------------------------------

def ref_pattern(nrows, tdofs, toff, rdofs, roff):
    '''(srowptr, scol, emap, eoff, maxcand) of nh_pattern_build: every (row, col) that some element couples, sorted lexicographically (srowptr int64 of
    nrows + 1, scol int32); emap[t] int32 the position of entry (e, m, n) inside its row, t running element by element, m-major, n inner; eoff int64 the prefix
    of nbt_e * nbr_e; maxcand the largest per-row sum of nbr_e over the (element, local test dof) entries of the row, duplicates counted.'''
    tdofs, rdofs, toff, roff = (numpy.asarray(a, dtype=I64) for a in (tdofs, rdofs, toff, roff))
    ne = len(toff) - 1
    assert len(roff) == ne + 1 and toff[0] == 0 and roff[0] == 0 and toff[-1] == len(tdofs) and roff[-1] == len(rdofs)
    nbt, nbr = numpy.diff(toff), numpy.diff(roff)
    eoff = numpy.concatenate([[0], numpy.cumsum(nbt * nbr)]).astype(I64)
    e = numpy.repeat(numpy.arange(ne, dtype=I64), nbt * nbr)  # the element of entry t
    local = numpy.arange(eoff[-1], dtype=I64) - eoff[e]
    row = tdofs[toff[e] + local // numpy.maximum(nbr[e], 1)]
    col = rdofs[roff[e] + local % numpy.maximum(nbr[e], 1)]
    assert not len(row) or (0 <= row.min() and row.max() < nrows and 0 <= col.min() and col.max() < 1 << 31)
    key, inverse = numpy.unique(row << 32 | col, return_inverse=True)
    srowptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(key >> 32, minlength=nrows))]).astype(I64)
    scol = (key & 0xffffffff).astype(numpy.int32)
    emap = (inverse.reshape(-1) - srowptr[row]).astype(numpy.int32)
    cand = numpy.zeros(nrows, dtype=I64)
    numpy.add.at(cand, tdofs, numpy.repeat(nbr, nbt))
    return srowptr, scol, emap, eoff, int(cand.max(initial=0))


def ref_expand(srowptr, scol, nct, ncr, mask=None):
    '''(rowptr, colidx) int64 of nh_pattern_expand: row r * nct + c holds, for every scalar column sc of row r in order, the columns sc * ncr + d of the d
    with mask[c, d], ascending; no mask: all d.'''
    mask = numpy.ones((nct, ncr), dtype=bool) if mask is None else numpy.asarray(mask).reshape(nct, ncr) != 0
    rows = []
    for r in range(len(srowptr) - 1):
        sc = numpy.asarray(scol[srowptr[r]:srowptr[r + 1]], dtype=I64)
        for c in range(nct):
            rows.append((sc[:, None] * ncr + numpy.flatnonzero(mask[c])[None, :]).reshape(-1))
    rowptr = numpy.concatenate([[0], numpy.cumsum([len(r) for r in rows])]).astype(I64)
    return rowptr, numpy.concatenate(rows + [numpy.zeros(0, dtype=I64)]).astype(I64)


def ref_union(parts):
    '''(rowptr, colidx, pos) of nh_pattern_union_*: the row-wise sorted union of the CSR patterns [(rowptr, colidx)], and for every entry of every part its
    index in the union'''
    nrows = len(parts[0][0]) - 1
    width = max([int(numpy.max(ci, initial=0)) for _, ci in parts]) + 1
    keys = []
    for rp, ci in parts:
        assert len(rp) == nrows + 1
        keys.append(numpy.repeat(numpy.arange(nrows, dtype=I64), numpy.diff(rp)) * width + numpy.asarray(ci, dtype=I64))
    union = numpy.unique(numpy.concatenate(keys))
    rowptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(union // width, minlength=nrows))]).astype(I64)
    return rowptr, (union % width).astype(I64), [numpy.searchsorted(union, k).astype(I64) for k in keys]


# ---- connectivities ---------------------------------------------------------------------------------------------------------------------------------

def hub(k, nb):
    '''k elements of nb functions that all hold dof 0 (at local position e % nb) and otherwise distinct dofs: row 0 has k * nb candidates, k * (nb - 1) + 1 of
    them distinct'''
    dofs = numpy.empty((k, nb), dtype=I64)
    for e in range(k):
        own = 1 + e * (nb - 1) + numpy.arange(nb - 1)
        dofs[e] = numpy.insert(own[::-1], e % nb, 0)  # (descending, so that the sort has work to do)
    n = 1 + k * (nb - 1)
    off = numpy.arange(k + 1) * nb
    return _conn(n, n, dofs.reshape(-1), off, dofs.reshape(-1), off)


def fan(k, nbr):
    '''k elements whose single test dof is 0 (nbt = 1) and whose trial dofs are all distinct: nrows = 1, ncols = k * nbr, and row 0 holds exactly k * nbr
    unique columns (in a seeded shuffle)'''
    rdofs = numpy.random.default_rng(k * 100003 + nbr).permutation(k * nbr)
    return _conn(1, k * nbr, numpy.zeros(k), numpy.arange(k + 1), rdofs, numpy.arange(k + 1) * nbr)


def repeated(k, nb):
    '''one element of nb distinct dofs listed k times: every row has k * nb candidates that compact to nb columns'''
    dofs = numpy.tile(numpy.arange(nb)[::-1], k)
    off = numpy.arange(k + 1) * nb
    return _conn(nb, nb, dofs, off, dofs, off)


def chain(n):
    '''a 1-D linear mesh of n nodes: element e holds dofs (e, e + 1); 3 n - 2 nonzeros'''
    dofs = (numpy.arange(n - 1, dtype=I64)[:, None] + numpy.arange(2)).reshape(-1)
    off = numpy.arange(n) * 2
    return _conn(n, n, dofs, off, dofs, off)


def _side(rng, ne, n, nb, repeats):
    '''dof lists of one side: nb an int (fixed) or (lo, hi) (ragged, both included).  The dofs come from a shuffled subset of range(n - 2) that leaves a fifth
    of it out, so that some dofs inside the range and the last two are held by no element; with `repeats` a quarter of the elements hold their first dof twice.'''
    counts = numpy.full(ne, nb, dtype=I64) if numpy.isscalar(nb) else rng.integers(nb[0], nb[1] + 1, ne)
    pool = rng.permutation(n - 2)[:max(int(counts.max(initial=0)), (n - 2) * 4 // 5)]
    lists = []
    for c in counts:
        d = rng.choice(pool, int(c), replace=False)
        if repeats and c >= 2 and rng.random() < .25:
            d[-1] = d[0]
        lists.append(d)
    return numpy.concatenate(lists + [numpy.zeros(0, dtype=I64)]), numpy.concatenate([[0], numpy.cumsum(counts)])


def random_mesh(seed, ne, nrows, ncols, nbt, nbr, repeats=True):
    '''a seeded random connectivity with separate test and trial maps; nbt, nbr: an int (fixed) or (lo, hi) (ragged)'''
    rng = numpy.random.default_rng(seed)
    tdofs, toff = _side(rng, ne, nrows, nbt, repeats)
    rdofs, roff = _side(rng, ne, ncols, nbr, repeats)
    return _conn(nrows, ncols, tdofs, toff, rdofs, roff)


def ragged_mesh(seed, ne=40, ndofs=70, nb=(1, 9)):
    '''the random ragged mesh: test and trial side share one map with shuffled numbering, dofs that no element holds (inside the range and at its end) and
    elements that repeat a dof'''
    rng = numpy.random.default_rng(seed)
    dofs, off = _side(rng, ne, ndofs, nb, True)
    return _conn(ndofs, ndofs, dofs, off, dofs, off)


def empty_mesh(nrows, ncols=None):
    '''no elements'''
    z = numpy.zeros(0)
    return _conn(nrows, nrows if ncols is None else ncols, z, [0], z, [0])


def random_csr(rng, nrows, ncols, density, empty_row=None):
    '''(rowptr, colidx) int64 of a random pattern with sorted unique rows; row `empty_row` is left empty where there is such a row'''
    mask = rng.random((nrows, ncols)) < density
    if empty_row is not None and empty_row < nrows:
        mask[empty_row] = False
    return numpy.concatenate([[0], numpy.cumsum(mask.sum(1))]).astype(I64), numpy.nonzero(mask)[1].astype(I64)
