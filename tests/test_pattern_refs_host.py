'''The references of tests/pattern_refs.py against constructions that share nothing with them: a dense boolean matrix filled by a triple Python loop with a
per-row sorted(set(...)), dictionaries for the expansion and the union, and the patterns stored in tests/golden/*.npz.  Everything is an integer and every
comparison exact.  No GPU, no library.'''
import glob
import os

import numpy
import pytest

import pattern_refs as refs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def brute_pattern(conn):
    '''(rows as sorted lists, candidates per row) by the triple loop'''
    dense = numpy.zeros((conn.nrows, conn.ncols), dtype=bool)
    cols = [[] for _ in range(conn.nrows)]
    for e in range(conn.nelems):
        for m in range(conn.toff[e], conn.toff[e + 1]):
            for n in range(conn.roff[e], conn.roff[e + 1]):
                dense[conn.tdofs[m], conn.rdofs[n]] = True
                cols[conn.tdofs[m]].append(int(conn.rdofs[n]))
    rows = [sorted(set(c)) for c in cols]
    assert all(rows[r] == list(numpy.flatnonzero(dense[r])) for r in range(conn.nrows))
    return rows, [len(c) for c in cols]


SMALL = {
    'hub(3, 4)': lambda: refs.hub(3, 4),
    'hub(9, 8)': lambda: refs.hub(9, 8),
    'fan(5, 3)': lambda: refs.fan(5, 3),
    'fan(1, 1)': lambda: refs.fan(1, 1),
    'repeated(4, 3)': lambda: refs.repeated(4, 3),
    'chain(2)': lambda: refs.chain(2),
    'chain(17)': lambda: refs.chain(17),
    'ragged': lambda: refs.ragged_mesh(1),
    'ragged, other seed': lambda: refs.ragged_mesh(2, ne=25, ndofs=33, nb=(1, 5)),
    'rectangular fixed': lambda: refs.random_mesh(3, 30, 41, 23, 3, 5),
    'ragged test side': lambda: refs.random_mesh(4, 30, 41, 23, (1, 6), 4),
    'ragged trial side': lambda: refs.random_mesh(5, 30, 23, 41, 4, (1, 6)),
    'both ragged, empty elements': lambda: refs.random_mesh(6, 30, 37, 29, (0, 5), (0, 7)),
    'no elements': lambda: refs.empty_mesh(5, 3),
    'no elements, no rows': lambda: refs.empty_mesh(0),
}


@pytest.mark.parametrize('name', SMALL)
def test_ref_pattern_is_the_brute_force_pattern(name):
    conn = SMALL[name]()
    srowptr, scol, emap, eoff, maxcand = refs.ref_pattern(*conn.args)
    rows, cand = brute_pattern(conn)
    assert srowptr.dtype == numpy.int64 and scol.dtype == numpy.int32 and emap.dtype == numpy.int32 and eoff.dtype == numpy.int64
    assert len(srowptr) == conn.nrows + 1 and srowptr[0] == 0 and srowptr[-1] == len(scol)
    for r in range(conn.nrows):
        assert list(scol[srowptr[r]:srowptr[r + 1]]) == rows[r], r
    assert maxcand == max(cand, default=0)
    # the element map, entry by entry: t runs element by element, m-major, n inner
    t = 0
    for e in range(conn.nelems):
        assert eoff[e] == t
        for m in range(conn.toff[e], conn.toff[e + 1]):
            for n in range(conn.roff[e], conn.roff[e + 1]):
                row, col = conn.tdofs[m], conn.rdofs[n]
                assert 0 <= emap[t] < srowptr[row + 1] - srowptr[row] and scol[srowptr[row] + emap[t]] == col, (e, m, n)
                t += 1
    assert len(emap) == t == eoff[-1] and len(eoff) == conn.nelems + 1


def test_the_ragged_mesh_has_what_it_promises():
    '''untouched dofs inside the range and at its end, a numbering that is not sorted, an element that repeats a dof, more than one element size'''
    conn = refs.ragged_mesh(1)
    held = numpy.zeros(conn.nrows, dtype=bool)
    held[conn.tdofs] = True
    assert not held[-2:].any() and not held[:-2].all() and held.any()
    lists = [conn.tdofs[a:b] for a, b in zip(conn.toff, conn.toff[1:])]
    assert any(len(set(d)) < len(d) for d in lists)
    assert any((numpy.diff(d) < 0).any() for d in lists)
    assert len({len(d) for d in lists}) > 2 and conn.nbt == 0 and conn.nbr == 0
    assert numpy.array_equal(conn.tdofs, refs.ragged_mesh(1).tdofs)  # seeded


CLASSES = [('hub', 8, 8, 64), ('hub', 9, 8, 72), ('hub', 32, 8, 256), ('hub', 33, 8, 264), ('hub', 32, 32, 1024), ('hub', 33, 32, 1056),
           ('hub', 128, 32, 4096), ('hub', 129, 32, 4128), ('hub', 128, 128, 16384), ('hub', 129, 128, 16512),
           ('fan', 8, 8, 64), ('fan', 32, 8, 256), ('fan', 32, 32, 1024), ('fan', 128, 32, 4096), ('fan', 128, 128, 16384),
           ('repeated', 8, 8, 64), ('repeated', 32, 8, 256), ('repeated', 32, 32, 1024), ('repeated', 128, 32, 4096), ('repeated', 128, 128, 16384)]


@pytest.mark.parametrize('builder,k,nb,maxcand', CLASSES)
def test_builders_give_the_candidate_counts_of_the_size_classes(builder, k, nb, maxcand):
    conn = getattr(refs, builder)(k, nb)
    assert int(conn.tdofs.min()) >= 0 and int(conn.tdofs.max()) < conn.nrows and int(conn.rdofs.min()) >= 0 and int(conn.rdofs.max()) < conn.ncols
    # candidates of a row, counted without the reference: every (element, local test dof) entry of the row brings the nbr of its element
    cand = numpy.zeros(conn.nrows, dtype=numpy.int64)
    for e in range(conn.nelems):
        for m in range(conn.toff[e], conn.toff[e + 1]):
            cand[conn.tdofs[m]] += conn.roff[e + 1] - conn.roff[e]
    assert cand.max() == maxcand
    srowptr, scol, emap, eoff, got = refs.ref_pattern(*conn.args)
    assert got == maxcand
    longest = int(numpy.diff(srowptr).max())
    assert longest == {'hub': k * (nb - 1) + 1, 'fan': k * nb, 'repeated': nb}[builder]
    if builder == 'fan':
        assert conn.nrows == 1 and conn.ncols == k * nb and conn.nbt == 1 and numpy.array_equal(scol, numpy.arange(k * nb))
    assert conn.nbt == (1 if builder == 'fan' else nb) and conn.nbr == nb


def test_chain_counts():
    conn = refs.chain(2 ** 20 + 3000)
    srowptr, scol, emap, eoff, maxcand = refs.ref_pattern(*conn.args)
    assert conn.nrows == 2 ** 20 + 3000 and conn.nelems == conn.nrows - 1 and maxcand == 4
    assert srowptr[-1] == len(scol) == 3154726
    assert numpy.array_equal(numpy.diff(srowptr), numpy.r_[2, numpy.full(conn.nrows - 2, 3), 2])
    assert numpy.array_equal(scol[:5], [0, 1, 0, 1, 2]) and numpy.array_equal(emap[:8], [0, 1, 0, 1, 1, 2, 0, 1])


MASKS = [(1, 1, None), (3, 2, None), (2, 3, None), (1, 8, None), (8, 8, None), (3, 3, [[1, 0, 1], [0, 0, 0], [1, 1, 0]]), (3, 2, [[1, 0], [1, 0], [1, 0]]),
         (2, 2, [[0, 0], [0, 0]])]


@pytest.mark.parametrize('nct,ncr,mask', MASKS)
def test_ref_expand_is_the_entry_by_entry_expansion(nct, ncr, mask):
    conn = refs.ragged_mesh(1)
    srowptr, scol = refs.ref_pattern(*conn.args)[:2]
    rowptr, colidx = refs.ref_expand(srowptr, scol, nct, ncr, mask)
    rows, _ = brute_pattern(conn)
    want = []
    for r in range(conn.nrows):
        for c in range(nct):
            want.append([sc * ncr + d for sc in rows[r] for d in range(ncr) if mask is None or mask[c][d]])
    assert rowptr.dtype == colidx.dtype == numpy.int64 and len(rowptr) == conn.nrows * nct + 1 and rowptr[0] == 0
    assert [list(colidx[a:b]) for a, b in zip(rowptr, rowptr[1:])] == want
    assert rowptr[-1] == len(colidx) == len(scol) * (nct * ncr if mask is None else int(numpy.sum(mask)))


@pytest.mark.parametrize('nparts,nrows', [(1, 5), (2, 1), (3, 7), (9, 4), (2, 0)])
def test_ref_union_is_the_rowwise_union_of_sets(nparts, nrows):
    rng = numpy.random.default_rng(nparts * 10 + nrows)
    parts = [refs.random_csr(rng, nrows, 12, dens, empty_row=2) for dens in rng.random(nparts) * .6]
    rowptr, colidx, pos = refs.ref_union(parts)
    sets = [sorted(set().union(*[set(ci[rp[r]:rp[r + 1]]) for rp, ci in parts])) for r in range(nrows)]
    assert [list(colidx[a:b]) for a, b in zip(rowptr, rowptr[1:])] == sets and len(rowptr) == nrows + 1 and rowptr[0] == 0
    assert nrows < 3 or rowptr[2] == rowptr[3]  # the row that is empty in every part
    for (rp, ci), p in zip(parts, pos):
        assert len(p) == len(ci)
        for r in range(nrows):
            for q in range(rp[r], rp[r + 1]):
                assert rowptr[r] <= p[q] < rowptr[r + 1] and colidx[p[q]] == ci[q]


def golden_files():
    '''the golden files that carry an element-to-dof map beside a stored CSR pattern'''
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, '*.npz'))):
        with numpy.load(path) as z:
            if {'dofs', 'dof_offsets', 'K_rowptr', 'K_colidx', 'K_values'} <= set(z.files):
                out.append(os.path.basename(path)[:-4])
    return out


@pytest.mark.parametrize('name', golden_files())
def test_ref_pattern_is_the_pattern_of_the_golden_matrices(name, golden):
    '''The stiffness matrices of tests/golden carry `dofs` / `dof_offsets` and a CSR pattern written by the sort-based construction, one block of nc x nc
    components per scalar entry.  Every stored entry must be one the reference has.  A file whose stored values hold an exact 0.0 shows by itself that its
    pattern keeps structural zeros: for those the stored pattern must EQUAL the expanded reference; the others (no stored zero: the file alone does not tell)
    are held to the inclusion only.'''
    z = golden(name)
    nc = z['u'].shape[1] if z['u'].ndim == 2 else 1
    rp, ci = z['K_rowptr'], z['K_colidx']
    assert (len(rp) - 1) % nc == 0
    n = (len(rp) - 1) // nc
    srowptr, scol = refs.ref_pattern(n, z['dofs'], z['dof_offsets'], z['dofs'], z['dof_offsets'])[:2]
    erp, eci = refs.ref_expand(srowptr, scol, nc, nc)
    width = n * nc
    stored = numpy.repeat(numpy.arange(n * nc), numpy.diff(rp)) * width + ci
    ours = numpy.repeat(numpy.arange(n * nc), numpy.diff(erp)) * width + eci
    assert numpy.isin(stored, ours).all()
    if (z['K_values'] == 0).any():
        assert numpy.array_equal(erp, rp) and numpy.array_equal(eci, ci)


def test_some_golden_file_keeps_structural_zeros():
    '''the equality branch of the test above is taken (else it would have to be reported as skipped)'''
    names = [name for name in golden_files() if (numpy.load(os.path.join(GOLDEN, name + '.npz'))['K_values'] == 0).any()]
    assert len(names) >= 5, names
