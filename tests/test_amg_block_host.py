'''CPU-side checks of the block plans of the AMG setup (preconargs=dict(nullspace=B, setup='block'), nutils_amd/amg.py): the symbolic phase on CPU tensors,
integer for integer against setup='entry'; the product counts; the three products evaluated by the numpy restatement of nh_block_segment_dot
(tests/amg_block_refs.py) on the values of the restatement of tests/test_amg_nullspace_host.py, under the rule of its test_plans_reproduce_the_products; the
`setup` argument with a lowered amg.MAX_NPROD; and the structural check that the block kernel's offsets rest on.

Cases: those of tests/test_amg_nullspace_host.py (k = 3, 2, 2, 3), and 'hex': 3-D elasticity on 4 x 3 x 3 elements with its six rigid-body modes, the face
x = 0 held, coarse=12.'''
import functools
import numpy
import pytest

from test_cg_host import gamma
from test_amg_nullspace_host import CASES as NULLSPACE_CASES, problem as nullspace_problem, reference as nullspace_reference, hierarchy, elasticity
from amg_block_refs import block_segment_dot, scalar_terms

CASES = NULLSPACE_CASES + [('hex', 12)]


@functools.lru_cache(maxsize=None)
def problem(name):
    '''(A, free, B) of a case.  Made once, never written.'''
    if name != 'hex':
        return nullspace_problem(name)
    from nutils_amd import amg
    A, coords = elasticity((4, 3, 3))
    free = numpy.ones((5, 4, 4, 3), dtype=bool)
    free[0] = False
    return A, free.ravel(), amg.check_args(dict(nullspace=amg.rigid_body_modes(coords)), A.shape[0])[2]


@functools.lru_cache(maxsize=None)
def reference(name, coarse):
    return nullspace_reference(name, coarse) if name != 'hex' else hierarchy(*problem(name), coarse)


def symbolic(name, coarse, setup, nullspace=True):
    import torch
    from nutils_amd import amg
    A, free, B = problem(name)
    return amg.symbolic(torch.from_numpy(A.indptr.astype(numpy.int64)), torch.from_numpy(A.indices.astype(numpy.int64)), torch.from_numpy(free), coarse,
                        B.shape[1] if nullspace else None, setup=setup)


INTEGERS = 'agg', 'mptr', 'midx', 'prowptr', 'prow', 'pcol', 'pcol32', 'tmap', 'rperm', 'rrowptr', 'rcol', 'rcol32'
PLAN_INTEGERS = 'ptr', 'ia', 'ib', 'sa', 'sb', 'of', 'os', 'brows', 'bcols'


def same(s, t):
    return (s is None and t is None) or (s.dtype == t.dtype and numpy.array_equal(s.numpy(), t.numpy()))


@pytest.mark.parametrize('name,coarse', CASES)
def test_patterns(name, coarse):
    '''every integer that the cycle and the numeric phase read is the one setup='entry' makes, level by level, and the block plans' outputs lie on the
    patterns of P, A P and A_c; a rebuild gives the same integers'''
    entry, block, again = symbolic(name, coarse, 'entry'), symbolic(name, coarse, 'block'), symbolic(name, coarse, 'block')
    k = problem(name)[2].shape[1]
    print(f'{name}: k = {k}, levels {[lv.nfree for lv in entry]}, kinds {[lv.kind for lv in entry]}')
    assert len(entry) >= 2 and [lv.kind for lv in block] == [lv.kind for lv in entry] == [lv.kind for lv in reference(name, coarse)]
    assert {lv.setup for lv in entry} == {'entry'} and {lv.setup for lv in block} == {'block'}
    for e, b, a in zip(entry, block, again):
        assert (b.n, b.nfree, b.nodesize, b.k) == (e.n, e.nfree, e.nodesize, e.k) and same(b.rowptr, e.rowptr) and same(b.colidx, e.colidx)  # (the next level's too)
        if e.kind != 'coarsen':
            continue
        assert (b.nagg, b.nc, b.rounds) == (e.nagg, e.nc, e.rounds)
        for what in INTEGERS:
            assert same(getattr(b, what), getattr(e, what)), what
            assert same(getattr(b, what), getattr(a, what)), what
        for what in ('at', 'ap', 'rap'):
            plan, scalar = getattr(b, what), getattr(e, what)
            rows, cols = plan.scalar_pattern()
            assert same(rows, scalar.rows) and same(cols, scalar.cols), what  # the value arrays of P, A P and A_c, entry by entry
            assert plan.nout == scalar.nseg and (plan.k, plan.p, plan.q) == (k, k if what == 'rap' else b.nodesize, b.nodesize)
            for field in PLAN_INTEGERS:
                assert same(getattr(plan, field), getattr(getattr(a, what), field)), (what, field)


@pytest.mark.parametrize('name,coarse', CASES)
def test_product_counts(name, coarse):
    '''block products times k (A T, A P) and k^2 (R (A P)) on level 0, times k^3 on the levels whose nodes have k dofs, are the entry plans' products'''
    k = problem(name)[2].shape[1]
    for l, (e, b) in enumerate(zip(symbolic(name, coarse, 'entry'), symbolic(name, coarse, 'block'))):
        if e.kind != 'coarsen':
            continue
        assert b.nodesize == (1 if l == 0 else k)
        factors = (k, k, k ** 2) if l == 0 else (k ** 3,) * 3
        print(f'{name} level {l}: block products {[getattr(b, what).nprod for what in ("at", "ap", "rap")]}, entry products {[getattr(e, what).nprod for what in ("at", "ap", "rap")]}')
        for what, factor in zip(('at', 'ap', 'rap'), factors):
            assert getattr(b, what).nprod * factor == getattr(e, what).nprod, what


@pytest.mark.parametrize('name,coarse', CASES)
def test_products(name, coarse):
    '''A_f T, A_f P and P^T A_f P by the restatement of the block kernel on the restatement's values against the restatement's own products: every entry within
    gamma(terms + 2) times the same sum of magnitudes, terms the scalar terms of the entry; the whole value array is compared, so every block lies where
    the scalar CSR has it'''
    for r, g in zip(reference(name, coarse), symbolic(name, coarse, 'block')):
        if r.kind != 'coarsen':
            continue
        a = r.A.data
        for what, plan, fa, fb, expect in (('A T', g.at, a, r.Q.ravel(), r.AT), ('A P', g.ap, a, r.P.data, r.AP), ('R A P', g.rap, r.R.data, r.AP.data, r.Ac)):
            assert plan.nout == expect.nnz
            rows, cols = plan.scalar_pattern()
            assert numpy.array_equal(rows.numpy(), numpy.repeat(numpy.arange(expect.shape[0]), numpy.diff(expect.indptr))) and numpy.array_equal(cols.numpy(), expect.indices)
            terms = block_segment_dot(plan, numpy.ones(len(fa)), numpy.ones(len(fb)), expect.nnz)  # the scalar terms of every entry, where it lies
            assert (terms >= 1).all() and terms.sum() == plan.nprod * plan.p * plan.q * plan.k and numpy.array_equal(numpy.unique(terms), numpy.unique(scalar_terms(plan)))
            err = abs(block_segment_dot(plan, fa, fb, expect.nnz) - expect.data)
            bound = gamma(terms + 2) * block_segment_dot(plan, abs(fa), abs(fb), expect.nnz)
            assert (err <= bound).all(), what
        assert numpy.array_equal(r.P.data[g.rperm.numpy()], r.R.data)


@pytest.mark.parametrize('name,coarse', [('elasticity', 32), ('hex', 12)])
def test_setup_argument(name, coarse, monkeypatch):
    '''with amg.MAX_NPROD between the counts of the two kinds, no `setup` gives block levels and 'entry' the MatrixError that names the way out; below the
    block counts 'block' raises too'''
    from nutils_amd import amg, matrix
    entry, block = symbolic(name, coarse, 'entry'), symbolic(name, coarse, 'block')
    assert {lv.setup for lv in symbolic(name, coarse, None)} == {'entry'}  # (where the entry plans fit they are the default)
    count = lambda levels: max(getattr(lv, what).nprod for lv in levels if lv.kind == 'coarsen' for what in ('at', 'ap', 'rap'))
    print(f'{name}: the largest plan has {count(entry)} products by entry, {count(block)} by block')
    assert count(block) < count(entry)
    monkeypatch.setattr(amg, 'MAX_NPROD', count(entry))
    levels = symbolic(name, coarse, None)
    assert {lv.setup for lv in levels} == {'block'} and len(levels) == len(entry)  # one kind for the whole hierarchy
    with pytest.raises(matrix.MatrixError, match=f"a sparse product of {count(entry)} terms exceeds the int32 indices of its plan.*setup='block'"):
        symbolic(name, coarse, 'entry')
    assert {lv.setup for lv in symbolic(name, coarse, 'block')} == {'block'}
    monkeypatch.setattr(amg, 'MAX_NPROD', count(block))
    for setup in ('block', None):
        with pytest.raises(matrix.MatrixError, match='exceeds the int32 indices of its plan'):
            symbolic(name, coarse, setup)


def test_setup_argument_errors():
    '''raised before anything else is looked at, and before anything touches a device (there is none here)'''
    from nutils_amd import amg, matrix
    A = matrix.HipMatrix(numpy.array([2., 3.]), numpy.array([0, 1, 2]), numpy.array([0, 1]), 2)
    b = numpy.ones(2)
    for preconargs, message in ((dict(setup='block'), "setup='block'.*needs `nullspace`"), (dict(setup='rows', nullspace=numpy.ones(2)), "setup must be 'entry', 'block' or None, got 'rows'"),
                                (dict(setup='rows', coarse=0), 'setup must be'), (dict(setup=1, nullspace=numpy.ones(2)), 'setup must be'),
                                (dict(setup='block', nullspace=None), 'needs `nullspace`'), (dict(setup='block', nullspace=numpy.ones(3)), 'nullspace must have the shape')):
        with pytest.raises(matrix.MatrixError, match=message):
            A.solve(b, solver='cg', rtol=1e-8, precon='amg', preconargs=preconargs)
    assert A._dev is None  # nothing was uploaded
    with pytest.raises(matrix.MatrixError, match='setup must be'):
        symbolic('orphan', 16, 'rows')
    with pytest.raises(matrix.MatrixError, match='needs `nullspace`'):
        symbolic('orphan', 16, 'block', nullspace=False)
    rest, setup = amg.split_setup(dict(coarse=8, setup='block', nullspace=numpy.ones(5)))
    assert setup == 'block' and sorted(rest) == ['coarse', 'nullspace'] and amg.split_setup(None) == ({}, None) and amg.split_setup(dict(setup='entry'))[1] == 'entry'
    checked = amg.check_args(rest, 5)
    assert len(checked) == 3 and checked[:2] == (8, 1) and checked[2].shape == (5, 1)
    with pytest.raises(matrix.MatrixError, match="invalid arguments \\['setup'\\]"):
        amg.check_args(dict(setup='block'))  # (the key is split off before, like the smoother's)
    assert amg.MAX_NPROD == 1 << 31


def test_structural_check():
    '''a level matrix that is not made of full blocks is refused: the offsets of the block plans would point elsewhere'''
    import torch
    from nutils_amd import amg, matrix
    A = reference('elasticity', 32)[1].A  # nodes of three dofs
    rowptr, colidx = A.indptr.astype(numpy.int64), A.indices.astype(numpy.int64)
    blocks = amg.node_blocks(torch.from_numpy(rowptr), torch.from_numpy(colidx), 3)
    assert len(blocks[0]) * 9 == A.nnz and (numpy.diff(rowptr) % 3 == 0).all()
    row = 4
    for drop in ([rowptr[row] + 1], [rowptr[row] + 1, rowptr[row + 1] + 2]):  # an entry of one row; entries of two rows of a node that leave them equally long
        keep = numpy.ones(A.nnz, dtype=bool)
        keep[drop] = False
        length = numpy.diff(rowptr) - numpy.bincount(numpy.repeat(numpy.arange(A.shape[0]), numpy.diff(rowptr))[~keep], minlength=A.shape[0])
        with pytest.raises(matrix.MatrixError, match="setup='block' needs a level matrix made of full 3 x 3 blocks"):
            amg.node_blocks(torch.from_numpy(numpy.r_[0, numpy.cumsum(length)]), torch.from_numpy(colidx[keep]), 3)
    with pytest.raises(matrix.MatrixError, match='full 3 x 3 blocks'):  # whole blocks, of another size
        amg.node_blocks(torch.from_numpy(numpy.array([0, 2, 4, 6, 8])), torch.from_numpy(numpy.array([0, 1, 0, 1, 2, 3, 2, 3])), 3)
    # and through the symbolic phase: a coarse level whose pattern lost an entry
    lv = symbolic('elasticity', 32, 'block')[1]
    keep = numpy.ones(A.nnz, dtype=bool)
    keep[rowptr[row] + 1] = False
    lv.rowptr, lv.colidx = torch.from_numpy(numpy.r_[0, numpy.cumsum(numpy.diff(rowptr) - (numpy.arange(A.shape[0]) == row))]), torch.from_numpy(colidx[keep])
    with pytest.raises(matrix.MatrixError, match='full 3 x 3 blocks'):
        amg._coarsen(lv)
