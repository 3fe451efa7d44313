'''The inputs of tests/test_gpu_generic.py as plain numpy data (no GPU, no library) in the `spec` format of tests/terms_refs.py, built with tests/terms_cases.py
(mesh, tables, geometry_of, quadrature, matrix_case with kind-0 terms only), and how each case is launched (`run`): flags, switches, the kernel family and the
launcher's choice that nh_generic_launch_record must show.  Added here: a basis made of a subset of the functions of every element (function counts no tensor
basis has), the ragged description of a uniform basis (offsets instead of a function count: the launches per size class), per-point coefficient tensors as two
scaled terms, the forms (mass, Laplace, last slot only, symmetric, elasticity) and the parity colouring of a `std` mesh.  tests/test_generic_refs_host.py runs the
float64 restatement and the mutants of tests/generic_refs.py on the same inputs.'''
import functools

import numpy

import generic_refs as gr
import terms_cases as tc
import terms_refs as tr

EXCLUSIVE, BY_ELEMENT, NO_MFMA = 1, 2, 4
MASK23 = [[1, 0, 1], [0, 1, 1]]


# ---- pieces --------------------------------------------------------------------------------------------------------------------------------------

def form_tensor(form, nd, nct, ncr, rng):
    from oracle import assemble as oa
    S = 1 + nd
    C = rng.normal(size=(nct, S, ncr, S))
    if form == 'random':
        return C
    if form == 'mass':  # value slots only: one active test slot
        C[:, 1:] = 0
        C[:, :, :, 1:] = 0
        return C
    if form == 'laplace':  # slot 0 inactive
        return oa.laplace_coefficient(nd, nct) * 1.25
    if form == 'last':  # the only active test slot is the last
        C[:, :S - 1] = 0
        return C
    if form == 'sym':  # C[c][a][d][b] == C[d][b][c][a], every slot
        return C + C.transpose(2, 3, 0, 1)
    if form == 'symgrad':  # symmetric, gradient slots only
        C = C + C.transpose(2, 3, 0, 1)
        C[:, 0] = 0
        C[:, :, :, 0] = 0
        return C
    if form == 'elastic':
        return oa.elasticity_coefficient(nd, 1.5, .75)
    raise ValueError(form)


def subset_basis(B, keep, ne):
    '''the functions `keep` of every element of a uniform basis, the dofs renumbered without gaps'''
    nb, nq, S = B['nb'], B['T'].shape[1], B['T'].shape[2]
    keep = numpy.asarray(keep)
    dofs, inverse = numpy.unique(numpy.asarray(B['dofs']).reshape(ne, nb)[:, keep], return_inverse=True)
    T = numpy.ascontiguousarray(B['T'].reshape(-1, nb, nq, S)[:, keep].reshape(-1, nq, S))
    return dict(T=T, dofs=inverse.reshape(-1).astype(numpy.int32), nb=len(keep), off=None, tab=B['tab'], ndofs=len(dofs))


def ragged_basis(B, ne):
    '''the same basis described by offsets (nb = 0): one table per element, first function of element e = off[e]'''
    nb, nq, S = B['nb'], B['T'].shape[1], B['T'].shape[2]
    tab = numpy.zeros(ne, dtype=numpy.int64) if B.get('tab') is None else numpy.asarray(B['tab'], dtype=numpy.int64)
    T = numpy.ascontiguousarray(B['T'].reshape(-1, nb, nq, S)[tab].reshape(-1, nq, S))
    return dict(T=T, dofs=B['dofs'], nb=0, off=numpy.arange(ne + 1, dtype=numpy.int64) * nb, tab=None, ndofs=B['ndofs'])


def mixed_basis(B, ne, keep):
    '''described by offsets, the odd elements with the functions `keep` only: two size classes'''
    R = ragged_basis(B, ne)
    nb, nq, S = B['nb'], B['T'].shape[1], B['T'].shape[2]
    sel = numpy.ones((ne, nb), dtype=bool)
    sel[1::2] = numpy.isin(numpy.arange(nb), keep)
    off = numpy.concatenate([[0], numpy.cumsum(sel.sum(1))]).astype(numpy.int64)
    return dict(R, T=numpy.ascontiguousarray(R['T'].reshape(ne, nb, nq, S)[sel]), dofs=numpy.asarray(B['dofs']).reshape(ne, nb)[sel], off=off)


def colours(shape):
    '''element lists of the parity colouring, in lexicographic order of the parities (element id: last axis fastest)'''
    idx = numpy.indices(shape).reshape(len(shape), -1)
    key = numpy.zeros(idx.shape[1], dtype=int)
    for i in idx:
        key = key * 2 + i % 2
    return [numpy.flatnonzero(key == k).astype(numpy.int32) for k in range(2 ** len(shape)) if (key == k).any()]


def matrix(shape, btype, p, *, form='random', subset=None, ragged=False, cq=False, own_dofs=False, other_tables=False, **kw):
    '''tc.matrix_case without fields, one kind-0 term (cq: two, each with a scale array -- the device gets cq = sum_t scale_t C_t)'''
    spec = tc.matrix_case(tuple(shape), btype, p, nfields=0, kinds=(0, 0) if cq else (0,), poly=False, qs=False, scale=cq or kw.pop('scale', False),
                          separate_tables=other_tables, **kw)
    rng = numpy.random.default_rng(kw.get('seed', 0) + 77)
    nd, ne = spec['ndims'], spec['mesh_nelems']
    for t in spec['terms']:
        t['C'] = form_tensor(form, nd, spec['nct'], spec['ncr'], rng)
    if other_tables:  # a trial table that differs from the test table in every entry
        spec['trial']['T'] = spec['trial']['T'] * rng.uniform(.5, 1.5, spec['trial']['T'].shape)
    if subset is not None:
        spec['test'] = spec['trial'] = subset_basis(spec['test'], subset, ne)
        spec['nrows'] = spec['ncols'] = spec['test']['ndofs']
    if ragged:
        spec['test'] = spec['trial'] = mixed_basis(spec['test'], ne, range(7)) if ragged == 'mixed' else ragged_basis(spec['test'], ne)
    if own_dofs:  # the tables of the test basis, a dof numbering of its own
        perm = rng.permutation(spec['test']['ndofs']).astype(numpy.int32)
        spec['trial'] = dict(spec['test'], dofs=perm[spec['test']['dofs']])
    spec['shape'] = tuple(shape)
    return spec


def ragged_kind0():
    '''the hierarchical spline fixture reduced to its kind-0 term'''
    spec = dict(tc.ragged('h', True))
    spec.update(fields=[], polys=[], terms=[dict(kind=0, C=spec['terms'][0]['C'])])
    return spec


def vector(shape, btype, p, *, nct=1, ncr=1, trial_p=None, local=False, scale=False, functional=False, **kw):
    '''one field, one block, one C term (with the scale array) and one f term'''
    spec = tc.vector_case(tuple(shape), btype, p, ncomps=(ncr,), ncts=(nct,), poly=False, qs=False, scale=False, local=local, **kw)
    rng = numpy.random.default_rng(kw.get('seed', 0) + 78)
    if trial_p is not None:
        msh = tc.mesh(tuple(shape), btype, trial_p)
        spec['fields'][0] = dict(basis=tc.basis_of(msh, spec['points']), u=rng.uniform(-1, 1, (msh['ndofs'], ncr)), ncomp=ncr)
    f, c = spec['terms']
    assert f.get('C') is None and c.get('C') is not None
    if scale:  # (nh_assemble_vector has ONE scale array for the whole integrand)
        f['scale'] = c['scale'] = rng.uniform(.5, 1.5, (spec['nelems'], spec['nq']))
    spec['functional'] = functional
    return spec


def ragged_vector():
    spec = dict(tc.ragged('t', False))
    spec.update(polys=[], terms=[{k: v for k, v in t.items() if k != 'poly'} for t in spec['terms']])
    return spec


# ---- cases: name -> (builder, args, keywords, run) ------------------------------------------------------------------------------------------------------------
# run: family that serves the case and `expect`, the entries of its record; flags; env; gather / store; launches (default 1); colours ('exclusive' | 'first_touch');
# symmetric: a branch that mirrors entries takes it; qchunk: the chunk of points the launcher must choose.

SUB20 = [i for i in range(27) if i not in (0, 5, 11, 13, 17, 22, 26)]
SUB16 = [i for i in SUB20 if i not in (2, 8, 19, 24)]  # (k_matrix_mfma<3, 1> takes exactly 16 functions in 3-D: M tiles = ceil(functions / 16))
SUB24 = [i for i in range(25) if i != 12]


def _mfma(nd, mt, nt, kt, nas):
    return dict(ND=nd, MT=mt, nt=nt, kt=kt, nas=nas)


MFMA = {
    '2_1-p3-scalar-nq16-iso': (matrix, ((3, 2), 'std', 3), dict(geom='iso', nq=16), dict(expect=_mfma(2, 1, 1, 12, 3))),
    '2_1-p3-scalar-nq9-tab': (matrix, ((3, 2), 'std', 3), dict(geom='tab', nq=9, seed=1), dict(expect=_mfma(2, 1, 1, 9, 3))),
    '2_2-p4-2comp-nq10-box': (matrix, ((2, 2), 'std', 4), dict(geom='box', nq=10, nct=2, ncr=2, seed=2), dict(expect=_mfma(2, 2, 4, 9, 3))),
    '3_1-sub16-scalar-iso': (matrix, ((2, 1, 2), 'std', 2), dict(geom='iso', nq=8, subset=SUB16, seed=3), dict(expect=_mfma(3, 1, 1, 8, 4))),
    '3_1-sub16-3comp-tab': (matrix, ((2, 1, 2), 'std', 2), dict(geom='tab', nq=7, subset=SUB16, nct=3, ncr=3, seed=4), dict(expect=_mfma(3, 1, 3, 8, 4))),
    '3_2-sub20-scalar-iso': (matrix, ((2, 1, 2), 'std', 2), dict(geom='iso', nq=8, subset=SUB20, seed=3), dict(expect=_mfma(3, 2, 2, 8, 4))),  # (12 padded rows)
    '3_2-sub20-3comp-tab': (matrix, ((2, 1, 2), 'std', 2), dict(geom='tab', nq=7, subset=SUB20, nct=3, ncr=3, seed=4), dict(expect=_mfma(3, 2, 4, 8, 4))),
    '3_2-p2-3x3-nq27-box': (matrix, ((2, 1, 1), 'std', 2), dict(geom='box', nq=27, nct=3, ncr=3, seed=5), dict(expect=_mfma(3, 2, 6, 28, 4))),
    '3_2-p2-2x3-masked-iso': (matrix, ((2, 1, 1), 'std', 2), dict(geom='iso', nq=27, nct=2, ncr=3, mask=MASK23, seed=6), dict(expect=_mfma(3, 2, 6, 28, 4))),
    '3_4-p3-nq30-2elements-tab': (matrix, ((1, 2, 1), 'std', 3), dict(geom='tab', nq=30, seed=7), dict(expect=_mfma(3, 4, 4, 32, 4))),
    '3_4-spline3-7x7x6-grid_stride': (matrix, ((7, 7, 6), 'spline', 3), dict(geom='iso', nq=30, form='laplace', seed=8), dict(expect=_mfma(3, 4, 4, 24, 3))),
    'slots-mass-p3': (matrix, ((3, 2), 'std', 3), dict(geom='tab', nq=16, form='mass', seed=9), dict(expect=_mfma(2, 1, 1, 4, 1))),
    'slots-laplace-p3': (matrix, ((3, 2), 'std', 3), dict(geom='box', nq=14, form='laplace', seed=10), dict(expect=_mfma(2, 1, 1, 8, 2))),
    'slots-last-p3': (matrix, ((3, 2), 'std', 3), dict(geom='iso', nq=9, form='last', seed=11), dict(expect=_mfma(2, 1, 1, 3, 1))),
    'subset-scale-by_position': (matrix, ((4, 3), 'std', 3), dict(geom='iso', nq=9, elist='subset', scale=True, seed=12), dict(expect=_mfma(2, 1, 1, 9, 3))),
    'subset-scale-by_element': (matrix, ((4, 3), 'std', 3), dict(geom='tab', nq=9, elist='subset', scale=True, by_element=True, seed=13),
                                dict(flags=BY_ELEMENT, expect=_mfma(2, 1, 1, 9, 3))),
    'more_elements_than_the_grid-p3-40x40': (matrix, ((40, 40), 'std', 3), dict(geom='box', nq=16, seed=14), dict(expect=_mfma(2, 1, 1, 12, 3))),
    'colours-exclusive-p3': (matrix, ((5, 4), 'std', 3), dict(geom='iso', nq=9, seed=15), dict(colours='exclusive', launches=4, expect=_mfma(2, 1, 1, 9, 3))),
    'colours-first_touch-p3': (matrix, ((5, 4), 'std', 3), dict(geom='iso', nq=9, seed=15), dict(colours='first_touch', launches=4, expect=_mfma(2, 1, 1, 9, 3))),
}


def _gen(branch, waves, use_w, qchunk, sym):
    return dict(branch=branch, waves=waves, use_w=use_w, qchunk=qchunk, sym=sym)


def _waves(name, entry, waves):
    '''the case with NUTILS_AMD_GENERIC_WAVES = each of `waves`'''
    fn, args, kw, run = entry
    return {f'{name}-{w}waves': (fn, args, kw, dict(run, env=dict(run.get('env', {}), NUTILS_AMD_GENERIC_WAVES=str(w)), expect=dict(run['expect'], waves=w))) for w in waves}


G = 'k_matrix_generic'
GENERIC = {}
# MFMA declined -> generic (no NH_MATRIX_NO_MFMA: the launcher itself declines)
GENERIC.update({
    'declined-2d-p5-mt3': (matrix, ((2, 1), 'std', 5), dict(geom='iso', nq=9, seed=20), dict(family=G, expect=_gen('entries', 2, 0, 9, 0))),
    'declined-2d-p6-mt4': (matrix, ((1, 2), 'std', 6), dict(geom='tab', nq=9, seed=21), dict(family=G, expect=_gen('entries', 2, 0, 9, 0))),
    'declined-3d-p3-nq64-lds': (matrix, ((1, 1, 2), 'std', 3), dict(geom='box', nq=64, seed=22), dict(family=G, expect=_gen('entries', 2, 0, 29, 0), qchunk=29)),
    'declined-1d-p15': (matrix, ((3,), 'std', 15), dict(geom='box', nq=5, seed=23), dict(family=G, expect=_gen('entries', 2, 1, 5, 0))),
    'declined-cq-p3': (matrix, ((3, 2), 'std', 3), dict(geom='iso', nq=9, cq=True, seed=24), dict(family=G, expect=_gen('entries', 2, 1, 9, 0))),
    'declined-other_tables-p3': (matrix, ((3, 2), 'std', 3), dict(geom='tab', nq=9, other_tables=True, seed=25), dict(family=G, expect=_gen('entries', 2, 0, 9, 0))),
})
# entries
GENERIC.update(_waves('entries-p1-2d-use_w', (matrix, ((3, 2), 'std', 1), dict(geom='iso', nq=4, seed=30), dict(family=G, expect=_gen('entries', 1, 1, 4, 0))), (1, 2)))
GENERIC.update(_waves('entries-p2-3d-nq27', (matrix, ((2, 1, 2), 'std', 2), dict(geom='tab', nq=27, seed=31), dict(family=G, flags=NO_MFMA, expect=_gen('entries', 1, 0, 27, 0))),
                      (1, 2, 4)))
GENERIC.update(_waves('entries-cq-scalar-p2', (matrix, ((3, 2), 'std', 2), dict(geom='box', nq=5, cq=True, seed=32), dict(family=G, expect=_gen('entries', 1, 1, 5, 0))), (1, 2)))
GENERIC.update(_waves('entries-cq-2x2-use_w-p1', (matrix, ((3, 2), 'std', 1), dict(geom='iso', nq=4, cq=True, nct=2, ncr=2, seed=33),
                                                 dict(family=G, expect=_gen('entries', 1, 1, 4, 0))), (1, 2)))
GENERIC.update(_waves('entries-cq-2x3-use_w-p1', (matrix, ((3, 2), 'std', 1), dict(geom='tab', nq=4, cq=True, nct=2, ncr=3, seed=34),
                                                 dict(family=G, expect=_gen('entries', 1, 1, 4, 0))), (1, 2)))
GENERIC.update(_waves('entries-test_p3-trial_p1', (matrix, ((3, 2), 'std', 3), dict(geom='iso', nq=6, trial_p=1, seed=35), dict(family=G, expect=_gen('entries', 1, 1, 6, 0))), (1, 2)))
GENERIC.update(_waves('entries-other_tables-p2', (matrix, ((3, 2), 'std', 2), dict(geom='box', nq=5, other_tables=True, seed=36), dict(family=G, expect=_gen('entries', 1, 1, 5, 0))),
                      (1, 2)))
# scalar symmetric
GENERIC.update(_waves('scalar_symmetric-p1-use_w', (matrix, ((3, 2), 'std', 1), dict(geom='tab', nq=4, form='sym', seed=40),
                                                   dict(family=G, symmetric=True, expect=_gen('scalar_symmetric', 1, 1, 4, 1))), (1, 2)))
GENERIC.update(_waves('scalar_symmetric-p2-nq24', (matrix, ((3, 2), 'std', 2), dict(geom='iso', nq=24, form='sym', seed=41),
                                                  dict(family=G, symmetric=True, expect=_gen('scalar_symmetric', 1, 0, 24, 1))), (1, 2)))
# Gram
GENERIC.update(_waves('gram-p1-3x3', (matrix, ((3, 2), 'std', 1), dict(geom='iso', nq=4, nct=3, ncr=3, seed=50), dict(family=G, expect=_gen('gram', 1, 0, 4, 0))), (1, 2)))
GENERIC.update(_waves('gram-p2-2x3-masked', (matrix, ((3, 2), 'std', 2), dict(geom='box', nq=5, nct=2, ncr=3, mask=MASK23, seed=51), dict(family=G, expect=_gen('gram', 1, 0, 5, 0))),
                      (1, 2)))
GENERIC.update(_waves('gram-p2-own_dofs', (matrix, ((3, 2), 'std', 2), dict(geom='tab', nq=5, nct=2, ncr=2, form='sym', own_dofs=True, seed=52),
                                          dict(family=G, expect=_gen('gram', 1, 0, 5, 0))), (1, 2)))
# Gram symmetric
GENERIC.update(_waves('gram_symmetric-p1-elastic', (matrix, ((3, 2), 'std', 1), dict(geom='iso', nq=4, nct=2, ncr=2, form='elastic', seed=60),
                                                   dict(family=G, symmetric=True, expect=_gen('gram_symmetric', 1, 0, 4, 1))), (1, 2)))
GENERIC.update(_waves('gram_symmetric-p2-sym', (matrix, ((3, 2), 'std', 2), dict(geom='tab', nq=6, nct=2, ncr=2, form='sym', seed=61),
                                               dict(family=G, symmetric=True, expect=_gen('gram_symmetric', 1, 0, 6, 1))), (1, 2)))
# points in chunks: 3-D p3, 32 points, 29 per chunk
_P3 = ((1, 2, 1), 'std', 3)
GENERIC.update(_waves('chunked-entries', (matrix, _P3, dict(geom='iso', nq=32, seed=70), dict(family=G, flags=NO_MFMA, qchunk=29, expect=_gen('entries', 1, 0, 29, 0))), (1, 2)))
GENERIC.update(_waves('chunked-scalar_symmetric', (matrix, _P3, dict(geom='tab', nq=32, form='sym', seed=71),
                                                  dict(family=G, flags=NO_MFMA, qchunk=29, symmetric=True, expect=_gen('scalar_symmetric', 1, 0, 29, 1))), (1, 2)))
GENERIC.update(_waves('chunked-gram', (matrix, _P3, dict(geom='box', nq=32, nct=2, ncr=2, seed=72), dict(family=G, flags=NO_MFMA, qchunk=29, expect=_gen('gram', 1, 0, 29, 0))), (1, 2)))
GENERIC['chunked-gram-gather'] = (matrix, _P3, dict(geom='box', nq=32, nct=2, ncr=2, seed=72),
                                  dict(family=G, gather=True, store=True, repeat=True, qchunk=29, env=dict(NUTILS_AMD_GENERIC_WAVES='2'), expect=_gen('gram', 2, 0, 29, 0)))
GENERIC['chunked-gram_symmetric-gather'] = (matrix, _P3, dict(geom='iso', nq=32, nct=3, ncr=3, form='sym', seed=73),
                                            dict(family=G, gather=True, store=True, repeat=True, qchunk=29, symmetric=True, env=dict(NUTILS_AMD_GENERIC_WAVES='2'),
                                                 expect=_gen('gram_symmetric', 2, 0, 29, 1)))
# ragged bases: one launch per size class of the pattern
GENERIC['ragged-size_classes'] = (ragged_kind0, (), {}, dict(family=G, launches='size classes', env=dict(NUTILS_AMD_GENERIC_WAVES='1'), expect=dict(branch='entries', waves=1, sym=0)))
GENERIC['ragged-two_size_classes'] = (matrix, ((4, 3), 'std', 3), dict(geom='iso', nq=5, ragged='mixed', seed=85),
                                      dict(family=G, launches='size classes', env=dict(NUTILS_AMD_GENERIC_WAVES='1'), expect=_gen('entries', 1, 1, 5, 0)))
# symmetric forms with NUTILS_AMD_NO_SYM_GRAM: the branches that form every entry
GENERIC['entries-symmetric_form-no_sym_gram'] = (matrix, ((3, 2), 'std', 2), dict(geom='iso', nq=24, form='sym', seed=41),
                                                 dict(family=G, env=dict(NUTILS_AMD_GENERIC_WAVES='1', NUTILS_AMD_NO_SYM_GRAM='1'), expect=_gen('entries', 1, 0, 24, 0)))
GENERIC['gram-symmetric_form-no_sym_gram'] = (matrix, ((3, 2), 'std', 2), dict(geom='tab', nq=6, nct=2, ncr=2, form='sym', seed=61),
                                              dict(family=G, env=dict(NUTILS_AMD_GENERIC_WAVES='2', NUTILS_AMD_NO_SYM_GRAM='1'), expect=_gen('gram', 2, 0, 6, 0)))
# element lists with a scale array, by list position and by element
for _el in ('subset', 'permutation'):
    for _by in (False, True):
        GENERIC[f'list-{_el}-scale-by_{"element" if _by else "position"}'] = (
            matrix, ((4, 3), 'std', 2), dict(geom='iso', nq=5, elist=_el, scale=True, by_element=_by, seed=80 + _by),
            dict(family=G, flags=BY_ELEMENT if _by else 0, env=dict(NUTILS_AMD_GENERIC_WAVES='1'), expect=_gen('entries', 1, 1, 5, 0)))
GENERIC['grid_stride-p1-96x96-tab'] = (matrix, ((96, 96), 'std', 1), dict(geom='tab', nq=4, seed=82),
                                       dict(family=G, env=dict(NUTILS_AMD_GENERIC_WAVES='1'), expect=_gen('entries', 1, 1, 4, 0)))
GENERIC['colours-exclusive-p2'] = (matrix, ((5, 4), 'std', 2), dict(geom='tab', nq=5, form='sym', seed=83),
                                   dict(family=G, colours='exclusive', launches=4, env=dict(NUTILS_AMD_GENERIC_WAVES='1'), expect=_gen('entries', 1, 1, 5, 0)))
GENERIC['colours-first_touch-p2'] = (matrix, ((5, 4), 'std', 2), dict(geom='tab', nq=5, form='sym', seed=83),
                                     dict(family=G, colours='first_touch', launches=4, env=dict(NUTILS_AMD_GENERIC_WAVES='2'), expect=_gen('entries', 2, 1, 5, 0)))
GENERIC['colours-first_touch-p2-2x2'] = (matrix, ((5, 4), 'std', 2), dict(geom='iso', nq=5, nct=2, ncr=2, seed=84),
                                         dict(family=G, colours='first_touch', launches=4, env=dict(NUTILS_AMD_GENERIC_WAVES='1'), expect=_gen('gram', 1, 0, 5, 0)))


def _gs(E, NC, USE0, TRI):
    return dict(E=E, W=4, NC=NC, USE0=USE0, TRI=TRI)


def _gram_sym(nb, basis, nq, geom, seed, E):
    '''two cases per function count: scalar with the value slot and the triangular scratch; two components, gradients only, full scratch'''
    shape, p, extra = basis
    a = (matrix, (shape, 'std', p), dict(geom=geom, nq=nq, form='sym', seed=seed, **extra[0]),
         dict(family='k_gram_sym', gather=True, store=True, repeat=True, symmetric=True, expect=_gs(E, 1, 1, 1)))
    b = (matrix, (shape, 'std', p), dict(geom=geom, nq=nq, nct=2, ncr=2, form='elastic', seed=seed + 1, **extra[1]),
         dict(family='k_gram_sym', gather=True, store=True, repeat=True, symmetric=True, env=dict(NUTILS_AMD_NO_TRI_SCRATCH='1'), expect=_gs(E, 2, 0, 0)))
    return {f'{nb}functions-scalar-use0-tri': a, f'{nb}functions-2comp-gradients-full': b}


# (uniform scalar blocks of 4, 9, 16, 25 functions and two-component blocks of 4, 9 have a thread pass in front of this kernel: described by offsets they reach it)
R, U = dict(ragged=True), {}
GRAM_SYM = {}
GRAM_SYM.update(_gram_sym(4, ((5, 3), 1, (R, R)), 4, 'iso', 100, 4))
GRAM_SYM.update(_gram_sym(9, ((5, 3), 2, (R, R)), 7, 'tab', 102, 4))
GRAM_SYM.update(_gram_sym(16, ((3, 3), 3, (R, U)), 9, 'box', 104, 4))
GRAM_SYM.update(_gram_sym(24, ((3, 2), 4, (dict(subset=SUB24), dict(subset=SUB24))), 10, 'iso', 106, 3))
GRAM_SYM.update(_gram_sym(25, ((3, 3), 4, (R, U)), 11, 'tab', 108, 2))
GRAM_SYM.update(_gram_sym(36, ((2, 3), 5, (U, U)), 17, 'iso', 110, 1))
GRAM_SYM['9functions-scalar-gradients-tri'] = (matrix, ((5, 3), 'std', 2), dict(geom='iso', nq=6, form='symgrad', ragged=True, seed=112),
                                               dict(family='k_gram_sym', gather=True, store=True, repeat=True, symmetric=True, expect=_gs(4, 1, 0, 1)))
GRAM_SYM['16functions-2comp-use0-tri'] = (matrix, ((3, 3), 'std', 3), dict(geom='iso', nq=9, nct=2, ncr=2, form='sym', seed=113),
                                          dict(family='k_gram_sym', gather=True, store=True, repeat=True, symmetric=True, expect=_gs(4, 2, 1, 1)))
GRAM_SYM['25functions-2comp-use0-tri'] = (matrix, ((3, 3), 'std', 4), dict(geom='box', nq=11, nct=2, ncr=2, form='sym', seed=114),
                                          dict(family='k_gram_sym', gather=True, store=True, repeat=True, symmetric=True, expect=_gs(2, 2, 1, 1)))
_W2 = dict(NUTILS_AMD_GENERIC_WAVES='2')
GRAM_SYM['declined-49functions'] = (matrix, ((2, 1), 'std', 6), dict(geom='iso', nq=9, form='sym', seed=115),
                                    dict(family=G, gather=True, store=True, repeat=True, symmetric=True, env=_W2, expect=_gen('scalar_symmetric', 2, 0, 9, 1)))
GRAM_SYM['declined-36functions-nq18'] = (matrix, ((2, 1), 'std', 5), dict(geom='tab', nq=18, form='sym', seed=116),
                                         dict(family=G, gather=True, store=True, repeat=True, symmetric=True, env=_W2, expect=_gen('scalar_symmetric', 2, 0, 18, 1)))
GRAM_SYM['declined-36functions-unsymmetric'] = (matrix, ((2, 1), 'std', 5), dict(geom='box', nq=9, seed=117),
                                                dict(family=G, gather=True, store=True, repeat=True, env=_W2, expect=_gen('entries', 2, 0, 9, 0)))

V = 'k_vector_generic'
VECTOR = {
    'chunked-p3-3d-nq32': (vector, ((1, 2, 1), 'std', 3), dict(geom='iso', nq=32, seed=120), dict(family=V, qchunk=28, expect=dict(qchunk=28))),
    'nct3-ncr1': (vector, ((3, 2), 'std', 2), dict(geom='tab', nq=5, nct=3, ncr=1, seed=121), dict(family=V, expect=dict(qchunk=5))),
    'nct1-ncr3': (vector, ((3, 2), 'std', 2), dict(geom='box', nq=5, nct=1, ncr=3, seed=122), dict(family=V, expect=dict(qchunk=5))),
    'test_p2-trial_p1': (vector, ((3, 2), 'std', 2), dict(geom='iso', nq=6, trial_p=1, seed=123), dict(family=V, expect=dict(qchunk=6))),
    'ragged': (ragged_vector, (), {}, dict(family=V, expect={})),
    'subset-scale': (vector, ((4, 3), 'std', 2), dict(geom='iso', nq=5, elist='subset', scale=True, seed=124), dict(family=V, expect=dict(qchunk=5))),
    'local': (vector, ((3, 2), 'std', 2), dict(geom='tab', nq=5, nct=2, ncr=2, local=True, seed=125), dict(family=V, expect=dict(qchunk=5))),
    'functional': (vector, ((3, 2), 'std', 2), dict(geom='iso', nq=5, nct=2, ncr=2, functional=True, seed=126), dict(family=V, expect=dict(qchunk=5))),
}

FAMILIES = dict(k_matrix_mfma=MFMA, k_matrix_generic=GENERIC, k_gram_sym=GRAM_SYM, k_vector_generic=VECTOR)
MATRIX_CASES = [(f, n) for f in ('k_matrix_mfma', 'k_matrix_generic', 'k_gram_sym') for n in FAMILIES[f]]


@functools.lru_cache(maxsize=None)
def _spec(fn, args, kw):
    return fn(*args, **dict(kw))


def build(family, name):
    '''(spec, run) of a case; cases that share their inputs share the spec'''
    fn, args, kw, run = FAMILIES[family][name]
    run = dict(run)
    run.setdefault('family', family)
    return _spec(fn, args, tuple(sorted((k, _freeze(v)) for k, v in kw.items()))), run


def _freeze(v):
    return tuple(_freeze(x) for x in v) if isinstance(v, (list, tuple)) else v


@functools.lru_cache(maxsize=None)
def reference(family, name):
    '''the longdouble reference of a case, computed once: matrix (value, magnitude, rowptr, colidx); vector [(value, magnitude, local value, local magnitude)]'''
    spec, _ = build(family, name)
    return tr.vector_terms(spec) if 'blocks' in spec else tr.matrix_terms(spec)


def list_pattern(spec, ref):
    '''An element list whose scale and element map go by LIST POSITION comes with the pattern of the listed elements only (uniform bases).  -> the reference
    (value, magnitude, rowptr, colidx) restricted to that pattern; what it leaves out receives no contribution: its magnitude must be zero.'''
    value, mag, rowptr, colidx = ref
    elist = numpy.asarray(spec['elist'], dtype=numpy.int64)

    def listed(B):
        return dict(B, dofs=numpy.asarray(B['dofs']).reshape(-1, B['nb'])[elist].reshape(-1), tab=None if B.get('tab') is None else numpy.asarray(B['tab'])[elist])
    sub = tr.pattern_keys(dict(spec, test=listed(spec['test']), trial=listed(spec['trial']), mesh_nelems=len(elist)))
    at = numpy.searchsorted(tr.pattern_keys(spec), sub)
    out = numpy.ones(len(value), dtype=bool)
    out[at] = False
    assert (mag[out] == 0).all() and (value[out] == 0).all()
    width = spec['ncols'] * spec['ncr']
    rp = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(sub // width, minlength=spec['nrows'] * spec['nct']))]).astype(numpy.int64)
    return value[at], mag[at], rp, (sub % width).astype(numpy.int64)


@functools.lru_cache(maxsize=None)
def functional_reference(family, name):
    '''(value, magnitude) of  sum_q w |det| scale (1/2 U . C U + f . U)  from vector_terms of the two terms apart: with the test basis for the field, u . r = sum_q w |det|
    U . F, so the functional is 1/2 u . r_C + u . r_f'''
    spec, _ = build(family, name)
    u = tr._ld(spec['fields'][0]['u'])
    assert spec['fields'][0]['basis'] is spec['blocks'][0]['basis'] and u.shape[1] == spec['blocks'][0]['nct']
    value = mag = 0
    for t in spec['terms']:
        (v, a, _, _), = tr.vector_terms(dict(spec, terms=[t]))
        half = tr.LD(.5) if t.get('C') is not None else tr.LD(1)
        value, mag = value + half * (u * v).sum(), mag + half * (numpy.abs(u) * a).sum()
    return value, mag


def size_classes(spec):
    '''non-empty size classes of the pattern of a ragged basis (functions per element <= 8, 16, 24, 32, 48, 64, 96, 128, more)'''
    sizes = numpy.diff(numpy.asarray(spec['test']['off']))
    return len(numpy.unique(numpy.searchsorted([8, 16, 24, 32, 48, 64, 96, 128], sizes)))


# ---- roundings of a case ------------------------------------------------------------------------------------------------------------------------------

def contributions(basis):
    return int(numpy.bincount(numpy.asarray(basis['dofs']).reshape(-1)).max())


def gamma_m(spec, run):
    '''(m, gamma_m) of a case: the count of tests/generic_refs.py for the family that serves it, from the shapes of the case'''
    nd, nq = spec['ndims'], spec['nq']
    common = dict(nd=nd, nq=nq, ngb=spec['geom'].get('ngb', 0), scale=any(t.get('scale') is not None for t in spec['terms']))
    family = run['family']
    if family == 'k_vector_generic':
        F = spec['fields'][0]
        every = numpy.arange(spec['nelems']) if spec.get('elist') is None else numpy.asarray(spec['elist'], dtype=numpy.int64)
        m = gr.m_vector_generic(nbr=int(tr.basis_sizes(F['basis'], every).max()), ncr=F['ncomp'], nct=spec['blocks'][0]['nct'], qchunk=run.get('qchunk'),
                                contributions=contributions(spec['blocks'][0]['basis']), functional_terms=spec['nelems'] * nq if spec.get('functional') else 0, **common)
        return m, tr.gamma(m)
    n = contributions(spec['test'])
    if family == 'k_matrix_mfma':
        m = gr.m_mfma(nas=len(gr.active_slots(spec)), contributions=n, **common)
    elif family == 'k_gram_sym':
        m = gr.m_gram_sym(contributions=n, **common)
    else:
        m = gr.m_generic(qchunk=run.get('qchunk'), contributions=n, cq_roundings=3 if len(spec['terms']) > 1 else 0, **common)
    return m, tr.gamma(m)
