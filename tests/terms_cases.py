'''The inputs of tests/test_gpu_terms.py as plain numpy data (no GPU, no library), in the `spec` format of tests/terms_refs.py; tests/test_terms_refs_host.py runs the
mutants of the reference on the same inputs.  Structured bases come from the knot-span polynomials of oracle.assemble.local_spline_coeffs: per axis the distinct
polynomial sets are the table CLASSES, an element's class is the tuple of its axes' classes, `tab` holds it.  A graded axis (non-uniform knots) has one class per
element.  Quadrature points and weights are arbitrary (the rule need not integrate anything exactly), 4 to 9 points.'''
import functools
import os

import numpy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ---- meshes and bases ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _axis(n, btype, p, graded):
    '''(class polynomials [ncls][p + 1][p + 1] highest power first, class per element [n], first dof per element [n], dofs) of one axis'''
    from oracle import assemble as oa
    c = p - 1 if btype == 'spline' else 0
    k = numpy.arange(n + 1, dtype=float)
    if graded:
        k = numpy.concatenate([[0.], numpy.cumsum(1. + .125 * (numpy.arange(n) % 8))])
    m = numpy.repeat(p - c, n + 1)
    m[0] = m[-1] = p
    km = numpy.repeat(k, m)
    start = numpy.cumsum(m[:n]) - m[0]
    keys, classes, cls = {}, [], numpy.empty(n, dtype=numpy.int64)
    for i, o in enumerate(start):
        lk = km[o:o + 2 * p] - km[o + p - 1]  # (the polynomials in the local coordinate depend on the knot differences only)
        key = lk.tobytes()
        if key not in keys:
            keys[key] = len(classes)
            classes.append(oa.local_spline_coeffs(lk))
        cls[i] = keys[key]
    return numpy.array(classes), cls, start.astype(numpy.int64), int(m[:n].sum()) + 1


@functools.lru_cache(maxsize=None)
def mesh(shape, btype, p, graded=()):
    '''dict(nelems, nd, nb, dofs [ne][nb] int32, tab [ne] int32, ndofs, axes): element id with the LAST axis fastest, local functions and dofs with the first axis slowest'''
    axes = [_axis(n, btype, p, i in graded) for i, n in enumerate(shape)]
    idx = numpy.indices(shape).reshape(len(shape), -1)
    tab = numpy.zeros(idx.shape[1], dtype=numpy.int64)
    dofs = numpy.zeros((idx.shape[1], 1), dtype=numpy.int64)
    for (classes, cls, start, nd_ax), i in zip(axes, idx):
        tab = tab * len(classes) + cls[i]
        dofs = (dofs[:, :, None] * nd_ax + (start[i][:, None] + numpy.arange(p + 1))[:, None, :]).reshape(len(tab), -1)
    return dict(nelems=len(tab), nd=len(shape), nb=dofs.shape[1], dofs=dofs.astype(numpy.int32), tab=tab.astype(numpy.int32), ndofs=int(numpy.prod([a[3] for a in axes])),
                axes=axes, shape=shape)


def tables(msh, points):
    '''T [classes nb][nq][1 + nd] of the classes of a mesh at the points [nq][nd]'''
    nd, nq = msh['nd'], len(points)
    val, der = [], []  # per axis [ncls][p + 1][nq]
    for ax, (classes, _, _, _) in enumerate(msh['axes']):
        val.append(numpy.array([[numpy.polyval(P, points[:, ax]) for P in cl] for cl in classes]))
        der.append(numpy.array([[numpy.polyval(numpy.polyder(P), points[:, ax]) if len(P) > 1 else 0 * points[:, ax] for P in cl] for cl in classes]))
    slots = []
    for s in range(1 + nd):
        t = numpy.ones((1, 1, nq))
        for ax in range(nd):
            f = der[ax] if s == 1 + ax else val[ax]
            t = numpy.einsum('cmq,dnq->cdmnq', t, f).reshape(t.shape[0] * f.shape[0], t.shape[1] * f.shape[1], nq)
        slots.append(t)
    return numpy.ascontiguousarray(numpy.stack(slots, -1).reshape(-1, nq, 1 + nd))


def basis_of(msh, points, tab=True):
    return dict(T=tables(msh, points), dofs=msh['dofs'].reshape(-1), nb=msh['nb'], off=None, tab=msh['tab'] if tab else None, ndofs=msh['ndofs'])


def classes_per_run(tab, elist=None, run=64):
    '''distinct table classes in every run of `run` consecutive list positions'''
    t = numpy.asarray(tab) if elist is None else numpy.asarray(tab)[numpy.asarray(elist)]
    return numpy.array([len(numpy.unique(t[i:i + run])) for i in range(0, len(t), run)])


def quadrature(nd, nq, seed, face=-1):
    rng = numpy.random.default_rng(1000 + seed)
    points = rng.uniform(.1, .9, (nq, nd))
    if face >= 0:
        points[:, face] = 1.
    return points, rng.uniform(.1, .3, nq)


def geometry_of(kind, shape, points, seed, face=-1):
    '''box: non-unit sizes, some negative;  tab: a perturbed diagonal Jacobian per element and point;  iso: the multilinear map of a perturbed vertex grid;
    iso2: the biquadratic map (9 geometry functions) of a perturbed node grid'''
    rng = numpy.random.default_rng(2000 + seed)
    nd, ne, nq = len(shape), int(numpy.prod(shape)), len(points)
    if kind == 'box':
        size = rng.uniform(.5, 1.5, (ne, nd)) * rng.choice([-1., 1.], (ne, nd), p=[.25, .75])
        return dict(kind='box', origin=rng.normal(size=(ne, nd)), size=size, bnd_axis=face)
    if kind == 'tab':
        jac = rng.uniform(.5, 1.5, (ne, nq, nd))[..., None] * numpy.eye(nd) + rng.uniform(-.2, .2, (ne, nq, nd, nd))
        return dict(kind='tab', jac=jac, bnd_axis=face)
    p = 2 if kind == 'iso2' else 1
    gm = mesh(shape, 'std', p)
    nodes = numpy.stack(numpy.meshgrid(*[numpy.arange(p * n + 1.) / p for n in shape], indexing='ij'), -1).reshape(-1, nd)
    verts = (nodes - nodes.max(0) / 2) * rng.uniform(.7, 1.3, nd) + rng.uniform(-.15, .15, nodes.shape) / p  # (centred: the sums of J cancel the least)
    return dict(kind='iso', ngb=gm['nb'], gT=tables(gm, points)[:gm['nb']], gdofs=gm['dofs'].reshape(-1), verts=verts, bnd_axis=face)


# ---- term lists ---------------------------------------------------------------------------------------------------------------------------------

POWERS = (0, 1, 2, 3, 5, 8)


def _common(shape, btype, p, geom, nq, seed, face, graded, elist):
    msh = mesh(tuple(shape), btype, p, tuple(graded))
    points, weights = quadrature(msh['nd'], nq, seed, face)
    rng = numpy.random.default_rng(seed)
    n = msh['nelems']
    if elist == 'subset':
        el = numpy.sort(rng.choice(n, size=max(1, (2 * n) // 3), replace=False)).astype(numpy.int32)
    elif elist == 'permutation':
        el = rng.permutation(n).astype(numpy.int32)
    else:
        el = None
    spec = dict(ndims=msh['nd'], nq=nq, weights=weights, points=points, geom=geometry_of(geom, tuple(shape), points, seed, face), nelems=n if el is None else len(el), elist=el)
    return msh, points, rng, spec


def vector_case(shape, btype, p, *, geom='box', nq=5, seed=0, face=-1, graded=(), elist=None, ncomps=(1,), ncts=(1,), poly=True, scale=True, qs=True, grad=True, nterms=None,
                npolys=1, local=False):
    '''fields with `ncomps` components and blocks with `ncts` components on ONE basis; per block a source term and per (block, field) a form with a full random tensor,
    the first polynomial on every second term, a scale array on the first and the last term, a point factor of the first and the last scalar field on the second term.
    grad=False: no tensor reads a gradient slot.  nterms: the list is padded to that many terms.'''
    msh, points, rng, spec = _common(shape, btype, p, geom, nq, seed, face, graded, elist)
    B = basis_of(msh, points)
    S = 1 + msh['nd']

    def tensor(*dims):
        t = rng.normal(size=dims)
        if not grad:
            t[:, 1:] = 0
            if t.ndim == 4:
                t[..., 1:] = 0
        return t
    fields = [dict(basis=B, u=rng.uniform(-1, 1, (msh['ndofs'], nc)), ncomp=nc) for nc in ncomps]
    blocks = [dict(basis=B, nct=nct, nrows=msh['ndofs'], local=local) for nct in ncts]
    terms = []
    for ib, blk in enumerate(blocks):
        terms.append(dict(block=ib, f=tensor(blk['nct'], S)))
        for jf, F in enumerate(fields):
            terms.append(dict(block=ib, field=jf, C=tensor(blk['nct'], S, F['ncomp'], S), f=tensor(blk['nct'], S) if jf == 1 else None))
    while nterms and len(terms) < nterms:
        t = dict(terms[len(terms) % max(1, len(blocks) * (1 + len(fields)))])
        terms.append(dict(t, f=tensor(*numpy.shape(t['f'])) if t.get('f') is not None else None, C=tensor(*numpy.shape(t['C'])) if t.get('C') is not None else None))
    scalars = [(j, 0) for j, F in enumerate(fields) if F['ncomp'] == 1] or [(j, c) for j, F in enumerate(fields) for c in range(F['ncomp'])]
    polys = []
    if poly and fields:
        for k in range(npolys):
            vars_ = [(j, c) for j, F in enumerate(fields) for c in range(F['ncomp'])][k:k + 4] if npolys > 1 else scalars[:2]
            nv = len(vars_)
            powers = numpy.array([[POWERS[(k + t + 2 * v) % 6] if (t + v) % 2 == 0 else 0 for v in range(nv)] for t in range(4)])
            polys.append((vars_, rng.uniform(.5, 1.5, 4) * numpy.array([1, -1, 1, -1]), powers))
        for i, t in enumerate(terms):
            if i % 2 == 1:
                t['poly'] = (i // 2) % len(polys)
    if scale:
        for t in {0: terms[0], 1: terms[-1]}.values():
            t['scale'] = rng.uniform(.5, 1.5, (spec['nelems'], nq))
    sc = [j for j, F in enumerate(fields) if F['ncomp'] == 1]
    if qs and sc:
        Bq = rng.normal(size=(S, S))
        if not grad:
            Bq[1:] = 0
            Bq[:, 1:] = 0
        terms[1 % len(terms)]['qs'] = (Bq, sc[0], sc[-1])
    spec.update(fields=fields, blocks=blocks, terms=terms, polys=polys)
    return spec


def matrix_case(shape, btype, p, *, geom='box', nq=4, seed=0, face=-1, graded=(), elist=None, by_element=False, nfields=1, nct=1, ncr=1, mask=None, trial_p=None,
                separate_tables=False, kinds=(0, 1, 2), poly=True, scale=True, qs=True):
    '''test (and trial) basis of degree p (trial_p: another degree for the trial basis), `nfields` scalar fields on the test basis; terms of the given kinds (kinds 1 and 2
    only with a field), the polynomial on the first and the last term, a scale array on the first two, a point factor on the second'''
    msh, points, rng, spec = _common(shape, btype, p, geom, nq, seed, face, graded, elist)
    test = basis_of(msh, points)
    S = 1 + msh['nd']
    if trial_p is not None:
        trial = basis_of(mesh(tuple(shape), btype, trial_p, tuple(graded)), points)
    elif separate_tables:
        trial = dict(test, T=test['T'].copy())
    else:
        trial = test
    fields = [dict(basis=test, u=rng.uniform(-1, 1, (msh['ndofs'], 1)), ncomp=1) for _ in range(nfields)]
    terms = []
    for i, kind in enumerate(k for k in kinds if k == 0 or (nfields and nct == ncr == 1)):
        t = dict(kind=kind, C=rng.normal(size=(nct, S, ncr, S)))
        if kind:
            t['field'] = (i + 1) % nfields
        if kind == 2:
            t['L'] = rng.normal(size=(1, S))
        terms.append(t)
    polys = []
    if poly and nfields:
        vars_ = [(j, 0) for j in range(nfields)]
        polys.append((vars_, [1.5, -.5, .25], numpy.array([[1, 0], [0, 2], [3, 1]])[:, :nfields]))
        terms[0]['poly'] = terms[-1]['poly'] = 0
    nsc = msh['nelems'] if by_element else spec['nelems']
    if scale:
        for t in terms[:2]:
            t['scale'] = rng.uniform(.5, 1.5, (nsc, nq))
    if qs and nfields:
        terms[1 % len(terms)]['qs'] = (rng.normal(size=(S, S)), 0, nfields - 1)
    spec.update(test=test, trial=trial, nct=nct, ncr=ncr, mask=None if mask is None else numpy.asarray(mask, dtype=numpy.uint8), nrows=test['ndofs'], ncols=trial['ndofs'],
                by_element=by_element, fields=fields, terms=terms, polys=polys, mesh_nelems=msh['nelems'])
    return spec


@functools.lru_cache(maxsize=None)
def ragged(key='t', matrix=False, seed=5):
    '''the hierarchical quadratic spline fixture (functions per element from the offsets): one scalar field, a form with a polynomial factor and a source'''
    from oracle import assemble as oa
    g = dict(numpy.load(os.path.join(GOLDEN, 'hier_spline2_2d.npz')))
    rng = numpy.random.default_rng(seed)
    points, weights = g['gauss_coords'], g['gauss_weights']
    N, dN = oa.tabulate(g[key + '_coeffs'][None], points)  # [1][nq][nfn], [1][nq][nfn][nd]
    T = numpy.ascontiguousarray(numpy.concatenate([N[0].T[:, :, None], dN[0].transpose(1, 0, 2)], -1))
    off, ndofs = g[key + '_dof_offsets'].astype(numpy.int64), int(g[key + '_ndofs'])
    B = dict(T=T, dofs=g[key + '_dofs'].astype(numpy.int32), nb=0, off=off, tab=None, ndofs=ndofs)
    spec = dict(ndims=2, nq=len(weights), weights=weights, points=points, geom=dict(kind='box', origin=g['elem_origin'], size=g['elem_size'], bnd_axis=-1), nelems=len(off) - 1,
                elist=None, fields=[dict(basis=B, u=rng.uniform(-1, 1, (ndofs, 1)), ncomp=1)], polys=[([(0, 0)], [1., -.5], [[0], [2]])])
    if matrix:
        spec.update(test=B, trial=B, nct=1, ncr=1, mask=None, nrows=ndofs, ncols=ndofs, by_element=False, mesh_nelems=len(off) - 1,
                    terms=[dict(kind=0, C=rng.normal(size=(1, 3, 1, 3)), poly=0), dict(kind=1, field=0, C=rng.normal(size=(1, 3, 1, 3)))])
    else:
        spec.update(blocks=[dict(basis=B, nct=1, nrows=ndofs, local=False)],
                    terms=[dict(block=0, field=0, C=rng.normal(size=(1, 3, 1, 3)), poly=0), dict(block=0, f=rng.normal(size=(1, 3)))])
    return spec


def field_with_own_dofs(seed=3):
    '''a scalar block on bilinear elements whose field lives on a basis with the tables of the test basis and a dof numbering of its own'''
    spec = matrix_case((38, 30), 'std', 1, geom='tab', nfields=1, seed=seed)
    perm = numpy.random.default_rng(seed).permutation(spec['test']['ndofs']).astype(numpy.int32)
    spec['fields'][0]['basis'] = dict(spec['test'], dofs=perm[spec['test']['dofs']])
    return spec


# ---- roundings of a case (the arguments of terms_refs.m_vector / m_matrix) ------------------------------------------------------------------------

def chain_arguments(spec):
    import terms_refs
    nd = spec['ndims']
    bases = [F['basis'] for F in spec['fields']]
    every = numpy.arange(spec['nelems']) if spec.get('elist') is None else numpy.asarray(spec['elist'], dtype=numpy.int64)
    nbf = max([int(terms_refs.basis_sizes(b, every).max()) for b in bases], default=0)
    polys = spec.get('polys', ())
    out = dict(nd=nd, nq=spec['nq'], nb_field=nbf, ngb=spec['geom'].get('ngb', 0), face=spec['geom'].get('bnd_axis', -1) >= 0,
               degree=max([int(numpy.asarray(pw).reshape(len(cf), -1).sum(1).max()) for _, cf, pw in polys], default=0), npoly_terms=max([len(cf) for _, cf, _ in polys], default=0),
               has_qs=any(t.get('qs') is not None for t in spec['terms']), nterms=len(spec['terms']))
    rows = [b['basis'] for b in spec['blocks']] if 'blocks' in spec else [spec['test']]
    out['contributions'] = max(int(numpy.bincount(numpy.asarray(b['dofs']).reshape(-1)).max()) for b in rows)
    if 'blocks' in spec:
        out['ncr'] = max([F['ncomp'] for F in spec['fields']], default=1)
    return out


def gamma_m(spec):
    '''(m, gamma_m) of a case'''
    import terms_refs
    m = terms_refs.m_vector(**chain_arguments(spec)) if 'blocks' in spec else terms_refs.m_matrix(**chain_arguments(spec))
    return m, terms_refs.gamma(m)


# ---- the cases of tests/test_gpu_terms.py, by kernel family ---------------------------------------------------------------------------------------
# (name -> (builder, positional arguments, keywords); built on demand and cached)

V, M = vector_case, matrix_case
K_TERMS = {
    'one_element_1d': (V, ((1,), 'std', 1), dict(geom='box')),
    'one_element_2d_spline2': (V, ((1, 1), 'spline', 2), dict(geom='iso', ncomps=(1, 1))),
    'one_element_3d': (V, ((1, 1, 1), 'std', 1), dict(geom='tab', ncomps=(1, 1), ncts=(1, 1))),
    'p1_7x5_box': (V, ((7, 5), 'std', 1), dict(geom='box', ncomps=(1, 1))),
    'p2_7x5_tab': (V, ((7, 5), 'std', 2), dict(geom='tab', ncomps=(1, 1), nq=6)),
    'spline2_7x5_iso': (V, ((7, 5), 'spline', 2), dict(geom='iso', nq=9)),
    'spline2_7x5_iso_ngb9': (V, ((7, 5), 'spline', 2), dict(geom='iso2', ncomps=(1, 1))),
    'p1_13x11x3_iso': (V, ((13, 11, 3), 'std', 1), dict(geom='iso', ncomps=(1, 1), ncts=(1, 1))),
    'p2_13x11x3_box': (V, ((13, 11, 3), 'std', 2), dict(geom='box', nq=4)),
    'spline2_13_1d_tab': (V, ((13,), 'spline', 2), dict(geom='tab', ncomps=(1, 1, 1))),
    'vector_valued_2d': (V, ((7, 5), 'std', 1), dict(geom='tab', ncomps=(2,), ncts=(2,))),
    'vector_valued_3d': (V, ((13, 11, 3), 'std', 1), dict(geom='iso', ncomps=(3,), ncts=(3,), nq=4)),
    'blocks_of_1_and_3': (V, ((13, 11, 3), 'std', 1), dict(geom='box', ncomps=(1, 3), ncts=(1, 3), nq=4)),
    'six_fields_four_polynomials': (V, ((7, 5), 'spline', 2), dict(geom='box', ncomps=(1, 1, 1, 1, 2, 2), npolys=4)),
    'thirty_two_terms': (V, ((7, 5), 'std', 1), dict(geom='iso', ncomps=(1, 1), ncts=(1, 1), nterms=32)),
    'scale_on_a_subset': (V, ((7, 5), 'spline', 2), dict(geom='iso', elist='subset', ncomps=(1, 1))),
    'ragged': (ragged, ('t',), {}),
    'no_gradient_slots': (V, ((7, 5), 'std', 1), dict(geom='iso', ncomps=(1, 1), grad=False)),
    'local_vectors': (V, ((7, 5), 'spline', 2), dict(geom='box', ncomps=(1, 1), ncts=(1, 1), local=True)),
    'face0_1d_box': (V, ((7,), 'std', 1), dict(geom='box', face=0)),
    'face0_2d_box': (V, ((7, 5), 'std', 1), dict(geom='box', face=0, ncomps=(1, 1))),
    'face1_2d_iso': (V, ((7, 5), 'spline', 2), dict(geom='iso', face=1, ncomps=(1, 1))),
    'face1_2d_iso_ngb9': (V, ((7, 5), 'std', 2), dict(geom='iso2', face=1)),
    'face0_3d_tab': (V, ((13, 11, 3), 'std', 1), dict(geom='tab', face=0, nq=4)),
    'face1_3d_iso': (V, ((13, 11, 3), 'std', 1), dict(geom='iso', face=1, nq=4, ncomps=(1, 1))),
    'face2_3d_box': (V, ((13, 11, 3), 'std', 1), dict(geom='box', face=2, nq=4)),
}

# eight lists of one launch and a ninth (on its own), a list of another dimension, an empty list, a list of 2^14 elements (a launch of its own)
MULTI_2D = [(V, ((7, 5), 'spline', 2), dict(geom=g, face=f, seed=10 + i, ncomps=(1, 1), ncts=(1, 1), elist=el, nterms=nt))
            for i, (g, f, el, nt) in enumerate([('iso', -1, None, None), ('iso', 0, 'subset', None), ('iso', 1, 'subset', None), ('box', -1, None, 32), ('tab', -1, 'subset', None),
                                                ('iso2', -1, None, None), ('box', 0, None, None), ('tab', 1, None, None), ('iso', -1, 'subset', None)])]
MULTI_OTHER = [(V, ((5, 4, 3), 'std', 1), dict(geom='iso', seed=30, ncomps=(1, 1))), (V, ((128, 128), 'std', 1), dict(geom='box', seed=31, ncomps=(1, 1), nq=4))]

# (dims, functions) of k_local_vterms2: every shape with 0 .. 3 fields and 1, 2 blocks; the geometry kinds take turns
LOCAL_VTERMS2_SHAPES = {
    'line_p1_16384': (((16384,), 'std', 1), {}),
    'line_p1_16385': (((16385,), 'std', 1), {}),
    'line_p2_16384': (((16384,), 'std', 2), {}),
    'line_spline2_16384': (((16384,), 'spline', 2), {}),
    'quad_p1_128x128': (((128, 128), 'std', 1), {}),
    'quad_p1_127x130': (((127, 130), 'std', 1), {}),
    'quad_p2_128x128': (((128, 128), 'std', 2), {}),
    'quad_spline2_4096x4': (((4096, 4), 'spline', 2), {}),
    'quad_spline2_16384x4': (((16384, 4), 'spline', 2), {}),
    'quad_spline2_graded_2048x8': (((2048, 8), 'spline', 2), dict(graded=(1,))),
    'hex_p1_32x32x16_box': (((32, 32, 16), 'std', 1), dict(geom='box')),
    'hex_p1_32x32x16_iso': (((32, 32, 16), 'std', 1), dict(geom='iso')),
}
K_LOCAL_VTERMS2 = {}
for _i, (_name, (_args, _kw)) in enumerate(LOCAL_VTERMS2_SHAPES.items()):
    for _nf in range(4):
        for _nblk in (1, 2):
            _k = dict(geom=('box', 'tab', 'iso')[(_i + _nf + _nblk) % 3], nq=4, seed=_nf, ncomps=(1,) * _nf, ncts=(1,) * _nblk)
            _k.update(_kw)
            K_LOCAL_VTERMS2[f'{_name}-{_nf}fields-{_nblk}blocks'] = (V, _args, _k)
K_LOCAL_VTERMS2['quad_p1_128x128-permutation'] = (V, ((128, 128), 'std', 1), dict(geom='iso', nq=4, ncomps=(1, 1), ncts=(1, 1), elist='permutation'))
K_LOCAL_VTERMS2['quad_spline2_4096x4-permutation'] = (V, ((4096, 4), 'spline', 2), dict(geom='box', nq=4, ncomps=(1,), elist='permutation'))
K_LOCAL_VTERMS2['quad_p2_128x128-iso_ngb9'] = (V, ((128, 128), 'std', 2), dict(geom='iso2', nq=4, ncomps=(1, 1), ncts=(1, 1)))
K_LOCAL_VTERMS2['quad_p1_128x128-local_vectors'] = (V, ((128, 128), 'std', 1), dict(geom='tab', nq=4, ncomps=(1, 1), ncts=(1, 1), local=True))

K_MTERMS = {
    'one_element_2d': (M, ((1, 1), 'spline', 2), dict(geom='iso', nfields=2)),
    'scalar_spline2_7x5_iso': (M, ((7, 5), 'spline', 2), dict(geom='iso', nfields=2, nq=9)),
    'scalar_p2_13_1d_box': (M, ((13,), 'std', 2), dict(geom='box', nfields=1)),
    'scalar_p1_13x11x3_iso': (M, ((13, 11, 3), 'std', 1), dict(geom='iso', nfields=2)),
    'scalar_p1_7x5_iso_ngb9_face': (M, ((7, 5), 'std', 1), dict(geom='iso2', nfields=1, face=0)),
    'vector_3x3_tab': (M, ((7, 5), 'std', 1), dict(geom='tab', nfields=1, nct=3, ncr=3, kinds=(0, 0))),
    'vector_2x3_masked': (M, ((7, 5), 'spline', 2), dict(geom='box', nfields=1, nct=2, ncr=3, mask=[[1, 0, 1], [0, 1, 1]], kinds=(0, 0))),
    'test_p1_trial_p2': (M, ((7, 5), 'std', 1), dict(geom='iso', nfields=2, trial_p=2)),
    'ragged': (ragged, ('h', True), {}),
    'field_with_own_dofs': (field_with_own_dofs, (), {}),
    'subset_by_element': (M, ((7, 5), 'spline', 2), dict(geom='tab', nfields=2, elist='subset', by_element=True)),
}

# NH_MATRIX_GATHER | NH_MATRIX_STORE: key (dims, test functions, trial functions) x 0 .. 2 fields x geometry kind
LOCAL_TERMS_SHAPES = {
    10202: ((300,), 'std', 1), 10303: ((300,), 'spline', 2), 20404: ((38, 30), 'std', 1), 20909: ((38, 30), 'spline', 2), 30808: ((9, 7, 5), 'std', 1),
}
K_LOCAL_TERMS, K_LOCAL_TERMS2 = {}, {}
for _key, _args in LOCAL_TERMS_SHAPES.items():
    for _nf in range(3):
        for _g in ('iso', 'box', 'tab'):
            (K_LOCAL_TERMS2 if _key in (20909, 30808) else K_LOCAL_TERMS)[f'{_key}-{_nf}fields-{_g}'] = (M, _args, dict(geom=_g, nfields=_nf, seed=_nf, kinds=(0, 1, 2) if _nf else (0, 0)))
K_LOCAL_TERMS['10303-p2-2fields-separate_tables'] = (M, ((300,), 'std', 2), dict(geom='tab', nfields=2, separate_tables=True))
K_LOCAL_TERMS['20404-1fields-separate_tables'] = (M, ((38, 30), 'std', 1), dict(geom='iso', nfields=1, separate_tables=True))
K_LOCAL_TERMS2['20909-spline2_5x4-2fields'] = (M, ((5, 4), 'spline', 2), dict(geom='iso', nfields=2))
K_LOCAL_TERMS2['20909-p2_20x17-1fields-iso_ngb9'] = (M, ((20, 17), 'std', 2), dict(geom='iso2', nfields=1))
K_LOCAL_TERMS2['20909-2fields-separate_tables'] = (M, ((38, 30), 'spline', 2), dict(geom='box', nfields=2, separate_tables=True))
K_LOCAL_TERMS2['30808-1fields-separate_tables'] = (M, ((9, 7, 5), 'std', 1), dict(geom='iso', nfields=1, separate_tables=True))
K_LOCAL_TERMS2['20909-spline2_16384x4-2fields'] = (M, ((16384, 4), 'spline', 2), dict(geom='box', nfields=2))

FAMILIES = dict(k_terms=K_TERMS, k_local_vterms2=K_LOCAL_VTERMS2, k_mterms=K_MTERMS, k_local_terms=K_LOCAL_TERMS, k_local_terms2=K_LOCAL_TERMS2)


@functools.lru_cache(maxsize=8)
def build(family, name):
    return build_entry(FAMILIES[family][name])


def build_entry(entry):
    fn, args, kw = entry
    return fn(*args, **kw)
