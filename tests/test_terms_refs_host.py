'''Pins tests/terms_refs.py, the longdouble restatement of the term-list assembly entries, on the CPU: against the golden fixtures of the reference, against exact
rational arithmetic on dyadic data (plain loops over the header formulas, written independently of the vectorised restatement), and shows with a table of deliberate
mistakes that the bound gamma_m x magnitude of tests/test_gpu_terms.py is not vacuous on the inputs of that file.'''
import math
import os
from fractions import Fraction

import numpy
import pytest

import terms_cases as tc
import terms_refs as tr

LD = numpy.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCALAR = ['lap1d_p1_5', 'lap2d_p1_4x4', 'lap2d_p1_4x3_iso', 'lap2d_p2_3x4_iso', 'lap2d_spline2_5x4_iso', 'lap3d_p1_234', 'lap3d_p1_543_iso', 'lap3d_p2_2_iso', 'lap3d_spline2_3_iso',
          'lap2d_spline2_5x4_per0', 'lap3d_p1_345_per02']
ELAST = ['elast2d_p1_3x3', 'elast2d_p2_3x2_iso', 'elast3d_p1_2_iso', 'elast3d_p2_2']


def golden_spec(g):
    '''sample, geometry and basis of a golden case, the tables from the reference's polynomial coefficients (one table per element)'''
    from oracle import assemble as oa
    shape = tuple(int(n) for n in g['shape'])
    nd, ne = len(shape), int(numpy.prod(shape))
    nb = len(g['dofs']) // ne
    pts, w = g['gauss_coords'], g['gauss_weights']

    def table(coeffs):
        N, dN = oa.tabulate(coeffs, pts)  # [n][nq][nb], [n][nq][nb][nd]
        return numpy.concatenate([N.transpose(0, 2, 1)[..., None], dN.transpose(0, 2, 1, 3)], -1).reshape(-1, len(pts), 1 + nd)
    ndofs = int(g['dofs'].max() + 1)
    B = dict(T=table(g['coeffs'].reshape(ne, nb, -1)), dofs=g['dofs'], nb=nb, off=None, tab=numpy.arange(ne), ndofs=ndofs)
    if int(g['iso']):
        ngb = 2 ** nd
        geom = dict(kind='iso', ngb=ngb, gT=table(g['gcoeffs'][None, :ngb]), gdofs=g['gdofs'], verts=g['verts'], bnd_axis=-1)
    else:
        geom = dict(kind='box', origin=numpy.array(list(numpy.ndindex(*shape)), dtype=float), size=numpy.ones((ne, nd)), bnd_axis=-1)
    return dict(ndims=nd, nq=len(w), weights=w, geom=geom, nelems=ne, elist=None, polys=[], mesh_nelems=ne), B


def within(got, value, mag, m):
    err = numpy.abs(LD(numpy.asarray(got)).reshape(-1) - value.reshape(-1))
    return float((err / (tr.gamma(m) * mag.reshape(-1))).max())


@pytest.mark.parametrize('name', SCALAR)
def test_scalar_golden(name):
    '''res_laplace + 2.5 res_mass + load_one as ONE term list, K + 2.5 M as one matrix term list: the golden vectors of the reference (float64, summed in another
    order: they carry roundings of their own, of a chain no longer than the one counted for the kernels) within the bound of the GPU tests'''
    from oracle import assemble as oa
    g = dict(numpy.load(os.path.join(GOLDEN, name + '.npz')))
    spec, B = golden_spec(g)
    nd = spec['ndims']
    f = numpy.zeros((1, 1 + nd))
    f[0, 0] = 1
    fields = [dict(basis=B, u=g['u'].reshape(-1, 1), ncomp=1)]
    vec = dict(spec, fields=fields, blocks=[dict(basis=B, nct=1, nrows=B['ndofs'])],
               terms=[dict(block=0, field=0, C=oa.laplace_coefficient(nd)), dict(block=0, field=0, C=2.5 * oa.mass_coefficient(nd)), dict(block=0, f=f)])
    (value, mag, _, _), = tr.vector_terms(vec)
    assert within(g['res_laplace'] + 2.5 * g['res_mass'] + g['load_one'], value, mag, tc.gamma_m(vec)[0] + 2) <= 1
    mat = dict(spec, fields=[], test=B, trial=B, nct=1, ncr=1, mask=None, nrows=B['ndofs'], ncols=B['ndofs'], by_element=False,
               terms=[dict(kind=0, C=oa.laplace_coefficient(nd)), dict(kind=0, C=2.5 * oa.mass_coefficient(nd))])
    value, mag, rowptr, colidx = tr.matrix_terms(mat)
    assert numpy.array_equal(rowptr, g['K_rowptr']) and numpy.array_equal(colidx, g['K_colidx']) and numpy.array_equal(colidx, g['M_colidx'])
    assert within(g['K_values'] + 2.5 * g['M_values'], value, mag, tc.gamma_m(mat)[0] + 1) <= 1


@pytest.mark.parametrize('name', ELAST)
def test_elasticity_golden(name):
    from oracle import assemble as oa
    g = dict(numpy.load(os.path.join(GOLDEN, name + '.npz')))
    spec, B = golden_spec(g)
    nd = spec['ndims']
    C = oa.elasticity_coefficient(nd, float(g['lam']), float(g['mu']))
    vec = dict(spec, fields=[dict(basis=B, u=g['u'].reshape(-1, nd), ncomp=nd)], blocks=[dict(basis=B, nct=nd, nrows=B['ndofs'])], terms=[dict(block=0, field=0, C=C)])
    (value, mag, _, _), = tr.vector_terms(vec)
    assert within(g['res'], value, mag, tc.gamma_m(vec)[0]) <= 1
    mat = dict(spec, fields=[], test=B, trial=B, nct=nd, ncr=nd, mask=oa.block_mask(C), nrows=B['ndofs'], ncols=B['ndofs'], by_element=False,
               terms=[dict(kind=0, C=.25 * C), dict(kind=0, C=.75 * C)])
    value, mag, rowptr, colidx = tr.matrix_terms(mat)
    assert numpy.array_equal(rowptr, g['K_rowptr']) and numpy.array_equal(colidx, g['K_colidx'])
    assert within(g['K_values'], value, mag, tc.gamma_m(mat)[0]) <= 1


# ---- exact arithmetic: plain loops over the formulas of include/nutils_hip.h -----------------------------------------------------------------------

def F(x):
    return Fraction(float(x))


class Exact:
    '''one or two linear elements, BOX or TAB geometry, dyadic data: every quantity a Fraction'''

    def __init__(self, spec):
        self.s, self.nd, self.nq = spec, spec['ndims'], spec['nq']

    def element(self, ie):
        return ie if self.s.get('elist') is None else int(self.s['elist'][ie])

    def geometry(self, e, q):
        nd, g = self.nd, self.s['geom']
        if g['kind'] == 'box':
            J = [[F(g['size'][e][i]) if i == j else Fraction(0) for j in range(nd)] for i in range(nd)]
        else:
            J = [[F(g['jac'][e][q][i][j]) for j in range(nd)] for i in range(nd)]
        if nd == 1:
            det, Jinv = J[0][0], [[1 / J[0][0]]]
        else:
            det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
            Jinv = [[J[1][1] / det, -J[0][1] / det], [-J[1][0] / det, J[0][0] / det]]
        return Jinv, abs(det)

    def D(self, B, e, q, m, Jinv):
        '''D[q,m,:] of function m of element e'''
        fn = (0 if B.get('tab') is None else int(B['tab'][e]) * B['nb']) + m
        T = [F(x) for x in B['T'][fn][q]]
        return [T[0]] + [sum(T[1 + j] * Jinv[j][i] for j in range(self.nd)) for i in range(self.nd)]

    def U(self, Fd, e, q, Jinv):
        '''U[d][b]'''
        B, nb, S = Fd['basis'], Fd['basis']['nb'], 1 + self.nd
        out = [[Fraction(0)] * S for _ in range(Fd['ncomp'])]
        for n in range(nb):
            Dn = self.D(B, e, q, n, Jinv)
            for d in range(Fd['ncomp']):
                un = F(Fd['u'][int(B['dofs'][e * nb + n])][d])
                for b in range(S):
                    out[d][b] += Dn[b] * un
        return out

    def factor(self, t, ie, e, q, U, by_element=False):
        S = 1 + self.nd
        g = Fraction(1)
        if t.get('scale') is not None:
            g *= F(t['scale'][e if by_element else ie][q])
        if t.get('poly', -1) >= 0:
            vars_, coeffs, powers = self.s['polys'][t['poly']]
            g *= sum(F(c) * math.prod(U[f][comp][0] ** int(p) for (f, comp), p in zip(vars_, pw)) for c, pw in zip(coeffs, powers))
        if t.get('qs') is not None:
            Bq, ft, fr = t['qs']
            g *= sum(F(Bq[a][b]) * U[ft][0][a] * U[fr][0][b] for a in range(S) for b in range(S))
        return g

    def vector(self):
        s, S = self.s, 1 + self.nd
        out = [[[Fraction(0)] * b['nct'] for _ in range(b['nrows'])] for b in s['blocks']]
        for ie in range(s['nelems']):
            e = self.element(ie)
            for q in range(self.nq):
                Jinv, meas = self.geometry(e, q)
                U = [self.U(Fd, e, q, Jinv) for Fd in s['fields']]
                for t in s['terms']:
                    blk = s['blocks'][t['block']]
                    g = self.factor(t, ie, e, q, U)
                    for c in range(blk['nct']):
                        Ft = [Fraction(0)] * S
                        for a in range(S):
                            if t.get('f') is not None:
                                Ft[a] += F(t['f'][c][a])
                            if t.get('C') is not None:
                                Ft[a] += sum(F(t['C'][c][a][d][b]) * U[t['field']][d][b] for d in range(s['fields'][t['field']]['ncomp']) for b in range(S))
                        for m in range(blk['basis']['nb']):
                            Dm = self.D(blk['basis'], e, q, m, Jinv)
                            out[t['block']][int(blk['basis']['dofs'][e * blk['basis']['nb'] + m])][c] += F(s['weights'][q]) * meas * g * sum(Dm[a] * Ft[a] for a in range(S))
        return out

    def matrix(self):
        '''{(row, col): value} of a scalar block'''
        s, S = self.s, 1 + self.nd
        out = {}
        for ie in range(s['nelems']):
            e = self.element(ie)
            for q in range(self.nq):
                Jinv, meas = self.geometry(e, q)
                U = [self.U(Fd, e, q, Jinv) for Fd in s['fields']]
                Cq = [[Fraction(0)] * S for _ in range(S)]
                for t in s['terms']:
                    g = self.factor(t, ie, e, q, U, s.get('by_element'))
                    kind = t.get('kind', 0)
                    for a in range(S):
                        if kind == 0:
                            for b in range(S):
                                Cq[a][b] += g * F(t['C'][0][a][0][b])
                        elif kind == 1:
                            Cq[a][0] += g * sum(F(t['C'][0][a][0][b]) * U[t['field']][0][b] for b in range(S))
                        else:
                            for b in range(S):
                                Cq[a][b] += g * F(t['L'][0][a]) * sum(F(t['C'][0][x][0][b]) * U[t['field']][0][x] for x in range(S))
                for m in range(s['test']['nb']):
                    Dm = self.D(s['test'], e, q, m, Jinv)
                    for n in range(s['trial']['nb']):
                        Dn = self.D(s['trial'], e, q, n, Jinv)
                        key = int(s['test']['dofs'][e * s['test']['nb'] + m]), int(s['trial']['dofs'][e * s['trial']['nb'] + n])
                        out[key] = out.get(key, 0) + F(s['weights'][q]) * meas * sum(Dm[a] * Cq[a][b] * Dn[b] for a in range(S) for b in range(S))
        return out


def dyadic(spec, seed):
    '''the case with every number replaced by a multiple of 1/8 (sizes: powers of two), so that nothing is rounded on the way in'''
    rng = numpy.random.default_rng(seed)

    def d(a):
        return rng.integers(-8, 9, numpy.shape(a)) / 8.
    nd, nq, ne = spec['ndims'], spec['nq'], spec['mesh_nelems']
    points = rng.integers(1, 4, (nq, nd)) / 4.
    spec['weights'] = rng.integers(1, 5, nq) / 8.
    if spec['geom']['kind'] == 'box':
        spec['geom']['size'] = rng.choice([.5, 1., 2., -2.], (ne, nd))
    else:
        spec['geom']['jac'] = numpy.eye(nd) * rng.choice([1., 2.], (ne, nq, nd, 1)) + rng.integers(-1, 2, (ne, nq, nd, nd)) / 4.
    seen = set()
    for B in [b['basis'] for b in spec.get('blocks', ())] + [spec[k] for k in ('test', 'trial') if k in spec] + [Fd['basis'] for Fd in spec['fields']]:
        if id(B) not in seen:
            seen.add(id(B))
            msh = tc.mesh(tuple(spec['shape']), 'std', 1)
            B['T'] = tc.tables(msh, points)  # (linear functions at dyadic points: dyadic)
    for Fd in spec['fields']:
        Fd['u'] = d(Fd['u'])
    for t in spec['terms']:
        for k in ('C', 'f', 'L'):
            if t.get(k) is not None:
                t[k] = d(t[k])
        if t.get('scale') is not None:
            t['scale'] = rng.integers(1, 9, numpy.shape(t['scale'])) / 8.
        if t.get('qs') is not None:
            t['qs'] = (d(t['qs'][0]),) + tuple(t['qs'][1:])
    spec['polys'] = [(v, d(c), p) for v, c, p in spec['polys']]
    return spec


EXACT_VECTOR = [((1,), 'box', None), ((2,), 'tab', None), ((2, 1), 'box', 'permutation'), ((1, 2), 'tab', None)]


@pytest.mark.parametrize('shape,geom,elist', EXACT_VECTOR)
def test_vector_terms_exact(shape, geom, elist):
    '''two fields, two blocks, a polynomial factor, a scale array, a point factor on one or two linear elements: the longdouble restatement equals the exact sums to
    longdouble rounding (m roundings of 2^-64 against the magnitude)'''
    spec = tc.vector_case(shape, 'std', 1, geom=geom, nq=3, seed=7, elist=elist, ncomps=(1, 1), ncts=(1, 1))
    spec['shape'] = shape
    spec['mesh_nelems'] = int(numpy.prod(shape))
    spec = dyadic(spec, 8)
    exact = Exact(spec).vector()
    m = tc.gamma_m(spec)[0]
    for (value, mag, _, _), ex in zip(tr.vector_terms(spec), exact):
        assert any(x != 0 for row in ex for x in row)
        for v, a, row in zip(value, mag, ex):
            for c, x in enumerate(row):
                assert abs(Fraction(float(v[c])) + Fraction(float(v[c] - LD(float(v[c])))) - x) <= m * Fraction(1, 2 ** 63) * Fraction(float(a[c]))


@pytest.mark.parametrize('shape,geom,elist', EXACT_VECTOR)
def test_matrix_terms_exact(shape, geom, elist):
    '''kinds 0, 1 and 2 with a polynomial factor, scale arrays and a point factor, exactly'''
    spec = tc.matrix_case(shape, 'std', 1, geom=geom, nq=3, seed=9, elist=elist, by_element=elist is not None, nfields=2)
    spec['shape'] = shape
    spec = dyadic(spec, 10)
    assert sorted(t['kind'] for t in spec['terms']) == [0, 1, 2]
    exact = Exact(spec).matrix()
    value, mag, rowptr, colidx = tr.matrix_terms(spec)
    m = tc.gamma_m(spec)[0]
    assert len(exact) == len(value) and any(x != 0 for x in exact.values())
    for row in range(spec['nrows']):
        for k in range(rowptr[row], rowptr[row + 1]):
            v = Fraction(float(value[k])) + Fraction(float(value[k] - LD(float(value[k]))))
            assert abs(v - exact[row, int(colidx[k])]) <= m * Fraction(1, 2 ** 63) * Fraction(float(mag[k]))


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------------

def uses_gradients(spec):
    return any(numpy.asarray(t[k])[..., 1:].any() for t in spec['terms'] for k in ('C', 'f') if t.get(k) is not None)


APPLIES = {
    'kinds_swapped': lambda s: any(t.get('kind', 0) for t in s['terms']),
    'scale_by_element': lambda s: s.get('elist') is not None and not s.get('by_element') and any(t.get('scale') is not None for t in s['terms']),
    'jinv_transposed': lambda s: s['ndims'] >= 2 and s['geom']['kind'] != 'box' and uses_gradients(s),
    'no_det': lambda s: True,
    'no_face': lambda s: s['geom']['bnd_axis'] >= 0,
    'power_off_by_one': lambda s: bool(s.get('polys')) and any(t.get('poly', -1) == 0 for t in s['terms']),
    'qs_swapped': lambda s: any(t.get('qs') is not None and t['qs'][1] != t['qs'][2] and (numpy.asarray(t['qs'][0]) != numpy.asarray(t['qs'][0]).T).any() for t in s['terms']),
    'mask_ignored': lambda s: s.get('mask') is not None and not numpy.asarray(s['mask']).all(),
}
MUTANT_CASES = [('k_terms', name) for name in sorted(tc.K_TERMS)] + [('k_mterms', name) for name in sorted(tc.K_MTERMS)]


@pytest.mark.parametrize('family,name', MUTANT_CASES)
def test_mutants_are_far_outside_the_bound(family, name):
    '''On the inputs of the GPU cases: every mistake of terms_refs.MUTANTS that the case can show (APPLIES) moves some entry by more than 100 x gamma_m x magnitude.'''
    spec = tc.build(family, name)
    g = tc.gamma_m(spec)[1]
    ref = tr.vector_terms(spec) if 'blocks' in spec else [tr.matrix_terms(spec)]
    for mutant in tr.MUTANTS:
        if not APPLIES[mutant](spec):
            continue
        mut = tr.vector_terms(spec, mutant) if 'blocks' in spec else [tr.matrix_terms(spec, mutant)]
        ratio = max(float((numpy.abs(r[0] - x[0])[r[1] > 0] / (g * r[1][r[1] > 0])).max()) for r, x in zip(ref, mut))
        assert ratio > 100, (mutant, ratio)


def test_every_mutant_is_shown_by_some_case():
    specs = [tc.build(family, name) for family, name in MUTANT_CASES]
    for mutant in tr.MUTANTS:
        assert any(APPLIES[mutant](s) for s in specs), mutant
