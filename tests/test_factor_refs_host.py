'''The references of tests/factor_refs.py against each other, against exact rational arithmetic and against integrals computed by hand.  No GPU, no library.

  dyadic data    every input a small dyadic number, every Jacobian with an exactly representable determinant (and, for a face, a power of two as determinant and a
                 Pythagorean cofactor column): the longdouble restatement makes no rounding error and must EQUAL the exact one, values and indices.  The exact one
                 gets its |det| from this file's own Fraction arithmetic (permutation expansion; the face measure as sqrt(sum of squared minors)), so the geometry
                 formulas are restated twice, independently.
  by hand        two linear elements of lengths 1 and 2 in one dimension: the entries of int N_i N_j N_k (N_l) are sums of  h a! b! / (a + b + 1)!  (beta integral)
  the fixture    the rank-3 arrays that the REFERENCE's evaluable.factor built for the cubic functional of tests/golden/factor_cubic2d_spline2_4.npz, with the
                 quadratic-spline tables of the 4 x 4 mesh made on the host (nutils_amd.basis / nutils_amd.poly: numpy only)'''
import itertools
import math
from fractions import Fraction as F

import numpy
import pytest

import factor_refs as refs

LD = numpy.longdouble
NAN = float('nan')
RTOL = F(1, 10 ** 18)


def exact(x):
    '''a longdouble as a Fraction: its 64 bits of mantissa split over two doubles'''
    x = LD(x)
    hi = float(x)
    return F(hi) + F(float(x - LD(hi)))


def frac_det(J):
    n = len(J)
    total = F(0)
    for perm in itertools.permutations(range(n)):
        sign = (-1) ** sum(perm[a] > perm[b] for a in range(n) for b in range(a + 1, n))
        total += sign * math.prod(J[i][perm[i]] for i in range(n))
    return total


def frac_measure(J, axis=-1):
    '''|det J|, or the measure of the face xi_axis = const: |det J| |J^-T e_axis| = sqrt(sum_i minor(i, axis)^2), which must be rational here'''
    J = [[F(x) for x in row] for row in J]
    n = len(J)
    if axis < 0:
        return abs(frac_det(J))
    if n == 1:
        return F(1)
    s = sum(frac_det([[J[r][c] for c in range(n) if c != axis] for r in range(n) if r != i]) ** 2 for i in range(n))
    root = F(math.isqrt(s.numerator), math.isqrt(s.denominator))
    assert root * root == s, 'the face measure of this case is not rational'
    return root


def jacobians(geom, nd, nq, nelems_all):
    '''J[e][q] as nested lists of Fractions, from the definition of each geometry kind'''
    out = []
    for e in range(nelems_all):
        if geom['kind'] == 'box':
            size = numpy.asarray(geom['size']).reshape(-1, nd)[e]
            Jq = [[[F(size[i]) if i == j else F(0) for j in range(nd)] for i in range(nd)]] * nq
        elif geom['kind'] == 'tab':
            jac = numpy.asarray(geom['jac']).reshape(-1, nq, nd, nd)[e]
            Jq = [[[F(jac[q, i, j]) for j in range(nd)] for i in range(nd)] for q in range(nq)]
        else:
            gT = numpy.asarray(geom['gT'])
            ngb = gT.shape[0]
            X = numpy.asarray(geom['verts']).reshape(-1, nd)[numpy.asarray(geom['gdofs']).reshape(-1, ngb)[e]]
            Jq = [[[sum(F(X[a, i]) * F(gT[a, q, 1 + j]) for a in range(ngb)) for j in range(nd)] for i in range(nd)] for q in range(nq)]
        out.append(Jq)
    return out


def multilinear_tables(points):
    '''gT[2^nd][nq][1 + nd] of the multilinear functions prod_i (xi_i or 1 - xi_i), the last axis fastest in the function index'''
    points = numpy.asarray(points, dtype=float)
    nq, nd = points.shape
    gT = numpy.zeros((2 ** nd, nq, 1 + nd))
    for a, corner in enumerate(itertools.product((0, 1), repeat=nd)):
        f = [points[:, i] if c else 1 - points[:, i] for i, c in enumerate(corner)]
        gT[a, :, 0] = numpy.prod(f, axis=0)
        for j in range(nd):
            gT[a, :, 1 + j] = numpy.prod([(1. if c else -1.) + 0 * points[:, i] if i == j else f[i] for i, c in enumerate(corner)], axis=0)
    return gT


def dyadic_geometry(rng, kind, nd, nq, ne, axis):
    if kind == 'box':
        return dict(kind='box', size=rng.choice([-4., -.5, .5, 1., 2., 4.], (ne, nd)), bnd_axis=axis)
    if kind == 'tab' and axis < 0:
        jac = rng.integers(-3, 4, (ne, nq, nd, nd)).astype(float)
        for e, q in itertools.product(range(ne), range(nq)):
            while frac_det(jac[e, q].tolist()) == 0:
                jac[e, q] = rng.integers(-3, 4, (nd, nd))
        return dict(kind='tab', jac=jac)
    if kind == 'tab':  # determinant a power of two, of either sign, and the cofactors of column `axis` a Pythagorean tuple
        if nd == 2:
            both = {0: ([[4, 4], [2, 3]], [[-4, 4], [-2, 3]]), 1: ([[3, 2], [4, 4]], [[3, 1], [4, 0]])}[axis]  # det 4, -4; cofactors (3, 4)
        else:
            base = [[2, 2, 2], [0, 1, 0], [0, 0, 1]]  # det 2, the cofactors of column 0: (1, -2, -2), norm 3
            roll = lambda M, k: [[M[(i - k) % 3][(j - k) % 3] for j in range(3)] for i in range(3)]  # the same with the axes renamed cyclically: column k
            mirrored = [[-x for x in row] if i == 0 else row for i, row in enumerate(base)]
            both = roll(base, axis), roll(mirrored, axis)
        assert frac_det(both[0]) > 0 > frac_det(both[1])
        pick = rng.integers(0, 2, (ne, nq))
        return dict(kind='tab', jac=numpy.array(both, dtype=float)[pick] * rng.choice([.5, 1., 2.], (ne, nq, 1, 1)), bnd_axis=axis)  # (a power of two keeps both)
    # iso
    ngb = kind[1]
    if ngb == 3:
        gT = numpy.zeros((3, nq, 3))
        gT[:, :, 1:] = numpy.array([[-1., -1.], [1., 0.], [0., 1.]])[:, None, :]
        gT[:, :, 0] = NAN  # (the value slot of the geometry tables is read only where coordinates are asked for)
    else:
        gT = multilinear_tables(rng.choice([.25, .5, .75], (nq, nd)))
    if axis < 0:
        corners = numpy.array(list(itertools.product((0., 1.), repeat=nd)))[:ngb] if ngb != 3 else numpy.array([[0., 0.], [1., 0.], [0., 1.]])
        verts = (corners[None] * rng.choice([1., 2.], (ne, 1, nd)) + rng.choice([-.25, 0., .25], (ne, ngb, nd)) + rng.integers(0, 4, (ne, 1, nd))).reshape(-1, nd)
    else:  # boxes with power-of-two edges: J is diagonal and everything stays exact
        corners = numpy.array(list(itertools.product((0., 1.), repeat=nd)))
        verts = (corners[None] * rng.choice([-2., .5, 1., 4.], (ne, 1, nd)) + rng.integers(0, 4, (ne, 1, nd))).reshape(-1, nd)
    gdofs = rng.permutation(ne * ngb).reshape(ne, ngb)
    verts_shuffled = numpy.zeros_like(verts)
    verts_shuffled[gdofs.reshape(-1)] = verts
    return dict(kind='iso', gT=gT, gdofs=gdofs, verts=verts_shuffled, bnd_axis=axis)


DYADIC = [(kind, nd, -1) for kind in ('box', 'tab', ('iso', None)) for nd in (1, 2, 3)] + [(('iso', 3), 2, -1)] \
    + [(kind, nd, axis) for kind in ('box', 'tab', ('iso', None)) for nd in (2, 3) for axis in (0, nd - 1)]


@pytest.mark.parametrize('kind, nd, axis', DYADIC, ids=lambda v: str(v).replace(' ', ''))
def test_longdouble_restatement_equals_exact_arithmetic_on_dyadic_data(kind, nd, axis):
    rng = numpy.random.default_rng(7)
    if isinstance(kind, tuple):
        kind = ('iso', kind[1] or 2 ** nd)
    ne, nq, nb, ndofs = 7, 3, 2, 5
    geom = dyadic_geometry(rng, kind, nd, nq, ne, axis)
    J = jacobians(geom, nd, nq, ne)
    absdet = [[frac_measure(J[e][q], axis) for q in range(nq)] for e in range(ne)]
    if kind in ('tab', ('iso', 3)) or axis < 0 and kind != 'box':
        assert len({x for row in absdet for x in row}) > 2  # the measure varies from point to point
    T = numpy.full((3 * nb, nq, 1 + nd), NAN)
    T[:, :, 0] = rng.choice([-2., -.5, .25, 1., 3.], (3 * nb, nq))
    dofs = rng.integers(0, ndofs, (ne, nb))
    dofs[2] = dofs[2, 0]  # an element that repeats a dof
    weights = rng.choice([.25, .5, 1.], nq)
    for rank, tab, elist, scaled in (3, None, None, False), (4, rng.integers(0, 3, ne), [5, 2, 2, 6, 0, 5], True), (3, rng.integers(0, 3, ne), [6, 3, 1], True):
        nl = ne if elist is None else len(elist)
        scale = rng.choice([-2., -.5, 0., .5, 1.], (nl, nq)) if scaled else None
        common = dict(nelems=nl, nq=nq, rank=rank, weights=weights, T=T, dofs=dofs, nb=nb, coeff=-.5, scale=scale, elist=elist, tab=tab)
        values, indices = refs.factor_tensor_exact(absdet=absdet, **common)
        value, mag, indices_ld, count = refs.factor_tensor_ld(ndims=nd, geom=geom, **common)
        assert numpy.array_equal(indices, indices_ld) and len(values) > 3
        assert [exact(v) for v in value] == list(values)
        assert all(m >= abs(v) for m, v in zip(mag, value))
        everything, all_indices = refs.factor_tensor_exact(absdet=absdet, keep_zeros=True, **common)
        assert len(everything) == len({tuple(k) for k in all_indices.T.tolist()}) >= len(values)
        assert [v for v in everything if v != 0] == list(values)
        all_counts = refs.factor_tensor_ld(ndims=nd, geom=geom, keep_zeros=True, **common)[3]
        assert all_counts.sum() == nb ** rank * nl and count.tolist() == [c for c, v in zip(all_counts, everything) if v != 0]


def test_measure_condition_is_one_without_cancellation_and_grows_with_it():
    box = dict(kind='box', size=[[2., -3., .5]])
    m, c = refs.measure_ld(box, 3, 2, 0)
    assert m.tolist() == [3, 3] and c.tolist() == [1, 1]
    m, c = refs.measure_ld(dict(box, bnd_axis=1), 3, 2, 0)
    assert m.tolist() == [1, 1] and c.tolist() == [1, 1]
    tab = dict(kind='tab', jac=[[[[3., 2.], [4., 3.]]]])  # det = 9 - 8: the expansion cancels, (9 + 8) / 1
    m, c = refs.measure_ld(tab, 2, 1, 0)
    assert m.tolist() == [1] and c.tolist() == [17]
    m, c = refs.measure_ld(dict(tab, bnd_axis=0), 2, 1, 0)  # row 0 of the inverse: (3, -2): single entries, no further cancellation
    assert exact(m[0] ** 2) == 13 and c.tolist() == [17]


def linear_elements(points, weights):
    '''two elements of lengths 1 and 2 with N_0 = 1 - xi, N_1 = xi; the gradient slot holds NaN'''
    T = numpy.empty((2, len(points), 2), dtype=object)
    T[:] = NAN
    T[0, :, 0], T[1, :, 0] = [1 - p for p in points], list(points)
    return dict(nelems=2, nq=len(points), weights=weights, T=T, dofs=[[0, 1], [1, 2]], nb=2)


def by_hand(rank):
    '''{multi-index: integral}: on an element of length h,  int N_0^a N_1^b = h a! b! / (a + b + 1)!  -- rank 3: 1/4 and 1/12, rank 4: 1/5, 1/20 and 1/30'''
    beta = lambda a, b: F(math.factorial(a) * math.factorial(b), math.factorial(a + b + 1))
    want = {}
    for first, h in (0, 1), (1, 2):
        for loc in itertools.product((0, 1), repeat=rank):
            key = tuple(first + l for l in loc)
            want[key] = want.get(key, 0) + h * beta(rank - sum(loc), sum(loc))
    return want


@pytest.mark.parametrize('rank', [3, 4])
def test_two_linear_elements_by_hand(rank):
    want = by_hand(rank)
    if rank == 3:  # written out: the corner entries, the mixed ones, and the middle dof that both elements share
        assert want[0, 0, 0] == F(1, 4) and want[2, 2, 2] == F(2, 4) and want[1, 1, 1] == F(1, 4) + F(2, 4)
        assert want[0, 0, 1] == want[0, 1, 0] == want[1, 0, 0] == want[0, 1, 1] == F(1, 12) and want[1, 2, 2] == want[2, 1, 1] == F(2, 12)
        assert len(want) == 15
        points, weights = [F(0), F(1, 2), F(1)], [F(1, 6), F(4, 6), F(1, 6)]  # Simpson: exact for cubics
    else:
        assert want[0, 0, 0, 0] == F(1, 5) and want[1, 1, 1, 1] == F(3, 5) and want[0, 0, 0, 1] == F(1, 20) and want[0, 1, 0, 1] == F(1, 30) and want[1, 2, 2, 1] == F(2, 30)
        assert len(want) == 31
        points, weights = [F(k, 4) for k in range(5)], [F(k, 90) for k in (7, 32, 12, 32, 7)]  # Boole: exact up to degree 5
    case = linear_elements(points, weights)
    values, indices = refs.factor_tensor_exact(rank=rank, absdet=[[1] * len(points), [2] * len(points)], coeff=1, **case)
    assert [tuple(k) for k in indices.T.tolist()] == sorted(want)
    assert list(values) == [want[k] for k in sorted(want)]
    # the longdouble restatement on the same rule with its weights rounded to doubles (a negative size: the measure is its absolute value): to 1e-18 the exact
    # tensor of those rounded weights, which is the one by hand to the rounding of a weight
    case['weights'] = [float(w) for w in weights]
    case['T'] = case['T'].astype(float)
    rounded, _ = refs.factor_tensor_exact(rank=rank, absdet=[[1] * len(points), [2] * len(points)], coeff=1, **case)
    value, mag, indices_ld, count = refs.factor_tensor_ld(rank=rank, ndims=1, geom=dict(kind='box', size=[[1.], [-2.]]), coeff=1., **case)
    assert numpy.array_equal(indices_ld, indices)
    assert all(abs(exact(v) - r) <= RTOL * r for v, r in zip(value, rounded))
    assert all(abs(r - want[k]) <= F(1, 2 ** 52) * want[k] for r, k in zip(rounded, sorted(want)))
    assert numpy.array_equal(value, mag)  # every term is positive and a 1 x 1 determinant has no cancellation
    assert count.tolist() == [2 if set(k) == {1} else 1 for k in sorted(want)]


def test_ordered_run_sums_keep_the_order_of_the_list():
    big = 2. ** 60
    keys = [[4, 4], [0, 1], [4, 4], [0, 0], [4, 4]]
    values, indices = refs.ordered_run_sums(keys, [big, 3., 1., -2., -big])  # (2^60 + 1) - 2^60 = 0 in float64: dropped
    assert values.tolist() == [-2., 3.] and indices.tolist() == [[0, 0], [0, 1]]
    values, indices = refs.ordered_run_sums(keys, [big, 3., -big, -2., 1.])  # (2^60 - 2^60) + 1 = 1
    assert values.tolist() == [-2., 3., 1.] and indices.tolist() == [[0, 0, 4], [0, 1, 4]]
    values, indices = refs.ordered_run_sums(numpy.zeros((0, 3)), [])
    assert values.shape == (0,) and indices.shape == (3, 0)
    # integers: any order, and equal to the exact tensor (nb = 1, T = 1, one point: a contribution is its scale)
    rng = numpy.random.default_rng(5)
    dofs, scale = rng.integers(0, 6, 40), rng.integers(-2, 3, 40)
    values, indices = refs.ordered_run_sums(numpy.repeat(dofs[:, None], 3, 1), scale.astype(float))
    exact_values, exact_indices = refs.factor_tensor_exact(nelems=40, nq=1, rank=3, weights=[1], absdet=numpy.ones((40, 1)), T=numpy.ones((1, 1, 2)), dofs=dofs, nb=1, scale=scale)
    assert numpy.array_equal(indices, exact_indices) and values.tolist() == list(exact_values)


# ---- the reference's own rank-3 tensor ------------------------------------------------------------------------------------------------------

def spline_tables(absolute=False):
    '''T[classes * 9][16][3] (slot 0 only), dofs, classes and the Gauss rule of degree 6 for quadratic splines on 4 x 4 elements; absolute: the sums of the
    |coefficient monomial| instead of the values, the scale of the rounding errors of a tabulated value'''
    from nutils_amd import basis, points, poly
    b = basis.StructuredBasis((4, 4), 'spline', 2)
    pts = points.gauss(6, 2)
    coeffs = b.all_class_coefficients()
    mono = poly.monomials(pts.coords, 2, poly.degree(2, coeffs.shape[1]))
    T = numpy.full((len(coeffs), pts.npoints, 3), NAN)
    T[:, :, 0] = numpy.abs(coeffs) @ numpy.abs(mono).T if absolute else coeffs @ mono.T
    return b, pts, T


def test_restatement_equals_the_rank3_tensor_of_the_reference(golden):
    '''Indices equal.  Values: the fixture holds float64 results of the reference's own integration of the same polynomials, ours are longdouble sums over float64
    tables; either side is off by its roundings, relative to the magnitude built from the sums of |coefficient monomial| of the tables.  Per entry, on our side:
    rank + 3 products, nq - 1 = 15 and count - 1 additions, 2 operations of the 2 x 2 determinant, and per tabulated factor 24 (two powers and their product, the
    coefficient, 14 additions, and 6 for the coefficients themselves, which come out of a recursion in float64); the reference's side is taken as no longer
    than that -- its operations are not ours to count -- so the bound is gamma_2m.'''
    g = golden('factor_cubic2d_spline2_4')
    i = next(i for i in range(int(g['nmonomials'])) if int(g[f'm{i}_nargs']) == 3)
    want_values, want_indices = g[f'm{i}_values'], numpy.stack([g[f'm{i}_idx{k}'] for k in range(3)])
    b, pts, T = spline_tables()
    common = dict(nelems=16, ndims=2, nq=pts.npoints, rank=3, weights=pts.weights, geom=dict(kind='box', size=numpy.full((16, 2), .25)),
                  dofs=[b.get_dofs(e) for e in range(16)], nb=9, coeff=1 / 3., tab=b.element_classes())
    value, _, indices, count = refs.factor_tensor_ld(T=T, **common)
    mag = refs.factor_tensor_ld(T=spline_tables(absolute=True)[2], **common)[0]
    assert b.nclasses == 9 and numpy.array_equal(indices, want_indices)
    m = 2 * ((3 + 3) + (pts.npoints - 1) + (count - 1) + 2 + 3 * 24)
    u = LD(2) ** -53
    bound = m * u / (1 - m * u) * mag
    err = numpy.abs(value - want_values.astype(LD))
    print(f'rank-3 fixture: max err / bound = {float((err / bound).max()):.3f}, m up to {m.max()}')
    assert (err <= bound).all()
