'''The references of tests/pointwise_refs.py on tiny inputs against exact rational arithmetic (fractions.Fraction), written out here entry by entry: every kind,
0 to 4 gathered arguments, a repeated output index, accumulation.  The references compute in longdouble, so they need not equal the exact result bit for bit, only
to 1e-18 relative (64 bits of mantissa: 5.4e-20 per operation); their magnitudes (the sums of absolute terms) are held to the same.  No GPU, no library.'''
import math
from fractions import Fraction as F

import numpy

import pointwise_refs as refs

RTOL = F(1, 10 ** 18)


def exact(x):
    '''a longdouble (or anything narrower) as a Fraction: its 64 bits of mantissa split over two doubles'''
    x = numpy.longdouble(x)
    hi = float(x)
    return F(hi) + F(float(x - numpy.longdouble(hi)))


def agree(got, want):
    got, want = numpy.asarray(got).reshape(-1), list(want)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert abs(exact(g) - w) <= RTOL * abs(w), (g, float(w))


def flat(nested):
    return [x for item in nested for x in (flat(item) if isinstance(item, list) else [item])]


def test_monomial_every_argument_count_repeated_outputs_and_an_output_without_entries():
    v = [1.5, -2.25, 3., .1, 7.]
    a = [[.5, -3., 1.25], [2., .3], [-1., 4., .75, 1.1], [3., -.7]]
    j = [[0, 2, 2, 1, 0], [1, 1, 0, 0, 1], [3, 0, 2, 2, 1], [0, 1, 1, 0, 0]]
    o = [2, 0, 2, 2, 0]
    out = [10., -.2, .6]
    alpha = -.5
    for nargs in range(5):
        t = [F(alpha) * F(v[i]) * math.prod(F(a[k][j[k][i]]) for k in range(nargs)) for i in range(5)]
        value, mag = refs.monomial(v, a[:nargs], j[:nargs], out, o, alpha)
        agree(value, [F(10.) + t[1] + t[4], F(-.2), F(.6) + t[0] + t[2] + t[3]])
        agree(mag, [10 + abs(t[1]) + abs(t[4]), F(.2), F(.6) + abs(t[0]) + abs(t[2]) + abs(t[3])])
        value, mag = refs.monomial(v, a[:nargs], j[:nargs], [.25], None, alpha)  # the scalar result
        agree(value, [F(.25) + sum(t)])
        agree(mag, [F(.25) + sum(map(abs, t))])
    # written out once in full: three arguments, entry 3 = -.5 * .1 * a0[1] * a1[0] * a2[2]
    value, _ = refs.monomial(v, a[:3], j[:3], [0., 0., 0.], o, alpha)
    agree(value[1:], [0, F(-.5) * F(1.5) * F(.5) * F(.3) * F(1.1) + F(-.5) * 3 * F(1.25) * 2 * F(.75) + F(-.5) * F(.1) * -3 * 2 * F(.75)])
    value, mag = refs.monomial([], [], [], [3., 4.], [], 2.)
    agree(value, [3, 4])
    agree(mag, [3, 4])


def test_monomial_csr_with_an_empty_row_a_repeated_column_and_a_filled_y():
    rowptr, colidx = [0, 2, 2, 5], [1, 1, 0, 2, 0]
    v, x, y, alpha = [1.5, .1, -2., .3, 4.], [.7, -1.25, 3.], [1., -2., .5], -.5
    value, mag = refs.monomial_csr(rowptr, colidx, v, x, y, alpha)
    a = F(alpha)
    agree(value, [1 + a * F(1.5) * F(-1.25) + a * F(.1) * F(-1.25), F(-2), F(.5) + a * -2 * F(.7) + a * F(.3) * 3 + a * 4 * F(.7)])
    agree(mag, [1 + F(.5) * F(1.5) * F(1.25) + F(.5) * F(.1) * F(1.25), F(2), F(.5) + F(.5) * 2 * F(.7) + F(.5) * F(.3) * 3 + F(.5) * 4 * F(.7)])
    value, mag = refs.monomial_csr([0], [], [], x, [], alpha)
    assert len(value) == len(mag) == 0


def test_index_copy_all_four_index_combinations_leave_the_rest_alone():
    src, dst = [10., 11., 12., 13., 14.], [-1.] * 6
    assert refs.index_copy(src[:3], dst).tolist() == [10, 11, 12, -1, -1, -1]
    assert refs.index_copy(src, dst, src_index=[4, 4, 0]).tolist() == [14, 14, 10, -1, -1, -1]
    assert refs.index_copy(src, dst, dst_index=[5, 0, 3]).tolist() == [11, -1, -1, 12, -1, 10]
    assert refs.index_copy(src, dst, src_index=[2, 2, 1, 4], dst_index=[3, 1, 5, 0]).tolist() == [14, 12, -1, 12, -1, 11]
    assert dst == [-1.] * 6


def test_pointwise_poly_powers_0_and_31_strides_and_no_terms():
    x0, x1 = [.9, -1.1, 2.], [.3, 99., -.7, 99., 1.5]  # x1 at stride 2
    coeffs, powers = [2., -.5, .1], [[0, 3], [2, 1], [31, 0]]
    value, mag = refs.pointwise_poly([x0, x1], [1, 2], coeffs, powers, 3)
    t = [[2 * F(b) ** 3, F(-.5) * F(a) ** 2 * F(b), F(.1) * F(a) ** 31] for a, b in zip(x0, x1[::2])]
    agree(value, [sum(ti) for ti in t])
    agree(mag, [sum(map(abs, ti)) for ti in t])
    value, mag = refs.pointwise_poly([], [], [1.5, .25], [[], []], 2)  # no variables: the sum of the coefficients
    agree(value, [F(1.75)] * 2)
    value, mag = refs.pointwise_poly([x0], [1], [], [], 3)
    assert value.tolist() == mag.tolist() == [0, 0, 0]


def test_point_forms_every_kind():
    Ut, Ur = [[.3, -1.5, .7], [2., .1, -.9]], [[1.1, .4, -2.], [-.6, 3., .2]]
    B, L, sc = [[1., 2., -3.], [.5, -.25, 4.], [.1, 7., -.3]], [.5, -2., 1.1], [.7, -1.3]  # B is not symmetric
    R = range(3)
    for scale in None, sc:
        s = [1, 1] if scale is None else [F(x) for x in sc]
        value, mag = refs.point_forms(0, Ut, B, Ur=Ur, scale=scale)
        agree(value, [sum(s[i] * F(B[a][b]) * F(Ut[i][a]) * F(Ur[i][b]) for a in R for b in R) for i in range(2)])
        agree(mag, [sum(abs(s[i] * F(B[a][b]) * F(Ut[i][a]) * F(Ur[i][b])) for a in R for b in R) for i in range(2)])
        value, mag = refs.point_forms(1, Ut, B, scale=scale)
        agree(value, [s[i] * sum(F(B[a][x]) * F(Ut[i][x]) for x in R) if b == 0 else 0 for i in range(2) for a in R for b in R])
        agree(mag, [abs(s[i]) * sum(abs(F(B[a][x]) * F(Ut[i][x])) for x in R) if b == 0 else 0 for i in range(2) for a in R for b in R])
        value, mag = refs.point_forms(2, Ut, B, L=L, scale=scale)
        agree(value, [s[i] * F(L[a]) * sum(F(B[x][b]) * F(Ut[i][x]) for x in R) for i in range(2) for a in R for b in R])
        agree(mag, [abs(s[i] * F(L[a])) * sum(abs(F(B[x][b]) * F(Ut[i][x])) for x in R) for i in range(2) for a in R for b in R])
    # one entry of each in full, S = 2: kind 1 contracts the SECOND index of B, kind 2 the first
    Ut2, B2 = [[.3, -1.5]], [[1., 2.], [.5, -.25]]
    agree(refs.point_forms(1, Ut2, B2)[0][0, 1], [F(.5) * F(.3) + F(-.25) * F(-1.5), 0])
    agree(refs.point_forms(2, Ut2, B2, L=[1., 1.])[0][0, 1], [1 * F(.3) + F(.5) * F(-1.5), 2 * F(.3) + F(-.25) * F(-1.5)])


def test_point_expr_two_runs_of_an_output_a_broadcast_factor_scale_and_accumulation():
    x0, x1 = [.3, -1.5, .7, 2., .1, -.9], [1.25, -.4]  # x0: stride 2 over 3 points, offsets 0..1; x1: stride 0, a constant table
    oidx, off, coef = [0, 2, 0], [[0, 1], [1, 0], [1, 1]], [1.5, -.2, 3.]
    sc, prev = [.7, -1.3, .5], [[1., 2., 3., 4.], [-1., -2., -3., -4.], [.5, .25, .125, 8.]]
    for scale in None, sc:
        s = [1] * 3 if scale is None else [F(x) for x in sc]
        t = [[s[i] * F(coef[e]) * F(x0[2 * i + off[e][0]]) * F(x1[off[e][1]]) for e in range(3)] for i in range(3)]
        value, mag = refs.point_expr([x0, x1], [2, 0], oidx, off, coef, 3, 4, scale=scale)
        agree(value, flat([[t[i][0] + t[i][2], 0, t[i][1], 0] for i in range(3)]))
        agree(mag, flat([[abs(t[i][0]) + abs(t[i][2]), 0, abs(t[i][1]), 0] for i in range(3)]))
        value, mag = refs.point_expr([x0, x1], [2, 0], oidx, off, coef, 3, 4, scale=scale, out=prev)
        agree(value, flat([[F(prev[i][0]) + t[i][0] + t[i][2], F(prev[i][1]), F(prev[i][2]) + t[i][1], F(prev[i][3])] for i in range(3)]))
        agree(mag, flat([[abs(F(prev[i][0])) + abs(t[i][0]) + abs(t[i][2]), abs(F(prev[i][1])), abs(F(prev[i][2])) + abs(t[i][1]), abs(F(prev[i][3]))] for i in range(3)]))
    value, mag = refs.point_expr([], [], [1, 1], None, [1.5, .25], 2, 2, scale=[2., 3.])  # no factors: the coefficients
    agree(value, [0, F(3.5), 0, F(5.25)])
    value, mag = refs.point_expr([x0], [2], [], [], [], 3, 2, out=prev[0] + prev[1][:2])  # no entries: `out` stays
    agree(value, [1, 2, 3, 4, -1, -2])


def _rational(B, w, W, dW, A=None, c=1):
    '''(N, dN_k) and their magnitudes for one function at one point in Fractions; B = (B, dB_0, ..)'''
    N = w * B[0] / W
    A = [abs(d) for d in dW] if A is None else A
    return ([N] + [w * B[1 + k] / W - w * B[0] * dW[k] / W ** 2 for k in range(len(dW))],
            [c * abs(N)] + [c * (abs(w * B[1 + k] / W) + abs(w * B[0] / W ** 2) * A[k]) for k in range(len(dW))])


def test_rationalize_given_and_summed_weight_function_uniform_and_ragged():
    # three functions of two points each, two dimensions: T[function][point] = (B, dB_0, dB_1); one sign change among the w B of the second element
    T = [[[.3, -1.5, .7], [2., .1, -.9]], [[1.1, .4, 2.], [.6, 3., .2]], [[-.2, .8, 1.3], [.9, -.5, -.35]]]
    weights, dofs = [1.5, .7, 2.], [1, 2, 1]  # the first and the last function share a dof
    Tf = [[[F(x) for x in pt] for pt in fn] for fn in T]
    w = [F(weights[d]) for d in dofs]
    # ragged: element 0 has the single function 0, element 1 the functions 1 and 2
    W, dW = [[.5, 2.], [1.25, -.8]], [[[.3, -1.], [2., .5]], [[-.7, .1], [.9, 4.]]]
    value, mag = refs.rationalize(T, 2, 0, dofs, weights, 2, 2, W=W, dW=dW, off=[0, 1, 3])
    want = [_rational(Tf[f][q], w[f], F(W[e][q]), [F(x) for x in dW[e][q]]) for f, e in ((0, 0), (1, 1), (2, 1)) for q in range(2)]
    agree(value, flat([list(v) for v, _ in want]))
    agree(mag, flat([list(m) for _, m in want]))
    value, mag = refs.rationalize(T, 2, 0, dofs, weights, 2, 2, off=[0, 1, 3])
    want = []
    for fns in (0,), (1, 2):
        for f in fns:
            for q in range(2):
                Ws = sum(w[g] * Tf[g][q][0] for g in fns)
                dWs = [sum(w[g] * Tf[g][q][1 + k] for g in fns) for k in range(2)]
                c = sum(abs(w[g] * Tf[g][q][0]) for g in fns) / abs(Ws)
                A = [sum(abs(w[g] * Tf[g][q][1 + k]) for g in fns) for k in range(2)]
                want.append(_rational(Tf[f][q], w[f], Ws, dWs, A, c))
    agree(value, flat([list(v) for v, _ in want]))
    agree(mag, flat([list(m) for _, m in want]))
    N = numpy.asarray(value).reshape(3, 2, 3)
    agree(N[0, :, 0], [1, 1])  # a single function: N = 1 ..
    assert abs(exact(N[0, 0, 1])) <= RTOL * exact(numpy.asarray(mag).reshape(3, 2, 3)[0, 0, 1])  # .. and dN = 0, to rounding
    agree(N[1, :, 0] + N[2, :, 0], [1, 1])
    # uniform: one element of nb = 3 functions in one dimension (the tables read as [3][2 points][2] need 12 numbers)
    T1 = [[[.3, -1.5], [.7, 2.]], [[.1, -.9], [1.1, .4]], [[2., .6], [3., .2]]]
    T1f = [[[F(x) for x in pt] for pt in fn] for fn in T1]
    value, mag = refs.rationalize(T1, 1, 3, dofs, weights, 2, 1)
    want = []
    for f in range(3):
        for q in range(2):
            Ws = sum(w[g] * T1f[g][q][0] for g in range(3))
            dWs = [sum(w[g] * T1f[g][q][1] for g in range(3))]
            A = [sum(abs(w[g] * T1f[g][q][1]) for g in range(3))]
            want.append(_rational(T1f[f][q], w[f], Ws, dWs, A, 1))  # every w B is positive: c = 1
    agree(value, flat([list(v) for v, _ in want]))
    agree(mag, flat([list(m) for _, m in want]))
    # .. and one entry in full: dN of function 1 at point 0 with W = 1.25, dW = -.8 given
    value, _ = refs.rationalize(T1, 1, 3, dofs, weights, 2, 1, W=[[1.25, 1.]], dW=[[[-.8], [0.]]])
    agree([value[5]], [F(2.) * F(-.9) / F(1.25) - F(2.) * F(.1) * F(-.8) / F(1.25) ** 2])


def test_structured_dofs_periodic_wrap_and_element_window():
    # one periodic axis with 3 elements, 3 dofs and 4 local functions: dofs repeat inside an element
    assert refs.structured_dofs((3,), (4,), (3,), [0, 1, 2], 0, 3).tolist() == [[0, 1, 2, 0], [1, 2, 0, 1], [2, 0, 1, 2]]
    assert refs.structured_dofs((3,), (4,), (3,), [0, 1, 2], 1, 1).tolist() == [[1, 2, 0, 1]]
    # 2 x 2 elements, 2 x 2 local functions, 3 x 2 dofs, the second axis periodic: dof = ((s0[i] + a) % 3) * 2 + (s1[j] + b) % 2
    start = [0, 1, 0, 1]
    assert refs.structured_dofs((2, 2), (2, 2), (3, 2), start, 0, 4).tolist() == [[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 4, 5], [3, 2, 5, 4]]
    assert refs.structured_dofs((2, 2), (2, 2), (3, 2), start, 1, 2).tolist() == [[1, 0, 3, 2], [2, 3, 4, 5]]
    assert refs.structured_dofs((2, 2), (2, 2), (3, 2), start, 3, 0).shape == (0, 4)
    # three axes, one element each but the last: the last axis is fastest in both the element and the function index
    assert refs.structured_dofs((1, 1, 2), (1, 2, 2), (1, 2, 3), [0, 0, 0, 1], 0, 2).tolist() == [[0, 1, 3, 4], [1, 2, 4, 5]]
