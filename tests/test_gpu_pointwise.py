'''The pointwise, gather and scatter helper kernels (nh_monomial.hip; nh_rationalize and nh_structured_dofs of nh_runtime.hip) one by one through the
nutils_amd.kernels wrappers, against the plain restatements of tests/pointwise_refs.py.  Every kernel gets two kinds of input:

  exact   small integers (dyadic numbers where a quotient enters), chosen so that every product and every partial sum is an integer far below 2^53 in any
          order of summation: float64 makes no rounding error and the result must EQUAL the reference (numpy.array_equal).  A dropped, doubled or misplaced
          entry shows whatever the order of the atomics.
  real    random doubles from a fixed seed, held per output to  |got - ref| <= (k + m + 1) 2^-53 1.01 sum |terms|,  k the multiplications (roundings of a
          product or quotient) a term goes through, m the summands into the output.  This is the forward bound of a sum of m products of k + 1 factors:
          a term passes at most k roundings as a product and m - 1 as part of a sum, (1 + u)^(k + m - 1) - 1 < (k + m + 1) u 1.01 for every count met here
          (k + m < 1.1e6), in any order of summation, with or without contraction to fma (which only removes roundings) -- derived, not measured.  The
          magnitude sum |terms| comes from the reference, an initial content of the output counted as one term; k and m stand beside each assertion,
          counted from the kernel source.

Sizes are the smallest at which the kernel takes another path: 0, 1, one entry either side of a wave (64) and of a workgroup (256), and one pass more than
the launch's cap on workgroups, where the grid-stride loops of k_monomial (256*16 workgroups: n > 1 048 576) and k_index_copy (8192 workgroups to device
memory: n > 2 097 152; 64 to page-locked host memory: n > 16 384) run a second trip.  "Rejected" cases are argument checks that return a status before any
launch.'''
import numpy
import pytest

import pointwise_refs as refs

pytestmark = pytest.mark.gpu

LD = numpy.longdouble
U = LD(2) ** -53


def dev(a, dtype='float64'):
    from nutils_amd import device
    return device.to_dev(numpy.asarray(a), dtype)


def host(t):
    from nutils_amd import device
    return device.to_host(t)


def within(got, value, mag, k, m, what=''):
    '''the per-output bound of the module docstring; m a number or an array of the outputs' shape.  A NaN fails.'''
    got, value, mag = numpy.asarray(got, dtype=LD).reshape(-1), numpy.asarray(value, dtype=LD).reshape(-1), numpy.asarray(mag, dtype=LD).reshape(-1)
    assert got.shape == value.shape == mag.shape, (got.shape, value.shape, mag.shape)
    bound = (k + numpy.asarray(m, dtype=LD).reshape(-1) + 1) * U * LD('1.01') * mag
    err = numpy.abs(got - value)
    bad = numpy.flatnonzero(~(err <= bound))
    assert not len(bad), f'{what}: {len(bad)} of {len(got)} outputs beyond the bound, the first at {bad[0]}: got {got[bad[0]]!r}, reference {value[bad[0]]!r}, ' \
                         f'error {err[bad[0]]!r}, bound {numpy.broadcast_to(bound, got.shape)[bad[0]]!r}'


def equal(got, value, what=''):
    '''exact inputs: the float64 result IS the reference'''
    got, value = numpy.asarray(got).reshape(-1), numpy.asarray(value).reshape(-1)
    assert got.shape == value.shape, (got.shape, value.shape)
    same = numpy.array_equal(got, value.astype(got.dtype))
    bad = numpy.flatnonzero(got != value.astype(got.dtype))
    assert same, f'{what}: {len(bad)} of {len(got)} outputs differ, the first at {bad[0]}: got {got[bad[0]]!r}, reference {value[bad[0]]!r}'


def ints(rng, lo, hi, shape):
    '''integers lo..hi (inclusive) as float64'''
    return rng.integers(lo, hi + 1, shape).astype(float)


@pytest.fixture
def nan_empty(monkeypatch):
    '''the wrappers allocate their result with device.empty: hand out NaN instead, so that an output the kernel should have written and did not shows'''
    from nutils_amd import device
    plain = device.empty

    def empty(n, dtype):
        out = plain(n, dtype)
        if dtype == 'float64':
            out.fill_(float('nan'))
        return out
    monkeypatch.setattr(device, 'empty', empty)


class Null:
    '''stands for a tensor whose pointer is NULL'''
    data_ptr = staticmethod(lambda: 0)


# ---- nh_monomial ------------------------------------------------------------------------------------------------------------------

def monomial_case(rng, n, nargs, nout, exact, spread=None):
    '''values, gathered arguments with their index arrays, an output index onto `spread` of the nout outputs (all of them if None; nout None: the scalar
    result) and a filled `out`'''
    lens = [5, 9, 6, 11][:nargs]
    if exact:  # |term| <= 3 * 8 * 2^4 = 384, a sum of 1.1e6 of them < 2^29
        values, args, out = ints(rng, -8, 8, n), [ints(rng, -2, 2, m) for m in lens], ints(rng, -8, 8, nout or 1)
    else:
        values, args, out = rng.standard_normal(n), [rng.uniform(-2, 2, m) for m in lens], rng.standard_normal(nout or 1)
    indices = [rng.integers(0, m, n) for m in lens]
    out_index = None if nout is None else rng.permutation(nout)[:spread or nout][rng.integers(0, spread or nout, n)]
    return values, args, indices, out, out_index


def run_monomial(case, alpha):
    from nutils_amd import kernels
    values, args, indices, out, out_index = case
    out_dev = dev(out)
    kwargs = {} if alpha is None else {'alpha': alpha}
    kernels.monomial(dev(values), [dev(a) for a in args], [dev(i, 'int64') for i in indices], out_dev, None if out_index is None else dev(out_index, 'int64'), **kwargs)
    return host(out_dev)


def check_monomial(rng, n, nargs, nout, alphas, spread=None):
    for exact, alpha in zip((True, False), alphas):
        case = monomial_case(rng, n, nargs, nout, exact, spread)
        values, args, indices, out, out_index = case
        got = run_monomial(case, alpha)
        value, mag = refs.monomial(values, args, indices, out, out_index, 1. if alpha is None else alpha)
        what = f'n={n} nargs={nargs} nout={nout} alpha={alpha}'
        if exact:
            equal(got, value, what)
        else:
            # k = 1 + nargs: alpha * values[i], then one product per gathered argument;  m = the entries onto the output and its initial content
            m = (n if out_index is None else numpy.bincount(out_index, minlength=nout)) + 1
            within(got, value, mag, 1 + nargs, m, what)


@pytest.mark.parametrize('scatter', [False, True], ids=['scalar', 'scattered'])
@pytest.mark.parametrize('nargs', range(5))
def test_monomial(nargs, scatter):
    '''0 to 4 gathered arguments, scalar and scattered, around a wave and a workgroup; alpha given or left at its default; `out` holds values before.  The
    scalar result takes the wave reduction with a last wave that is partly past n.'''
    rng = numpy.random.default_rng(100 + nargs)
    for n in 0, 1, 63, 64, 65, 255, 257:
        check_monomial(rng, n, nargs, 7 if scatter else None, (None, None) if n == 64 else (-3., .37))


def test_monomial_heavy_repeats():
    '''every entry onto 3 of 5 outputs: the other two keep their content'''
    rng = numpy.random.default_rng(110)
    check_monomial(rng, 257, 3, 5, (2., -1.7), spread=3)


@pytest.mark.parametrize('scatter', [False, True], ids=['scalar', 'scattered'])
def test_monomial_second_grid_stride_trip(scatter):
    '''n = 256 * 16 * 256 + 300: every thread of the capped grid has a second entry, 300 of them a third'''
    rng = numpy.random.default_rng(120 + scatter)
    check_monomial(rng, 1048576 + 300, 2, 4099 if scatter else None, (-3., .37))


def test_monomial_rejects_five_arguments():
    from nutils_amd import _lib, kernels
    x, i, out = dev(numpy.ones(4)), dev(numpy.zeros(4), 'int64'), dev(numpy.zeros(1))
    with pytest.raises(_lib.NutilsHipError, match='at most 4 gathered'):
        kernels.monomial(x, [x] * 5, [i] * 5, out)
    assert host(out)[0] == 0


# ---- nh_monomial_csr --------------------------------------------------------------------------------------------------------------

ROWLENS = 33, 0, 100, 1, 64, 7, 31, 0, 32, 65, 2  # 11 rows: the last wave of the second workgroup holds row 10 and a half-wave past the end


def test_monomial_csr():
    '''one half-wave per row: rows of 0, 1, 31, 32, 33, 64, 100 entries (none, one lane, one short of / exactly / one more than a trip of the half-wave, two
    trips, four with a partial last) in shuffled order, columns repeating inside a row, alpha = -0.5, y filled before'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(200)
    ncols = 37
    rowptr = numpy.concatenate([[0], numpy.cumsum(ROWLENS)])
    colidx = rng.integers(0, ncols, rowptr[-1])
    colidx[rowptr[2]:rowptr[2] + 3] = colidx[rowptr[2] + 40]  # (100 entries over 37 columns repeat anyway; and so do the first three of that row)
    colidx[rowptr[10]:rowptr[11]] = 5  # the row of 2: one column twice
    for exact in True, False:
        if exact:  # |term| <= 8 * 2 / 2, a row sums to at most 800
            values, x, y = ints(rng, -8, 8, rowptr[-1]), ints(rng, -2, 2, ncols), ints(rng, -8, 8, len(ROWLENS))
        else:
            values, x, y = rng.standard_normal(rowptr[-1]), rng.uniform(-2, 2, ncols), rng.standard_normal(len(ROWLENS))
        y_dev = dev(y)
        kernels.monomial_csr(dev(rowptr, 'int64'), dev(colidx, 'int64'), dev(values), dev(x), y_dev, alpha=-.5)
        value, mag = refs.monomial_csr(rowptr, colidx, values, x, y, -.5)
        if exact:
            equal(host(y_dev), value)
        else:
            # k = 2: values[k] * x[colidx[k]], then alpha * (the row's sum);  m = the entries of the row and the initial y[r].  (The butterfly adds the 32
            # lane sums in a tree; lanes without entries add exact zeros.)
            within(host(y_dev), value, mag, 2, numpy.array(ROWLENS) + 1)


def test_monomial_csr_without_rows():
    from nutils_amd import kernels
    kernels.monomial_csr(dev([0], 'int64'), dev([], 'int64'), dev([]), dev(numpy.ones(3)), dev([]), alpha=-.5)


# ---- nh_index_copy ----------------------------------------------------------------------------------------------------------------

SENTINEL = -7.25


def index_copy_case(rng, n, with_src, with_dst, size=None):
    '''src and dst of one length `size` (n + 9 if an index array is given), so that either index array is a valid index of either; dst_index distinct'''
    size = size or (n + 9 if with_src or with_dst else n)
    src = rng.standard_normal(size if with_src or with_dst else n)
    return src, rng.integers(0, size, n) if with_src else None, rng.permutation(size)[:n] if with_dst else None, numpy.full(size, SENTINEL)


@pytest.mark.parametrize('with_dst', [False, True], ids=['', 'dst_index'])
@pytest.mark.parametrize('with_src', [False, True], ids=['', 'src_index'])
def test_index_copy(with_src, with_dst):
    '''the four combinations of index arrays; what dst_index does not name keeps the sentinel'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(300)
    for n in 1, 255, 256, 257:
        for exact in True, False:
            src, sidx, didx, dst = index_copy_case(rng, n, with_src, with_dst)
            if exact:
                src = numpy.arange(len(src)) + 1.
            dst_dev = dev(dst)
            kernels.index_copy(dev(src), dst_dev, None if sidx is None else dev(sidx, 'int64'), None if didx is None else dev(didx, 'int64'))
            want = refs.index_copy(src, dst, sidx, didx)
            assert (want == SENTINEL).sum() == len(dst) - n
            # k = 0, m = 1: a copy has no rounding, the bound for random doubles is equality too
            equal(host(dst_dev), want, f'n={n}')


def test_index_copy_second_grid_stride_trip_on_the_device():
    '''n = 8192 * 256 + 300 to device memory'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(310)
    n = 2097152 + 300
    src, sidx, didx, dst = index_copy_case(rng, n, True, True)
    dst_dev = dev(dst)
    kernels.index_copy(dev(src), dst_dev, dev(sidx, 'int64'), dev(didx, 'int64'))
    equal(host(dst_dev), refs.index_copy(src, dst, sidx, didx))  # (k = 0, m = 1)


def test_index_copy_second_grid_stride_trip_to_page_locked_host_memory():
    '''n = 64 * 256 + 300 into a page-locked host tensor, allocated as solver._HostMirror allocates its buffers: the path of the Cahn-Hilliard step'''
    from nutils_amd import device, kernels
    t = device.require_gpu()
    rng = numpy.random.default_rng(320)
    n = 16384 + 300
    src, sidx, didx, dst = index_copy_case(rng, n, True, True)
    src_dev = dev(src)
    buf = t.empty(src_dev.shape, dtype=src_dev.dtype, pin_memory=True)
    buf.fill_(SENTINEL)
    kernels.index_copy(src_dev, buf, dev(sidx, 'int64'), dev(didx, 'int64'))
    device.synchronize()
    equal(buf.numpy(), refs.index_copy(src, dst, sidx, didx))  # (k = 0, m = 1)


def test_index_copy_refuses_pageable_host_memory():
    from nutils_amd import device, kernels
    t = device.require_gpu()
    with pytest.raises(ValueError, match='page-locked'):
        kernels.index_copy(dev(numpy.ones(4)), t.zeros(4, dtype=t.float64))


# ---- nh_pointwise_poly ------------------------------------------------------------------------------------------------------------

def poly_powers(rng, nterms, nvars):
    '''per term one variable with a power up to 31 (31 itself in every third term), the others up to 3; term 5 is the constant'''
    powers = rng.integers(0, 4, (nterms, nvars))
    for t in range(nterms if nvars else 0):
        powers[t, t % nvars] = 31 if t % 3 == 0 else rng.integers(0, 32)
    if nterms > 5:
        powers[5] = 0
    return powers


@pytest.mark.parametrize('nvars', range(5))
def test_pointwise_poly(nvars, nan_empty):
    '''0 to 4 variables, 0, 1 and 32 terms, powers 0..31, contiguous variables and the stride 1 + nd of the (value, gradient) arrays sample.py passes'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(400 + nvars)
    for nterms in 0, 1, 32:
        powers = poly_powers(rng, nterms, nvars)
        assert nterms < 32 or not nvars or (powers.max() == 31 and powers.min() == 0)
        for n, stride in (1, 1), (255, 4), (257, 1), (257, 3):
            for exact in True, False:
                if exact:  # |x| <= 2, total degree <= 31 + 9, |coefficient| <= 4: a term is below 2^42, 32 of them below 2^47
                    xs, coeffs = [ints(rng, -1, 2, n * stride) for v in range(nvars)], ints(rng, -4, 4, nterms)
                else:
                    xs, coeffs = [rng.uniform(-1.5, 1.5, n * stride) for v in range(nvars)], rng.standard_normal(nterms)
                got = host(kernels.pointwise_poly([dev(x) for x in xs], [stride] * nvars, coeffs, powers, n))
                value, mag = refs.pointwise_poly(xs, [stride] * nvars, coeffs, powers, n)
                what = f'nterms={nterms} n={n} stride={stride}'
                if exact:
                    equal(got, value, what)
                else:
                    # k = the largest total degree: a term is its coefficient times x_v, powers[t][v] times over;  m = nterms
                    within(got, value, mag, int(powers.sum(1).max()) if nterms else 0, nterms, what)


def test_pointwise_poly_rejections():
    from nutils_amd import _lib, kernels
    x = dev(numpy.ones(4))
    with pytest.raises(_lib.NutilsHipError, match='at most 4 variables and 32 terms'):
        kernels.pointwise_poly([x] * 5, [1] * 5, [1.], [[1] * 5], 4)
    with pytest.raises(_lib.NutilsHipError, match='at most 4 variables and 32 terms'):
        kernels.pointwise_poly([x], [1], [1.] * 33, [[1]] * 33, 4)
    with pytest.raises(_lib.NutilsHipError, match='power out of range'):
        kernels.pointwise_poly([x, x], [1, 1], [1., 1.], [[1, 1], [0, 32]], 4)
    with pytest.raises(_lib.NutilsHipError, match='NULL variable 1'):
        kernels.pointwise_poly([x, Null], [1, 1], [1.], [[1, 1]], 4)


# ---- nh_point_forms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('scaled', [False, True], ids=['', 'scale'])
@pytest.mark.parametrize('S', [2, 3, 4])
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_point_forms(kind, S, scaled, nan_empty):
    '''B is a full matrix without symmetry, so kind 1 (which contracts its second index) and kind 2 (its first) tell a transposed index; the result buffer
    holds NaN before, and kind 1 must have written exact zeros beside its value column'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(500 + 10 * kind + S)
    n = 257
    for exact in True, False:
        if exact:  # |term| <= 2 * 3 * 8 * 2 * 2, at most 16 of them
            Ut, Ur, B, L, scale = ints(rng, -2, 2, (n, S)), ints(rng, -2, 2, (n, S)), ints(rng, -8, 8, (S, S)), ints(rng, -3, 3, S), ints(rng, -2, 2, n)
            B[0, 1], B[1, 0] = 5, -6
        else:
            Ut, Ur, B, L, scale = rng.standard_normal((n, S)), rng.standard_normal((n, S)), rng.standard_normal((S, S)), rng.standard_normal(S), rng.standard_normal(n)
        if not scaled:
            scale = None
        got = host(kernels.point_forms(kind, dev(Ut), B, Ur=dev(Ur) if kind == 0 else None, L=L if kind == 2 else None, scale=None if scale is None else dev(scale)))
        value, mag = refs.point_forms(kind, Ut, B, Ur=Ur, L=L, scale=scale)
        if exact:
            equal(got, value)
        elif kind == 0:
            within(got, value, mag, 3, S * S)  # k = 3: B[a][b] * ur[b], ut[a] * (..), sc * (..);  m = S^2
        elif kind == 1:
            within(got, value, mag, 2, S)  # k = 2: B[a][x] * ut[x], sc * (..);  m = S
        else:
            within(got, value, mag, 3, S)  # k = 3: B[x][b] * ut[x], sc * L[a], (..) * t[b];  m = S
        if kind == 1:
            assert numpy.array_equal(got.reshape(n, S, S)[:, :, 1:], numpy.zeros((n, S, S - 1)))


def test_point_forms_rejections():
    from nutils_amd import _lib, kernels
    for S in 1, 5:
        with pytest.raises(_lib.NutilsHipError, match='nh_point_forms: invalid argument'):
            kernels.point_forms(1, dev(numpy.ones((4, S))), numpy.ones((S, S)))
    U3 = dev(numpy.ones((4, 3)))
    with pytest.raises(_lib.NutilsHipError, match='nh_point_forms: invalid argument'):
        kernels.point_forms(3, U3, numpy.ones((3, 3)))
    with pytest.raises(_lib.NutilsHipError, match='kind 0 needs both fields'):
        kernels.point_forms(0, U3, numpy.ones((3, 3)))
    with pytest.raises(_lib.NutilsHipError, match='kind 2 needs L'):
        kernels.point_forms(2, U3, numpy.ones((3, 3)))


# ---- nh_point_expr ----------------------------------------------------------------------------------------------------------------

OUT_INDEX = {1: [0] * 9, 5: [0, 0, 1, 3, 3, 0, 4, 1, 1]}  # of 5 outputs, 0 and 1 come in two separate runs and nothing names 2


@pytest.mark.parametrize('nout', [1, 5])
@pytest.mark.parametrize('nvars', range(7))
def test_point_expr(nvars, nout, nan_empty):
    '''0 to 6 factors of 1 to 3 slots per point, the last of two or more (and the only one, second time round) a constant table at stride 0; with and without
    scale; stored into a fresh result (NaN before: outputs without an entry must come back 0) and accumulated onto a filled one (they must stay)'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(600 + 10 * nvars + nout)
    oidx = numpy.array(OUT_INDEX[nout])
    named = numpy.isin(numpy.arange(nout), oidx)
    for n in 1, 257:
        for broadcast_last in (False, True) if nvars == 1 else (nvars >= 2,):
            slots = [1 + v % 3 for v in range(nvars)]
            strides = [0 if broadcast_last and v == nvars - 1 else slots[v] for v in range(nvars)]
            off = numpy.stack([rng.integers(0, s, len(oidx)) for s in slots], 1) if nvars else numpy.zeros((len(oidx), 0), dtype=int)
            for exact in True, False:
                sizes = [max(n * st, sl) for st, sl in zip(strides, slots)]
                if exact:  # |term| <= 2 * 8 * 2^6 = 2^10, at most 9 of them and the content before
                    xs, coef, scale, prev = [ints(rng, -2, 2, m) for m in sizes], ints(rng, -8, 8, len(oidx)), ints(rng, -2, 2, n), ints(rng, -8, 8, n * nout)
                else:
                    xs, coef, scale, prev = [rng.uniform(-2, 2, m) for m in sizes], rng.standard_normal(len(oidx)), rng.standard_normal(n), rng.standard_normal(n * nout)
                tables = dev(oidx, 'int32'), dev(off.reshape(-1), 'int32'), dev(coef)
                for sc in None, scale:
                    for out in None, prev:
                        out_dev = None if out is None else dev(out)
                        got = host(kernels.point_expr([dev(x) for x in xs], strides, *tables, n, nout, scale=None if sc is None else dev(sc), out=out_dev))
                        value, mag = refs.point_expr(xs, strides, oidx, off, coef, n, nout, scale=sc, out=out)
                        what = f'n={n} strides={strides} scale={sc is not None} accumulate={out is not None}'
                        if exact:
                            equal(got, value, what)
                        else:
                            # k = nvars + 1: coef[t] times one value of every factor, then sc * (the sum of a run);  m = the entries of the output and
                            # what it held before (0 on a fresh call)
                            within(got, value, mag, nvars + 1, numpy.tile(numpy.bincount(oidx, minlength=nout) + 1, n), what)
                        rest = got.reshape(n, nout)[:, ~named]
                        assert numpy.array_equal(rest, 0 * rest if out is None else out.reshape(n, nout)[:, ~named]), what


def test_point_expr_without_entries(nan_empty):
    from nutils_amd import kernels
    empty = dev([], 'int32'), dev([], 'int32'), dev([])
    x, prev = dev(numpy.ones(6)), numpy.arange(9.) - 4
    for n in 1, 3:
        assert numpy.array_equal(host(kernels.point_expr([x], [2], *empty, n, 3)), numpy.zeros(3 * n))
        assert numpy.array_equal(host(kernels.point_expr([x], [2], *empty, n, 3, out=dev(prev[:3 * n]))), prev[:3 * n])


def test_point_expr_rejections():
    from nutils_amd import _lib, kernels
    x = dev(numpy.ones(4))
    tables = dev([0], 'int32'), dev([0] * 7, 'int32'), dev([1.])
    with pytest.raises(_lib.NutilsHipError, match='at most 6 factors'):
        kernels.point_expr([x] * 7, [1] * 7, *tables, 4, 1)
    with pytest.raises(_lib.NutilsHipError, match='nh_point_expr: invalid argument'):
        kernels.point_expr([x], [1], *tables, 4, 0, out=x)


# ---- nh_rationalize ---------------------------------------------------------------------------------------------------------------

NELEMS, NQ = 45, 3  # 135 (element, point) pairs: one workgroup of 128 and 7 threads of a second


def rational_case(rng, ndims, ragged, exact, given):
    '''tables, dofs (20 of them, shared among the elements) and weights of 45 elements with 1, 2, .., 7, 1, .. functions (ragged) or 5 each'''
    sizes = numpy.array([1 + e % 7 for e in range(NELEMS)] if ragged else [5] * NELEMS)
    off = numpy.concatenate([[0], numpy.cumsum(sizes)])
    nfn, S = off[-1], 1 + ndims
    dofs = rng.integers(0, 20, nfn)
    if exact:  # dyadic: 1 / W, w / W, (w / W) B, B dW / W and the difference are all exact
        T, weights = ints(rng, -8, 8, (nfn, NQ, S)), rng.choice([.5, 1., 2., 3.], 20)
        W, dW = rng.choice([.25, .5, 1., 2., 4.], (NELEMS, NQ)), ints(rng, -4, 4, (NELEMS, NQ, ndims))
    else:  # positive weights and values, as B-splines have them; gradients of either sign
        T, weights = rng.standard_normal((nfn, NQ, S)), rng.uniform(.5, 2., 20)
        T[:, :, 0] = rng.uniform(.1, 1., (nfn, NQ))
        W, dW = rng.uniform(.5, 2., (NELEMS, NQ)), rng.standard_normal((NELEMS, NQ, ndims))
    return sizes, off, dofs, T, weights, (W, dW) if given else (None, None)


def run_rationalize(ndims, ragged, sizes, off, dofs, T, weights, W, dW):
    from nutils_amd import kernels
    T_dev = dev(T.reshape(-1))
    kernels.rationalize(T_dev, NELEMS, 0 if ragged else int(sizes[0]), dev(dofs, 'int32'), dev(weights), NQ, ndims, W=None if W is None else dev(W.reshape(-1)),
                        dW=None if dW is None else dev(dW.reshape(-1)), off=dev(off, 'int64') if ragged else None)
    return host(T_dev)


@pytest.mark.parametrize('ragged', [False, True], ids=['uniform', 'ragged'])
@pytest.mark.parametrize('ndims', [1, 2, 3])
def test_rationalize_with_the_weight_function_given(ndims, ragged):
    rng = numpy.random.default_rng(700 + 10 * ndims + ragged)
    for exact in True, False:
        sizes, off, dofs, T, weights, (W, dW) = rational_case(rng, ndims, ragged, exact, True)
        got = run_rationalize(ndims, ragged, sizes, off, dofs, T, weights, W, dW).reshape(-1, NQ, 1 + ndims)
        value, mag = (a.reshape(got.shape) for a in refs.rationalize(T, NELEMS, 0 if ragged else 5, dofs, weights, NQ, ndims, W=W, dW=dW, off=off if ragged else None))
        if exact:
            equal(got, value)
        else:
            # N = ((w * r) * B), r = 1 / W:  k = 3 (the quotient, w * r, the product), m = 1
            within(got[:, :, 0], value[:, :, 0], mag[:, :, 0], 3, 1)
            # dN = (w * r) * (dB - (B * dW) * r): two terms; the longer one passes B * dW, * r, the difference, w * r and the last product, and holds the
            # rounded r twice:  k = 7, m = 2
            within(got[:, :, 1:], value[:, :, 1:], mag[:, :, 1:], 7, 2)


@pytest.mark.parametrize('ragged', [False, True], ids=['uniform', 'ragged'])
@pytest.mark.parametrize('ndims', [1, 2, 3])
def test_rationalize_with_the_weight_function_summed(ndims, ragged):
    '''W = sum_j w_j B_j and dW = sum_j w_j dB_j over the n functions of the element are computed quantities: W carries a relative error of n u c,
    c = sum |w_j B_j| / |W| (1 here: all positive), dW_k an absolute one of n u A_k, A_k = sum |w_j dB_jk|.  The reference's magnitude is built from c and A_k
    (pointwise_refs.rationalize), and the counts below follow every place these errors enter.  The quotient keeps this path from an exact-input test; the
    partition of unity is its second, independent check: per point the values sum to 1 and every gradient component to 0, within the sum of the bounds.'''
    rng = numpy.random.default_rng(750 + 10 * ndims + ragged)
    sizes, off, dofs, T, weights, _ = rational_case(rng, ndims, ragged, False, False)
    got = run_rationalize(ndims, ragged, sizes, off, dofs, T, weights, None, None).reshape(-1, NQ, 1 + ndims)
    value, mag = (a.reshape(got.shape) for a in refs.rationalize(T, NELEMS, 0 if ragged else 5, dofs, weights, NQ, ndims, off=off if ragged else None))
    n = numpy.repeat(sizes, sizes)[:, None, None]  # the number of functions of the element a function belongs to
    # N = (w * r) * B, r = 1 / W:  k = 3 as above;  m = n, the summands of W, whose error N inherits
    within(got[:, :, :1], value[:, :, :1], mag[:, :, :1], 3, n + 0 * mag[:, :, :1])
    # dN = (w * r) * (dB - (B * dW) * r):  k = 7 as above;  m = 3 n: the n summands of W where the first term holds r once and twice more where the second holds
    # it twice (weighed 2 n c |w B dW / W^2| <= 2 n c |w B / W^2| A_k), and the n summands of dW_k (n |w B / W^2| A_k)
    within(got[:, :, 1:], value[:, :, 1:], mag[:, :, 1:], 7, 3 * n + 0 * mag[:, :, 1:])
    bound = numpy.concatenate([(3 + n + 1) * mag[:, :, :1], (7 + 3 * n + 1) * mag[:, :, 1:]], 2) * U * LD('1.01')
    total = numpy.add.reduceat(got.astype(LD), off[:-1], axis=0)  # per element, point and slot the sum over the element's functions
    limit = numpy.add.reduceat(bound, off[:-1], axis=0)
    assert total.shape == (NELEMS, NQ, 1 + ndims)
    assert (numpy.abs(total[:, :, 0] - 1) <= limit[:, :, 0]).all()
    assert (numpy.abs(total[:, :, 1:]) <= limit[:, :, 1:]).all()


def test_rationalize_rejections():
    from nutils_amd import _lib, kernels
    T, dofs, w, off = dev(numpy.ones(8)), dev(numpy.zeros(4), 'int32'), dev(numpy.ones(1)), dev([0, 2, 4], 'int64')
    with pytest.raises(_lib.NutilsHipError, match='give either nb or off_dev'):
        kernels.rationalize(T, 2, 2, dofs, w, 1, 1, off=off)
    with pytest.raises(_lib.NutilsHipError, match='give either nb or off_dev'):
        kernels.rationalize(T, 2, 0, dofs, w, 1, 1)
    with pytest.raises(_lib.NutilsHipError, match='W_dev without dW_dev'):
        kernels.rationalize(T, 2, 2, dofs, w, 1, 1, W=dev(numpy.ones(2)))
    assert numpy.array_equal(host(T), numpy.ones(8))


# ---- nh_structured_dofs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape, nloc, ndofs, windows', [
    ((2,), (3,), (2,), [(0, 2), (1, 1)]),  # a periodic axis of 2 elements and 2 dofs under 3 local functions: % ndofs wraps and a dof repeats inside an element
    ((301,), (4,), (301,), [(0, 301), (7, 290)]),  # periodic, more than a workgroup: the last three elements wrap
    ((37, 2), (3, 3), (39, 2), [(0, 74), (5, 40)]),  # the second axis periodic as in the first case
    ((5, 2, 7), (2, 3, 2), (6, 2, 8), [(0, 70), (3, 50)]),  # .. and the middle one of three
], ids=['1d-tiny', '1d', '2d', '3d'])
def test_structured_dofs(shape, nloc, ndofs, windows):
    '''an integer kernel: equality with the integer reference is the exact-input test and the real-input one at once (k = m = 0: nothing rounds).  Windows
    (elem_begin, nelems): the whole mesh, and one that starts past element 0 and ends before the last; and no element at all.'''
    from nutils_amd import kernels
    start = numpy.concatenate([numpy.arange(n) for n in shape])
    start_dev = dev(start, 'int32')
    for elem_begin, nelems in windows + [(windows[1][0], 0)]:
        assert elem_begin + nelems <= numpy.prod(shape)
        got = host(kernels.structured_dofs(shape, nloc, ndofs, start_dev, elem_begin, nelems))
        want = refs.structured_dofs(shape, nloc, ndofs, start, elem_begin, nelems)
        assert got.dtype == numpy.int32
        equal(got, want, f'elements {elem_begin}..{elem_begin + nelems}')
        if 2 in ndofs:  # three local functions over two dofs: a dof repeats inside every element
            assert all(len(set(row)) < len(row) for row in want.tolist())
