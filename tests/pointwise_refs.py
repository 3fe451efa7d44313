'''Plain restatements of the pointwise, gather and scatter helper kernels (nh_monomial.hip; nh_rationalize and nh_structured_dofs of nh_runtime.hip), each
straight from the formula in the kernel's header comment, in numpy.longdouble -- or in Python integers for the two index kernels.  No GPU, no library.

Every floating-point function returns (value, magnitude): per output the value and the sum of the absolute values of the terms that enter it, an initial
content of the output counted as one term.  The bounds of tests/test_gpu_pointwise.py are multiples of that magnitude.  (`rationalize` weighs its magnitude
with the condition of the weight sum, see there.)  tests/test_pointwise_refs_host.py pins all of this against exact rational arithmetic.'''
import numpy

LD = numpy.longdouble


def _ld(a):
    return numpy.array(a, dtype=LD)


def monomial(values, args, indices, out, out_index=None, alpha=1.):
    '''out[out_index[i]] += alpha values[i] prod_k args[k][indices[k][i]];  out_index None: everything into out[0].'''
    term = LD(alpha) * _ld(values)
    for arg, index in zip(args, indices):
        term = term * _ld(arg)[numpy.asarray(index, dtype=numpy.int64)]
    where = numpy.zeros(len(term), dtype=numpy.int64) if out_index is None else numpy.asarray(out_index, dtype=numpy.int64)
    value, mag = _ld(out).copy(), numpy.abs(_ld(out))
    numpy.add.at(value, where, term)
    numpy.add.at(mag, where, numpy.abs(term))
    return value, mag


def monomial_csr(rowptr, colidx, values, x, y, alpha=1.):
    '''y[r] += alpha sum_{rowptr[r] <= k < rowptr[r+1]} values[k] x[colidx[k]]'''
    values, x = _ld(values), _ld(x)
    value, mag = _ld(y).copy(), numpy.abs(_ld(y))
    for r in range(len(rowptr) - 1):
        for k in range(int(rowptr[r]), int(rowptr[r + 1])):
            term = LD(alpha) * values[k] * x[int(colidx[k])]
            value[r] += term
            mag[r] += abs(term)
    return value, mag


def index_copy(src, dst, src_index=None, dst_index=None):
    '''dst[dst_index[i]] = src[src_index[i]], a missing index array standing for i; every other position of dst keeps its content.  Plain stores: the positions
    that dst_index names must be distinct for the result to be defined.  Returns the new dst.'''
    n = len(src_index) if src_index is not None else len(dst_index) if dst_index is not None else len(src)
    s = numpy.arange(n) if src_index is None else numpy.asarray(src_index, dtype=numpy.int64)
    d = numpy.arange(n) if dst_index is None else numpy.asarray(dst_index, dtype=numpy.int64)
    assert len(s) == len(d) == n and len(numpy.unique(d)) == n
    new = numpy.array(dst)
    new[d] = numpy.asarray(src)[s]
    return new


def pointwise_poly(xs, strides, coeffs, powers, n):
    '''out[i] = sum_t coeffs[t] prod_v xs[v][i strides[v]]^powers[t][v]'''
    at = [_ld(x)[numpy.arange(n) * int(s)] for x, s in zip(xs, strides)]
    value, mag = numpy.zeros(n, dtype=LD), numpy.zeros(n, dtype=LD)
    for c, row in zip(coeffs, powers):
        term = numpy.full(n, c, dtype=LD)
        for xv, p in zip(at, row):
            for _ in range(int(p)):
                term = term * xv
        value += term
        mag += numpy.abs(term)
    return value, mag


def point_forms(kind, Ut, B, Ur=None, L=None, scale=None):
    '''kind 0: out[i]       = sc_i sum_ab B[a][b] Ut[i][a] Ur[i][b]
    kind 1: out[i][a][b] = sc_i (b == 0 ? sum_x B[a][x] Ut[i][x] : 0)
    kind 2: out[i][a][b] = sc_i L[a] sum_x B[x][b] Ut[i][x]
    sc_i = scale[i] or 1'''
    Ut, B = _ld(Ut), _ld(B)
    n, S = Ut.shape
    sc = numpy.ones(n, dtype=LD) if scale is None else _ld(scale)
    value = numpy.zeros((n,) if kind == 0 else (n, S, S), dtype=LD)
    mag = numpy.zeros_like(value)
    if kind == 0:
        Ur = _ld(Ur)
        for a in range(S):
            for b in range(S):
                term = sc * B[a, b] * Ut[:, a] * Ur[:, b]
                value += term
                mag += numpy.abs(term)
    elif kind == 1:
        for a in range(S):
            for x in range(S):
                term = sc * B[a, x] * Ut[:, x]
                value[:, a, 0] += term
                mag[:, a, 0] += numpy.abs(term)
    elif kind == 2:
        L = _ld(L)
        for a in range(S):
            for b in range(S):
                for x in range(S):
                    term = sc * L[a] * B[x, b] * Ut[:, x]
                    value[:, a, b] += term
                    mag[:, a, b] += numpy.abs(term)
    else:
        raise ValueError(kind)
    return value, mag


def point_expr(xs, strides, out_index, offsets, coef, n, nout, scale=None, out=None):
    '''out[i][f] (+)= sc_i sum_{t: out_index[t] == f} coef[t] prod_v xs[v][i strides[v] + offsets[t][v]];  without `out` the sum starts from 0.'''
    xs = [_ld(x) for x in xs]
    sc = numpy.ones(n, dtype=LD) if scale is None else _ld(scale)
    value = numpy.zeros((n, nout), dtype=LD) if out is None else _ld(out).reshape(n, nout).copy()
    mag = numpy.abs(value)
    point = numpy.arange(n)
    for t in range(len(coef)):
        term = sc * LD(coef[t])
        for v, x in enumerate(xs):
            term = term * x[point * int(strides[v]) + int(offsets[t][v])]
        value[:, int(out_index[t])] += term
        mag[:, int(out_index[t])] += numpy.abs(term)
    return value, mag


def rationalize(T, nelems, nb, dofs, weights, nq, ndims, W=None, dW=None, off=None):
    '''T[(e, i)][q][1 + ndims] = (B, dB) of function (e, i) = e nb + i (or off[e] + i) at point q becomes (N, dN),
        N = w B / W,   dN_k = w dB_k / W - w B dW_k / W^2,   w = weights[dofs[(e, i)]],
    with W [nelems][nq] and dW [nelems][nq][ndims] given, or W = sum_j w_j B_j, dW_k = sum_j w_j dB_jk over the functions j of the element.

    Magnitudes.  W given: |N|, and |w dB_k / W| + |w B dW_k / W^2|.  W summed: the two sums are computed quantities with errors of their own, relative to
    sum_j |w_j B_j| and A_k = sum_j |w_j dB_jk|, not to |W| and |dW_k|; with c = sum_j |w_j B_j| / |W| >= 1 the magnitudes are c |N| and
    c (|w dB_k / W| + |w B / W^2| A_k), which are the given-W ones when all w_j B_j have one sign and all w_j dB_jk have one sign.'''
    S = 1 + ndims
    T = _ld(T).reshape(-1, nq, S)
    weights = _ld(weights)
    value, mag = numpy.zeros_like(T), numpy.zeros_like(T)
    for e in range(nelems):
        f0, n = (e * nb, nb) if off is None else (int(off[e]), int(off[e + 1]) - int(off[e]))
        w = [weights[int(dofs[f0 + i])] for i in range(n)]
        if W is not None:
            We, dWe = _ld(W).reshape(nelems, nq)[e], _ld(dW).reshape(nelems, nq, ndims)[e]
            c, A = numpy.ones(nq, dtype=LD), numpy.abs(dWe)
        else:
            We, dWe, c, A = numpy.zeros(nq, dtype=LD), numpy.zeros((nq, ndims), dtype=LD), numpy.zeros(nq, dtype=LD), numpy.zeros((nq, ndims), dtype=LD)
            for i in range(n):
                We += w[i] * T[f0 + i, :, 0]
                dWe += w[i] * T[f0 + i, :, 1:]
                c += numpy.abs(w[i] * T[f0 + i, :, 0])
                A += numpy.abs(w[i] * T[f0 + i, :, 1:])
            c = c / numpy.abs(We)
        for i in range(n):
            B, dB = T[f0 + i, :, 0], T[f0 + i, :, 1:]
            value[f0 + i, :, 0] = w[i] * B / We
            mag[f0 + i, :, 0] = c * numpy.abs(w[i] * B / We)
            for k in range(ndims):
                value[f0 + i, :, 1 + k] = w[i] * dB[:, k] / We - w[i] * B * dWe[:, k] / (We * We)
                mag[f0 + i, :, 1 + k] = c * (numpy.abs(w[i] * dB[:, k] / We) + numpy.abs(w[i] * B / (We * We)) * A[:, k])
    return value.reshape(-1), mag.reshape(-1)


def structured_dofs(shape, nloc, ndofs_axis, start_concat, elem_begin, nelems):
    '''dofs[e - elem_begin][l] of the elements elem_begin <= e < elem_begin + nelems of a structured mesh with shape[a] elements along axis a (element and
    local function index: last axis fastest): along every axis the dof (start[a][index of the element] + index of the function) modulo ndofs_axis[a], the
    axes raveled with ndofs_axis.  start_concat holds the start arrays of the axes one after the other.  Python integers throughout.'''
    nd = len(shape)
    starts, pos = [], 0
    for a in range(nd):
        starts.append([int(s) for s in start_concat[pos:pos + shape[a]]])
        pos += shape[a]
    dofs = []
    for e in range(elem_begin, elem_begin + nelems):
        idx, rest = [0] * nd, e
        for a in reversed(range(nd)):
            rest, idx[a] = divmod(rest, shape[a])
        row = []
        for l in range(int(numpy.prod(nloc))):
            loc, rest = [0] * nd, l
            for a in reversed(range(nd)):
                rest, loc[a] = divmod(rest, nloc[a])
            dof = 0
            for a in range(nd):
                dof = dof * ndofs_axis[a] + (starts[a][idx[a]] + loc[a]) % ndofs_axis[a]
            row.append(dof)
        dofs.append(row)
    return numpy.array(dofs, dtype=numpy.int64).reshape(nelems, int(numpy.prod(nloc)))
