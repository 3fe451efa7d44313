'''Plain restatements of the factor-tensor builder (nh_factor_tensor / nh_factor_fetch, nutils_amd/csrc/nh_factor.hip), straight from the formula in its header
comment.  No GPU, no library.

The tensor of rank k of  coeff int s u^k dV:  for every list position ie (element e = elist[ie], or ie without a list) and every local multi-index
(loc_1, .., loc_k), in C order, the moment

    coeff  sum_q  w_q  |det_e,q|  s[ie][q]  prod_a T[tab[e] nb + loc_a][q][0]

is added under the key (dofs[e][loc_1], .., dofs[e][loc_k]).  Keys are sorted lexicographically, sums that are zero are dropped.  T is [functions][nq][S] and only
slot 0 of the last axis (the value; the others hold gradients) is read; without `tab` every element uses the functions 0 .. nb-1.  dofs, tab and the geometry are
indexed by the ELEMENT, scale by the LIST POSITION.

  factor_tensor_exact   Python integers / fractions.Fraction throughout, |det| given
  factor_tensor_ld      numpy.longdouble, |det| (or the surface measure of a face) restated from the formulas of nh_geom.inc; per entry the value and a magnitude
  ordered_run_sums      the float64 sum of each run front to back in list order, the order the kernel promises

tests/test_factor_refs_host.py pins the three against each other and against integrals computed by hand.'''
from fractions import Fraction

import numpy

LD = numpy.longdouble


def _ld(a):
    return numpy.array(a, dtype=LD)


def _rational(a):
    '''an object array of Python integers where a number is integral, Fractions elsewhere (a float converts exactly)'''
    a = numpy.asarray(a)
    out = numpy.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, x in enumerate(a.reshape(-1).tolist()):
        f = x if isinstance(x, (int, Fraction)) else Fraction(x)
        flat[i] = int(f) if f == int(f) else f
    return out


def _local_indices(nb, rank):
    '''[rank][nb^rank]: the local multi-indices in C order'''
    return numpy.indices((nb,) * rank).reshape(rank, -1)


def _moments(w, Te, rank):
    '''sum_q w[q] prod_a Te[loc_a][q] for every local multi-index in C order; any dtype that multiplies and adds'''
    P = w
    for _ in range(rank):
        P = P[..., None, :] * Te
    return P.sum(-1).reshape(-1)


def factor_tensor_exact(*, nelems, nq, rank, weights, absdet, T, dofs, nb, coeff=1, scale=None, elist=None, tab=None, keep_zeros=False):
    '''(values[nnz], indices[rank][nnz]) in exact arithmetic: values an object array of integers / Fractions, indices int64.  absdet [elements][nq]: |det| per
    element and point; scale [nelems][nq] per list position.  keep_zeros: leave the sums that are zero in (to count the distinct keys).'''
    weights, absdet, coeff = _rational(weights).reshape(nq), _rational(absdet).reshape(-1, nq), _rational(coeff).item()
    Tarr = numpy.asarray(T)
    T0 = _rational(Tarr.reshape(Tarr.shape[0], nq, -1)[:, :, 0])
    dofs = numpy.asarray(dofs, dtype=numpy.int64).reshape(-1, nb)
    scale = None if scale is None else _rational(scale).reshape(nelems, nq)
    loc = _local_indices(nb, rank)
    sums = {}
    for ie in range(nelems):
        e = ie if elist is None else int(elist[ie])
        w = coeff * weights * absdet[e]
        if scale is not None:
            w = w * scale[ie]
        f0 = 0 if tab is None else int(tab[e]) * nb
        moments = _moments(w, T0[f0:f0 + nb], rank)
        for key, m in zip(zip(*dofs[e][loc].tolist()), moments.tolist()):
            sums[key] = sums.get(key, 0) + m
    keys = sorted(k for k, v in sums.items() if keep_zeros or v != 0)
    values = numpy.empty(len(keys), dtype=object)
    values[:] = [sums[k] for k in keys]
    return values, numpy.array(keys, dtype=numpy.int64).reshape(len(keys), rank).T.copy()


def measure_ld(geom, ndims, nq, e):
    '''(m[nq], c[nq]) of element e in longdouble: m = |det J|, or for bnd_axis = j >= 0 the surface measure |det J| |row j of J^-1| of the face xi_j = const, with
    J^-1 = adj J / det J as nh_geom.inc forms it;  c >= 1 the condition of that computation, the factor by which cancellation magnifies the rounding errors:
    (sum of the |terms| of the expanded determinant) / |det|, times -- for a face -- the same for the row norm, sum_i |C_i| A_i / sum_i C_i^2 with C_i the cofactors
    of the row and A_i the sums of their |terms|.

    geom: dict(kind='box', size[elements][ndims]) -- J = diag(size);  dict(kind='tab', jac[elements][nq][ndims][ndims]) -- J given;
    dict(kind='iso', gT[ngb][nq][1 + ndims], gdofs[elements][ngb], verts[.][ndims]) -- J[i][j] = sum_a verts[gdofs[e][a]][i] gT[a][q][1 + j];  bnd_axis optional.'''
    nd = ndims
    kind = geom['kind']
    if kind == 'box':
        size = _ld(geom['size']).reshape(-1, nd)[e]
        J = numpy.zeros((nq, nd, nd), dtype=LD)
        for i in range(nd):
            J[:, i, i] = size[i]
        A = numpy.abs(J)
    elif kind == 'tab':
        J = _ld(geom['jac']).reshape(-1, nq, nd, nd)[e]
        A = numpy.abs(J)
    elif kind == 'iso':
        gT = _ld(geom['gT']).reshape(-1, nq, 1 + nd)
        X = _ld(geom['verts']).reshape(-1, nd)[numpy.asarray(geom['gdofs']).reshape(-1, len(gT))[e]]  # [ngb][nd]
        J, A = numpy.zeros((nq, nd, nd), dtype=LD), numpy.zeros((nq, nd, nd), dtype=LD)
        for a in range(len(gT)):
            for i in range(nd):
                for j in range(nd):
                    term = X[a, i] * gT[a, :, 1 + j]
                    J[:, i, j] += term
                    A[:, i, j] += numpy.abs(term)
    else:
        raise ValueError(kind)

    def cofactor(M, i, j, absolute):
        '''signed cofactor of entry (i, j); absolute: the sum of the |terms| instead'''
        if nd == 1:
            return numpy.ones(nq, dtype=LD)
        if nd == 2:
            return M[:, 1 - i, 1 - j] * (1 if absolute or i == j else -1)
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return M[:, i1, j1] * M[:, i2, j2] + (1 if absolute else -1) * M[:, i1, j2] * M[:, i2, j1]

    det = sum(J[:, 0, j] * cofactor(J, 0, j, False) for j in range(nd))
    adet = sum(A[:, 0, j] * cofactor(A, 0, j, True) for j in range(nd))
    m, c = numpy.abs(det), adet / numpy.abs(det)
    axis = geom.get('bnd_axis', -1)
    if axis >= 0:  # row `axis` of J^-1: the cofactors of column `axis` of J over det
        C = [cofactor(J, i, axis, False) for i in range(nd)]
        AC = [cofactor(A, i, axis, True) for i in range(nd)]
        s2 = sum((Ci / det) ** 2 for Ci in C)
        m = m * numpy.sqrt(s2)
        c = c * sum(numpy.abs(Ci) * Ai for Ci, Ai in zip(C, AC)) / sum(Ci * Ci for Ci in C)
    return m, c


def factor_tensor_ld(*, nelems, ndims, nq, rank, weights, geom, T, dofs, nb, coeff=1., scale=None, elist=None, tab=None, keep_zeros=False):
    '''(value[nnz], magnitude[nnz], indices[rank][nnz], count[nnz]) in longdouble.  magnitude: the sum of the absolute values of the terms
    coeff w_q |det| s prod T  of the entry, each weighted by the condition c of its point's measure (measure_ld); count: the number of moments (list position, local
    multi-index) that the entry sums, the length of its run in the sorted keys.'''
    weights, coeff = _ld(weights).reshape(nq), LD(coeff)
    Tarr = numpy.asarray(T)
    T0 = _ld(Tarr.reshape(Tarr.shape[0], nq, -1)[:, :, 0])
    dofs = numpy.asarray(dofs, dtype=numpy.int64).reshape(-1, nb)
    scale = None if scale is None else _ld(scale).reshape(nelems, nq)
    loc = _local_indices(nb, rank)
    keys, vals, mags, measures = [], [], [], {}
    for ie in range(nelems):
        e = ie if elist is None else int(elist[ie])
        if e not in measures:
            measures[e] = measure_ld(geom, ndims, nq, e)
        m, c = measures[e]
        w = coeff * weights * m
        if scale is not None:
            w = w * scale[ie]
        f0 = 0 if tab is None else int(tab[e]) * nb
        vals.append(_moments(w, T0[f0:f0 + nb], rank))
        mags.append(_moments(numpy.abs(w) * c, numpy.abs(T0[f0:f0 + nb]), rank))
        keys.append(dofs[e][loc].T)
    if not keys:
        return numpy.zeros(0, dtype=LD), numpy.zeros(0, dtype=LD), numpy.zeros((rank, 0), dtype=numpy.int64), numpy.zeros(0, dtype=numpy.int64)
    uniq, inverse = numpy.unique(numpy.concatenate(keys), axis=0, return_inverse=True)  # rows in lexicographic order
    inverse = inverse.reshape(-1)
    value, mag = numpy.zeros(len(uniq), dtype=LD), numpy.zeros(len(uniq), dtype=LD)
    numpy.add.at(value, inverse, numpy.concatenate(vals))
    numpy.add.at(mag, inverse, numpy.concatenate(mags))
    count = numpy.bincount(inverse, minlength=len(uniq))
    keep = numpy.ones(len(uniq), dtype=bool) if keep_zeros else value != 0
    return value[keep], mag[keep], uniq[keep].T.copy(), count[keep]


def ordered_run_sums(keys, contributions):
    '''(values[nnz] float64, indices[rank][nnz]): contributions[i] (exactly representable float64 numbers) is added under keys[i] ([n][rank]); each key's
    contributions are summed FRONT TO BACK in the order of the list, the first one taken as it is, with float64 scalar additions; keys sorted lexicographically,
    sums that are zero dropped.'''
    keys = numpy.asarray(keys, dtype=numpy.int64)
    rank = keys.shape[1]
    sums = {}
    for key, c in zip(map(tuple, keys.tolist()), numpy.asarray(contributions, dtype=numpy.float64)):
        sums[key] = sums[key] + c if key in sums else c
    kept = sorted(k for k, v in sums.items() if v != 0)
    return numpy.array([sums[k] for k in kept], dtype=numpy.float64), numpy.array(kept, dtype=numpy.int64).reshape(len(kept), rank).T.copy()
