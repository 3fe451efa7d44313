'''Plain restatements of the term-list assembly entries (nh_assemble_terms, nh_assemble_terms_multi, nh_assemble_matrix_terms; nutils_amd/csrc/nh_assemble_batched.hip),
written from the comments of nh_terms_args / nh_matrix_terms_args in include/nutils_hip.h.  No GPU, no library: numpy.longdouble on the host.

Geometry at point q of element e (nh_geometry):   J[i][j] = d x_i / d xi_j
    BOX  J = diag(size[e]);   TAB  J = jac[e][q];   ISO  J[i][j] = sum_a verts[gdofs[e][a]][i] gT[a][q][1 + j]
    Jinv = adj J / det J,  measure = |det J|,  and for bnd_axis = a >= 0 the surface measure |det J| |row a of Jinv|.
Physical tables of a basis:   D[q,m,0] = T[m][q][0],   D[q,m,1+i] = sum_j T[m][q][1+j] Jinv[j][i]      (first function of element e: off[e], or tab[e] nb, or 0)
Field values:                 U_f[q,d,b] = sum_n D_f[q,n,b] u_f[dofs_f[e][n]][d]
Pointwise polynomial k:       P_k(q) = sum_t coeffs[t] prod_v x_v^powers[t][v],   x_v = U_{field[v]}[q, comp[v], 0]
Point factor of a term:       s(q) = sum_ab B[a][b] U_t[q,0,a] U_r[q,0,b]
Factor of term t:             g_t(q) = scale_t[ie][q] P_{poly(t)}(q) s_t(q)      (each optional; scale is indexed by the LIST POSITION ie, everything else by the element e =
                              elist[ie]; the matrix entry with NH_MATRIX_EMAP_BY_ELEMENT indexes scale, like emap, by the element -- as nh_assemble_matrix does)
Linear forms:    r_blk[(m,c)] += sum_q w_q measure sum_a Dt_blk[q,m,a] sum_t g_t(q) F_t[q,c,a],    F_t[q,c,a] = f_t[c][a] + sum_db C_t[c,a,d,b] U_{field(t)}[q,d,b]
Bilinear forms:  A[(m,c),(n,d)] += sum_q w_q measure sum_ab Dt[q,m,a] Cq[q][c,a,d,b] Dr[q,n,b],   Cq = sum_t g_t(q) C_t(q),  only where mask[c][d]
    kind 0: C_t = C;   kind 1 (scalar): C_t[a][0] += sum_b B[a][b] U[q][b];   kind 2 (scalar): C_t[a][b] += L[a] sum_x B[x][b] U[q][x]

Every function returns a VALUE and a MAGNITUDE per entry.  The magnitude is the same chain of sums with every factor replaced by its absolute value.  The entries
of J come with A >= |J|, the sums of the |terms| that form them (ISO: sum_a |verts| |gT|; BOX, TAB: |J|); the cofactor products of Jinv and det are summed in absolute
value with one factor of every product taken from A (acof, adet: what the roundings of the products and of the entries can move them by), and the quotient
cofactor / det carries both:
    |measure| -> adet,   |Jinv[j][i]| -> acof(i,j) / |det| + |cof(i,j)| adet / det^2,   face factor -> sqrt(sum_i aJinv[a][i]^2)
so that  m u magnitude  bounds the rounding error of ANY evaluation of the formulas with m roundings along its longest chain, cancellation included (the condition-
weighted magnitude of tests/factor_refs.py).  `mutant` injects one deliberate mistake (tests/test_terms_refs_host.py shows that each is far outside the bound).'''
import numpy

LD = numpy.longdouble
MUTANTS = ('kinds_swapped', 'scale_by_element', 'jinv_transposed', 'no_det', 'no_face', 'power_off_by_one', 'qs_swapped', 'mask_ignored')
CHUNK = 4096  # list positions evaluated at once


def _ld(a):
    return numpy.array(a, dtype=LD)


def gamma(m):
    '''gamma_m = m u / (1 - m u), u = 2^-53'''
    u = LD(2) ** -53
    return m * u / (1 - m * u)


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------

def _cofactor(J, i, j, nd):
    '''cofactor of entry (i, j) of the stack J[..., nd, nd]'''
    if nd == 1:
        return numpy.ones(J.shape[:-2], dtype=LD)
    if nd == 2:
        return J[..., 1 - i, 1 - j] * (1 if i == j else -1)
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return J[..., i1, j1] * J[..., i2, j2] - J[..., i1, j2] * J[..., i2, j1]


def _cofactor_magnitude(J, A, i, j, nd):
    '''its magnitude: every product |a| |b| of two entries replaced by |a| A_b + A_a |b| (>= 2 |a b|: the roundings of the product and those its factors bring along)'''
    if nd == 1:
        return numpy.ones(J.shape[:-2], dtype=LD)
    if nd == 2:
        return A[..., 1 - i, 1 - j]
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    J = numpy.abs(J)
    return J[..., i1, j1] * A[..., i2, j2] + A[..., i1, j1] * J[..., i2, j2] + J[..., i1, j2] * A[..., i2, j1] + A[..., i1, j2] * J[..., i2, j1]


def jacobians(geom, nd, nq, elems):
    '''(J, A) [n][nq][nd][nd] in longdouble: the Jacobian and the sums of the |terms| that form its entries'''
    kind = geom['kind']
    n = len(elems)
    if kind == 'box':
        size = _ld(geom['size']).reshape(-1, nd)[elems]
        J = numpy.zeros((n, nq, nd, nd), dtype=LD)
        for i in range(nd):
            J[:, :, i, i] = size[:, None, i]
        return J, numpy.abs(J)
    if kind == 'tab':
        J = _ld(geom['jac']).reshape(-1, nq, nd, nd)[elems]
        return J, numpy.abs(J)
    if kind == 'iso':
        gT = _ld(geom['gT']).reshape(-1, nq, 1 + nd)
        X = _ld(geom['verts']).reshape(-1, nd)[numpy.asarray(geom['gdofs']).reshape(-1, len(gT))[elems]]  # [n][ngb][nd]
        J = numpy.einsum('eai,aqj->eqij', X, gT[:, :, 1:])
        A = numpy.einsum('eai,aqj->eqij', numpy.abs(X), numpy.abs(gT[:, :, 1:]))
        return J, A
    raise ValueError(kind)


def geometry(geom, nd, nq, elems, absolute=False, mutant=None):
    '''(Jinv [n][nq][nd][nd] indexed [j][i] = d xi_j / d x_i, measure [n][nq]); absolute: their magnitudes'''
    J, A = jacobians(geom, nd, nq, elems)
    det = sum(J[..., 0, j] * _cofactor(J, 0, j, nd) for j in range(nd))
    if nd == 1:
        adet = A[..., 0, 0]
    else:
        adet = sum(numpy.abs(J[..., 0, j]) * _cofactor_magnitude(J, A, 0, j, nd) + A[..., 0, j] * numpy.abs(_cofactor(J, 0, j, nd)) for j in range(nd))
    Jinv = numpy.empty_like(J)
    for i in range(nd):
        for j in range(nd):
            cof = _cofactor(J, i, j, nd)
            Jinv[..., j, i] = (_cofactor_magnitude(J, A, i, j, nd) + numpy.abs(cof) * adet / numpy.abs(det)) / numpy.abs(det) if absolute else cof / det
    measure = adet if absolute else numpy.abs(det)
    axis = geom.get('bnd_axis', -1)
    if axis >= 0 and mutant != 'no_face':
        measure = measure * numpy.sqrt((Jinv[..., axis, :] ** 2).sum(-1))
    if mutant == 'no_det':
        measure = measure / numpy.abs(det)
    if mutant == 'jinv_transposed':
        Jinv = numpy.swapaxes(Jinv, -1, -2)
    return Jinv, measure


# ---- bases, fields, point factors ---------------------------------------------------------------------------------------------------------------

def basis_sizes(basis, elems):
    if basis.get('off') is not None:
        off = numpy.asarray(basis['off'], dtype=numpy.int64)
        return off[elems + 1] - off[elems]
    return numpy.full(len(elems), basis['nb'], dtype=numpy.int64)


def _first(basis, elems):
    '''(first function, first dof position) of the elements'''
    if basis.get('off') is not None:
        off = numpy.asarray(basis['off'], dtype=numpy.int64)[elems]
        return off, off
    nb = basis['nb']
    tab = basis.get('tab')
    return (numpy.zeros(len(elems), dtype=numpy.int64) if tab is None else numpy.asarray(tab, dtype=numpy.int64)[elems] * nb), elems * nb


def physical_tables(basis, nd, nq, elems, Jinv, absolute):
    '''(D [n][nb][nq][S], dofs [n][nb], positions [n][nb] of the (element, function) pairs in the dof array) for elements with the same number of functions'''
    nb = int(basis_sizes(basis, elems[:1])[0]) if len(elems) else 0
    fn0, pos0 = _first(basis, elems)
    T = numpy.asarray(basis['T'], dtype=float).reshape(-1, nq, 1 + nd)
    Te = _ld(T[fn0[:, None] + numpy.arange(nb)])  # [n][nb][nq][S]
    if absolute:
        Te = numpy.abs(Te)
    D = numpy.empty_like(Te)
    D[..., 0] = Te[..., 0]
    D[..., 1:] = numpy.einsum('enqj,eqji->enqi', Te[..., 1:], Jinv)
    pos = pos0[:, None] + numpy.arange(nb)
    return D, numpy.asarray(basis['dofs'], dtype=numpy.int64).reshape(-1)[pos], pos


def _power(x, p):
    out = numpy.ones_like(x)
    for _ in range(int(p)):
        out = out * x
    return out


def _point_factors(spec, terms, U, ie, elems, absolute, mutant, by_element=False):
    '''g_t [n][nq] of every term'''
    nq = spec['nq']
    fix = numpy.abs if absolute else (lambda a: a)
    pv = []
    for k, (vars_, coeffs, powers) in enumerate(spec.get('polys', ())):
        powers = numpy.asarray(powers, dtype=int).reshape(len(coeffs), len(vars_)).copy()
        if mutant == 'power_off_by_one' and k == 0:
            t, v = numpy.unravel_index(numpy.argmax(powers), powers.shape)
            powers[t, v] += 1
        x = [U[f][:, :, c, 0] for f, c in vars_]
        s = numpy.zeros((len(elems), nq), dtype=LD)
        for cf, pw in zip(fix(_ld(coeffs)), powers):
            m = cf
            for xv, p in zip(x, pw):
                m = m * _power(xv, p)
            s = s + m
        pv.append(s)
    g = []
    for t in terms:
        c = numpy.ones((len(elems), nq), dtype=LD)
        if t.get('scale') is not None:
            sc = fix(_ld(t['scale'])).reshape(-1, nq)
            index = elems if by_element else ie
            if mutant == 'scale_by_element' and not by_element:
                index = elems % len(sc)
            c = c * sc[index]
        if t.get('poly', -1) >= 0:
            c = c * pv[t['poly']]
        if t.get('qs') is not None:
            B, ft, fr = t['qs']
            if mutant == 'qs_swapped':
                ft, fr = fr, ft
            c = c * numpy.einsum('ab,eqa,eqb->eq', fix(_ld(B)), U[ft][:, :, 0, :], U[fr][:, :, 0, :])
        g.append(c)
    return g


def _fields(spec, elems, Jinv, absolute):
    nd, nq = spec['ndims'], spec['nq']
    U = []
    for F in spec.get('fields', ()):
        D, dofs, _ = physical_tables(F['basis'], nd, nq, elems, Jinv, absolute)
        u = _ld(F['u']).reshape(-1, F['ncomp'])
        if absolute:
            u = numpy.abs(u)
        U.append(numpy.einsum('enqs,end->eqds', D, u[dofs]))
    return U


def _groups(spec, bases):
    '''list positions grouped by the sizes of the bases on their elements (ragged bases), each group in chunks'''
    n = spec['nelems']
    elist = spec.get('elist')
    elems = numpy.arange(n, dtype=numpy.int64) if elist is None else numpy.asarray(elist, dtype=numpy.int64)[:n]
    sizes = numpy.stack([basis_sizes(b, elems) for b in bases], 1) if n else numpy.zeros((0, len(bases)), dtype=numpy.int64)
    for key in numpy.unique(sizes, axis=0):
        ie = numpy.flatnonzero((sizes == key).all(1))
        for i in range(0, len(ie), CHUNK):
            yield ie[i:i + CHUNK], elems[ie[i:i + CHUNK]]


# ---- linear forms -------------------------------------------------------------------------------------------------------------------------------

def _vector_pass(spec, absolute, mutant):
    nd, nq = spec['ndims'], spec['nq']
    fix = numpy.abs if absolute else (lambda a: a)
    w = fix(_ld(spec['weights']).reshape(nq))
    blocks, terms = spec['blocks'], spec['terms']
    out = [numpy.zeros((b['nrows'], b['nct']), dtype=LD) for b in blocks]
    local = [numpy.zeros((len(numpy.asarray(b['basis']['dofs']).reshape(-1)), b['nct']), dtype=LD) for b in blocks]
    bases = [b['basis'] for b in blocks] + [F['basis'] for F in spec.get('fields', ())]
    for ie, elems in _groups(spec, bases):
        Jinv, measure = geometry(spec['geom'], nd, nq, elems, absolute, mutant)
        U = _fields(spec, elems, Jinv, absolute)
        g = _point_factors(spec, terms, U, ie, elems, absolute, mutant)
        for ib, b in enumerate(blocks):
            F = numpy.zeros((len(elems), nq, b['nct'], 1 + nd), dtype=LD)
            for t, gt in zip(terms, g):
                if t['block'] != ib:
                    continue
                Ft = numpy.zeros_like(F)
                if t.get('f') is not None:
                    Ft = Ft + fix(_ld(t['f']))
                if t.get('C') is not None:
                    Ft = Ft + numpy.einsum('cadb,eqdb->eqca', fix(_ld(t['C'])), U[t['field']])
                F = F + gt[:, :, None, None] * Ft
            D, dofs, pos = physical_tables(b['basis'], nd, nq, elems, Jinv, absolute)
            r = numpy.einsum('q,eq,emqa,eqca->emc', w, measure, D, F)
            numpy.add.at(out[ib], dofs.reshape(-1), r.reshape(-1, b['nct']))
            local[ib][pos.reshape(-1)] = r.reshape(-1, b['nct'])
    return out, local


def vector_terms(spec, mutant=None):
    '''nh_assemble_terms of one list: per output block (value [nrows][nct], magnitude, local value [positions][nct], local magnitude); the local arrays
    are the element-major local vectors of nh_block.local_dev (zero at the positions of elements that are not in the list)'''
    val, loc = _vector_pass(spec, False, mutant)
    mag, lmag = _vector_pass(spec, True, None)
    return [(v, m, lv, lm) for v, m, lv, lm in zip(val, mag, loc, lmag)]


# ---- bilinear forms -----------------------------------------------------------------------------------------------------------------------------

def _matrix_pass(spec, absolute, mutant):
    '''(keys, contributions): key = (row nct + c) (ncols ncr) + col ncr + d of every local entry with mask[c][d]'''
    nd, nq, nct, ncr = spec['ndims'], spec['nq'], spec['nct'], spec['ncr']
    S = 1 + nd
    fix = numpy.abs if absolute else (lambda a: a)
    w = fix(_ld(spec['weights']).reshape(nq))
    mask = numpy.ones((nct, ncr), dtype=bool) if spec.get('mask') is None else numpy.asarray(spec['mask'], dtype=bool).reshape(nct, ncr)
    dmap = numpy.tile(numpy.arange(ncr), (nct, 1))
    if mutant == 'mask_ignored':  # an absent block (c, d) lands on the next present block of its row (the last one behind them), as a position counted over the present blocks does
        for c in range(nct):
            present = numpy.flatnonzero(mask[c])
            for d in range(ncr):
                if len(present) and not mask[c, d]:
                    dmap[c, d] = present[present > d][0] if (present > d).any() else present[-1]
        mask = numpy.broadcast_to(mask.any(1)[:, None], mask.shape)
    terms = spec['terms']
    bases = [spec['test'], spec['trial']] + [F['basis'] for F in spec.get('fields', ())]
    keys, vals = [], []
    for ie, elems in _groups(spec, bases):
        Jinv, measure = geometry(spec['geom'], nd, nq, elems, absolute, mutant)
        U = _fields(spec, elems, Jinv, absolute)
        g = _point_factors(spec, terms, U, ie, elems, absolute, mutant, by_element=bool(spec.get('by_element')))
        Cq = numpy.zeros((len(elems), nq, nct, S, ncr, S), dtype=LD)
        for t, gt in zip(terms, g):
            kind = t.get('kind', 0)
            if mutant == 'kinds_swapped' and kind:
                kind = 3 - kind
            C = fix(_ld(t['C']))
            if kind == 0:
                Cq += gt[:, :, None, None, None, None] * C
            elif kind == 1:
                Cq[:, :, 0, :, 0, 0] += gt[:, :, None] * numpy.einsum('ab,eqb->eqa', C[0, :, 0, :], U[t['field']][:, :, 0, :])
            else:
                L = fix(_ld(t['L'] if t.get('L') is not None else numpy.ones((1, S)))).reshape(-1)[:S]
                Cq[:, :, 0, :, 0, :] += gt[:, :, None, None] * L[:, None] * numpy.einsum('xb,eqx->eqb', C[0, :, 0, :], U[t['field']][:, :, 0, :])[:, :, None, :]
        Dt, tdofs, _ = physical_tables(spec['test'], nd, nq, elems, Jinv, absolute)
        Dr, rdofs, _ = physical_tables(spec['trial'], nd, nq, elems, Jinv, absolute)
        W = numpy.einsum('eqcadb,enqb->eqcand', Cq, Dr)
        A = numpy.einsum('emqa,eqcand->emcnd', Dt * (w[None, None, :, None] * measure[:, None, :, None]), W)
        rows = tdofs[:, :, None, None, None] * nct + numpy.arange(nct)[None, None, :, None, None]
        cols = rdofs[:, None, None, :, None] * ncr + dmap[None, None, :, None, :]
        key = numpy.broadcast_to(rows * (spec['ncols'] * ncr) + cols, A.shape)
        keep = numpy.broadcast_to(mask[None, None, :, None, :], A.shape)
        keys.append(key[keep])
        vals.append(A[keep])
    if not keys:
        return numpy.zeros(0, dtype=numpy.int64), numpy.zeros(0, dtype=LD)
    return numpy.concatenate(keys), numpy.concatenate(vals)


def pattern_keys(spec):
    '''sorted keys (row nct + c) (ncols ncr) + col ncr + d of the pattern of nh_pattern_build expanded by nh_pattern_expand: every pair of a test and a trial dof of
    every element of the MESH (not only of the list), every block with mask[c][d]'''
    nct, ncr = spec['nct'], spec['ncr']
    mask = numpy.ones((nct, ncr), dtype=bool) if spec.get('mask') is None else numpy.asarray(spec['mask'], dtype=bool).reshape(nct, ncr)
    elems = numpy.arange(spec.get('mesh_nelems', spec['nelems']), dtype=numpy.int64)
    sizes = numpy.stack([basis_sizes(spec['test'], elems), basis_sizes(spec['trial'], elems)], 1)
    pairs = []
    for key in numpy.unique(sizes, axis=0):
        sel = elems[(sizes == key).all(1)]
        t = numpy.asarray(spec['test']['dofs'], dtype=numpy.int64).reshape(-1)[_first(spec['test'], sel)[1][:, None] + numpy.arange(key[0])]
        r = numpy.asarray(spec['trial']['dofs'], dtype=numpy.int64).reshape(-1)[_first(spec['trial'], sel)[1][:, None] + numpy.arange(key[1])]
        pairs.append((t[:, :, None] * spec['ncols'] + r[:, None, :]).reshape(-1))
    scalar = numpy.unique(numpy.concatenate(pairs))
    row, col = scalar // spec['ncols'], scalar % spec['ncols']
    c, d = numpy.nonzero(mask)
    return numpy.unique(((row[:, None] * nct + c) * (spec['ncols'] * ncr) + col[:, None] * ncr + d).reshape(-1))


def matrix_terms(spec, mutant=None):
    '''nh_assemble_matrix_terms: (value [nnz], magnitude [nnz], rowptr int64 [nrows nct + 1], colidx int64 [nnz]) in the layout of nh_pattern_expand -- rows
    (row, c), columns (col, d) strictly increasing within a row, every entry of the pattern of the MESH (zero where no element of the list contributes)'''
    nct, ncr = spec['nct'], spec['ncr']
    width = spec['ncols'] * ncr
    keys, vals = _matrix_pass(spec, False, mutant)
    akeys, avals = _matrix_pass(spec, True, None)
    uniq = pattern_keys(spec)
    value, mag = numpy.zeros(len(uniq), dtype=LD), numpy.zeros(len(uniq), dtype=LD)
    numpy.add.at(value, numpy.searchsorted(uniq, keys), vals)
    numpy.add.at(mag, numpy.searchsorted(uniq, akeys), avals)
    rowptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(uniq // width, minlength=spec['nrows'] * nct))]).astype(numpy.int64)
    return value, mag, rowptr, (uniq % width).astype(numpy.int64)


# ---- rounding counts ------------------------------------------------------------------------------------------------------------------------------

def rounding_counts(nd, ngb, face):
    '''(roundings in an entry of Jinv, in the measure) of nh_geom.inc, against the magnitudes above.  g = roundings of an entry of J: the ngb products and
    ngb - 1 additions of the isoparametric sum (0 for BOX and TAB, which read J).  Cofactor: nd = 3 a difference of two products of two entries, 2 g + 2; nd = 2 an
    entry, g; nd = 1 the constant 1.  det: nd = 1 g; nd = 2 2 g + 2; nd = 3 three products entry x cofactor and two additions, 3 g + 5.  Jinv = cofactor x (1 / det):
    cofactor + det + 2.  Face: s2 = nd squares of entries of Jinv and nd - 1 additions, its root, one product with det: 2 Jinv + nd + 2 (the root is charged a full
    rounding of its argument).'''
    g = ngb
    cof = {1: 0, 2: g, 3: 2 * g + 2}[nd]
    det = {1: g, 2: 2 * g + 2, 3: 3 * g + 5}[nd]
    jinv = cof + det + 2
    return jinv, det + (2 * jinv + nd + 2 if face else 0)


def chain_common(nd, nb_field, ngb, face, degree, npoly_terms, has_qs):
    '''(jinv, wdet, U, coef): roundings of an entry of Jinv, of w |det|, of a field value / gradient U = sum_n T u (nb products and sums) transformed by Jinv
    (nd products and sums of entries that carry jinv), and of g_t = scale x polynomial x point factor: a monomial of total degree `degree` is at most `degree`
    products of values carrying nb roundings each (multiplied out one by one, or by repeated squaring, which takes fewer products) plus the sum over the monomials;
    the point factor S^2 products B U U and their sum.'''
    S = 1 + nd
    jinv, det = rounding_counts(nd, ngb, face)
    wdet = det + 1
    mU = nb_field + jinv + nd if nb_field else 0
    poly = degree * (nb_field + 1) + npoly_terms
    qs = 2 * mU + 2 + S * S if has_qs else 0
    return jinv, wdet, mU, poly + qs + 2


def m_vector(*, nd, nq, nb_field, ngb=0, face=False, degree=0, npoly_terms=0, has_qs=False, nterms=1, ncr=1, contributions=1):
    '''roundings along the longest chain of an entry of nh_assemble_terms (k_terms, k_terms_multi, k_local_vterms2 evaluate the same chain):
    F_t = f + sum_db C U: the roundings of U, a product, ncr S additions;  coef x F_t and the sum over the terms;  the transform to the reference form, nd products with
    Jinv and their sum, times w |det|;  the contraction with the test table over nq S products;  the sum of the element contributions of a dof.'''
    S = 1 + nd
    jinv, wdet, mU, coef = chain_common(nd, nb_field, ngb, face, degree, npoly_terms, has_qs)
    return coef + (mU + 1 + ncr * S) + 1 + nterms + (jinv + nd) + wdet + 1 + (1 + nq * S) + contributions


def m_matrix(*, nd, nq, nb_field, ngb=0, face=False, degree=0, npoly_terms=0, has_qs=False, nterms=1, contributions=1):
    '''roundings along the longest chain of an entry of nh_assemble_matrix_terms (k_mterms folds Jinv into the coefficient tensor, k_local_terms into the tables,
    k_local_terms2 into the tensor: the same factors either way): C_t(q) of kinds 1 / 2 a sum of S products with U and up to two more products, times coef, summed
    over the terms;  Jinv on both sides, nd products and sums each;  w |det|;  the S x S contraction with the test and trial rows (two products, S sums per side) over
    nq points;  the sum of the element contributions of an entry.'''
    S = 1 + nd
    jinv, wdet, mU, coef = chain_common(nd, nb_field, ngb, face, degree, npoly_terms, has_qs)
    return coef + (mU + S + 3) + nterms + 2 * (jinv + nd) + wdet + 1 + (2 + 2 * S + nq * S) + contributions
