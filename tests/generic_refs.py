'''Rounding counts and deliberate mistakes for the element kernels of nh_assemble_matrix and nh_assemble_vector (nutils_amd/csrc/nh_assemble_generic.hip,
nh_gram_sym.inc): k_matrix_mfma, k_matrix_generic, k_gram_sym, k_vector_generic.  No GPU, no library.

The REFERENCE is tests/terms_refs.py unchanged: matrix_terms of a list of kind-0 terms is the formula of nh_assemble_matrix (a per-point tensor cq is the sum of
two terms with a scale array each, Cq = sum_t scale_t C_t), vector_terms that of nh_assemble_vector; both return a value and a magnitude per entry, and
|got - ref| <= gamma_m magnitude bounds any evaluation with m roundings along its longest chain.  The functions m_* below count that chain from the kernel sources.
Common to all (terms_refs.rounding_counts): jinv, det roundings of an entry of Jinv and of det;  D = T . Jinv: nd products and sums of entries that carry jinv
(jinv + nd per side; a product Dt Dr carries both);  w |det| (x scale): det + 1 (+ 1).  The element contributions of an entry are added in any order (atomics, plain
read-modify-write of a colour, owner-side sums): one rounding per contribution, and per chunk of points where the kernel adds chunk by chunk.

`mutant_matrix` evaluates the reference with ONE deliberate mistake of the kind these kernels could make (MUTANTS); tests/test_generic_refs_host.py shows that
each is far outside the bound on the inputs of tests/test_gpu_generic.py.'''
import copy

import numpy

import terms_refs as tr

LD = numpy.longdouble
MUTANTS = ('padded_point', 'padded_column', 'slots_not_compacted', 'active_slot_dropped', 'mirror_untransposed', 'scale_wrong_index', 'chunk_stores', 'mask_ignored',
           'trial_is_test')


# ---- rounding counts ----------------------------------------------------------------------------------------------------------------------------------

def _common(nd, ngb, scale):
    jinv, det = tr.rounding_counts(nd, ngb, False)
    return jinv, det + 1 + bool(scale)


def m_generic(*, nd, nq, ngb=0, scale=False, qchunk=None, contributions=1, cq_roundings=0):
    '''k_matrix_generic, the longest of its branches.  Per side D: jinv + nd.  Then
      entries without W:  t = sum_b C dr[b] (S), sq = sum_a dt[a] t (S), acc += w|det| sq (a product; nq sums)         2 S + 1 + nq
      entries with W:     w[a] = w|det| sum_b C dr[b] (S + 1), acc += dt[a] w[a] over the points and slots (nq S)       S + 1 + nq S     (scalar symmetric: the same two)
      Gram (both):        wa = w|det| dt[a] (1), G[a][b] += wa dr[b] (nq), acc = sum_ab C G (S S)                        1 + nq + S S
    A launch whose points are chunked (qchunk < nq) adds an element's entry once per chunk: contributions x chunks additions.  A per-point tensor cq formed on the
    host from two scaled terms brings cq_roundings of its own.'''
    S = 1 + nd
    jinv, wdet = _common(nd, ngb, scale)
    nchunks = -(-nq // (qchunk or nq))
    return 2 * (jinv + nd) + wdet + max(2 * S + 1 + nq, S + 1 + nq * S, 1 + nq + S * S) + cq_roundings + contributions * nchunks


def m_mfma(*, nd, nq, nas, ngb=0, scale=False, contributions=1):
    '''k_matrix_mfma: D per side jinv + nd;  the B operand b = (sum_b C dr[b]) w|det|: S + 1;  the accumulator takes one fused multiply-add per k index,
    k = (active test slot, point padded to a multiple of 4): nas nqp;  the contributions of the elements.'''
    S = 1 + nd
    jinv, wdet = _common(nd, ngb, scale)
    return 2 * (jinv + nd) + wdet + S + 1 + nas * ((nq + 3) & ~3) + contributions


def m_gram_sym(*, nd, nq, ngb=0, scale=False, contributions=1):
    '''k_gram_sym: as the Gram branches -- w = w|det| D[m][a] (1), G += w D[n][b] over the points (nq), K = sum_ab C G (at most S S) -- and the owner-side sum of the
    contributions.  With the triangular scratch the roles of m and n may be swapped: the same count.'''
    S = 1 + nd
    jinv, wdet = _common(nd, ngb, scale)
    return 2 * (jinv + nd) + wdet + 1 + nq + S * S + contributions


def m_vector_generic(*, nd, nq, nbr, ncr, nct=1, ngb=0, scale=False, qchunk=None, contributions=1, functional_terms=0):
    '''k_vector_generic: U = sum_n Dr u (Dr: jinv + nd; nbr);  F = f + sum_db C U (ncr S);  s = sum_a Dt F (Dt: jinv + nd; S);  acc += w|det| s (a product, nq
    sums);  contributions x chunks additions into the dof.  The functional (functional_terms = nelems nq > 0) instead: h = sum U (F - f) carries U twice (2 (jinv + nd
    + nbr) + ncr S + 1 + nct S), halved and added to f0 and f . U (nct S + 3), times w|det|, and all points of all elements are summed in some order.'''
    S = 1 + nd
    jinv, wdet = _common(nd, ngb, scale)
    nchunks = -(-nq // (qchunk or nq))
    if functional_terms:
        return 2 * (jinv + nd + nbr) + ncr * S + 1 + 2 * nct * S + 3 + wdet + 1 + functional_terms
    return 2 * (jinv + nd) + nbr + ncr * S + S + wdet + 1 + nq + contributions * nchunks


# ---- mutants --------------------------------------------------------------------------------------------------------------------------------------

def active_slots(spec):
    '''test slots a with a nonzero coefficient C[c][a][d][b] in some term'''
    return [a for a in range(1 + spec['ndims']) if any(numpy.asarray(t['C'])[:, a].any() for t in spec['terms'])]


def _elements(spec):
    n = spec['nelems']
    return numpy.arange(n) if spec.get('elist') is None else numpy.asarray(spec['elist'], dtype=numpy.int64)[:n]


def _local_mutant(spec, mutant):
    '''mistakes in where an entry of the local matrix goes: uniform bases, every block present, one group of elements'''
    assert spec.get('mask') is None and spec['test'].get('off') is None and spec['nelems'] <= tr.CHUNK
    nct, ncr, nbt, nbr = spec['nct'], spec['ncr'], spec['test']['nb'], spec['trial']['nb']
    keys, vals = tr._matrix_pass(spec, False, None)
    A = vals.reshape(spec['nelems'], nbt, nct, nbr, ncr).copy()
    if mutant == 'padded_column':  # the columns j >= nbr ncr of the last N tile read and write column 0: node 0, component 0 receives them too
        A[:, :, :, 0, 0] *= 1 + (-(nbr * ncr) % 16)
    else:  # mirror_untransposed: the pair (n, m), n > m, computed for (m, n) and written as [c][d] where [d][c] belongs
        assert nbt == nbr and nct == ncr
        upper = numpy.triu(numpy.ones((nbt, nbr), dtype=bool), 1)
        A = numpy.where(upper[None, :, None, :, None], A.transpose(0, 1, 4, 3, 2), A)
    uniq = tr.pattern_keys(spec)
    value = numpy.zeros(len(uniq), dtype=LD)
    numpy.add.at(value, numpy.searchsorted(uniq, keys), A.reshape(-1))
    return value


def mutant_matrix(spec, mutant, qchunk=None):
    '''value [nnz] of the reference with one mistake'''
    if mutant == 'mask_ignored':
        return tr.matrix_terms(spec, mutant)[0]
    if mutant in ('padded_column', 'mirror_untransposed'):
        return _local_mutant(spec, mutant)
    s = copy.copy(spec)
    s['terms'] = [dict(t) for t in spec['terms']]
    nq, S = spec['nq'], 1 + spec['ndims']
    if mutant == 'padded_point':  # the points nq .. nqp - 1 of the last k-step are the clamped point nq - 1 with its weight kept
        w = numpy.array(spec['weights'], dtype=float)
        w[-1] *= 1 + (-nq % 4)
        s['weights'] = w
    elif mutant == 'chunk_stores':  # a later chunk of points stores its sum where it should add: the last chunk alone remains
        w = numpy.array(spec['weights'], dtype=float)
        w[:(nq - 1) // qchunk * qchunk] = 0
        s['weights'] = w
    elif mutant in ('slots_not_compacted', 'active_slot_dropped'):
        act = active_slots(spec)
        for t in s['terms']:
            C = numpy.array(t['C'], dtype=float)
            if mutant == 'active_slot_dropped':
                C[:, act[-1]] = 0
            else:  # the a-th ACTIVE slot read from table slot a: an inactive slot kept in the place of an active one
                C2 = numpy.zeros_like(C)
                C2[:, :len(act)] = C[:, act]
                C = C2
            t['C'] = C
    elif mutant == 'scale_wrong_index':  # list position for element and the reverse
        elems, ie = _elements(spec), numpy.arange(spec['nelems'])
        for t in s['terms']:
            if t.get('scale') is not None:
                sc = numpy.asarray(t['scale']).reshape(-1, nq)
                new = sc.copy()
                if spec.get('by_element'):
                    new[elems] = sc[ie]
                else:
                    new[ie] = sc[elems % len(sc)]
                t['scale'] = new
    elif mutant == 'trial_is_test':  # the n-th trial function read from the test table
        nbt, nbr = spec['test']['nb'], spec['trial']['nb']
        T = numpy.asarray(spec['test']['T'])
        s['trial'] = dict(spec['trial'], T=numpy.ascontiguousarray(T.reshape(-1, nbt, nq, S)[:, :nbr].reshape(-1, nq, S)))
    else:
        raise ValueError(mutant)
    return tr.matrix_terms(s)[0]


def applies(spec, mutant, run):
    '''can this case show the mistake?  run: how tests/test_gpu_generic.py launches it (tests/generic_cases.py)'''
    nct, ncr = spec['nct'], spec['ncr']
    uniform = spec['test'].get('off') is None
    scaled = any(t.get('scale') is not None for t in spec['terms'])
    local = uniform and spec.get('mask') is None and spec['nelems'] <= tr.CHUNK
    if mutant == 'padded_point':
        return spec['nq'] % 4 != 0
    if mutant == 'padded_column':
        return local and run.get('family') == 'k_matrix_mfma' and (spec['trial']['nb'] * ncr) % 16 != 0
    if mutant == 'slots_not_compacted':
        act = active_slots(spec)
        return act != list(range(len(act)))
    if mutant == 'active_slot_dropped':
        return True
    if mutant == 'mirror_untransposed':
        return local and nct == ncr > 1 and spec['test'] is spec['trial'] and run.get('symmetric', False)
    if mutant == 'scale_wrong_index':
        return scaled and spec.get('elist') is not None
    if mutant == 'chunk_stores':
        return bool(run.get('qchunk')) and run['qchunk'] < spec['nq']
    if mutant == 'mask_ignored':
        return spec.get('mask') is not None and not numpy.asarray(spec['mask']).all()
    if mutant == 'trial_is_test':
        return uniform and spec['trial'] is not spec['test'] and not (numpy.shape(spec['trial']['T']) == numpy.shape(spec['test']['T']) and
                                                                      numpy.array_equal(spec['trial']['T'], spec['test']['T']))
    raise ValueError(mutant)
