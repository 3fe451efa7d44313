'''The term-list assembly kernels (nh_assemble_terms, nh_assemble_terms_multi, nh_assemble_matrix_terms; nutils_amd/csrc/nh_assemble_batched.hip) against the
longdouble restatement of their header formulas (tests/terms_refs.py), entry by entry:

    |got - ref| <= gamma_m magnitude,    gamma_m = m u / (1 - m u),  u = 2^-53

magnitude: the same sums over absolute values (terms_refs); m: the roundings along the longest chain of the kernels, counted from their source in
terms_refs.m_vector / m_matrix (docstrings there) from the shapes of the case -- nothing is taken from what the kernels return.  Index arrays must be equal.  Every
case asserts, through nh_terms_launch_counts, which kernel family served it.  The inputs are those of tests/terms_cases.py; tests/test_terms_refs_host.py shows on
the same inputs that the mistakes a kernel could make (kinds swapped, scale by element, transposed inverse, dropped measure ...) are far outside this bound.'''
import functools

import numpy
import pytest

import terms_cases as tc
import terms_refs as tr

pytestmark = pytest.mark.gpu

LD = numpy.longdouble
GATHER, STORE, BY_ELEMENT = 64, 128, 2


# ---- references, computed once --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def vector_reference(family, name):
    spec = tc.build(family, name)
    return spec, tr.vector_terms(spec), tc.gamma_m(spec)


@functools.lru_cache(maxsize=4)
def matrix_reference(family, name):
    spec = tc.build(family, name)
    return spec, tr.matrix_terms(spec), tc.gamma_m(spec)


# ---- host data -> device arguments ------------------------------------------------------------------------------------------------------------

class Device:
    '''device copies of the bases and the geometry of a spec; one copy per host array, so that bases that share a table or a dof array on the host share it on the device'''

    def __init__(self, spec):
        from nutils_amd import device, kernels
        self.spec, self.bases, self.arrays = spec, {}, {}
        self.weights = device.to_dev(spec['weights'], 'float64')
        self.elist = None if spec.get('elist') is None else device.to_dev(spec['elist'], 'int32')
        g = spec['geom']
        if g['kind'] == 'box':
            self.geom = kernels.geometry_box(device.to_dev(g['origin'], 'float64'), device.to_dev(g['size'], 'float64'), g['bnd_axis'])
        elif g['kind'] == 'tab':
            self.geom = kernels.geometry_tab(device.to_dev(g['jac'], 'float64'), None, g['bnd_axis'])
        else:
            self.geom = kernels.geometry_iso(g['ngb'], device.to_dev(g['gT'], 'float64'), device.to_dev(g['gdofs'], 'int32'), device.to_dev(g['verts'], 'float64'), g['bnd_axis'])
        self.fields = [(self.basis(F['basis']), device.to_dev(F['u'], 'float64'), F['ncomp']) for F in spec.get('fields', ())]
        self.polys = [(list(v), numpy.asarray(c, dtype=float), numpy.asarray(p, dtype=numpy.int32)) for v, c, p in spec.get('polys', ())]

    def array(self, a, dtype):
        from nutils_amd import device
        if a is None:
            return None
        if id(a) not in self.arrays:
            self.arrays[id(a)] = device.to_dev(a, dtype), a
        return self.arrays[id(a)][0]

    def basis(self, B):
        from nutils_amd import kernels
        if id(B) not in self.bases:
            self.bases[id(B)] = kernels.basis(self.array(B['T'], 'float64'), self.array(B['dofs'], 'int32'), nb=B['nb'], off=self.array(B.get('off'), 'int64'),
                                              tab=self.array(B.get('tab'), 'int32'))
        return self.bases[id(B)]

    def terms(self, keys):
        from nutils_amd import device
        out = []
        for t in self.spec['terms']:
            d = {k: t[k] for k in keys if t.get(k) is not None}
            if t.get('scale') is not None:
                d['scale'] = device.to_dev(t['scale'], 'float64')
            out.append(d)
        return out

    def vector_arguments(self, outs=None):
        '''(keywords of kernels.assemble_terms, out tensors, local tensors or None per block)'''
        from nutils_amd import device
        spec = self.spec
        outs = outs or [device.zeros(b['nrows'] * b['nct'], 'float64') for b in spec['blocks']]
        local = [device.zeros(len(numpy.asarray(b['basis']['dofs']).reshape(-1)) * b['nct'], 'float64') if b.get('local') else None for b in spec['blocks']]
        blocks = [(self.basis(b['basis']), b['nct'], o) + ((l,) if l is not None else ()) for b, o, l in zip(spec['blocks'], outs, local)]
        kw = dict(nelems=spec['nelems'], ndims=spec['ndims'], nq=spec['nq'], weights=self.weights, geom=self.geom, fields=self.fields, blocks=blocks,
                  terms=self.terms(('block', 'field', 'poly', 'C', 'f', 'qs')), polys=self.polys, elist=self.elist)
        return kw, outs, local


def counts():
    from nutils_amd import kernels
    return kernels.terms_launch_counts()


def launched(before):
    after = counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def worst(got, ref, mag, g):
    '''max |got - ref| / (gamma_m magnitude); an entry of magnitude zero must be exactly zero'''
    got, ref, mag = LD(numpy.asarray(got)).reshape(-1), ref.reshape(-1), mag.reshape(-1)
    assert got.shape == ref.shape
    assert numpy.isfinite(got).all()
    err = numpy.abs(got - ref)
    assert (err[mag == 0] == 0).all()
    return float((err[mag > 0] / (g * mag[mag > 0])).max()) if (mag > 0).any() else 0.


def run_vector(family, name, expect):
    from nutils_amd import device, kernels
    spec, ref, (m, g) = vector_reference(family, name)
    dev = Device(spec)
    kw, outs, local = dev.vector_arguments()
    before = counts()
    kernels.assemble_terms(**kw)
    assert launched(before) == expect
    ratios = []
    for o, l, (value, mag, lvalue, lmag) in zip(outs, local, ref):
        if l is not None:
            assert not device.to_host(o).any()  # (the local vectors are stored, nothing is added into out)
            ratios.append(worst(device.to_host(l), lvalue, lmag, g))
        else:
            ratios.append(worst(device.to_host(o), value, mag, g))
    print(f'{family} {name}: m = {m}, largest err/bound = {max(ratios):.2e}')
    assert max(ratios) <= 1
    return spec


def run_matrix(family, name, flags, expect, repeat=False, refused=None):
    from nutils_amd import device, kernels
    spec, (value, mag, rowptr, colidx), (m, g) = matrix_reference(family, name)
    dev = Device(spec)
    test, trial = dev.basis(spec['test']), dev.basis(spec['trial'])
    pattern = kernels.Pattern(spec['mesh_nelems'], spec['nrows'], spec['ncols'], test._keep[1], trial._keep[1], nbt=spec['test']['nb'], nbr=spec['trial']['nb'],
                              toff=test._keep[2], roff=trial._keep[2])
    rp, ci = pattern.expand(spec['nct'], spec['ncr'], spec['mask'])
    assert numpy.array_equal(device.to_host(rp), rowptr) and numpy.array_equal(device.to_host(ci), colidx)
    results = []
    for _ in range(2 if repeat else 1):
        values = device.to_dev(numpy.full(len(colidx), numpy.nan), 'float64') if flags & STORE else device.zeros(len(colidx), 'float64')
        before = counts()
        kw = dict(nelems=spec['nelems'], ndims=spec['ndims'], nq=spec['nq'], weights=dev.weights, geom=dev.geom, test=test, trial=trial, nct=spec['nct'], ncr=spec['ncr'],
                  mask=spec['mask'], pattern=pattern, values=values, terms=dev.terms(('kind', 'field', 'poly', 'C', 'L', 'qs')), fields=dev.fields, polys=dev.polys,
                  elist=dev.elist, flags=flags, gather=False)
        if refused:
            from nutils_amd import _lib
            with pytest.raises(_lib.NutilsHipError, match=refused):
                kernels.assemble_matrix_terms(**kw)
            assert launched(before) == {} and numpy.isnan(device.to_host(values)).all()
            return spec
        kernels.assemble_matrix_terms(**kw)
        assert launched(before) == expect
        results.append(device.to_host(values))
    ratio = worst(results[0], value, mag, g)  # (finite everywhere: no NaN of the prefill survives)
    print(f'{family} {name}: m = {m}, largest err/bound = {ratio:.2e}')
    assert ratio <= 1
    if repeat:
        assert results[0].tobytes() == results[1].tobytes()
    return spec


# ---- k_terms --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(tc.K_TERMS))
def test_k_terms(name):
    '''Lists of fewer than 2^14 elements: the batched kernel.  m = terms_refs.m_vector: the factor g_t (polynomial of total degree d: d (nb + 1) + its terms;
    point factor 2 U + 2 + S^2; two products), F_t (U + 1 + ncr S, U = nb + Jinv + nd), the sum over the terms, the transform to the reference form (Jinv + nd),
    w |det| (det + 1, with the face factor 2 Jinv + nd + 2 more), the contraction over nq S, the contributions of the elements of a dof; Jinv and det as in
    terms_refs.rounding_counts.'''
    run_vector('k_terms', name, {'k_terms': 1})


# ---- k_terms_multi ----------------------------------------------------------------------------------------------------------------------------------

def test_k_terms_multi():
    '''Eight lists of one launch and a ninth, a list of another dimension, an empty list and a list of 2^14 elements: ONE k_terms_multi launch, the ninth and the
    3-D list through k_terms, the large one through k_local_vterms2.  The 2-D lists add into the same two vectors: the result is the sum of the references, the bound
    the sum of their bounds with m = m_vector + the number of lists (the additions of the lists' contributions to a dof).'''
    from nutils_amd import device, kernels
    specs2 = [tc.build_entry(e) for e in tc.MULTI_2D]
    spec3, big = [tc.build_entry(e) for e in tc.MULTI_OTHER]
    assert len(specs2) == 9 and big['nelems'] >= 2 ** 14 and spec3['ndims'] == 3
    nlists = len(specs2)
    shared = [device.zeros(b['nrows'], 'float64') for b in specs2[0]['blocks']]
    devs = [Device(s) for s in specs2 + [spec3, big]]
    args = [d.vector_arguments(shared if i < nlists else None) for i, d in enumerate(devs)]
    empty = dict(args[0][0], nelems=0)
    lists = [a[0] for a in args[:4]] + [args[nlists][0], empty] + [a[0] for a in args[4:nlists]] + [args[nlists + 1][0]]
    before = counts()
    kernels.assemble_terms_multi(lists)
    assert launched(before) == {'k_terms_multi': 1, 'k_terms': 2, 'k_local_vterms2': 1}
    value = [numpy.zeros(b['nrows'] * b['nct'], dtype=LD) for b in specs2[0]['blocks']]
    bound = [numpy.zeros_like(v) for v in value]
    for s in specs2:
        g = tr.gamma(tc.gamma_m(s)[0] + nlists)
        for b, (v, mag, _, _) in enumerate(tr.vector_terms(s)):
            value[b] += v.reshape(-1)
            bound[b] += g * mag.reshape(-1)
    ratios = [worst(device.to_host(o), v, bd, 1) for o, v, bd in zip(shared, value, bound)]
    for s, (_, outs, _) in zip([spec3, big], args[nlists:]):
        g = tc.gamma_m(s)[1]
        ratios += [worst(device.to_host(o), v, mag, g) for o, (v, mag, _, _) in zip(outs, tr.vector_terms(s))]
    print(f'k_terms_multi: largest err/bound = {max(ratios):.2e}')
    assert max(ratios) <= 1


# ---- k_local_vterms2 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(tc.K_LOCAL_VTERMS2))
def test_k_local_vterms2(name):
    '''Lists of 2^14 elements and more with scalar blocks and fields on ONE small uniform basis: a lane per element.  m = terms_refs.m_vector, as for k_terms (the
    polynomial by repeated squaring takes fewer products than the degree; the partial sums of the four waves are a reordering of the nq S additions).
    The table classes per run of 64 list positions, computed here from `tab`, decide between the staged and the unstaged branch.'''
    spec = tc.build('k_local_vterms2', name)
    classes = tc.classes_per_run(spec['blocks'][0]['basis']['tab'], spec.get('elist'))
    assert spec['nelems'] >= 2 ** 14
    if name.startswith('quad_spline2_4096x4-') and not name.endswith('permutation'):
        assert classes.max() <= 6 and ((classes >= 2) & (classes <= 6)).any()  # (multi-class staging, every run staged)
    if name.startswith('quad_spline2_graded_2048x8'):
        assert (classes > 6).any()  # (more classes than a workgroup stages: global table reads)
    if name.startswith('quad_spline2_16384x4'):
        assert spec['nelems'] >= 2 ** 16 and (classes > 2).any()  # (from 2^16 elements on two classes are staged)
    if name.startswith(('line_p1_16385', 'quad_p1_127x130')):
        assert spec['nelems'] % 64  # (tail lanes)
    run_vector('k_local_vterms2', name, {'k_local_vterms2': 1})


# ---- k_mterms ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(tc.K_MTERMS))
def test_k_mterms(name):
    '''The batched matrix kernel (no NH_MATRIX_GATHER).  m = terms_refs.m_matrix: the factor g_t as for the linear forms, C_t(q) of the point-dependent kinds (U + S + 3),
    the sum over the terms, Jinv on both sides (2 (Jinv + nd)), w |det|, the S x S contraction with the two table rows over nq points (2 + 2 S + nq S), the
    contributions of the elements of an entry.'''
    spec = tc.build('k_mterms', name)
    run_matrix('k_mterms', name, BY_ELEMENT if spec['by_element'] else 0, {'k_mterms': 1})


def test_gather_without_store_falls_back_to_k_mterms():
    '''NH_MATRIX_GATHER alone on a block that does not qualify for the thread-per-element pass (3 x 3 components): the batched kernel takes over, values are added.'''
    run_matrix('k_mterms', 'vector_3x3_tab', GATHER, {'k_mterms': 1})


def test_a_field_with_its_own_dofs_is_not_a_field_on_the_test_basis():
    '''A field whose basis shares the TABLES of the test basis but numbers its dofs differently: the thread-per-element pass reads field coefficients through the
    test dofs, so the block does not qualify and the batched kernel, which gathers through the field's own dofs, takes over.'''
    spec = tc.build('k_mterms', 'field_with_own_dofs')
    assert spec['fields'][0]['basis']['T'] is spec['test']['T'] and spec['fields'][0]['basis']['dofs'] is not spec['test']['dofs']
    run_matrix('k_mterms', 'field_with_own_dofs', GATHER, {'k_mterms': 1})
    run_matrix('k_mterms', 'field_with_own_dofs', GATHER | STORE, {}, refused='does not qualify')


def test_store_refuses_a_block_that_does_not_qualify():
    '''NH_MATRIX_GATHER | NH_MATRIX_STORE on such a block is an error: nothing is launched, nothing is written.'''
    run_matrix('k_mterms', 'vector_3x3_tab', GATHER | STORE, {}, refused='does not qualify')


# ---- k_local_terms / k_local_terms2 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(tc.K_LOCAL_TERMS))
def test_k_local_terms(name):
    '''NH_MATRIX_GATHER | NH_MATRIX_STORE into NaN-filled values, keys 10202 / 10303 / 20404: a thread per element, then the owner-side sums.  m = terms_refs.m_matrix
    (here Jinv is folded into the table rows instead of the tensor: the same factors).  No NaN survives; a repeat is byte-identical.'''
    run_matrix('k_local_terms', name, GATHER | STORE, {'k_local_terms': 1}, repeat=True)


@pytest.mark.parametrize('name', sorted(tc.K_LOCAL_TERMS2))
def test_k_local_terms2(name):
    '''As test_k_local_terms for the keys 20909 / 30808 (two-phase kernel, Jinv folded into the tensor; multilinear ISO geometry or any other).  The table classes per
    run of 64 elements: up to six are staged below 2^16 elements, two from there on.'''
    spec = tc.build('k_local_terms2', name)
    classes = tc.classes_per_run(spec['test']['tab'])
    if name.startswith('20909-spline2_5x4'):
        assert (classes > 6).any()
    elif name.startswith('20909-spline2_16384x4'):
        assert spec['nelems'] >= 2 ** 16 and (classes > 2).any()
    elif name.startswith('20909-') and 'fields-' in name and 'p2' not in name:
        assert 2 <= classes.max() <= 6
    run_matrix('k_local_terms2', name, GATHER | STORE, {'k_local_terms2': 1}, repeat=True)
