'''The element kernels underneath every other assembly path -- k_matrix_mfma, k_matrix_generic, k_gram_sym (nh_assemble_matrix) and k_vector_generic
(nh_assemble_vector; nutils_amd/csrc/nh_assemble_generic.hip, nh_gram_sym.inc) -- against the longdouble restatement of tests/terms_refs.py, entry by entry:

    |got - ref| <= gamma_m magnitude,    gamma_m = m u / (1 - m u),  u = 2^-53

m: the roundings along the longest chain of the kernel that serves the case, counted from its source in tests/generic_refs.py (m_mfma, m_generic, m_gram_sym,
m_vector_generic) from the shapes of the case -- nothing is taken from what the kernels return.  Index arrays must be equal, entries of magnitude zero exactly zero.
Every case asserts through nh_generic_launch_record WHICH kernel served it and what the launcher chose (tiles, branch, waves, W table, chunk of points, elements per
workgroup): kernels.assemble_matrix is called with `gather` and `fused` given, so nothing is routed elsewhere.  The inputs are those of tests/generic_cases.py;
tests/test_generic_refs_host.py shows on the same inputs that float64 in another order is inside the bound and that the mistakes these kernels could make (a padded
point counted, a padded column aliased, slots mixed up, an untransposed mirror, scale by the wrong index, a chunk that stores, the mask ignored, the wrong table) are
far outside.'''
import numpy
import pytest

import generic_cases as gc
from test_gpu_terms import Device, worst

pytestmark = pytest.mark.gpu

FAMILIES = ('k_matrix_mfma', 'k_matrix_generic', 'k_gram_sym', 'k_vector_generic')


def record():
    from nutils_amd import kernels
    return kernels.generic_launch_record()


def check_record(before, run, launches):
    '''the family of the case was launched `launches` times, no other family of the record at all, and its last launch made the choices the case names'''
    counts, choice = record()
    got = {f: counts[f] - before[f] for f in FAMILIES if counts[f] != before[f]}
    print(f'record: {got} {choice[run["family"]]}')
    assert got == {run['family']: launches}
    for key, value in run['expect'].items():
        assert choice[run['family']][key] == value, (key, choice[run['family']])


def nan_or_zeros(n, nan):
    from nutils_amd import device
    return device.to_dev(numpy.full(n, numpy.nan), 'float64') if nan else device.zeros(n, 'float64')


def run_matrix(family, name, monkeypatch):
    from nutils_amd import device, kernels
    spec, run = gc.build(family, name)
    ref = gc.reference(family, name)
    m, g = gc.gamma_m(spec, run)
    for key, value in run.get('env', {}).items():
        monkeypatch.setenv(key, value)
    dev = Device(spec)
    test, trial = dev.basis(spec['test']), dev.basis(spec['trial'])
    nbt, nbr = spec['test']['nb'], spec['trial']['nb']
    if spec.get('elist') is not None and not spec['by_element']:  # scale and element map by list position: the pattern of the listed elements
        ref = gc.list_pattern(spec, ref)
        listed = [device.to_dev(numpy.asarray(B['dofs']).reshape(-1, B['nb'])[spec['elist']].reshape(-1), 'int32') for B in (spec['test'], spec['trial'])]
        pattern = kernels.Pattern(spec['nelems'], spec['nrows'], spec['ncols'], listed[0], listed[1], nbt=nbt, nbr=nbr)
    else:
        pattern = kernels.Pattern(spec['mesh_nelems'], spec['nrows'], spec['ncols'], test._keep[1], trial._keep[1], nbt=nbt, nbr=nbr, toff=test._keep[2], roff=trial._keep[2])
    value, mag, rowptr, colidx = ref
    rp, ci = pattern.expand(spec['nct'], spec['ncr'], spec['mask'])
    assert numpy.array_equal(device.to_host(rp), rowptr) and numpy.array_equal(device.to_host(ci), colidx)
    terms = spec['terms']
    kw = dict(ndims=spec['ndims'], nq=spec['nq'], weights=dev.weights, geom=dev.geom, test=test, trial=trial, nct=spec['nct'], ncr=spec['ncr'], C=terms[0]['C'],
              mask=spec['mask'], pattern=pattern, fused=False)
    if len(terms) > 1:  # per-point tensors cq[e][q] = sum_t scale_t[e][q] C_t
        kw['cq'] = device.to_dev(sum(numpy.asarray(t['scale'])[:, :, None, None, None, None] * numpy.asarray(t['C']) for t in terms), 'float64')
    elif terms[0].get('scale') is not None:
        kw['scale'] = device.to_dev(terms[0]['scale'], 'float64')
    store, results = bool(run.get('store')), []
    for _ in range(2 if run.get('repeat') else 1):
        before = record()[0]
        if run.get('colours'):
            first_touch = (spec['shape'], round(nbt ** (1 / spec['ndims']))) if run['colours'] == 'first_touch' else None
            values = nan_or_zeros(len(colidx), first_touch is not None)
            lists = gc.colours(spec['shape'])
            for el in lists:
                kernels.assemble_matrix(nelems=len(el), elist=device.to_dev(el, 'int32'), flags=gc.EXCLUSIVE | gc.BY_ELEMENT, first_touch=first_touch, gather=False,
                                        values=values, **kw)
            launches = len(lists)
            assert launches == run['launches']
        else:
            values = nan_or_zeros(len(colidx), store)
            kernels.assemble_matrix(nelems=spec['nelems'], elist=dev.elist, flags=run.get('flags', 0), gather=bool(run.get('gather')), store=store, values=values, **kw)
            launches = gc.size_classes(spec) if run.get('launches') == 'size classes' else 1
        results.append(device.to_host(values))
        check_record(before, run, launches)
    ratio = worst(results[0], value, mag, g)  # (finite everywhere: no NaN of a prefill survives; magnitude zero: exactly zero)
    print(f'{family} {name}: m = {m}, largest err/bound = {ratio:.2e}')
    assert ratio <= 1
    if run.get('repeat'):
        assert results[0].tobytes() == results[1].tobytes()


@pytest.mark.parametrize('name', list(gc.MFMA))
def test_k_matrix_mfma(name, monkeypatch):
    '''m = generic_refs.m_mfma: D on both sides (2 (Jinv + nd)), w |det| (det + 1, a scale array one more), the B operand (S + 1), one fused multiply-add per k index
    of the matrix pipe (active slots x points padded to 4), the contributions of the elements of an entry.  The record names the instantiation <ND, MT>, the N tiles,
    the k-steps and the active test slots.'''
    run_matrix('k_matrix_mfma', name, monkeypatch)


@pytest.mark.parametrize('name', list(gc.GENERIC))
def test_k_matrix_generic(name, monkeypatch):
    '''m = generic_refs.m_generic, the longest of the branches (entries with and without the W table, scalar symmetric, Gram, Gram symmetric), one addition per
    contribution and chunk of points.  The record names the branch, the waves per element, the W table, the chunk and the symmetry the launcher found; the cases
    `declined-*` carry no NH_MATRIX_NO_MFMA: the launcher itself must decline the MFMA kernel.'''
    run_matrix('k_matrix_generic', name, monkeypatch)


@pytest.mark.parametrize('name', list(gc.GRAM_SYM))
def test_k_gram_sym(name, monkeypatch):
    '''NH_MATRIX_GATHER | NH_MATRIX_STORE into NaN-filled values, twice with identical bytes.  m = generic_refs.m_gram_sym.  The record names E, W, NC, USE0 and
    TRI; the cases `declined-*` must go to k_matrix_generic's branches with the scratch instead.'''
    run_matrix('k_gram_sym', name, monkeypatch)


@pytest.mark.parametrize('name', list(gc.VECTOR))
def test_k_vector_generic(name):
    '''nh_assemble_vector with one field, one block, a C and an f term.  m = generic_refs.m_vector_generic.  `local`: the local vectors are stored and nothing is added
    into out; `functional`: out_scalar against 1/2 u . r_C + u . r_f of the restatement.'''
    from nutils_amd import device, kernels
    family = 'k_vector_generic'
    spec, run = gc.build(family, name)
    (value, mag, lvalue, lmag), = gc.reference(family, name)
    m, g = gc.gamma_m(spec, run)
    dev = Device(spec)
    blk, (fbasis, u, ncr) = spec['blocks'][0], dev.fields[0]
    c, = [t for t in spec['terms'] if t.get('C') is not None]
    f, = [t for t in spec['terms'] if t.get('C') is None]
    out = device.zeros(blk['nrows'] * blk['nct'], 'float64')
    local = nan_or_zeros(len(numpy.asarray(blk['basis']['dofs']).reshape(-1)) * blk['nct'], True) if blk.get('local') else None
    scalar = device.zeros(1, 'float64') if spec.get('functional') else None
    before = record()[0]
    kernels.assemble_vector(nelems=spec['nelems'], ndims=spec['ndims'], nq=spec['nq'], weights=dev.weights, geom=dev.geom, test=dev.basis(blk['basis']), trial=fbasis,
                            nct=blk['nct'], ncr=ncr, C=c['C'], f=f['f'], u=u, out=out, out_scalar=scalar, elist=dev.elist,
                            scale=None if c.get('scale') is None else device.to_dev(c['scale'], 'float64'), local=local)
    check_record(before, run, 1)
    if local is not None:
        assert not device.to_host(out).any()
        ratio = worst(device.to_host(local), lvalue, lmag, g)
    else:
        ratio = worst(device.to_host(out), value, mag, g)
        if scalar is not None:
            fvalue, fmag = gc.functional_reference(family, name)
            ratio = max(float(abs(numpy.longdouble(device.to_host(scalar)[0]) - fvalue) / (g * fmag)), worst(device.to_host(out), value, mag, gc.tr.gamma(gc.gamma_m(dict(spec, functional=False), run)[0])))
    print(f'{family} {name}: m = {m}, largest err/bound = {ratio:.2e}')
    assert ratio <= 1
