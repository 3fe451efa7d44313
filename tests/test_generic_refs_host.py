'''On the CPU, for the inputs of tests/test_gpu_generic.py (tests/generic_cases.py): (a) the bound gamma_m x magnitude is not too tight -- a plain float64 evaluation of
the formulas of nh_assemble_matrix / nh_assemble_vector, contracted in another order (einsum, contributions added element by element) and through
oracle.assemble where it applies, stays within it;  (b) it is not vacuous -- every mistake of generic_refs.MUTANTS that a case can show moves some entry by more than
100 bounds, and every mistake is shown by some case;  (c) no entry is left out -- every stored entry of every case is compared, entries of magnitude zero are exactly
zero.'''
import numpy
import pytest

import generic_cases as gc
import generic_refs as gr
import terms_refs as tr

LD = numpy.longdouble
VECTOR_CASES = [('k_vector_generic', n) for n in gc.VECTOR]


# ---- float64, another order ---------------------------------------------------------------------------------------------------------------------------

def geometry64(geom, nd, nq, elems):
    '''(Jinv [n][nq][j][i], |det| [n][nq]) by cofactors in float64'''
    n = len(elems)
    if geom['kind'] == 'box':
        J = numpy.zeros((n, nq, nd, nd))
        J[:, :, range(nd), range(nd)] = numpy.asarray(geom['size'], dtype=float).reshape(-1, nd)[elems][:, None]
    elif geom['kind'] == 'tab':
        J = numpy.asarray(geom['jac'], dtype=float).reshape(-1, nq, nd, nd)[elems]
    else:
        gT = numpy.asarray(geom['gT'], dtype=float).reshape(-1, nq, 1 + nd)
        X = numpy.asarray(geom['verts'], dtype=float).reshape(-1, nd)[numpy.asarray(geom['gdofs']).reshape(-1, len(gT))[elems]]
        J = numpy.einsum('aqj,eai->eqij', gT[:, :, 1:], X)
    if nd == 1:
        det = J[..., 0, 0]
        adj = numpy.ones_like(J)
    elif nd == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        adj = numpy.stack([numpy.stack([J[..., 1, 1], -J[..., 0, 1]], -1), numpy.stack([-J[..., 1, 0], J[..., 0, 0]], -1)], -2)
    else:
        r0, r1, r2 = J[..., 0, :], J[..., 1, :], J[..., 2, :]
        adj = numpy.stack([numpy.cross(r1, r2), numpy.cross(r2, r0), numpy.cross(r0, r1)], -1)
        det = (r0 * adj[..., :, 0]).sum(-1)
    return adj * (1 / det)[..., None, None], numpy.abs(det)


def tables64(basis, nd, nq, elems, Jinv):
    nb = int(tr.basis_sizes(basis, elems[:1])[0])
    fn0, pos0 = tr._first(basis, elems)
    T = numpy.asarray(basis['T'], dtype=float).reshape(-1, nq, 1 + nd)[fn0[:, None] + numpy.arange(nb)]
    D = numpy.concatenate([T[..., :1], numpy.einsum('eqji,enqj->enqi', Jinv, T[..., 1:])], -1)
    return D, numpy.asarray(basis['dofs'], dtype=numpy.int64).reshape(-1)[pos0[:, None] + numpy.arange(nb)], pos0[:, None] + numpy.arange(nb)


def scale64(t, spec, ie, elems):
    if t.get('scale') is None:
        return 1.
    return numpy.asarray(t['scale'], dtype=float).reshape(-1, spec['nq'])[elems if spec.get('by_element') else ie]


def matrix64(spec):
    '''values [nnz] in the layout of terms_refs.matrix_terms'''
    nd, nq, nct, ncr = spec['ndims'], spec['nq'], spec['nct'], spec['ncr']
    mask = numpy.ones((nct, ncr), dtype=bool) if spec.get('mask') is None else numpy.asarray(spec['mask'], dtype=bool).reshape(nct, ncr)
    uniq = tr.pattern_keys(spec)
    out = numpy.zeros(len(uniq))
    w = numpy.asarray(spec['weights'], dtype=float)
    for ie, elems in tr._groups(spec, [spec['test'], spec['trial']]):
        Jinv, meas = geometry64(spec['geom'], nd, nq, elems)
        Dt, tdofs, _ = tables64(spec['test'], nd, nq, elems, Jinv)
        Dr, rdofs, _ = tables64(spec['trial'], nd, nq, elems, Jinv)
        A = 0
        for t in spec['terms']:  # trial side first, then the points, then the test side
            H = numpy.einsum('cadb,enqb->eqcand', numpy.asarray(t['C'], dtype=float), Dr) * (w * meas * scale64(t, spec, ie, elems))[:, :, None, None, None, None]
            A = A + numpy.einsum('emqa,eqcand->emcnd', Dt, H)
        rows = tdofs[:, :, None, None, None] * nct + numpy.arange(nct)[None, None, :, None, None]
        cols = rdofs[:, None, None, :, None] * ncr + numpy.arange(ncr)
        key = numpy.broadcast_to(rows * (spec['ncols'] * ncr) + cols, A.shape)
        keep = numpy.broadcast_to(mask[None, None, :, None, :], A.shape)
        numpy.add.at(out, numpy.searchsorted(uniq, key[keep]), A[keep])
    return out


def vector64(spec):
    '''(out [nrows][nct], functional) of the single block'''
    nd, nq = spec['ndims'], spec['nq']
    blk, F = spec['blocks'][0], spec['fields'][0]
    out, fun = numpy.zeros((blk['nrows'], blk['nct'])), 0.
    w = numpy.asarray(spec['weights'], dtype=float)
    u = numpy.asarray(F['u'], dtype=float).reshape(-1, F['ncomp'])
    for ie, elems in tr._groups(spec, [blk['basis'], F['basis']]):
        Jinv, meas = geometry64(spec['geom'], nd, nq, elems)
        Dt, tdofs, _ = tables64(blk['basis'], nd, nq, elems, Jinv)
        Dr, rdofs, _ = tables64(F['basis'], nd, nq, elems, Jinv)
        U = numpy.einsum('end,enqs->eqds', u[rdofs], Dr)
        for t in spec['terms']:
            Ft = numpy.zeros((len(elems), nq, blk['nct'], 1 + nd))
            if t.get('f') is not None:
                Ft = Ft + numpy.asarray(t['f'], dtype=float)
            if t.get('C') is not None:
                Ft = Ft + numpy.einsum('eqdb,cadb->eqca', U, numpy.asarray(t['C'], dtype=float))
            wq = w * meas * scale64(t, spec, ie, elems)
            numpy.add.at(out, tdofs.reshape(-1), numpy.einsum('eqca,emqa,eq->emc', Ft, Dt, wq).reshape(-1, blk['nct']))
            if spec.get('functional'):
                fun += (.5 if t.get('C') is not None else 1.) * numpy.einsum('eq,eqca,eqca->', wq, U, Ft)
    return out, fun


def ratio(got, value, mag, g):
    '''largest |got - value| / (g magnitude) over ALL entries; entries of magnitude zero must be exactly zero'''
    got, value, mag = LD(numpy.asarray(got)).reshape(-1), value.reshape(-1), mag.reshape(-1)
    assert got.shape == value.shape == mag.shape
    err = numpy.abs(got - value)
    assert (err[mag == 0] == 0).all() and (value[mag == 0] == 0).all()
    return float((err[mag > 0] / (g * mag[mag > 0])).max()), int((mag > 0).sum() + (mag == 0).sum())


# ---- (a) and (c) ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family,name', gc.MATRIX_CASES)
def test_float64_in_another_order_is_within_the_bound(family, name):
    spec, run = gc.build(family, name)
    value, mag, rowptr, colidx = gc.reference(family, name)
    m, g = gc.gamma_m(spec, run)
    assert len(value) == len(colidx) == rowptr[-1] and numpy.array_equal(tr.pattern_keys(spec) % (spec['ncols'] * spec['ncr']), colidx)
    r, compared = ratio(matrix64(spec), value, mag, g)
    assert compared == len(colidx)  # (c): every stored entry
    assert r <= 1, (m, r)
    if spec.get('elist') is not None and not spec.get('by_element'):  # the pattern of the listed elements leaves out entries without a contribution only
        v2, m2, rp2, ci2 = gc.list_pattern(spec, (value, mag, rowptr, colidx))
        assert len(v2) == len(ci2) == rp2[-1] and (m2 > 0).sum() == (mag > 0).sum()


@pytest.mark.parametrize('family,name', VECTOR_CASES)
def test_float64_vector_in_another_order_is_within_the_bound(family, name):
    spec, run = gc.build(family, name)
    (value, mag, _, _), = gc.reference(family, name)
    m, g = gc.gamma_m(spec, run)
    out, fun = vector64(spec)
    if spec.get('functional'):
        fvalue, fmag = gc.functional_reference(family, name)
        assert fmag > 0 and abs(LD(fun) - fvalue) <= g * fmag
        g = tr.gamma(gc.gamma_m(dict(spec, functional=False), run)[0])
    r, compared = ratio(out, value, mag, g)
    assert compared == value.size and r <= 1, (m, r)


SCALAR_GOLDEN = ['lap2d_p1_4x3_iso', 'lap2d_p2_3x4_iso', 'lap3d_p2_2_iso', 'lap3d_p1_234']


@pytest.mark.parametrize('name', SCALAR_GOLDEN)
def test_oracle_assembly_is_within_the_bound(name):
    '''K + 2.5 M of the golden fixtures as ONE kind-0 term through oracle.assemble (local matrices by einsum, scatter in the reference's order) against the
    restatement, within the bounds of all three matrix kernels (the smallest count decides)'''
    import os
    from oracle import assemble as oa
    from test_terms_refs_host import golden_spec, GOLDEN
    g = dict(numpy.load(os.path.join(GOLDEN, name + '.npz')))
    spec, B = golden_spec(g)
    nd = spec['ndims']
    C = oa.laplace_coefficient(nd) + 2.5 * oa.mass_coefficient(nd)
    mat = dict(spec, fields=[], test=B, trial=B, nct=1, ncr=1, mask=None, nrows=B['ndofs'], ncols=B['ndofs'], by_element=False, terms=[dict(kind=0, C=C)])
    value, mag, rowptr, colidx = tr.matrix_terms(mat)
    N, dN = oa.tabulate(g['coeffs'].reshape(spec['nelems'], B['nb'], -1), g['gauss_coords'])
    ne = spec['nelems']
    dofs = g['dofs'].reshape(ne, -1)
    if int(g['iso']):
        gN, gdN = oa.tabulate(g['gcoeffs'][None, :2 ** nd], g['gauss_coords'])
        _, J = oa.geometry_iso(g['verts'], g['gdofs'].reshape(ne, -1), gN, gdN)
    else:
        J = numpy.broadcast_to(numpy.eye(nd), (ne, len(g['gauss_weights']), nd, nd))
    D, det = oa.physical_tables(N, dN, J)
    vo, rpo, cio = oa.assemble_csr(oa.local_matrices(D, D, det * g['gauss_weights'], C), dofs, dofs, B['ndofs'], B['ndofs'])
    assert numpy.array_equal(rpo, rowptr) and numpy.array_equal(cio, colidx)
    common = dict(nd=nd, nq=spec['nq'], ngb=spec['geom'].get('ngb', 0), contributions=gc.contributions(B))
    m = min(gr.m_generic(**common), gr.m_mfma(nas=1 + nd, **common), gr.m_gram_sym(**common))
    assert ratio(vo, value, mag, tr.gamma(m))[0] <= 1


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family,name', gc.MATRIX_CASES)
def test_mutants_are_far_outside_the_bound(family, name):
    spec, run = gc.build(family, name)
    value, mag, _, _ = gc.reference(family, name)
    g = gc.gamma_m(spec, run)[1]
    for mutant in gr.MUTANTS:
        if not gr.applies(spec, mutant, run):
            continue
        mut = gr.mutant_matrix(spec, mutant, run.get('qchunk'))
        r = float((numpy.abs(mut - value)[mag > 0] / (g * mag[mag > 0])).max())
        assert r > 100, (mutant, r)


def test_every_mutant_is_shown_by_some_case():
    cases = [gc.build(family, name) for family, name in gc.MATRIX_CASES]
    for mutant in gr.MUTANTS:
        assert any(gr.applies(spec, mutant, run) for spec, run in cases), mutant


def test_every_kernel_family_and_branch_has_a_case():
    '''what the issue's tables ask of the launch record: the five MFMA instantiations, the four branches of k_matrix_generic chunked and not with 1 and 2 waves (one
    shape with 4), E = 1 .. 4 of k_gram_sym with NC = 1 and 2, USE0 and TRI both ways'''
    runs = [gc.build(family, name)[1] for family, name in gc.MATRIX_CASES]
    mf = {(r['expect']['ND'], r['expect']['MT']) for r in runs if r['family'] == 'k_matrix_mfma'}
    assert mf == {(2, 1), (2, 2), (3, 1), (3, 2), (3, 4)}
    ge = [r['expect'] for r in runs if r['family'] == 'k_matrix_generic' and 'qchunk' in r['expect']]
    for branch in ('entries', 'scalar_symmetric', 'gram', 'gram_symmetric'):
        for waves in (1, 2):
            assert any(e['branch'] == branch and e['waves'] == waves for e in ge), (branch, waves)
        assert any(e['branch'] == branch and r.get('qchunk') for r in runs for e in [r['expect']] if r['family'] == 'k_matrix_generic'), branch
    assert any(e['waves'] == 4 for e in ge) and {e['use_w'] for e in ge} == {0, 1}
    gs = [r['expect'] for r in runs if r['family'] == 'k_gram_sym']
    assert {(e['E'], e['NC']) for e in gs} == {(E, NC) for E in (1, 2, 3, 4) for NC in (1, 2)}
    assert {e['USE0'] for e in gs} == {0, 1} and {e['TRI'] for e in gs} == {0, 1}
