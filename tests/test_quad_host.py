'''Host checks of the structured 2-D write-once path (nh_assemble_quad.hip, sample._quad_form): the closed-form nnz against the oracle's assembled
pattern, and the recogniser's accept / decline decision -- neither needs a device.'''
import numpy
import pytest

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (7, 3)]
BASES = [('std', 1), ('std', 2), ('spline', 2)]


@pytest.mark.parametrize('btype,degree', BASES)
@pytest.mark.parametrize('shape', SHAPES)
def test_nnz_matches_the_oracle_pattern(shape, btype, degree):
    from nutils_amd import kernels
    from oracle import assemble as oa
    dofs, coeffs, ndofs = oa.structured_basis(shape, btype, degree)
    nb = dofs.shape[1]
    values, rowptr, colidx = oa.assemble_csr(numpy.ones((len(dofs), nb, 1, nb, 1)), dofs, dofs, ndofs, ndofs)  # (local matrices [e][m][c][n][d])
    for nc in (1, 2):
        assert kernels.quad_nnz(shape, btype, degree, nc) == len(colidx) * nc * nc


def _plan(shape=(4, 3), btype='std', degree=1, geom='rect', form='laplace', periodic=(), nc=1, sample=None):
    from nutils_amd import mesh, function, sample as S
    if geom == 'graded':
        domain, g = mesh.rectilinear([numpy.linspace(0, 1, n + 1) ** 2 for n in shape])
    elif geom == 'flat':
        axes = [numpy.linspace(0, 1, n + 1) for n in shape]
        axes[0][1] = axes[0][0]
        domain, g = mesh.rectilinear(axes)
    else:
        domain, g = mesh.rectilinear(list(shape), periodic=periodic)
    if geom == 'iso':
        g = domain.basis('std', degree=1) @ numpy.random.default_rng(0).uniform(size=(numpy.prod([n + 1 for n in shape]), 2))
    dV = function.J(g)
    if nc == 2:
        u = domain.field('u', btype=btype, degree=degree, shape=[2])
        v = domain.field('v', btype=btype, degree=degree, shape=[2])
        eps = lambda w: function.symgrad(w, g)
        res = domain.integral(function.inner(eps(v), function.div(u, g) * function.eye(2) + eps(u)) * dV, degree=2 * degree)
        return S._MatrixPlan(function.derivative(function.derivative(res, 'v'), 'u').terms)
    basis = domain.basis(btype, degree=degree)
    other = domain.basis('std', degree=2) if btype != 'std' or degree != 2 else domain.basis('std', degree=1)
    smp = domain.sample('gauss', 2 * degree) if sample is None else (domain.boundary['left'].sample('gauss', 2) if sample == 'boundary' else sample)
    if form == 'laplace':
        f = function.outer(function.grad(basis, g)).sum(-1) * dV
    elif form == 'both':
        f = function.outer(function.grad(basis, g)).sum(-1) * dV + function.outer(basis) * dV
    elif form == 'coefficient':
        f = function.outer(function.grad(basis, g)).sum(-1) * function.PointFunc(lambda x: 1 + x[:, 0] ** 2, g) * dV
    elif form == 'field':
        u = domain.field('u', btype=btype, degree=degree)
        nrg = domain.integral((.25 * function.value(u) ** 4 + .5 * (function.grad(u, g) * function.grad(u, g)).sum(-1)) * dV, degree=2 * degree)
        return S._MatrixPlan(function.derivative(function.derivative(nrg, 'u'), 'u').terms)
    elif form == 'mixed':
        f = function.outer(basis, other) * dV
    if sample == 'boundary':
        return S._MatrixPlan(domain.boundary['left'].integral(f, degree=2).terms)
    return S._MatrixPlan(smp.integral(f).terms)


@pytest.mark.parametrize('btype,degree', BASES)
@pytest.mark.parametrize('geom,mode', [('rect', 'uniform'), ('iso', 'iso'), ('graded', 'box')])
def test_recogniser_accepts(btype, degree, geom, mode, monkeypatch):
    from nutils_amd import sample as S
    if geom != 'rect' and (btype, degree) != ('std', 1):
        assert S._quad_form(_plan(btype=btype, degree=degree, geom=geom)) is None  # (by default: generic path, see sample.QUAD_GEOMETRIC_BASES)
        monkeypatch.setattr(S, 'QUAD_GEOMETRIC_BASES', S.QUAD_BASES)
    for form in ('laplace', 'both'):
        out = S._quad_form(_plan(btype=btype, degree=degree, geom=geom, form=form))
        assert out is not None and out[2] == mode and out[0].shape == (1, 3, 1, 3)
    out = S._quad_form(_plan(btype=btype, degree=degree, geom=geom, nc=2))
    assert out is not None and out[0].shape == (2, 3, 2, 3)


def test_recogniser_switches(monkeypatch):
    from nutils_amd import sample as S
    monkeypatch.setenv('NUTILS_AMD_NO_UNIFORM', '1')
    assert S._quad_form(_plan())[2] == 'box'
    monkeypatch.setenv('NUTILS_AMD_NO_FAST_PATH', '1')
    assert S._quad_form(_plan()) is None


@pytest.mark.parametrize('kw', [dict(periodic=(1,), degree=2), dict(sample='boundary'), dict(form='coefficient'), dict(form='field'),
                                dict(form='mixed'), dict(geom='flat'), dict(btype='std', degree=3), dict(btype='spline', degree=1)],
                         ids=['periodic', 'boundary', 'coefficient', 'field', 'mixed', 'flat', 'p3', 'spline1'])
def test_recogniser_declines(kw):
    from nutils_amd import sample as S
    try:
        plan = _plan(**kw)
    except NotImplementedError:
        return  # (not even a plan of one sample)
    assert S._quad_form(plan) is None


def test_one_sample_serves_several_bases():
    '''the premise of the launcher key (sample._MatrixPlan._quad): bases integrated at one degree share the sample and the geometry'''
    from nutils_amd import mesh, function, sample as S
    domain, geom = mesh.rectilinear([8, 8])
    plans = [S._MatrixPlan(domain.integral(function.outer(function.grad(domain.basis(bt, degree=p), geom)).sum(-1) * function.J(geom), degree=4).terms)
             for bt, p in (('std', 2), ('spline', 2), ('std', 1))]
    assert len({id(p.smp0) for p in plans}) == 1
    assert len({S._quad_form(p)[1] is geom for p in plans}) == 1
