'''Host checks of the trilinear 3-D write-once path (nh_assemble_hex1.hip, sample._hex1_form): the closed-form nnz against the oracle's assembled
pattern, and the recogniser's accept / decline decision -- neither needs a device.'''
import numpy
import pytest


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 5), (5, 1, 1), (2, 3, 4), (7, 2, 3)])
def test_nnz_matches_the_oracle_pattern(shape):
    from nutils_amd import kernels
    from oracle import assemble as oa
    dofs, coeffs, ndofs = oa.structured_basis(shape, 'std', 1)
    values, rowptr, colidx = oa.assemble_csr(numpy.ones((len(dofs), 8, 1, 8, 1)), dofs, dofs, ndofs, ndofs)
    for nc in (1, 2, 3):
        assert kernels.hex1_nnz(shape, nc) == len(colidx) * nc * nc


def _elasticity(domain, g, nc=3, degree=2):
    from nutils_amd import function
    u = domain.field('u', btype='std', degree=1, shape=[nc])
    v = domain.field('v', btype='std', degree=1, shape=[nc])
    eps = lambda w: function.symgrad(w, g)
    res = domain.integral(function.inner(eps(v), function.div(u, g) * function.eye(nc) + 1.3 * eps(u)) * function.J(g), degree=degree)
    return function.derivative(function.derivative(res, 'v'), 'u')


def _vector_mass(domain, g, nc, degree):
    from nutils_amd import function
    u = domain.field('u', btype='std', degree=1, shape=[nc])
    v = domain.field('v', btype='std', degree=1, shape=[nc])
    return function.derivative(function.derivative(domain.integral(function.inner(v, u) * function.J(g), degree=degree), 'v'), 'u')


ANISO = numpy.array([[2., .3, .1], [.3, 1., -.2], [.1, -.2, 1.5]])


def form_tensor(form, nc):
    '''the constant tensor C [nc][4][nc][4] of the 'dense' (random, value slots included) and 'aniso' (full diffusion tensor) forms'''
    if form == 'aniso':
        C = numpy.zeros((1, 4, 1, 4))
        C[0, 1:, 0, 1:] = ANISO
        return C
    return numpy.random.default_rng(nc).normal(size=(nc, 4, nc, 4))


def with_tensor(f, C):
    '''the terms of a one-term matrix integral with its tensor replaced by C'''
    (smp, itg, fac), = f.terms
    return [(smp, itg._copy(B=C), 1.)]


def _plan(shape=(3, 4, 2), geom='rect', form='elasticity', periodic=(), nc=3, degree=2):
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
        verts = numpy.stack(numpy.meshgrid(*[numpy.arange(n + 1.) for n in shape], indexing='ij'), -1).reshape(-1, 3)
        g = domain.basis('std', degree=1) @ (verts + numpy.random.default_rng(0).uniform(-.2, .2, verts.shape))
    dV = function.J(g)
    basis = domain.basis('std', degree=1)
    if form == 'elasticity':
        f = _elasticity(domain, g, nc, degree)
    elif form in ('dense', 'aniso'):  # a dense random constant tensor with value slots / a full diffusion tensor: the elasticity / Laplace terms, re-weighted
        return S._MatrixPlan(with_tensor(_vector_mass(domain, g, nc, degree) if form == 'dense' else
                                         domain.integral(function.outer(function.grad(basis, g)).sum(-1) * dV, degree=degree), form_tensor(form, nc)))
    elif form == 'laplace':
        f = domain.integral(function.outer(function.grad(basis, g)).sum(-1) * dV, degree=degree)
    elif form == 'both':
        f = domain.integral((function.outer(function.grad(basis, g)).sum(-1) + function.outer(basis)) * dV, degree=degree)
    elif form == 'vector-laplace':  # block-diagonal C: a masked block pattern
        u = domain.field('u', btype='std', degree=1, shape=[3])
        v = domain.field('v', btype='std', degree=1, shape=[3])
        res = domain.integral(function.inner(function.grad(v, g), function.grad(u, g)) * dV, degree=degree)
        f = function.derivative(function.derivative(res, 'v'), 'u')
    elif form == 'coefficient':
        f = _elasticity(domain, g, 3, degree)
        (smp, itg, fac), = f.terms
        return S._MatrixPlan([(smp, itg.with_scale(function.PointFunc(lambda x: 1 + x[:, 0] ** 2, g)), fac)])
    elif form == 'field':
        u = domain.field('u', btype='std', degree=1)
        nrg = domain.integral((.25 * function.value(u) ** 4 + .5 * (function.grad(u, g) * function.grad(u, g)).sum(-1)) * dV, degree=degree)
        f = function.derivative(function.derivative(nrg, 'u'), 'u')
    elif form == 'two-geometries':
        g2 = mesh.rectilinear([numpy.linspace(0, 2, n + 1) for n in shape])[1]
        f = _elasticity(domain, g) + _elasticity(domain, g2)
    elif form == 'boundary':
        u = domain.field('u', btype='std', degree=1, shape=[3])
        v = domain.field('v', btype='std', degree=1, shape=[3])
        res = domain.boundary['left'].integral(function.inner(v, u) * dV, degree=degree)
        f = function.derivative(function.derivative(res, 'v'), 'u')
    return S._MatrixPlan(f.terms)


@pytest.fixture
def all_modes(monkeypatch):
    '''the recogniser for every (mode, components) of the class (by default sample.HEX1_ROUTED)'''
    from nutils_amd import sample
    monkeypatch.setattr(sample, 'HEX1_ROUTED', sample.HEX1_ALL)


@pytest.mark.usefixtures('all_modes')
@pytest.mark.parametrize('geom,mode', [('iso', 'iso'), ('rect', 'uniform'), ('graded', 'box')])
def test_recogniser_accepts_elasticity(geom, mode):
    from nutils_amd import sample as S
    for degree in (2, 4):  # (2^3 and 3^3 Gauss points)
        out = S._hex1_form(_plan(geom=geom, degree=degree))
        assert out is not None and out[2] == mode and out[0].shape == (3, 4, 3, 4)
        assert not out[0][:, 0].any() and not out[0][:, :, :, 0].any()


@pytest.mark.usefixtures('all_modes')
def test_recogniser_switches(monkeypatch):
    from nutils_amd import sample as S
    monkeypatch.setenv('NUTILS_AMD_NO_UNIFORM', '1')
    assert S._hex1_form(_plan())[2] == 'box'
    monkeypatch.setenv('NUTILS_AMD_NO_FAST_PATH', '1')
    assert S._hex1_form(_plan()) is None


@pytest.mark.usefixtures('all_modes')
@pytest.mark.parametrize('nc', [2, 3])
def test_recogniser_accepts_dense_forms(nc):
    from nutils_amd import sample as S
    out = S._hex1_form(_plan(geom='iso', form='dense', nc=nc))
    assert out is not None and out[0].shape == (nc, 4, nc, 4) and out[0][:, 0, :, 0].any() and out[0][:, 1:, :, 1:].any()


@pytest.mark.usefixtures('all_modes')
def test_recogniser_accepts_anisotropic_scalar_forms():
    from nutils_amd import sample as S
    for geom in ('iso', 'rect'):
        out = S._hex1_form(_plan(geom=geom, form='aniso'))
        assert out is not None and out[0].shape == (1, 4, 1, 4)
        assert out[0][0, 1, 0, 2] == .3


@pytest.mark.usefixtures('all_modes')
@pytest.mark.parametrize('kw', [dict(form='laplace'), dict(form='both'), dict(form='laplace', geom='iso'), dict(form='both', degree=4), dict(periodic=(1,)),
                                dict(form='boundary'), dict(form='vector-laplace'), dict(form='coefficient'), dict(form='field'), dict(form='two-geometries'),
                                dict(geom='flat')],
                         ids=['laplace', 'laplace+mass', 'laplace-iso', 'laplace+mass-27', 'periodic', 'boundary', 'masked', 'coefficient', 'field', 'two-geometries',
                              'flat'])
def test_recogniser_declines(kw):
    from nutils_amd import sample as S
    try:
        plan = _plan(**kw)
    except NotImplementedError:
        return  # (not even a plan of one sample)
    assert S._hex1_form(plan) is None


def test_default_routing():
    '''by default: equidistant cells with 1 or 3 components take the new path; isoparametric and graded cells stay generic (sample.HEX1_ROUTED)'''
    from nutils_amd import sample as S
    assert set(S.HEX1_ROUTED) <= set(S.HEX1_ALL) and len(S.HEX1_ALL) == 9
    assert S._hex1_form(_plan(geom='rect'))[2] == 'uniform'
    assert S._hex1_form(_plan(geom='rect', form='aniso'))[2] == 'uniform'
    for kw in (dict(geom='iso'), dict(geom='graded'), dict(geom='iso', form='aniso'), dict(geom='rect', form='dense', nc=2)):
        assert S._hex1_form(_plan(**kw)) is None, kw
