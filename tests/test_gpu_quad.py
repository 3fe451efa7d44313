'''The structured 2-D write-once path (nh_assemble_quad.hip): closed-form pattern, the reference fixtures through the front end, full-size
meshes against the generic path (NUTILS_AMD_NO_FAST_PATH=1), the uniform-cell replication, the forms it declines, and singular Jacobians.'''
import os

import numpy
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-13
BASES = [('std', 1), ('std', 2), ('spline', 2)]


def close(a, b, scale=None):
    a, b = numpy.asarray(a), numpy.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = numpy.abs(b).max() if scale is None else scale
    err = numpy.abs(a - b).max()
    assert err <= RTOL * max(s, 1e-300), err / s


@pytest.fixture(autouse=True)
def all_bases(monkeypatch):
    '''the kernel for every basis of the class on every geometry (by default the biquadratic and spline bases on non-uniform cells stay generic)'''
    from nutils_amd import sample
    monkeypatch.setattr(sample, 'QUAD_GEOMETRIC_BASES', sample.QUAD_BASES)


@pytest.fixture
def env(monkeypatch):
    def set_(**kw):
        for k, v in kw.items():
            if v:
                monkeypatch.setenv(k, '1')
            else:
                monkeypatch.delenv(k, raising=False)
    return set_


def csr(f, arguments=None):
    from nutils_amd import function, _lib
    with _lib.trace() as calls:
        out = function.eval(function.as_csr(f), arguments or {})
    return out, list(calls)


@pytest.mark.parametrize('btype,degree', BASES)
@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (2, 2), (7, 3), (3, 64), (130, 97)])
def test_pattern(shape, btype, degree):
    from nutils_amd import mesh, device, kernels
    domain, _ = mesh.rectilinear(list(shape))
    b = domain.basis(btype, degree=degree)
    smp = domain.sample('gauss', 2)
    for nc in (1, 2):
        rp, ci = kernels.quad_pattern(shape, btype, degree, nc)
        rp0, ci0 = smp.pattern(b, b).expand(nc, nc, None)
        rp, ci, rp0, ci0 = (device.to_host(a) for a in (rp, ci, rp0, ci0))
        assert rp.dtype == ci.dtype == numpy.int64
        assert numpy.array_equal(rp, rp0) and numpy.array_equal(ci, ci0)


def _setup(g):
    from nutils_amd import mesh
    domain, geom = mesh.rectilinear([int(n) for n in g['shape']])
    if int(g['iso']):
        geom = domain.basis('std', degree=1) @ g['verts']
    return domain, geom


def _quad_ran(calls):
    return any(c in ('nh_quad_matrix', 'nh_quad_rows_uniform') for c in calls) and not any(c.startswith('nh_assemble_matrix') for c in calls)


@pytest.mark.parametrize('name,btype', [('lap2d_p1_4x4', 'std'), ('lap2d_p1_4x3_iso', 'std'), ('lap2d_p2_3x4_iso', 'std'), ('lap2d_spline2_4x4', 'spline'),
                                        ('lap2d_spline2_5x4_iso', 'spline')])
def test_scalar_fixtures(golden, name, btype):
    from nutils_amd import function
    g = golden(name)
    domain, geom = _setup(g)
    basis = domain.basis(btype, degree=int(g['degree']))
    smp = domain.sample('gauss', 2 * int(g['degree']))
    dV = function.J(geom)
    K = smp.integral(function.outer(function.grad(basis, geom)).sum(-1) * dV)
    M = smp.integral(function.outer(basis) * dV)
    for f, expect in ((K, g['K_values']), (M, g['M_values']), (K + M, None)):
        (v, rp, ci), calls = csr(f)
        assert _quad_ran(calls), calls
        assert numpy.array_equal(rp, g['K_rowptr']) and numpy.array_equal(ci, g['K_colidx'])
        if expect is None:
            close(v, g['K_values'] + g['M_values'], numpy.abs(g['K_values']).max())
        else:
            close(v, expect)


@pytest.mark.parametrize('name', ['elast2d_p1_3x3', 'elast2d_p2_3x2_iso'])
def test_elasticity_fixtures(golden, name):
    from nutils_amd import function
    g = golden(name)
    degree = int(g['degree'])
    domain, geom = _setup(g)
    u = domain.field('u', btype='std', degree=degree, shape=[2])
    v = domain.field('v', btype='std', degree=degree, shape=[2])
    lam, mu = float(g['lam']), float(g['mu'])
    eps = lambda w: function.symgrad(w, geom)
    res = domain.integral(function.inner(eps(v), lam * function.div(u, geom) * function.eye(2) + 2 * mu * eps(u)) * function.J(geom), degree=2 * degree)
    mass = domain.integral(function.inner(v, u) * function.J(geom), degree=2 * degree)
    K = function.derivative(function.derivative(res, 'v'), 'u')
    for f in (K, K + function.derivative(function.derivative(mass, 'v'), 'u')):
        (vals, rp, ci), calls = csr(f)
        assert _quad_ran(calls), calls
        assert numpy.array_equal(rp, g['K_rowptr']) and numpy.array_equal(ci, g['K_colidx'])
        if f is K:
            close(vals, g['K_values'])


FULL = [([2048] * 2, 'std', 1, 1), ([1024] * 2, 'std', 2, 1), ([1024] * 2, 'spline', 2, 1), ([1024] * 2, 'std', 1, 2), ([512] * 2, 'std', 2, 2)]


def full_form(shape, btype, degree, nc, uniform=False):
    from nutils_amd import workloads
    return workloads.quad_form(shape, btype, degree, nc, uniform)


@pytest.mark.parametrize('shape,btype,degree,nc', FULL, ids=['p1_2048', 'p2_1024', 'spline2_1024', 'p1_elast_1024', 'p2_elast_512'])
def test_full_size_against_generic(env, shape, btype, degree, nc):
    import torch
    f = full_form(shape, btype, degree, nc)
    (v1, rp, ci), calls = csr(f)
    assert _quad_ran(calls), calls
    (v2, _, _), _ = csr(f)
    assert numpy.array_equal(v1, v2)  # bit-identical re-assembly
    env(NUTILS_AMD_NO_FAST_PATH=True)
    (v0, rp0, ci0), calls = csr(f)
    assert not any(c.startswith('nh_quad') for c in calls)
    assert numpy.array_equal(rp, rp0) and numpy.array_equal(ci, ci0)
    close(v1, v0)
    del v0, v1, v2
    torch.cuda.empty_cache()


@pytest.mark.parametrize('shape,btype,degree,nc', [([300, 257], 'std', 1, 1), ([67, 70], 'spline', 2, 2), ([9, 12], 'std', 2, 2), ([6, 4], 'spline', 2, 1)])
def test_uniform(env, shape, btype, degree, nc):
    f = full_form(shape, btype, degree, nc, uniform=True)
    (v1, rp, ci), calls = csr(f)
    assert 'nh_quad_rows_uniform' in calls and not any(c.startswith('nh_assemble_matrix') for c in calls), calls
    env(NUTILS_AMD_NO_UNIFORM=True)
    (v2, rp2, ci2), calls = csr(f)
    assert 'nh_quad_matrix' in calls and 'nh_quad_rows_uniform' not in calls
    assert numpy.array_equal(rp, rp2) and numpy.array_equal(ci, ci2)
    close(v1, v2)
    env(NUTILS_AMD_NO_FAST_PATH=True)
    (v0, _, _), _ = csr(f)
    close(v1, v0)


def _decline_cases(golden):
    from nutils_amd import mesh, function
    g = golden('lap2d_p2_4x3_per1')
    domain, geom = mesh.rectilinear([int(n) for n in g['shape']], periodic=tuple(int(i) for i in g['periodic']))
    basis = domain.basis('std', degree=2)
    yield 'periodic', domain.integral(function.outer(function.grad(basis, geom)).sum(-1) * function.J(geom), degree=4), None
    domain, geom = mesh.rectilinear([5, 4])
    basis = domain.basis('std', degree=1)
    dV = function.J(geom)
    yield 'boundary', domain.boundary['left'].integral(function.outer(basis) * dV, degree=2), None
    yield 'coefficient', domain.integral(function.outer(function.grad(basis, geom)).sum(-1) * function.PointFunc(lambda x: 1 + x[:, 0] ** 2, geom) * dV, degree=2), None
    u = domain.field('u', btype='std', degree=1)
    nrg = domain.integral((.25 * function.value(u) ** 4 + .5 * (function.grad(u, geom) * function.grad(u, geom)).sum(-1)) * dV, degree=4)
    yield 'field', function.derivative(function.derivative(nrg, 'u'), 'u'), {'u': numpy.linspace(1, 2, len(basis))}
    yield 'mixed', domain.integral(function.outer(basis, domain.basis('std', degree=2)) * dV, degree=4), None


def test_declines(golden, env):
    from nutils_amd import mesh, function
    for name, f, args in _decline_cases(golden):
        (v, rp, ci), calls = csr(f, args)
        assert not any(c.startswith('nh_quad') for c in calls), name
        env(NUTILS_AMD_NO_FAST_PATH=True)
        (v0, rp0, ci0), _ = csr(f, args)
        env(NUTILS_AMD_NO_FAST_PATH=False)
        assert numpy.array_equal(rp, rp0) and numpy.array_equal(ci, ci0), name
        close(v, v0)
    g = golden('lap2d_p1_singular')
    domain, geom = mesh.rectilinear([g[f'coords{i}'] for i in range(2)])
    basis = domain.basis('std', degree=1)
    (v, rp, ci), calls = csr(domain.integral(function.outer(function.grad(basis, geom)).sum(-1) * function.J(geom), degree=2))
    assert not any(c.startswith('nh_quad') for c in calls)
    bad = numpy.isnan(g['K_values'])
    assert numpy.array_equal(numpy.isnan(v), bad)
    close(v[~bad], g['K_values'][~bad])


def test_singular_jacobian(env):
    '''one quadrilateral collapsed to a point (det J = 0 at every point) in an isoparametric mesh'''
    from nutils_amd import mesh, function
    shape = (6, 5)
    domain, _ = mesh.rectilinear(list(shape))
    verts = numpy.stack(numpy.meshgrid(*[numpy.arange(n + 1.) for n in shape], indexing='ij'), -1) - 2.5
    verts[2:4, 2:4] = 0.  # (element (2, 2) collapsed to its centre, the origin: J = 0 exactly on both paths; its neighbours stay convex)
    geom = domain.basis('std', degree=1) @ verts.reshape(-1, 2)
    for btype, degree in BASES:
        basis = domain.basis(btype, degree=degree)
        f = domain.integral(function.outer(function.grad(basis, geom)).sum(-1) * function.J(geom), degree=2 * degree)
        (v, rp, ci), calls = csr(f)
        assert _quad_ran(calls), calls
        env(NUTILS_AMD_NO_FAST_PATH=True)
        (v0, rp0, ci0), _ = csr(f)
        env(NUTILS_AMD_NO_FAST_PATH=False)
        bad = numpy.isnan(v0)
        assert bad.any() and numpy.array_equal(numpy.isnan(v), bad) and numpy.array_equal(ci, ci0)
        close(v[~bad], v0[~bad])


def test_default_routing(monkeypatch):
    '''by default: bilinear on any geometry and every basis on uniform cells take the new kernels; biquadratic / spline isoparametric meshes stay generic'''
    from nutils_amd import sample
    monkeypatch.setattr(sample, 'QUAD_GEOMETRIC_BASES', (('std', 1),))
    for (btype, degree, nc), uniform, expect in [(('std', 1, 1), False, True), (('std', 1, 2), False, True), (('std', 2, 1), False, False),
                                                  (('spline', 2, 1), False, False), (('std', 2, 2), True, True), (('spline', 2, 1), True, True)]:
        (v, rp, ci), calls = csr(full_form([6, 5], btype, degree, nc, uniform))
        assert _quad_ran(calls) == expect, (btype, degree, nc, uniform, calls)


@pytest.mark.parametrize('uniform', [True, False], ids=['uniform', 'iso'])
def test_bases_sharing_a_sample(env, uniform):
    '''Integrals of different bases at the same Gauss degree share ONE sample (and geometry): each must get a launcher of its own basis, in either order.'''
    from nutils_amd import mesh, function
    for order in ([('std', 2), ('spline', 2), ('std', 1)], [('std', 1), ('spline', 2), ('std', 2)]):
        domain, geom = mesh.rectilinear([8, 7])
        if not uniform:
            verts = numpy.stack(numpy.meshgrid(numpy.arange(9.), numpy.arange(8.), indexing='ij'), -1).reshape(-1, 2)
            geom = domain.basis('std', degree=1) @ (verts + numpy.random.default_rng(1).uniform(-.2, .2, verts.shape))
        forms = []
        for btype, degree in order:
            b = domain.basis(btype, degree=degree)
            forms.append(domain.integral(function.outer(function.grad(b, geom)).sum(-1) * function.J(geom), degree=4))
        assert len({id(f.terms[0][0]) for f in forms}) == 1  # (one sample)
        env(NUTILS_AMD_NO_FAST_PATH=False)
        fast = []
        for f in forms:
            out, calls = csr(f)
            assert _quad_ran(calls), calls
            fast.append(out)
        env(NUTILS_AMD_NO_FAST_PATH=True)
        for f, (v, rp, ci) in zip(forms, fast):
            (v0, rp0, ci0), _ = csr(f)
            assert numpy.array_equal(rp, rp0) and numpy.array_equal(ci, ci0)
            close(v, v0)
        env(NUTILS_AMD_NO_FAST_PATH=False)
