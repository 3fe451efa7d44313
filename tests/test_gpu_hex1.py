'''The trilinear 3-D write-once path (nh_assemble_hex1.hip): closed-form pattern, the reference fixture through the front end, small meshes against the
oracle, full-size meshes against the generic path (NUTILS_AMD_NO_FAST_PATH=1) and the C port, the uniform-cell replication, bit-identical repeats,
singular Jacobians, several forms on one sample, and a solve.'''
import numpy
import pytest

from test_hex1_host import form_tensor, with_tensor, _vector_mass

pytestmark = pytest.mark.gpu
RTOL = 1e-13


def close(a, b, scale=None):
    a, b = numpy.asarray(a), numpy.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = numpy.abs(b).max() if scale is None else scale
    err = numpy.abs(a - b).max()
    assert err <= RTOL * max(s, 1e-300), err / s


@pytest.fixture(autouse=True)
def all_modes(monkeypatch):
    '''the kernel for every (mode, components) of the class (by default sample.HEX1_ROUTED)'''
    from nutils_amd import sample
    monkeypatch.setattr(sample, 'HEX1_ROUTED', sample.HEX1_ALL)


@pytest.fixture
def env(monkeypatch):
    def set_(**kw):
        for k, v in kw.items():
            if v:
                monkeypatch.setenv(k, '1')
            else:
                monkeypatch.delenv(k, raising=False)
    return set_


def run(terms):
    from nutils_amd import sample, device, _lib
    with _lib.trace() as calls:
        v, rp, ci, _ = sample._MatrixPlan(terms).run()
    return (device.to_host(v), device.to_host(rp), device.to_host(ci)), list(calls)


def ran(calls):
    return any(c in ('nh_hex1_matrix', 'nh_hex1_rows_uniform') for c in calls) and not any(c.startswith('nh_assemble_matrix') for c in calls)


def mesh3(shape, geom='iso', seed=0, amp=.2):
    from nutils_amd import mesh
    if geom == 'graded':
        return mesh.rectilinear([numpy.linspace(0, 1, n + 1) ** 2 for n in shape])
    domain, g = mesh.rectilinear(list(shape))
    if geom == 'iso':
        verts = numpy.stack(numpy.meshgrid(*[numpy.arange(n + 1.) for n in shape], indexing='ij'), -1).reshape(-1, 3)
        g = domain.basis('std', degree=1) @ (verts + numpy.random.default_rng(seed).uniform(-amp, amp, verts.shape))
    return domain, g


def elasticity(domain, g, degree=2, lam=1., mu=.65):
    from nutils_amd import function
    u = domain.field('u', btype='std', degree=1, shape=[3])
    v = domain.field('v', btype='std', degree=1, shape=[3])
    eps = lambda w: function.symgrad(w, g)
    res = domain.integral(function.inner(eps(v), lam * function.div(u, g) * function.eye(3) + 2 * mu * eps(u)) * function.J(g), degree=degree)
    return function.derivative(function.derivative(res, 'v'), 'u')


def against_generic(env, terms, nan=False):
    (v, rp, ci), calls = run(terms)
    assert ran(calls), calls
    env(NUTILS_AMD_NO_FAST_PATH=True)
    (v0, rp0, ci0), calls0 = run(terms)
    env(NUTILS_AMD_NO_FAST_PATH=False)
    assert not any(c.startswith('nh_hex1') for c in calls0)
    assert numpy.array_equal(rp, rp0) and numpy.array_equal(ci, ci0)
    bad = numpy.isnan(v0)
    assert bad.any() == nan and numpy.array_equal(numpy.isnan(v), bad)
    close(v[~bad], v0[~bad], numpy.abs(v0[~bad]).max())
    return v


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 9), (3, 5, 2), (17, 4, 9)])
def test_pattern(shape):
    from nutils_amd import mesh, device, kernels
    domain, _ = mesh.rectilinear(list(shape))
    b = domain.basis('std', degree=1)
    smp = domain.sample('gauss', 2)
    for nc in (1, 2, 3):
        rp, ci = kernels.hex1_pattern(shape, nc)
        rp0, ci0 = smp.pattern(b, b).expand(nc, nc, None)
        rp, ci, rp0, ci0 = (device.to_host(a) for a in (rp, ci, rp0, ci0))
        assert rp.dtype == ci.dtype == numpy.int64
        assert numpy.array_equal(rp, rp0) and numpy.array_equal(ci, ci0)


def test_elasticity_fixture(golden):
    from nutils_amd import mesh
    g = golden('elast3d_p1_2_iso')
    domain, _ = mesh.rectilinear([int(n) for n in g['shape']])
    geom = domain.basis('std', degree=1) @ g['verts']
    K = elasticity(domain, geom, 2 * int(g['degree']), float(g['lam']), float(g['mu']))
    (v, rp, ci), calls = run(K.terms)
    assert 'nh_hex1_matrix' in calls and ran(calls), calls
    assert numpy.array_equal(rp, g['K_rowptr']) and numpy.array_equal(ci, g['K_colidx'])
    close(v, g['K_values'])


@pytest.mark.parametrize('degree', [2, 4], ids=['gauss2', 'gauss3'])
@pytest.mark.parametrize('nc', [1, 2, 3])
def test_small_meshes_against_the_oracle(nc, degree):
    from nutils_amd import function
    from oracle import assemble as oa
    shape = (3, 4, 5)
    domain, geom = mesh3(shape, seed=nc)
    C = form_tensor('dense', nc)
    if nc == 1:
        base = domain.integral(function.outer(domain.basis('std', degree=1)) * function.J(geom), degree=degree)
    else:
        base = _vector_mass(domain, geom, nc, degree)
    (v, rp, ci), calls = run(with_tensor(base, C))
    assert 'nh_hex1_matrix' in calls and ran(calls), calls
    dofs, coeffs, ndofs = oa.structured_basis(shape, 'std', 1)
    pts, w = oa.gauss(degree, 3)
    N, dN = oa.tabulate(coeffs, pts)
    x, J = oa.geometry_iso(geom.verts, dofs, N, dN)
    D, det = oa.physical_tables(N, dN, J)
    vo, rpo, cio = oa.assemble_csr(oa.local_matrices(D, D, det * w, C), dofs, dofs, ndofs, ndofs)
    assert numpy.array_equal(rp, rpo) and numpy.array_equal(ci, cio)
    close(v, vo)


@pytest.mark.parametrize('shape,geom', [((32, 32, 32), 'iso'), ((40, 24, 16), 'graded')])
def test_full_size_against_generic(env, shape, geom):
    import torch
    domain, g = mesh3(list(shape), geom)
    against_generic(env, elasticity(domain, g).terms)
    torch.cuda.empty_cache()


def test_anisotropic_and_dense_forms_against_generic(env):
    from nutils_amd import function
    domain, g = mesh3((9, 7, 8))
    basis = domain.basis('std', degree=1)
    lap = domain.integral(function.outer(function.grad(basis, g)).sum(-1) * function.J(g), degree=2)
    against_generic(env, with_tensor(lap, form_tensor('aniso', 1)))
    for nc in (2, 3):
        against_generic(env, with_tensor(_vector_mass(domain, g, nc, 4), form_tensor('dense', nc)))


def test_full_size_against_the_c_port():
    import torch
    from nutils_amd import sample, _lib
    from oracle import assemble as oa, port
    if not port.available():
        pytest.skip('C port not built')
    n = 64
    domain, geom = mesh3([n] * 3)
    with _lib.trace() as calls:
        values, rowptr, colidx, _ = sample._MatrixPlan(elasticity(domain, geom, lam=1., mu=.5 / .3 - 1).terms).run()
    assert 'nh_hex1_matrix' in calls
    dev = values.device
    scale = float(values.abs().max())
    _, coeffs, _ = oa.structured_basis((1, 1, 1), 'std', 1)
    pts, w = oa.gauss(2, 3)
    N, dN = oa.tabulate(coeffs[0], pts)
    T = numpy.concatenate([N.T[:, :, None], dN.transpose(1, 0, 2)], axis=2)
    C = oa.elasticity_coefficient(3, 1., .5 / .3 - 1)
    V = geom.verts.reshape(n + 1, n + 1, n + 1, 3)
    plane = 3 * (n + 1) ** 2  # dofs per node plane
    step, checked, worst = 16, 0, 0.
    for a in range(0, n, step):
        lo, hi = max(0, a - 1), min(n, a + step + 1)  # element layers of the slab
        vo, rpo, cio, _ = port.form3d((hi - lo, n, n), 1, C, T, T, w, V[lo:hi + 1].reshape(-1, 3), threads=16)
        # node planes whose rows are complete in the slab matrix and belong to this step: [a, a + step) (+ the last plane of the mesh)
        p0, p1 = a, (a + step if a + step < n else n + 1)
        r0, r1 = (p0 - lo) * plane, (p1 - lo) * plane
        R0, R1 = p0 * plane, p1 * plane
        rps = torch.as_tensor(rpo[r0:r1 + 1], device=dev)
        rpf = rowptr[R0:R1 + 1]
        assert bool((rps[1:] - rps[:-1] == rpf[1:] - rpf[:-1]).all()), f'row lengths differ in node planes {p0}..{p1}'
        k0, k1, K0, K1 = int(rpo[r0]), int(rpo[r1]), int(rpf[0]), int(rpf[-1])
        assert bool((torch.as_tensor(cio[k0:k1], device=dev) + lo * plane == colidx[K0:K1]).all()), f'column indices differ in node planes {p0}..{p1}'
        worst = max(worst, float((torch.as_tensor(vo[k0:k1], device=dev) - values[K0:K1]).abs().max()))
        checked += r1 - r0
        del vo, rpo, cio
    assert checked == len(rowptr) - 1 == 3 * (n + 1) ** 3
    assert worst < 1e-13 * scale, worst / scale
    del values, rowptr, colidx
    torch.cuda.empty_cache()


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 1), (33, 33, 33)])
def test_uniform(env, shape):
    domain, g = mesh3(list(shape), 'rect')
    terms = elasticity(domain, g).terms
    (v1, rp, ci), calls = run(terms)
    assert 'nh_hex1_rows_uniform' in calls and ran(calls), calls
    (v1b, _, _), _ = run(terms)
    assert numpy.array_equal(v1, v1b)  # (bit-identical replication)
    env(NUTILS_AMD_NO_UNIFORM=True)
    (v2, rp2, ci2), calls = run(terms)
    assert 'nh_hex1_matrix' in calls and 'nh_hex1_rows_uniform' not in calls
    assert numpy.array_equal(rp, rp2) and numpy.array_equal(ci, ci2)
    close(v1, v2)
    env(NUTILS_AMD_NO_UNIFORM=False)


def test_repeats_are_bit_identical():
    domain, g = mesh3((19, 6, 11))
    terms = elasticity(domain, g, degree=4).terms
    (v1, _, _), calls = run(terms)
    assert 'nh_hex1_matrix' in calls
    (v2, _, _), _ = run(terms)
    assert numpy.array_equal(v1, v2)


def test_singular_jacobian(env):
    '''one hexahedron collapsed to a point (det J = 0 at every point) in an isoparametric mesh'''
    from nutils_amd import mesh
    shape = (6, 5, 4)
    domain, _ = mesh.rectilinear(list(shape))
    verts = numpy.stack(numpy.meshgrid(*[numpy.arange(n + 1.) for n in shape], indexing='ij'), -1) - 2.5
    verts[2:4, 2:4, 2:4] = 0.  # (element (2, 2, 2) collapsed to the origin: J = 0 exactly on both paths)
    geom = domain.basis('std', degree=1) @ verts.reshape(-1, 3)
    against_generic(env, elasticity(domain, geom).terms, nan=True)


def test_forms_sharing_a_sample(env):
    '''Two forms and two component counts integrated on one sample: each gets a launcher of its own, in either order; the launcher cache stays bounded.'''
    from nutils_amd import function, sample
    domain, g = mesh3((7, 6, 5))
    basis = domain.basis('std', degree=1)
    lap = domain.integral(function.outer(function.grad(basis, g)).sum(-1) * function.J(g), degree=2)
    forms = [elasticity(domain, g).terms, with_tensor(_vector_mass(domain, g, 2, 2), form_tensor('dense', 2)), with_tensor(lap, form_tensor('aniso', 1))]
    assert len({id(t[0][0]) for t in forms}) == 1  # (one sample)
    smp = forms[0][0][0]
    for order in (forms, forms[::-1]):
        for terms in order:
            against_generic(env, terms)
    for i in range(12):  # (more forms than the cache holds)
        C = form_tensor('aniso', 1) * (1 + i)
        against_generic(env, with_tensor(lap, C))
    assert all(len(by_form) <= 8 for by_form in (e[1] if isinstance(e, tuple) else e for e in smp._hex1_fns.values()))


def test_solver(env):
    '''3-D linear elasticity on a 6^3 trilinear mesh, clamped at x = 0, displaced at x = 1: the same displacement with and without the write-once path'''
    from nutils_amd import mesh, function, solver
    cons = numpy.full((7, 7, 7, 3), numpy.nan)
    cons[0] = 0.
    cons[-1] = [0., .05, -.1]
    out = []
    for off in (False, True):
        env(NUTILS_AMD_NO_FAST_PATH=off)
        domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 7)] * 3)
        u = domain.field('u', btype='std', degree=1, shape=[3])
        v = domain.field('v', btype='std', degree=1, shape=[3])
        eps = lambda w: function.symgrad(w, geom)
        res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(3) + 1.3 * eps(u)) * function.J(geom), degree=2)
        out.append(numpy.asarray(solver.System(res, trial='u', test='v').solve(constrain={'u': cons.reshape(-1, 3)})['u']))
    env(NUTILS_AMD_NO_FAST_PATH=False)
    free = numpy.isnan(cons.reshape(-1, 3))
    assert numpy.abs(out[0][free]).max() > 1e-3
    close(out[0], out[1], numpy.abs(out[1]).max() * 10)


def test_default_routing(monkeypatch):
    '''by default equidistant cells take the row replication; isoparametric and graded cells keep the generic path (sample.HEX1_ROUTED)'''
    from nutils_amd import sample
    monkeypatch.setattr(sample, 'HEX1_ROUTED', (('uniform', 1), ('uniform', 3)))
    for geom, expect in (('rect', True), ('iso', False), ('graded', False)):
        domain, g = mesh3((5, 4, 3), geom)
        (v, rp, ci), calls = run(elasticity(domain, g).terms)
        assert ran(calls) == expect, (geom, calls)
        assert ('nh_hex1_rows_uniform' in calls) == expect
