'''The sum-factorised P1-hex element routine (nh_p1hex_math.inc) uses that the 2-point rule is symmetric about 1/2.  Entry by entry
against the textbook formula G = grad(N) J^-1, K = sum_q w_q |det J_q| (kappa_q G G^T + m N N^T) on single-element meshes, where no
summation over elements can hide a wrong entry; the same through the any-mesh entry (k_fused_p1hex); and the guard: a rule that is
not symmetric is refused by the structured entries and takes the general kernel of the any-mesh entry.

The reference is evaluated in extended precision (numpy.longdouble) from the float64 vertices the device gets, so that its own
rounding does not count against the tolerance: a float64 evaluation of sum_a X_a dN_a loses 8 * 100 * 1.1e-16 ~ 1e-13 on the
elements translated by 100, the whole of RTOL.'''
import functools
import numpy
import pytest
from test_gpu_kernels import RTOL, close

pytestmark = pytest.mark.gpu

LD = numpy.longdouble


def reference(verts, gx, gw, kappa=1., mass=0., qs=None):
    '''Element matrices [ne, 8, 8] of kappa grad.grad + mass phi phi for the vertices [ne, 8, 3] (node a = 4 a0 + 2 a1 + a2) with the tensor
    rule gx, gw on [0, 1] (point q = 4 qa + 2 qb + qc); qs [ne, 8]: factor of kappa at the points.'''
    X = numpy.asarray(verts, dtype=float).astype(LD)
    ne = len(X)
    gx = numpy.asarray(gx, dtype=float).astype(LD)
    gw = numpy.asarray(gw, dtype=float).astype(LD)
    K = numpy.zeros((ne, 8, 8), dtype=LD)
    bits = numpy.array([[a >> 2, (a >> 1) & 1, a & 1] for a in range(8)])
    for q in range(8):
        xi = gx[bits[q]]
        f = numpy.where(bits == 1, xi, 1 - xi)  # [a][axis]: factor of N_a along the axis
        s = numpy.where(bits == 1, LD(1), LD(-1))
        N = f.prod(1)
        dN = numpy.stack([s[:, j] * numpy.delete(f, j, 1).prod(1) for j in range(3)], 1)  # [a][j]
        w = gw[bits[q]].prod()
        J = numpy.einsum('eai,aj->eij', X, dN)
        c = lambda i, j: J[:, (i + 1) % 3, (j + 1) % 3] * J[:, (i + 2) % 3, (j + 2) % 3] - J[:, (i + 1) % 3, (j + 2) % 3] * J[:, (i + 2) % 3, (j + 1) % 3]
        cof = numpy.stack([numpy.stack([c(i, j) for j in range(3)], -1) for i in range(3)], -2)  # cofactors: J^-1 = cof^T / det
        det = (J[:, 0, :] * cof[:, 0, :]).sum(-1)
        G = numpy.einsum('aj,eij->eai', dN, cof) / det[:, None, None]  # G[a][i] = sum_j dN[a][j] Jinv[j][i]
        kq = kappa * (LD(1) if qs is None else numpy.asarray(qs, dtype=float).astype(LD)[:, q])
        K += (w * abs(det) * kq)[:, None, None] * numpy.einsum('eai,ebi->eab', G, G)
        K += (w * abs(det) * mass)[:, None, None] * numpy.multiply.outer(N, N)[None]
    return K.astype(float)


CUBE = numpy.array([[a >> 2, (a >> 1) & 1, a & 1] for a in range(8)], dtype=float)


@functools.lru_cache(maxsize=None)
def elements():
    '''30 elements: the unit cube with corners perturbed by +-0.3; the same scaled by (1, 10, 0.1); the same translated by 100.'''
    rng = numpy.random.default_rng(20240)
    base = CUBE + rng.uniform(-.3, .3, (10, 8, 3))
    verts = numpy.concatenate([base, base * numpy.array([1., 10., .1]), base + 100.])
    qs = rng.uniform(.5, 2., (len(verts), 8))
    verts.setflags(write=False)
    qs.setflags(write=False)
    return verts, qs


@functools.lru_cache(maxsize=None)
def element_reference(variant):
    from nutils_amd import points
    verts, qs = elements()
    x1, w1 = points.gauss1(2)
    K = reference(verts, x1, w1, kappa=1.3, mass=.7 if variant == 'mass' else 0., qs=qs if variant == 'qscale' else None)
    K.setflags(write=False)
    return K


@pytest.mark.parametrize('variant', ['plain', 'mass', 'qscale'])
def test_element_matrix_entry_by_entry(variant):
    '''shape = (1, 1, 1): the 8 x 8 CSR block IS the element matrix.  plain: k_p1hex_skew<.., false, false>, mass: the MASS, qscale: the COEF
    instantiation.'''
    from nutils_amd import device, kernels, points
    verts, qs = elements()
    Kref = element_reference(variant)
    x1, w1 = points.gauss1(2)
    rowptr, colidx = kernels.p1hex_pattern((1, 1, 1))
    assert numpy.array_equal(device.to_host(rowptr), numpy.arange(9) * 8) and numpy.array_equal(device.to_host(colidx), numpy.tile(numpy.arange(8), 8))
    worst = 0.
    got = []
    for e in range(len(verts)):
        values = device.empty(64, 'float64')
        values.fill_(float('nan'))
        kw = {}
        if variant == 'mass':
            kw['mass'] = .7
        if variant == 'qscale':
            kw['qscale'] = device.to_dev(qs[e], 'float64')
        kernels.p1hex_laplace(shape=(1, 1, 1), values=values, gauss_x=x1, gauss_w=w1, verts=device.to_dev(verts[e], 'float64'), kappa=1.3, **kw)
        got.append(device.to_host(values).reshape(8, 8))
        worst = max(worst, numpy.abs(got[-1] - Kref[e]).max() / numpy.abs(Kref[e]).max())
    print(f'{variant}: max abs(K - Kref) / max abs(Kref) over {len(verts)} elements = {worst:.3e} (RTOL {RTOL:g})')
    for e in range(len(verts)):
        close(got[e], Kref[e])


def _any_mesh(shape, gx, gw, mass, seed=7):
    '''Perturbed structured mesh through the any-mesh entry (nh_assemble_matrix with the tables of the caller) -> CSR values, and the dense
    reference matrix picked at the pattern's positions.'''
    from nutils_amd import device, kernels
    from oracle import assemble as oa
    rng = numpy.random.default_rng(seed)
    dofs, coeffs, ndofs = oa.structured_basis(shape, 'std', 1)
    verts = numpy.stack(numpy.meshgrid(*[numpy.arange(n + 1.) for n in shape], indexing='ij'), -1).reshape(-1, 3) + rng.uniform(-.2, .2, (ndofs, 3))
    bits = numpy.array([[q >> 2, (q >> 1) & 1, q & 1] for q in range(8)])
    pts = numpy.asarray(gx, dtype=float)[bits]
    w = numpy.asarray(gw, dtype=float)[bits].prod(1)
    ne = len(dofs)
    C = oa.laplace_coefficient(3)
    C[0, 0, 0, 0] = mass
    T = kernels.tabulate(device.to_dev(coeffs[0], 'float64'), 8, coeffs.shape[2], device.to_dev(pts, 'float64'), 8, 3)
    d = device.to_dev(dofs, 'int32')
    b = kernels.basis(T, d, nb=8)
    geom = kernels.geometry_iso(8, T, d, device.to_dev(verts, 'float64'))
    pat = kernels.Pattern(ne, ndofs, ndofs, d, d, nbt=8, nbr=8)
    rowptr, colidx = pat.expand()
    values = device.to_dev(numpy.full(colidx.numel(), numpy.nan), 'float64')
    kernels.assemble_matrix(nelems=ne, ndims=3, nq=8, weights=device.to_dev(w, 'float64'), geom=geom, test=b, trial=b, nct=1, ncr=1, C=C, mask=None, pattern=pat,
                            values=values, fused=True, store=True)
    Ke = reference(verts[dofs], gx, gw, mass=mass)
    dense = numpy.zeros((ndofs, ndofs))
    numpy.add.at(dense, (dofs[:, :, None], dofs[:, None, :]), Ke)
    rp, ci = device.to_host(rowptr), device.to_host(colidx)
    rows = numpy.repeat(numpy.arange(ndofs), numpy.diff(rp))
    assert numpy.count_nonzero(dense) <= len(ci)
    return device.to_host(values), dense[rows, ci]


@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 2, 4)])
@pytest.mark.parametrize('mass', [0., .7])
def test_any_mesh_entry(shape, mass):
    '''Owner blocks of the any-mesh entry with the tables of the 2 x 2 x 2 Gauss scheme: k_fused_p1hex<MASS>, the same element routine.'''
    from nutils_amd import points
    x1, w1 = points.gauss1(2)
    got, ref = _any_mesh(shape, x1, w1, mass)
    print(f'{shape} mass {mass}: max abs err / max abs = {numpy.abs(got - ref).max() / numpy.abs(ref).max():.3e}')
    close(got, ref)


def test_unsymmetric_rule_is_refused_by_the_structured_entries():
    from nutils_amd import _lib, device, kernels
    device.require_gpu()
    values = device.zeros(64, 'float64')
    verts = device.to_dev(CUBE, 'float64')
    with pytest.raises(_lib.NutilsHipError, match='symmetric 2-point rule'):
        kernels.p1hex_laplace(shape=(1, 1, 1), values=values, gauss_x=[.2, .7], gauss_w=[.5, .5], verts=verts)
    with pytest.raises(_lib.NutilsHipError, match='symmetric 2-point rule'):
        kernels.p1hex_unit_matrix(shape=(1, 1, 1), gauss_x=[.2, .7], gauss_w=[.5, .5])
    assert not device.to_host(values).any()  # nothing was launched


@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 2, 4)])
def test_unsymmetric_rule_takes_the_general_kernel(shape):
    '''Tables tabulated at the tensor points of [.2, .7]: not the rule the sum-factorised routine is written for, so the any-mesh entry
    must not recognise it and still returns the matrix of THAT rule.'''
    got, ref = _any_mesh(shape, [.2, .7], [.45, .55], .7)
    print(f'{shape}: max abs err / max abs = {numpy.abs(got - ref).max() / numpy.abs(ref).max():.3e}')
    close(got, ref)
