'''The block plans of the AMG setup (preconargs=dict(nullspace=B, setup='block'), nutils_amd/amg.py, nh_block_segment_dot of nh_amg.hip) on the GPU, with the
problems, the restatement and the yardsticks of tests/test_gpu_amg_nullspace.py: the kernel alone against its numpy restatement (tests/amg_block_refs.py) on
synthetic plans, the numeric setup level by level, one cycle, the solve contract with the iteration counts and the entries it calls, and solver.System with
the plan cache.  No tolerance is new: values are held to `within` (8 times the distance of the float64 restatement from the longdouble one).'''
import functools
import types
import numpy
import pytest

from test_amg_host import cycle
from test_amg_nullspace_host import level, ld
from test_gpu_cg import same_bytes, RTOL
from test_gpu_amg import download, solve
from test_gpu_amg_nullspace import system, within, residual_contract, reference_iterations
from amg_block_refs import block_segment_dot

pytestmark = pytest.mark.gpu


# ---- 1. nh_block_segment_dot alone -------------------------------------------------------------------------------------------

LENGTHS = 1, 2, 63, 64, 65, 1000


def synthetic(k, p, q, rng, common_stride=False):
    '''(plan on the device, a, b, nout): 50 x 6 segments of 1, 2, 63, 64, 65 and 1000 products side by side (300 p k output entries: more than one workgroup
    of 256 for every shape), the blocks of both factors scattered over their arrays with row strides wider than the blocks, those of the output in shuffled
    order with gaps between them and between their rows'''
    from nutils_amd import device
    lengths = numpy.tile(LENGTHS, 50)
    nseg = len(lengths)
    ptr = numpy.r_[0, numpy.cumsum(lengths)].astype(numpy.int64)
    nprod = int(ptr[-1])
    na = nb = 20000
    sa = rng.integers(q, q + 6, nseg)
    sb = numpy.full(nprod, k + 2) if common_stride else rng.integers(k, k + 5, nprod)
    ia = rng.integers(0, na - (p - 1) * (q + 5) - q + 1, nprod)
    ib = rng.integers(0, nb - (q - 1) * (k + 4) - k + 1, nprod)
    os = rng.integers(k, k + 4, nseg)
    order = rng.permutation(nseg)
    start = numpy.zeros(nseg, dtype=numpy.int64)
    start[order] = numpy.cumsum(numpy.r_[0, (p * os + 3)[order][:-1]])  # (three entries between a block and the next)
    nout = int((p * os + 3).sum())
    dev = lambda v: device.to_dev(v.astype(numpy.int32), 'int32')
    plan = types.SimpleNamespace(k=k, p=p, q=q, nseg=nseg, nprod=nprod, nout=nout, ptr=device.to_dev(ptr, 'int64'), ia=dev(ia), ib=dev(ib), sa=dev(sa) if p > 1 else None,
                                 sb=None if common_stride else dev(sb), bstride=k + 2 if common_stride else 0, of=dev(start), os=dev(os) if p > 1 else None)
    return plan, rng.normal(size=na), rng.normal(size=nb), nout


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize('shape', ['1x1 1xk', 'kx1 1xk', 'kxk kxk', 'kxk rows of Q'])
def test_block_segment_dot(shape, k):
    '''the three shapes of the products of a hierarchy, and (k x k) blocks times rows of a dense [n x k] (no stride array), for every k: against the numpy
    restatement in float64 and longdouble under `within`; entries outside every block stay zero; a repeat is byte-equal'''
    from nutils_amd import device, kernels
    p, q = {'1x1 1xk': (1, 1), 'kx1 1xk': (k, 1), 'kxk kxk': (k, k), 'kxk rows of Q': (k, k)}[shape]
    plan, a, b, nout = synthetic(k, p, q, numpy.random.default_rng(100 * k + p + 10 * q), shape == 'kxk rows of Q')
    assert plan.nseg * p * k > 256
    a_dev, b_dev = device.to_dev(a, 'float64'), device.to_dev(b, 'float64')
    got = device.to_host(kernels.block_segment_dot(plan, a_dev, b_dev))
    assert got.shape == (nout,) and same_bytes(got, device.to_host(kernels.block_segment_dot(plan, a_dev, b_dev)))
    r64, exact = block_segment_dot(plan, a, b, nout), block_segment_dot(plan, a.astype(ld), b.astype(ld), nout)
    untouched = block_segment_dot(plan, numpy.ones(len(a)), numpy.ones(len(b)), nout) == 0
    assert untouched.sum() == nout - plan.nseg * p * k > 0 and not got[untouched].any()
    within(f'{shape}, k = {k}', got, r64, exact)
    out = device.to_dev(numpy.full(nout, 7.), 'float64')  # a result array of the caller's: only the blocks are written
    assert kernels.block_segment_dot(plan, a_dev, b_dev, out) is out
    again = device.to_host(out)
    assert same_bytes(again[~untouched], got[~untouched]) and (again[untouched] == 7.).all()


def variant(plan, **changes):
    '''a copy of a synthetic plan with some fields replaced (and without the wrapper's note that it has been looked at)'''
    fields = {**vars(plan), **changes}
    fields.pop('checked', None)
    return types.SimpleNamespace(**fields)


def test_block_segment_dot_argument_errors():
    '''sizes, the range of k and NULL pointers are the C entry's to refuse, indices that leave their arrays the wrapper's'''
    from nutils_amd import device, kernels, _lib
    rng = numpy.random.default_rng(7)
    plan, a, b, nout = synthetic(3, 3, 3, rng)
    a_dev, b_dev = device.to_dev(a, 'float64'), device.to_dev(b, 'float64')
    for k in (0, 7):
        bad = variant(plan, **{'k': k, 'p': k, 'q': k})
        with pytest.raises(_lib.NutilsHipError, match='k must be between 1 and 6'):
            kernels.block_segment_dot(bad, a_dev, b_dev)
    with pytest.raises(_lib.NutilsHipError, match='p and q either 1 or k'):
        kernels.block_segment_dot(variant(plan, **{'p': 2}), a_dev, b_dev)
    for what, array, value in (('a', 'ia', len(a) - 3 - 2 * 3 + 1), ('b', 'ib', len(b) - 3 - 2 * 3 + 1), ('out', 'of', nout - 3 - 2 * 3 + 1)):
        index = device.to_host(getattr(plan, array)).copy()
        index[-1] = value  # (the last entry a 3 x 3 block of the narrowest stride can start at, plus one)
        bad = variant(plan, **{array: device.to_dev(index.astype(numpy.int32), 'int32')})
        with pytest.raises(ValueError, match=f'a block reaches entry [0-9]+ of {what}'):
            kernels.block_segment_dot(bad, a_dev, b_dev)
    index = device.to_host(plan.ia).copy()
    index[0] = -1
    with pytest.raises(ValueError, match='no index or stride may be negative'):
        kernels.block_segment_dot(variant(plan, **{'ia': device.to_dev(index.astype(numpy.int32), 'int32')}), a_dev, b_dev)
    with pytest.raises(ValueError, match='ptr must rise from 0'):
        kernels.block_segment_dot(variant(plan, **{'nprod': plan.nprod - 1, 'ia': plan.ia[:-1], 'ib': plan.ib[:-1], 'sb': plan.sb[:-1]}), a_dev, b_dev)
    with pytest.raises(ValueError, match='blocks of several rows need sa and os'):
        kernels.block_segment_dot(variant(plan, **{'sa': None}), a_dev, b_dev)
    out = device.zeros(nout, 'float64')
    args = lambda a_ptr, b_ptr, sa: (3, 3, 3, plan.nseg, device.ptr(plan.ptr), plan.nprod, device.ptr(plan.ia), device.ptr(plan.ib), sa, device.ptr(plan.sb), 0, device.ptr(plan.of),
                                     device.ptr(plan.os), a_ptr, b_ptr, device.ptr(out), device.stream())
    with pytest.raises(_lib.NutilsHipError, match='NULL first factor'):
        _lib.call('nh_block_segment_dot', *args(None, device.ptr(b_dev), device.ptr(plan.sa)))
    with pytest.raises(_lib.NutilsHipError, match='NULL second factor'):
        _lib.call('nh_block_segment_dot', *args(device.ptr(a_dev), None, device.ptr(plan.sa)))
    with pytest.raises(_lib.NutilsHipError, match='without the row strides'):
        _lib.call('nh_block_segment_dot', *args(device.ptr(a_dev), device.ptr(b_dev), None))
    assert not device.to_host(out).any()  # nothing was launched


# ---- 2. the numeric setup, level by level -------------------------------------------------------------------------------------

def nullspace_of(name, k):
    '''the near-nullspace of `system(name)`, or on 'wide' the first k of [1, x, y, x y, x^2]'''
    B = system(name)[7]
    if k is None:
        return B
    assert name == 'wide'
    x, y = B[:, 1], B[:, 2]
    return numpy.ascontiguousarray(numpy.stack([B[:, 0], x, y, x * y, x * x], 1)[:, :k])


@functools.lru_cache(maxsize=None)
def device_hierarchy(name, coarse, k=None):
    '''`device_hierarchy` of tests/test_gpu_amg_nullspace.py with setup='block': (amg.Hierarchy, its levels downloaded as the restatement's namespaces)'''
    from nutils_amd import amg, device
    A, ref, cons, rhs, free, start, r0, B = system(name)
    B = nullspace_of(name, k)
    values, rowptr, colidx = A.triplet()
    levels = amg.symbolic(rowptr, colidx, device.to_dev(free, 'uint8') != 0, coarse, B.shape[1], setup='block')
    assert {lv.setup for lv in levels} == {'block'}
    h = amg.Hierarchy(levels, values, 1, device.to_dev(B.ravel(), 'float64').reshape(B.shape))
    levels = download(h)
    for ns, lv, d in zip(levels, h.levels, h.data):
        ns.B, ns.nodesize = device.to_host(d.B), lv.nodesize
        if lv.kind == 'coarsen':
            ns.Q = device.to_host(d.q)
    return h, levels


@pytest.mark.parametrize('name,coarse,k', [('quad', 64, None), ('wide', 16, None), ('hex', 64, None), ('wide', 16, 1), ('wide', 16, 2), ('wide', 16, 4), ('wide', 16, 5)])
def test_numeric_setup(name, coarse, k):
    '''the body of test_numeric_setup of tests/test_gpu_amg_nullspace.py on hierarchies made with setup='block': every level against the restatement fed with
    the device's matrix and near-nullspace of that level; the patterns integer-equal; Q, P, A_c and Rc within 8 times the distance of the float64 restatement
    from the longdouble one; R is P transposed value for value; two builds give the same bytes; and the trace has the block entry alone'''
    from nutils_amd import amg, device, _lib
    h, levels = device_hierarchy(name, coarse, k)
    print(f'{name}: k = {levels[0].B.shape[1]}, levels {[lv.nfree for lv in levels]}, kinds {[lv.kind for lv in levels]}')
    assert levels[-1].kind == 'dense' and len(levels) >= 2
    if k is None and name != 'hex':
        assert len(levels) == (3 if name == 'quad' else 4)
    for l, lv in enumerate(levels[:-1]):
        r64, exact = (level(lv.A, lv.free, coarse, lv.B, lv.nodesize, dtype) for dtype in (float, ld))
        assert r64.kind == 'coarsen' and r64.nc == lv.nc and numpy.array_equal(r64.dropped, exact.dropped)
        for got, want in ((lv.P, r64.P), (lv.R, r64.R), (levels[l + 1].A, r64.Ac)):
            assert numpy.array_equal(got.indptr, want.indptr) and numpy.array_equal(got.indices, want.indices)
        Rc = levels[l + 1].B
        assert numpy.array_equal(numpy.diagonal(Rc.reshape(-1, lv.B.shape[1], lv.B.shape[1]), axis1=1, axis2=2) == 0, exact.dropped)
        for what in ('rho', 'omega'):
            got, want = getattr(lv, what), getattr(r64, what)
            print(f'level {l}: {what} = {got!r}, {(got - want) / numpy.spacing(want):+.0f} ulp from the restatement')
            assert abs(got - want) <= 4 * numpy.spacing(want)
        within(f'level {l}: Q', lv.Q, r64.x.q, exact.x.q)
        within(f'level {l}: P', lv.P.data, r64.x.p, exact.x.p)
        within(f'level {l}: A_c', levels[l + 1].A.data, r64.x.ac, exact.x.ac)
        within(f'level {l}: Rc', Rc, r64.x.rc, exact.x.rc)
        assert numpy.array_equal(lv.R.data, lv.P.T.tocsr().data)  # R is P transposed, value for value
    A, B = system(name)[0], nullspace_of(name, k)
    with _lib.trace() as calls:
        again = amg.Hierarchy(h.levels, A.triplet()[0], 1, device.to_dev(B.ravel(), 'float64').reshape(B.shape))
    assert calls.count('nh_block_segment_dot') == 3 * (len(levels) - 1) and 'nh_segment_dot' not in calls
    for d, e in zip(h.data, again.data):
        for what in ('values', 'dinv', 'w', 'B', 'q', 'atvalues', 'pvalues', 'rvalues', 'apvalues', 'ainv'):
            if getattr(d, what, None) is not None:
                assert same_bytes(device.to_host(getattr(d, what)), device.to_host(getattr(e, what))), what


# ---- 3. one cycle ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,coarse', [('quad', 64), ('wide', 16), ('orphan', 16)])
def test_cycle(name, coarse):
    '''test_cycle of tests/test_gpu_amg_nullspace.py on a hierarchy made with setup='block': nh_amg_apply against the restatement's cycle in longdouble on the same
    hierarchy values; 'orphan' has dropped columns on every level'''
    from nutils_amd import device
    h, levels = device_hierarchy(name, coarse)
    A, ref, cons, rhs, free, start, r0, B = system(name)
    if name == 'orphan':
        assert all((lv.dinv == 0).sum() == 2 for lv in levels[1:-1])
    r = numpy.where(free, numpy.random.default_rng(13).normal(size=len(rhs)), 0.)
    exact = cycle(levels, r.astype(ld))
    d64 = float(numpy.abs(cycle(levels, r) - exact).max())
    r_dev = device.to_dev(r, 'float64')
    got = device.to_host(h.apply(r_dev))
    dist = float(numpy.abs(got - exact).max())
    print(f'{name}: {len(levels)} levels: |float64 restatement - longdouble| = {d64:.3e}, |device - longdouble| = {dist:.3e}, |z| = {float(numpy.abs(exact).max()):.3e}')
    assert d64 > 0 and dist <= 8 * d64
    assert not got[~free].any()
    assert same_bytes(got, device.to_host(h.apply(r_dev)))


# ---- 4. the solve -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['quad', 'hex'])
def test_solve_contract(name):
    '''elasticity with the rigid-body modes, coarse=64, setup='block': the residual contract, a repeat byte-equal, the restatement's iteration count, the block
    entry in the trace and the scalar one not; with setup='entry' and with no `setup` the other way round, byte-equal to each other'''
    from nutils_amd import _lib
    A, ref, cons, rhs, free, start, r0, B = system(name)
    args = dict(rtol=RTOL, constrain=cons, check=1)
    with _lib.trace() as calls:
        x = solve(A, rhs, preconargs=dict(coarse=64, nullspace=B, setup='block'), **args)
    it = A.iterations
    assert 'nh_block_segment_dot' in calls and 'nh_segment_dot' not in calls and 'nh_aggregate_qr' in calls
    assert A._amg[4] == 'block' and {lv.setup for lv in A._amg[3]} == {'block'} and A._amg[2] == B.shape[1]
    residual_contract(name, x)
    assert same_bytes(solve(A, rhs, preconargs=dict(coarse=64, nullspace=B, setup='block'), **args), x)
    it_ref, sizes, kinds = reference_iterations(name, 64)
    print(f'{name}: levels {sizes}, {it} iterations on the device with block plans, {it_ref} in numpy')
    assert [lv.nfree for lv in A._amg[3]] == sizes and [lv.kind for lv in A._amg[3]] == kinds
    assert it <= 1.1 * it_ref + 2
    results = []
    for preconargs in (dict(coarse=64, nullspace=B, setup='entry'), dict(coarse=64, nullspace=B, setup=None), dict(coarse=64, nullspace=B)):
        with _lib.trace() as calls:
            results.append(solve(A, rhs, preconargs=preconargs, **args))
        assert 'nh_segment_dot' in calls and 'nh_block_segment_dot' not in calls
        assert {lv.setup for lv in A._amg[3]} == {'entry'} and A._amg[4] == preconargs.get('setup')
    assert same_bytes(results[0], results[2]) and same_bytes(results[1], results[2])
    residual_contract(name, results[2])
    print(f'{name}: {A.iterations} iterations with entry plans')


def test_chain():
    '''test_chain of tests/test_gpu_amg_nullspace.py with setup='block': the chain of 262 444 with B = [1, x] ends in its 'diagonal' level of 526 dofs'''
    from nutils_amd import device, _lib
    A, ref, cons, rhs, free, start, r0, B = system('chain')
    with _lib.trace() as calls:
        x = solve(A, rhs, rtol=RTOL, constrain=cons, check=1, preconargs=dict(nullspace=device.to_dev(B.ravel(), 'float64').reshape(B.shape), setup='block'))
    it = A.iterations
    assert 'nh_block_segment_dot' in calls and 'nh_segment_dot' not in calls
    residual_contract('chain', x)
    levels = A._amg[3]
    it_ref, sizes, kinds = reference_iterations('chain', 256)
    print(f'chain: levels {sizes}, {it} iterations on the device, {it_ref} in numpy')
    assert [lv.kind for lv in levels] == kinds and [lv.nfree for lv in levels] == sizes and {lv.setup for lv in levels} == {'block'}
    assert levels[-1].kind == 'diagonal' and levels[-1].n == 526 and A._amg[2] == 2
    assert it <= 1.1 * it_ref + 2


# ---- 5. solver.System and the plan cache -------------------------------------------------------------------------------------------

def test_system_and_plan_cache(monkeypatch):
    '''the 16 x 16 elasticity problem of test_system_and_plan_cache of tests/test_gpu_amg_nullspace.py under matrix.backend('hip') with linargs carrying
    setup='block', against the 'diag' route as that test measures it; the symbolic phase runs once for two solves of one kind and again when `setup` changes'''
    from nutils_amd import amg, matrix, mesh, function, _lib
    from nutils_amd.solver import System
    nelems = 16
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, nelems + 1)] * 2)
    u = domain.field('u', btype='std', degree=1, shape=[2])
    v = domain.field('v', btype='std', degree=1, shape=[2])
    eps = lambda w: function.symgrad(w, geom)
    res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(2) + 1.3 * eps(u)) * function.J(geom), degree=2)
    cons = numpy.full((nelems + 1, nelems + 1, 2), numpy.nan)
    cons[0] = 0.
    cons[-1] = [0., .05]
    cons = {'u': cons.reshape(-1, 2)}
    grid = numpy.linspace(0, 1, nelems + 1)
    B = amg.rigid_body_modes(numpy.stack(numpy.meshgrid(grid, grid, indexing='ij'), -1).reshape(-1, 2))
    calls, symbolic = [], amg.symbolic
    monkeypatch.setattr(amg, 'symbolic', lambda *args, **kwargs: calls.append(kwargs.get('setup')) or symbolic(*args, **kwargs))
    rtol = 1e-10
    with matrix.backend('hip'):
        dev = System(res, trial='u', test='v')
        with _lib.trace() as trace:
            x = dev.solve(constrain=cons, linargs=dict(solver='cg', precon='amg', rtol=rtol, preconargs=dict(coarse=64, nullspace=B, setup='block')))['u']
        jac = dev._device_jac[1]
        it = dev.linear_iterations[-1]
        y = System(res, trial='u', test='v').solve(constrain=cons, linargs=dict(solver='cg', precon='diag', rtol=rtol))['u']
    assert 'nh_pcg_iterate' in trace and 'nh_amg_create' in trace and 'nh_block_segment_dot' in trace and 'nh_segment_dot' not in trace and calls == ['block']
    assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None and jac._amg[2] == 3 and len(jac._amg[3]) >= 2 and jac._amg[4] == 'block'
    free = numpy.isnan(cons['u']).ravel()
    assert numpy.array_equal(x.ravel()[~free], y.ravel()[~free])
    # both routes solve K x = b to |r| <= rtol |r0|: they differ by at most (|r_x| + |r_y|) / lmin <= 2 rtol |r0| / lmin
    host = System(res, trial='u', test='v')
    K = host.assemble_jacobian({}).export('dense')
    r0 = numpy.linalg.norm(numpy.asarray(host.assemble_residual({'u': numpy.nan_to_num(cons['u'])})).ravel()[free])
    lmin = numpy.linalg.eigvalsh(K[free][:, free])[0]
    dist = numpy.linalg.norm((x - y).ravel()[free])
    print(f'{it} iterations; |x_amg - x_diag| = {dist:.3e}, bound {2 * rtol * r0 * (1 + 1e-3) / lmin:.3e}')
    assert lmin > 0 and dist <= 2 * rtol * r0 * (1 + 1e-3) / lmin
    # the Jacobian of a next Newton step: new values on the same index tensors
    again = jac._with_values(jac.triplet()[0] * 2.)
    rhs = numpy.random.default_rng(15).normal(size=jac.shape[0])
    args = dict(solver='cg', precon='amg', rtol=rtol, constrain=~free)
    z = again.solve(rhs, preconargs=dict(coarse=64, nullspace=B, setup='block'), **args)
    assert calls == ['block'] and again._hostcsr is None
    assert numpy.linalg.norm((rhs - 2 * (K @ z))[free]) <= rtol * numpy.linalg.norm(rhs[free]) * (1 + 1e-3)
    again.solve(rhs, preconargs=dict(coarse=64, nullspace=B, setup='entry'), **args)  # (another kind is another hierarchy)
    assert calls == ['block', 'entry']
    again.solve(rhs, preconargs=dict(coarse=64, nullspace=B), **args)
    assert calls == ['block', 'entry', None]
    again.solve(rhs, preconargs=dict(coarse=64, nullspace=B * 2.), **args)  # (other values of the same kind are not)
    assert calls == ['block', 'entry', None]
