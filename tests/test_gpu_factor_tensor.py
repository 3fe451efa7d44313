'''The factor-tensor builder nh_factor_tensor / nh_factor_fetch (nutils_amd/csrc/nh_factor.hip) called directly through kernels.factor_tensor, against the plain
restatements of tests/factor_refs.py (pinned to exact rational arithmetic and to integrals by hand in tests/test_factor_refs_host.py).  Three kinds of input:

  exact   integers: tables in {1, 2, 3}, weights in {1, 2}, coeff +-1 or +-2, box sizes in +-{1, 2, 4}, scales in -3 .. 3: every product and every partial sum is
          an integer far below 2^53 (a term is at most 2 * 2 * 64 * 3 * 81 < 2^18, a moment five of them, the longest run 2^18 moments), exact in any order, fused or
          not.  Values and indices must EQUAL those of factor_tensor_exact (numpy.array_equal, no tolerance).  The elements come in pairs with the same dofs, table and
          |sizes|; dofs are drawn per element from one block of the dof range, and in every second block the scales of a pair are opposite: all keys of such a block
          cancel to an exact zero and must be pruned, between blocks that survive.  The test asserts that the reference pruned at least a quarter of its distinct
          keys and kept at least a quarter.  Without scale_dev every term has the sign of coeff, so nothing can cancel: those cases assert that nothing was pruned.
  order   contributions such as 2^60, 1, -2^60 onto one key, whose float64 sum depends on the order: against ordered_run_sums, byte for byte
  real    random doubles, against factor_tensor_ld within gamma_m times the magnitude of the reference (see `bound`)

"Rejected" cases are argument checks that return a status before any launch; no case passes a dof outside [0, ndofs) or any other index a kernel would follow
out of its arrays.'''
import ctypes
import itertools

import numpy
import pytest

import factor_refs as refs

pytestmark = pytest.mark.gpu

LD = numpy.longdouble
NAN = float('nan')


def dev(a, dtype='float64'):
    from nutils_amd import device
    return device.to_dev(numpy.asarray(a), dtype)


def host(t):
    from nutils_amd import device
    return device.to_host(t)


class Null:
    '''stands for a tensor whose pointer is NULL'''
    data_ptr = staticmethod(lambda: 0)


@pytest.fixture(autouse=True)
def poisoned_empty(monkeypatch):
    '''kernels.factor_tensor allocates its results with device.empty: hand out NaN and -1 instead, so that an entry the compaction should have written and did not
    shows'''
    from nutils_amd import device
    plain = device.empty

    def empty(n, dtype):
        out = plain(n, dtype)
        out.fill_(NAN if dtype == 'float64' else -1)
        return out
    monkeypatch.setattr(device, 'empty', empty)


def device_geometry(geom, nd):
    from nutils_amd import kernels
    axis = geom.get('bnd_axis', -1)
    if geom['kind'] == 'box':
        size = numpy.asarray(geom['size'], dtype=float).reshape(-1, nd)
        return kernels.geometry_box(dev(numpy.zeros_like(size)), dev(size), axis)
    if geom['kind'] == 'tab':
        return kernels.geometry_tab(dev(numpy.asarray(geom['jac']).reshape(-1)), None, axis)
    gT = numpy.asarray(geom['gT'])
    return kernels.geometry_iso(gT.shape[0], dev(gT), dev(geom['gdofs'], 'int32'), dev(geom['verts']), axis)


def device_args(case):
    '''the keyword arguments of kernels.factor_tensor for a case of the references (dict with their keywords and ndofs)'''
    from nutils_amd import kernels
    c = case
    return dict(nelems=c['nelems'], ndims=c['ndims'], nq=c['nq'], rank=c['rank'], weights=dev(c['weights']), geom=device_geometry(c['geom'], c['ndims']),
                basis=kernels.basis(dev(c['T']), dev(c['dofs'], 'int32'), nb=c['nb'], tab=None if c.get('tab') is None else dev(c['tab'], 'int32')),
                ndofs=c['ndofs'], coeff=c.get('coeff', 1.), scale=None if c.get('scale') is None else dev(c['scale']),
                elist=None if c.get('elist') is None else dev(c['elist'], 'int32'))


def run(case):
    from nutils_amd import kernels
    values, indices = kernels.factor_tensor(**device_args(case))
    values, indices = host(values), host(indices)
    assert values.dtype == numpy.float64 and indices.dtype == numpy.int64 and indices.shape == (case['rank'], len(values))
    return values, indices


def run_twice(case):
    '''every case runs twice and delivers the same bytes'''
    values, indices = run(case)
    again = run(case)
    assert values.tobytes() == again[0].tobytes() and indices.tobytes() == again[1].tobytes()
    return values, indices


def reference_keywords(case):
    return {k: v for k, v in case.items() if k not in ('ndofs', 'ndims', 'geom')}


# ---- exact ----------------------------------------------------------------------------------------------------------------------------------

def exact_case(seed, *, rank, ndims, nq, nb, tabs, scaled, elist, nbase, blocks, coeff, hub=0, cancel=1):
    '''2 nbase elements, element e + nbase the partner of e; `blocks`: the dof sets, an element draws its nb dofs (with repeats) from one of them; blocks of parity
    `cancel` get opposite scales within a pair.  hub: that many extra pairs whose dofs are all the single dof of the middle block (which is kept).
    elist: None, 'descending' (a strict subset in descending order) or 'repeats' (all elements in shuffled order, a fifth of the pairs named twice).'''
    rng = numpy.random.default_rng(seed)
    block_of = rng.integers(0, len(blocks), nbase)
    k = min(len(blocks), nbase)
    block_of[:k] = numpy.arange(k)  # (every block is used)
    dofs = numpy.array([rng.choice(blocks[b], nb) for b in block_of])
    dofs[0] = numpy.resize(blocks[block_of[0]][:2], nb)  # an element that repeats dofs: [0 1 0 1] for nb = 4
    if hub:
        mid = len(blocks) // 2
        assert len(blocks[mid]) == 1 and mid % 2 != cancel
        block_of = numpy.concatenate([block_of, numpy.full(hub, mid)])
        dofs = numpy.concatenate([dofs, numpy.full((hub, nb), blocks[mid][0])])
        nbase += hub
    order = rng.permutation(nbase)  # (the hub elements lie spread over the list)
    block_of, dofs = block_of[order], dofs[order]
    ntab = 3 if tabs else 1
    T = numpy.full((ntab * nb, nq, 1 + ndims), NAN)
    T[:, :, 0] = rng.integers(1, 4, (ntab * nb, nq))
    size = rng.choice([1., 2., 4.], (nbase, ndims))
    size = numpy.concatenate([size * rng.choice([-1., 1.], size.shape), size * rng.choice([-1., 1.], size.shape)])
    if elist is None:
        elems = numpy.arange(2 * nbase)
    elif elist == 'descending':
        chosen = numpy.sort(rng.permutation(nbase)[:max(2 * nbase // 3, 1)])[::-1]
        elems = numpy.concatenate([chosen + nbase, chosen])
        assert (numpy.diff(elems) < 0).all() and len(elems) < 2 * nbase
    else:
        twice = rng.permutation(nbase)[:max(nbase // 5, 1)]
        elems = rng.permutation(numpy.concatenate([numpy.arange(2 * nbase), twice, twice + nbase]))
        assert len(numpy.unique(elems)) < len(elems)
    scale = None
    if scaled:  # the k-th naming of a partner answers the k-th naming of its element
        scale = rng.integers(-3, 4, (len(elems), nq)).astype(float)
        seen, first = {}, {}
        for ie, e in enumerate(elems):
            k = seen[e] = seen.get(e, -1) + 1
            if e < nbase:
                first[e, k] = ie
        seen = {}
        for ie, e in enumerate(elems):
            k = seen[e] = seen.get(e, -1) + 1
            if e >= nbase and block_of[e - nbase] % 2 == cancel:
                scale[ie] = -scale[first[e - nbase, k]]
    return dict(nelems=len(elems), ndims=ndims, nq=nq, rank=rank, weights=rng.integers(1, 3, nq).astype(float), geom=dict(kind='box', size=size), T=T,
                dofs=numpy.concatenate([dofs, dofs]), nb=nb, ndofs=int(max(b.max() for b in blocks)) + 1, coeff=float(coeff), scale=scale,
                elist=None if elist is None else elems, tab=numpy.tile(numpy.arange(nbase) % 3, 2) if tabs else None)


def chunks(ndofs, width):
    return [numpy.arange(i, min(i + width, ndofs)) for i in range(0, ndofs, width)]


def near_capacity(ndofs):
    '''dofs at 0, mid-range and ndofs - 1: the highest bits of the key decide the order and the decode divides keys of 63 bits'''
    mid = ndofs // 2
    return [numpy.array(b) for b in ([0, 1], [mid - 1, mid + 2], [mid, mid + 1], [0, mid, ndofs - 1], [ndofs - 2, ndofs - 1], [1, ndofs - 2])]


HUB = chunks(20, 4)[:2] + [numpy.array([9])] + chunks(20, 4)[3:]

EXACT = {
    # fewer than 2048 local entries: one block of the sort
    'r3-1d-q1-nb1': dict(rank=3, ndims=1, nq=1, nb=1, tabs=False, scaled=True, elist=None, nbase=100, blocks=chunks(40, 1), coeff=1),
    'r4-2d-q5-nb2-tab-descending': dict(rank=4, ndims=2, nq=5, nb=2, tabs=True, scaled=True, elist='descending', nbase=60, blocks=chunks(30, 3), coeff=-2),
    'r3-3d-q5-nb4-tab-repeats': dict(rank=3, ndims=3, nq=5, nb=4, tabs=True, scaled=True, elist='repeats', nbase=12, blocks=chunks(24, 4), coeff=-1),
    'r4-1d-q5-nb1-tab-repeats-noscale': dict(rank=4, ndims=1, nq=5, nb=1, tabs=True, scaled=False, elist='repeats', nbase=200, blocks=chunks(50, 2), coeff=2),
    'r3-2d-q1-nb2-descending-noscale': dict(rank=3, ndims=2, nq=1, nb=2, tabs=False, scaled=False, elist='descending', nbase=100, blocks=chunks(30, 3), coeff=-1),
    'r4-3d-q1-nb4': dict(rank=4, ndims=3, nq=1, nb=4, tabs=False, scaled=True, elist=None, nbase=3, blocks=chunks(12, 4), coeff=2),
    'r3-ndofs1-cancels': dict(rank=3, ndims=1, nq=1, nb=2, tabs=False, scaled=True, elist=None, nbase=20, blocks=chunks(1, 1), coeff=1, cancel=0),
    'r4-ndofs1': dict(rank=4, ndims=2, nq=5, nb=2, tabs=True, scaled=True, elist='repeats', nbase=20, blocks=chunks(1, 1), coeff=-1),
    'r4-ndofs54000': dict(rank=4, ndims=2, nq=5, nb=2, tabs=True, scaled=True, elist='descending', nbase=24, blocks=near_capacity(54000), coeff=1),
    'r3-ndofs2000000': dict(rank=3, ndims=3, nq=1, nb=4, tabs=False, scaled=True, elist=None, nbase=12, blocks=near_capacity(2000000), coeff=-2),
    # more: several blocks of the heads kernel and of the scan; 720 elements on one dof give a run of 720 * 8 moments, across more than two workgroups
    'r3-2d-q5-nb2-tab-hub': dict(rank=3, ndims=2, nq=5, nb=2, tabs=True, scaled=True, elist=None, nbase=60, blocks=HUB, coeff=1, hub=360),
    # at least 2^18 local entries: the sort in several passes
    'r4-3d-q5-nb4-tab-repeats-large': dict(rank=4, ndims=3, nq=5, nb=4, tabs=True, scaled=True, elist='repeats', nbase=512, blocks=chunks(300, 3), coeff=-1),
    'r4-1d-q1-nb4-large-noscale': dict(rank=4, ndims=1, nq=1, nb=4, tabs=False, scaled=False, elist=None, nbase=512, blocks=chunks(90, 3), coeff=1),
}


@pytest.mark.parametrize('name', list(EXACT))
def test_exact(name):
    spec = EXACT[name]
    case = exact_case(sorted(EXACT).index(name), **spec)
    n = case['nelems'] * case['nb'] ** case['rank']
    assert n >= 2 ** 18 if 'large' in name else n > 4096 if 'hub' in name else n < 2048, n
    everything, all_indices = refs.factor_tensor_exact(absdet=numpy.abs(case['geom']['size']).prod(1)[:, None].repeat(case['nq'], 1), keep_zeros=True,
                                                       **reference_keywords(case))
    keep = everything != 0
    want_values, want_indices = everything[keep].astype(numpy.float64), all_indices[:, keep]
    assert all(abs(v) < 2 ** 53 for v in everything)
    nkeys, nkept = len(keep), int(keep.sum())
    print(f'{name}: {n} local entries, {nkeys} distinct keys, {nkeys - nkept} pruned ({(nkeys - nkept) / nkeys:.2f}), {nkept} kept ({nkept / nkeys:.2f})')
    if not spec['scaled']:
        assert nkept == nkeys
    elif case['ndofs'] == 1:
        assert nkeys == 1 and nkept == (0 if spec.get('cancel', 1) == 0 else 1)
    else:
        assert 4 * (nkeys - nkept) >= nkeys and 4 * nkept >= nkeys
        pruned, kept = numpy.flatnonzero(~keep), numpy.flatnonzero(keep)
        assert ((pruned > kept[0]) & (pruned < kept[-1])).any()  # survivors on both sides of pruned keys
    if 'hub' in name:
        assert numpy.bincount(case['dofs'].reshape(-1))[9] > 600 * case['nb'] and (want_indices == 9).all(0).any()
    if 'ndofs5' in name or 'ndofs2' in name:
        ndofs = case['ndofs']
        assert 2 ** 62 < ndofs ** case['rank'] < 9e18  # keys of 63 bits, just under the capacity
        assert {0, ndofs // 2, ndofs - 1} <= set(want_indices[0].tolist()) and int(want_indices[0, -1]) * ndofs ** (case['rank'] - 1) > 2 ** 62
    values, indices = run_twice(case)
    assert numpy.array_equal(indices, want_indices)
    assert numpy.array_equal(values, want_values)


# ---- order ----------------------------------------------------------------------------------------------------------------------------------

def order_case(n, scale, elist=None):
    '''nb = 1, T = 1, one point of weight 1, unit boxes, coeff = 1: the contribution of list position ie is scale[ie] exactly.  Element e has dof e, but the
    elements in `shared` all have dof n // 3.'''
    T = numpy.full((1, 1, 2), NAN)
    T[0, 0, 0] = 1
    return dict(nelems=n, ndims=1, nq=1, rank=3, weights=[1.], geom=dict(kind='box', size=numpy.ones((n, 1))), T=T, dofs=numpy.arange(n), nb=1, ndofs=n, coeff=1.,
                scale=scale, elist=elist)


FIVE = [2. ** 53 + 2, 2. ** 53, -(2. ** 53 + 2), -(2. ** 52 + 1), 1.5]


def test_five_contributions_tell_their_order():
    '''(no GPU work: the premise of test_order) the front-to-back float64 sum of FIVE differs from that of every other order, but for the exchange of the first
    two, which is the same sum (a + b = b + a)'''
    def total(p):
        t = numpy.float64(p[0])
        for x in p[1:]:
            t = t + numpy.float64(x)
        return t
    others = [total(p) for p in itertools.permutations(FIVE) if list(p) not in (FIVE, [FIVE[1], FIVE[0]] + FIVE[2:])]
    assert len(others) == 118 and total(FIVE) == 2. ** 52 - 1.5 and total(FIVE) not in others


@pytest.mark.parametrize('n', [2000, 2 ** 18], ids=['one-block', 'several-passes'])
def test_order(n):
    '''Equal keys are summed in the order of the list.  This is the ONLY test that can tell a stable sort from an unstable one, or a run summed back to front or
    as a tree from one summed front to back: everywhere else the sums are exact in any order, or compared within a bound that holds for any order.
    Three elements share a dof, at list positions 0, n / 2 and n - 1, with scales 2^60, 1, -2^60: (2^60 + 1) - 2^60 = 0 in float64, the entry must be absent.  The
    list reordered through elist_dev to 2^60, -2^60, 1: the entry must be there with the value 1.  Then five contributions (FIVE) spread over the list.  All other
    elements have dofs of their own and small integer scales.'''
    rng = numpy.random.default_rng(n)
    shared = n // 3
    spots = [0, n // 2, n - 1]
    base = order_case(n, rng.integers(1, 8, n).astype(float))
    base['dofs'][spots] = shared
    base['scale'][shared] = 0  # (its own element: nothing)
    base['scale'][spots] = [2. ** 60, 1., -2. ** 60]
    keys = lambda case: numpy.repeat(case['dofs'][numpy.arange(n) if case['elist'] is None else case['elist']][:, None], 3, 1)
    # in the order of the elements
    want_values, want_indices = refs.ordered_run_sums(keys(base), base['scale'])
    assert len(want_values) == n - 4 and shared not in want_indices[0]
    values, indices = run_twice(base)
    assert numpy.array_equal(indices, want_indices) and values.tobytes() == want_values.tobytes()
    # reordered: 0, n - 1, then the rest
    elist = numpy.concatenate([[0, n - 1], numpy.arange(1, n - 1)])
    moved = dict(base, elist=elist, scale=base['scale'][elist])
    want_values, want_indices = refs.ordered_run_sums(keys(moved), moved['scale'])
    at = numpy.flatnonzero(want_indices[0] == shared)
    assert len(want_values) == n - 3 and len(at) == 1 and want_values[at[0]] == 1
    values, indices = run_twice(moved)
    assert numpy.array_equal(indices, want_indices) and values.tobytes() == want_values.tobytes()
    # five contributions whose sum tells their order
    spots = [3, n // 4, n // 2, n - n // 4, n - 2]
    five = order_case(n, rng.integers(1, 8, n).astype(float))
    five['dofs'][spots] = shared
    five['scale'][shared] = 0
    five['scale'][spots] = FIVE
    want_values, want_indices = refs.ordered_run_sums(keys(five), five['scale'])
    assert want_values[numpy.flatnonzero(want_indices[0] == shared)].tolist() == [2. ** 52 - 1.5]
    values, indices = run_twice(five)
    assert numpy.array_equal(indices, want_indices) and values.tobytes() == want_values.tobytes()


# ---- real -----------------------------------------------------------------------------------------------------------------------------------

def multilinear_tables(points):
    '''gT[2^nd][nq][1 + nd] of the multilinear functions prod_i (xi_i or 1 - xi_i)'''
    nq, nd = points.shape
    gT = numpy.zeros((2 ** nd, nq, 1 + nd))
    for a, corner in enumerate(itertools.product((0, 1), repeat=nd)):
        f = [points[:, i] if c else 1 - points[:, i] for i, c in enumerate(corner)]
        gT[a, :, 0] = numpy.prod(f, axis=0)
        for j in range(nd):
            gT[a, :, 1 + j] = numpy.prod([(1. if c else -1.) + 0 * points[:, i] if i == j else f[i] for i, c in enumerate(corner)], axis=0)
    return gT


def real_geometry(rng, kind, nd, nq, ne, axis):
    if kind == 'box':
        return dict(kind='box', size=rng.uniform(.5, 2., (ne, nd)) * rng.choice([-1., 1.], (ne, nd)), bnd_axis=axis)
    if kind == 'tab':  # J = I + 0.2 U(-1, 1), a third of the elements mirrored: det < 0
        jac = numpy.eye(nd) + .2 * rng.uniform(-1, 1, (ne, nq, nd, nd))
        jac[::3, :, :, 0] *= -1
        return dict(kind='tab', jac=jac, bnd_axis=axis)
    if kind == 'iso3':  # triangles: the general loop over the geometry functions
        gT = numpy.zeros((3, nq, 3))
        gT[:, :, 1:] = numpy.array([[-1., -1.], [1., 0.], [0., 1.]])[:, None, :]
        corners = numpy.array([[0., 0.], [1., 0.], [0., 1.]])
    else:  # 2^nd functions: the unrolled branch
        gT = multilinear_tables(rng.uniform(.05, .95, (nq, nd)))
        corners = numpy.array(list(itertools.product((0., 1.), repeat=nd)))
    ngb = len(corners)
    verts = corners[None] - .5 + .15 * rng.uniform(-1, 1, (ne, ngb, nd))  # (centred on the origin: J = sum x dN then cancels little, and the bound stays sharp)
    verts[::3, :, 0] *= -1  # mirrored
    gdofs = rng.permutation(ne * ngb).reshape(ne, ngb)
    shuffled = numpy.zeros((ne * ngb, nd))
    shuffled[gdofs.reshape(-1)] = verts.reshape(-1, nd)
    return dict(kind='iso', gT=gT, gdofs=gdofs, verts=shuffled, bnd_axis=axis)


def operations(case, count):
    '''m of the bound, per entry, counted from the kernels.  A term  coeff w |det| s T .. T  goes through
        3 products in k_fac_wdet (coeff * w, * |det|, * s) and `rank` in k_fac_moments;  nq - 1 additions of the moment;  count - 1 additions of its run (k_fac_runs);
        the determinant (invert of nh_geom.inc): none in 1-D; a product and a difference in 2-D; in 3-D a cofactor (a product, a difference) and the expansion (a
        product, two additions): 5 on the longest path;  an isoparametric J entry is a sum of ngb products, ngb roundings per entry, nd entries in a determinant term.
    A face (bnd_axis >= 0) multiplies det by sqrt(sum_i (C_i r)^2), r = 1 / det: det's own roundings enter again through r, plus the quotient; a cofactor C_i of a
    3 x 3 matrix is a product and a difference (2; none below), of nd - 1 J entries; then C_i * r, the square, nd - 1 additions, the root and the last product:
    m_det + 1 + (2 if nd = 3) + (nd - 1) ngb + 1 + 1 + (nd - 1) + 1 + 1 further roundings.  Contraction to fma only removes roundings.
    Each of these errors is relative to the sum of the |terms| of what it rounds, which the reference carries as the condition factors of its magnitude
    (factor_refs.measure_ld: both factors are >= 1, so their product covers the sum of the two contributions).  That product is the one generous step: for a face
    det * r is 1 to two roundings, so the determinant's own condition hardly enters the measure, yet it multiplies the bound -- the isoparametric faces in 3-D, where
    it is largest, come out a hundred times below their bound where the other cases reach a tenth to a half of it.'''
    nd, geom = case['ndims'], case['geom']
    ngb = numpy.asarray(geom['gT']).shape[0] if geom['kind'] == 'iso' else 0
    m_det = {1: 0, 2: 2, 3: 5}[nd] + nd * ngb
    m_face = m_det + 1 + (2 if nd == 3 else 0) + (nd - 1) * ngb + 4 + (nd - 1) if geom.get('bnd_axis', -1) >= 0 else 0
    return (case['rank'] + 3) + (case['nq'] - 1) + (numpy.asarray(count) - 1) + m_det + m_face


def bound(case, mag, count):
    '''gamma_m(2^-53) magnitude for the kernel's float64 roundings, plus gamma_m(2^-64) magnitude for the longdouble reference's own'''
    m = operations(case, count).astype(LD)
    gamma = lambda u: m * u / (1 - m * u)
    return (gamma(LD(2) ** -53) + gamma(LD(2) ** -64)) * mag


REAL = [(kind, nd, -1) for kind in ('box', 'tab', 'iso') for nd in (1, 2, 3)] + [('iso3', 2, -1)] \
    + [(kind, nd, axis) for kind in ('box', 'tab', 'iso') for nd in (2, 3) for axis in (0, nd - 1)] + [('iso3', 2, 0), ('iso3', 2, 1)]


@pytest.mark.parametrize('kind, nd, axis', REAL, ids=lambda v: str(v))
def test_real(kind, nd, axis):
    '''random normal tables (NaN in the gradient slots: only slot 0 may be read), scales of either sign, three tables, a list that names elements twice and leaves
    some out; rank 3 and 4.  Indices equal; values within `bound`, whose operation count m is derived in `operations`.'''
    rng = numpy.random.default_rng(1000 + 100 * REAL.index((kind, nd, axis)))
    ne, nl, nq, nb, ndofs = 320, 300, 3, 2, 120
    for rank in 3, 4:
        T = numpy.full((3 * nb, nq, 1 + nd), NAN)
        T[:, :, 0] = rng.standard_normal((3 * nb, nq))
        case = dict(nelems=nl, ndims=nd, nq=nq, rank=rank, weights=rng.uniform(.1, 1., nq), geom=real_geometry(rng, kind, nd, nq, ne, axis), T=T,
                    dofs=rng.integers(0, ndofs, (ne, nb)), nb=nb, ndofs=ndofs, coeff=-.7, scale=rng.uniform(.5, 1.5, (nl, nq)) * rng.choice([-1., 1.], (nl, nq)),
                    elist=rng.integers(0, ne, nl), tab=numpy.arange(ne) % 3)
        value, mag, want_indices, count = refs.factor_tensor_ld(keep_zeros=True, **{k: v for k, v in case.items() if k != 'ndofs'})
        assert (value != 0).all() and count.max() > 1 and len(numpy.unique(case['elist'])) < nl
        values, indices = run_twice(case)
        assert numpy.array_equal(indices, want_indices)
        err = numpy.abs(values.astype(LD) - value)
        limit = bound(case, mag, count)
        print(f'{kind} {nd}-D bnd_axis={axis} rank {rank}: {len(values)} entries, m = {operations(case, count).min()} .. {operations(case, count).max()}, '
              f'max err / bound = {float((err / limit).max()):.3f}')
        assert (err <= limit).all()


# ---- protocol and rejections ----------------------------------------------------------------------------------------------------------------

def small_case(**changes):
    T = numpy.full((2, 2, 3), NAN)
    T[:, :, 0] = [[1, 2], [3, 1]]
    case = dict(nelems=3, ndims=2, nq=2, rank=3, weights=[1., 2.], geom=dict(kind='box', size=numpy.ones((3, 2))), T=T, dofs=[[0, 1], [1, 2], [2, 3]], nb=2,
                ndofs=4, coeff=1., scale=None)
    return dict(case, **changes)


def build(args):
    '''nh_factor_tensor alone: the number of entries of the tensor it leaves in the library'''
    from nutils_amd import _lib, device
    a = _lib.FactorArgs(args['nelems'], device.ptr(args['elist']), args['ndims'], args['nq'], args['rank'], device.ptr(args['weights']), args['geom'], args['basis'],
                        device.ptr(args['scale']), float(args['coeff']), int(args['ndofs']))
    nnz = ctypes.c_int64(-1)
    _lib.call('nh_factor_tensor', ctypes.byref(a), ctypes.byref(nnz), device.stream())
    return nnz.value


def fetch(rank, nnz):
    from nutils_amd import _lib, device
    values, indices = device.empty(nnz, 'float64'), device.empty(rank * nnz, 'int64')
    _lib.call('nh_factor_fetch', device.ptr(values), device.ptr(indices), device.stream())
    return host(values), host(indices).reshape(rank, nnz)


def expected(case):
    values, indices = refs.factor_tensor_exact(absdet=numpy.ones((len(case['dofs']), case['nq'])), **reference_keywords(case))
    return values.astype(numpy.float64), indices


def test_protocol():
    from nutils_amd import _lib, device
    first, second = small_case(), small_case(rank=4, coeff=-2., dofs=[[3, 1], [0, 0], [2, 3]])
    a1, a2 = device_args(first), device_args(second)
    # build, fetch; a fetch after a fetch finds nothing, and so does a fetch before any build
    nnz = build(a1)
    values, indices = fetch(3, nnz)
    assert numpy.array_equal(values, expected(first)[0]) and numpy.array_equal(indices, expected(first)[1]) and nnz == 22
    for _ in range(2):
        with pytest.raises(_lib.NutilsHipError, match='no tensor has been built'):
            fetch(3, nnz)
    # a fetch with NULL buffers fails and leaves the tensor in place
    nnz = build(a1)
    with pytest.raises(_lib.NutilsHipError, match='nh_factor_fetch: NULL buffer'):
        _lib.call('nh_factor_fetch', None, None, device.stream())
    values, indices = fetch(3, nnz)
    assert numpy.array_equal(values, expected(first)[0]) and numpy.array_equal(indices, expected(first)[1])
    # two builds, one fetch: the second tensor
    assert build(a1) == 22
    nnz = build(a2)
    values, indices = fetch(4, nnz)
    assert numpy.array_equal(values, expected(second)[0]) and numpy.array_equal(indices, expected(second)[1]) and nnz != 22
    with pytest.raises(_lib.NutilsHipError, match='no tensor has been built'):
        fetch(4, nnz)


def test_a_tensor_whose_entries_all_cancel():
    from nutils_amd import _lib, device
    case = small_case(nelems=4, elist=[0, 2, 2, 0], scale=[[1., -2.], [3., 1.], [-3., -1.], [-1., 2.]])
    assert len(expected(case)[0]) == 0 and len(refs.factor_tensor_exact(absdet=numpy.ones((3, 2)), keep_zeros=True, **reference_keywords(case))[0]) == 16
    assert build(device_args(case)) == 0
    _lib.call('nh_factor_fetch', None, None, device.stream())  # empty buffers: NULL
    with pytest.raises(_lib.NutilsHipError, match='no tensor has been built'):
        _lib.call('nh_factor_fetch', None, None, device.stream())
    values, indices = run(case)
    assert values.shape == (0,) and indices.shape == (3, 0)


@pytest.mark.parametrize('rank', [3, 4])
def test_no_elements(rank):
    '''nelems == 0 is a build like any other: a tensor without entries that a fetch finds and releases (it used to leave the library in the state "nothing built",
    and kernels.factor_tensor, which always fetches, raised)'''
    from nutils_amd import _lib, device
    case = small_case(nelems=0, rank=rank)
    values, indices = run(case)
    assert values.shape == (0,) and indices.shape == (rank, 0)
    with pytest.raises(_lib.NutilsHipError, match='no tensor has been built'):
        _lib.call('nh_factor_fetch', None, None, device.stream())
    # .. also with a list and a scale that are empty, and it replaces a tensor built before
    assert build(device_args(small_case())) == 22
    values, indices = run(dict(case, elist=numpy.zeros(0, dtype=int), scale=numpy.zeros((0, 2))))
    assert values.shape == (0,) and indices.shape == (rank, 0)


def test_rejections():
    '''every one of these is refused on the host, before anything is launched or allocated'''
    from nutils_amd import _lib, kernels
    good = device_args(small_case())
    T, dofs = good['basis']._keep[:2]

    def refused(match, **changes):
        with pytest.raises(_lib.NutilsHipError, match=match):
            kernels.factor_tensor(**dict(good, **changes))

    for rank in 2, 5:
        refused(rf'rank must be 3 or 4 \(got {rank}\)', rank=rank)
    for ndims in 0, 4:
        refused('nh_factor_tensor: quadrature / dimension', ndims=ndims)
    refused('nh_factor_tensor: quadrature / dimension', nq=0)
    refused('nh_factor_tensor: quadrature / dimension', weights=Null)
    ragged = 'a basis with a uniform number of functions per element is required'
    refused(ragged, basis=kernels.basis(T, dofs, nb=0))
    refused(ragged, basis=kernels.basis(T, dofs, nb=2, off=dev([0, 2, 4, 6], 'int64')))
    refused(ragged, basis=kernels.basis(Null, dofs, nb=2))
    refused(ragged, basis=kernels.basis(T, Null, nb=2))
    refused('nh_factor_tensor: ndofs', ndofs=0)
    refused('55109 dofs to the power 4 does not fit the 64-bit key', ndofs=55109, rank=4)
    refused('2097152 dofs to the power 3 does not fit the 64-bit key', ndofs=2 ** 21, rank=3)
    values, indices = kernels.factor_tensor(**good)  # and the arguments they were derived from are fine
    assert values.numel() == 22
