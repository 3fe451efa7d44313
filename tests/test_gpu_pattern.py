'''The sparsity-pattern kernels of nh_pattern.hip (stage K6: nh_pattern_build / _info / _expand / _expanded_nnz / _union_count / _union_fill) and the device
prefix sum behind them (nh_scan_exclusive of nh_runtime.hip), output by output against the plain numpy restatements of tests/pattern_refs.py.  Everything is
an integer: every comparison is numpy.array_equal, there is no tolerance anywhere.

The scalar pattern and the element map are read through the pointers of the handle (Pattern.srowptr_ptr, scol_ptr, emap_ptr, eoff_ptr) with nh_memcpy_d2h on
the current stream and nh_stream_sync.

Sizes are the ones at which the code takes another path:
  k_row_unique   compiled for 64, 256, 1024, 4096 and 16384 candidates of a row (`maxcand`, duplicates counted): every class at its limit -- the key array
                 then has no sentinel padding -- and one element past it, with almost all candidates distinct (hub), all distinct (fan: the unique count
                 equals CAP, every head flag set) and all duplicates (repeated); 16385 and more is refused (NH_ELIMIT); rows by grid stride above 2^20 rows
  gather         fixed nbr (index arithmetic) and roff (serial offsets), the latter also at the class limits
  k_count_rows, k_fill_rows, k_emap and the host-side eoff: the four combinations of a fixed count / offsets on the test and the trial side, rectangular
  scan           one level up to 2048 entries, two up to 2048^2 = 4 194 304, three beyond
  pattern_union  one merge for up to UNION_MAX = 8 parts, folded beyond

Every dof handed to a kernel lies inside [0, nrows) resp. [0, ncols): the kernels do not check it (asserted on the host before each build).'''
import ctypes
import functools

import numpy
import pytest

import pattern_refs as refs

pytestmark = pytest.mark.gpu


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------------------

def d2h(ptr, n, dtype):
    '''n entries at the device pointer `ptr` (a ctypes.c_void_p; None: NULL) as a numpy array: nh_memcpy_d2h on the current stream, then nh_stream_sync'''
    from nutils_amd import _lib, device
    out = numpy.full(n, -7, dtype=dtype)
    if ptr.value is None:
        assert n == 0, 'NULL pointer for a non-empty array'
        return out
    if n:
        _lib.call('nh_memcpy_d2h', ctypes.c_void_p(out.ctypes.data), ptr, ctypes.c_size_t(out.nbytes), device.stream())
    _lib.call('nh_stream_sync', device.stream())
    return out


def build(conn, t='fixed', r='fixed', nbt=None, nbr=None):
    '''kernels.Pattern of a connectivity; per side 'fixed' (the count nbt / nbr, which must be uniform) or 'ragged' (offsets)'''
    from nutils_amd import device, kernels
    assert not len(conn.tdofs) or (0 <= conn.tdofs.min() and conn.tdofs.max() < conn.nrows)
    assert not len(conn.rdofs) or (0 <= conn.rdofs.min() and conn.rdofs.max() < conn.ncols)
    nbt, nbr = nbt or conn.nbt, nbr or conn.nbr
    assert (t == 'ragged' or nbt) and (r == 'ragged' or nbr)
    return kernels.Pattern(conn.nelems, conn.nrows, conn.ncols, device.to_dev(conn.tdofs, 'int32'), device.to_dev(conn.rdofs, 'int32'),
                           nbt=nbt if t == 'fixed' else 0, nbr=nbr if r == 'fixed' else 0,
                           toff=device.to_dev(conn.toff, 'int64') if t == 'ragged' else None, roff=device.to_dev(conn.roff, 'int64') if r == 'ragged' else None)


def read(pat, ragged):
    '''(srowptr, scol, emap, eoff) of a pattern; eoff is None (a NULL pointer, asserted) when both sides have a fixed count'''
    if ragged:
        eoff = d2h(pat.eoff_ptr, pat.nelems + 1, numpy.int64)
    else:
        assert pat.eoff_ptr.value is None
        eoff = None
    return d2h(pat.srowptr_ptr, pat.nrows + 1, numpy.int64), d2h(pat.scol_ptr, pat.nnz_scalar, numpy.int32), d2h(pat.emap_ptr, pat.emap_len, numpy.int32), eoff


def same(got, want, what):
    got, want = numpy.asarray(got), numpy.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape}, reference {want.shape}'
    if not numpy.array_equal(got, want):
        bad = numpy.flatnonzero(got != want)
        raise AssertionError(f'{what}: {len(bad)} of {len(got)} entries differ, the first at {bad[0]}: got {got[bad[0]]}, reference {want[bad[0]]}')


def check_pattern(conn, ref, t='fixed', r='fixed', **kw):
    '''build, compare all four arrays and the two counts with the reference; returns what was read'''
    srowptr, scol, emap, eoff, _ = ref
    pat = build(conn, t, r, **kw)
    ragged = 'ragged' in (t, r)
    assert pat.nnz_scalar == len(scol), f'nnz_scalar {pat.nnz_scalar}, reference {len(scol)}'
    assert pat.emap_len == len(emap), f'emap_len {pat.emap_len}, reference {len(emap)}'
    got = read(pat, ragged)
    same(got[0], srowptr, 'srowptr')
    same(got[1], scol, 'scol')
    same(got[2], emap, 'emap')
    if ragged:
        same(got[3], eoff, 'eoff')
    return got


@functools.lru_cache(maxsize=None)
def case(builder, *args):
    '''a connectivity of pattern_refs and its reference, computed once'''
    conn = getattr(refs, builder)(*args)
    return conn, refs.ref_pattern(*conn.args)


@pytest.fixture
def marked_empty(monkeypatch):
    '''the wrappers allocate their results with device.empty: hand out -1 instead, so that an entry the kernel should have written and did not shows'''
    from nutils_amd import device
    plain = device.empty

    def empty(n, dtype):
        out = plain(n, dtype)
        return out.fill_(-1) if dtype in ('int32', 'int64') else out
    monkeypatch.setattr(device, 'empty', empty)


# ---- a. the size classes of k_row_unique ------------------------------------------------------------------------------------------------------------

HUBS = [(8, 8, 64, 64), (9, 8, 72, 256), (32, 8, 256, 256), (33, 8, 264, 1024), (32, 32, 1024, 1024), (33, 32, 1056, 4096), (128, 32, 4096, 4096),
        (129, 32, 4128, 16384), (128, 128, 16384, 16384)]
LIMITS = [(8, 8, 64), (32, 8, 256), (32, 32, 1024), (128, 32, 4096), (128, 128, 16384)]


@pytest.mark.parametrize('k,nb,maxcand,cls', HUBS, ids=[f'hub({k},{nb})-{m}-class{c}' for k, nb, m, c in HUBS])
def test_class_hub(k, nb, maxcand, cls):
    '''k elements share dof 0: its row has k * nb candidates, k * (nb - 1) + 1 of them distinct -- each class at its limit and one element past it (fixed
    gather, both sides fixed in k_emap)'''
    conn, ref = case('hub', k, nb)
    assert ref[4] == maxcand and cls // 4 < maxcand <= cls
    check_pattern(conn, ref)


@pytest.mark.parametrize('k,nbr,maxcand', LIMITS, ids=[f'fan({k},{n})-{m}' for k, n, m in LIMITS])
def test_class_fan_every_candidate_unique(k, nbr, maxcand):
    '''one row of exactly CAP distinct columns: no sentinel in the key array, every head flag of the chunked scan set, a unique count of CAP'''
    conn, ref = case('fan', k, nbr)
    assert ref[4] == maxcand == len(ref[1])
    srowptr, scol, emap, eoff = check_pattern(conn, ref)
    same(scol, numpy.arange(maxcand), 'scol against 0 .. CAP-1')


@pytest.mark.parametrize('k,nb,maxcand', LIMITS, ids=[f'repeated({k},{n})-{m}' for k, n, m in LIMITS])
def test_class_repeated_every_candidate_a_duplicate(k, nb, maxcand):
    '''one element listed k times: k * nb candidates in every row compact to nb columns'''
    conn, ref = case('repeated', k, nb)
    assert ref[4] == maxcand and len(ref[1]) == nb * nb
    check_pattern(conn, ref)


@pytest.mark.parametrize('k,nb,maxcand', LIMITS, ids=[f'hub({k},{n})-{m}' for k, n, m in LIMITS])
def test_class_limits_through_the_ragged_gather(k, nb, maxcand):
    '''the hub meshes at the class limits handed over with offsets on both sides: the serial gather of k_row_unique fills the key array to its last entry;
    the result is the one of the fixed counts'''
    conn, ref = case('hub', k, nb)
    check_pattern(conn, ref, 'ragged', 'ragged')


# ---- b. the limit -----------------------------------------------------------------------------------------------------------------------------------

def test_more_than_16384_candidates_are_refused_and_the_next_build_is_correct():
    from nutils_amd import _lib
    conn = refs.hub(129, 128)
    with pytest.raises(_lib.NutilsHipError) as info:
        build(conn)
    assert str(info.value) == 'libnutils_hip status -3: nh_pattern_build: a row has 16512 candidate columns; the row-wise kernel supports at most 16384'
    conn, ref = case('hub', 9, 8)
    check_pattern(conn, ref)


# ---- c. the shapes of the product path ----------------------------------------------------------------------------------------------------------------

SHAPES = {  # name: (builder, arguments, test side, trial side)
    'rectangular, nbt=3 nbr=5': ('random_mesh', (3, 200, 301, 157, 3, 5), 'fixed', 'fixed'),
    'toff with a fixed nbr': ('random_mesh', (4, 200, 301, 157, (1, 6), 4), 'ragged', 'fixed'),
    'fixed nbt with roff': ('random_mesh', (5, 200, 157, 301, 4, (1, 6)), 'fixed', 'ragged'),
    'both ragged, other offsets per side, empty elements': ('random_mesh', (6, 200, 211, 173, (0, 5), (0, 7)), 'ragged', 'ragged'),
    'uniform counts as toff, fixed nbr': ('random_mesh', (3, 200, 301, 157, 3, 5), 'ragged', 'fixed'),
    'uniform counts as roff, fixed nbt': ('random_mesh', (3, 200, 301, 157, 3, 5), 'fixed', 'ragged'),
    'random ragged mesh': ('ragged_mesh', (1, 300, 400), 'ragged', 'ragged'),
    'no elements, 7 x 5, fixed': ('empty_mesh', (7, 5), 'fixed', 'fixed'),
    'no elements, 7 x 5, offsets': ('empty_mesh', (7, 5), 'ragged', 'ragged'),
    'no elements, no rows, fixed': ('empty_mesh', (0,), 'fixed', 'fixed'),
    'no elements, no rows, offsets': ('empty_mesh', (0,), 'ragged', 'ragged'),
}


@pytest.mark.parametrize('name', SHAPES)
def test_shapes_of_the_product_path(name):
    '''rectangular patterns with different test and trial maps in the four combinations of a fixed count and offsets, holes in the numbering, repeated dofs,
    no elements, no rows; built twice, the arrays must be byte-equal (the order of the atomics of k_fill_rows must not show)'''
    builder, args, t, r = SHAPES[name]
    conn, ref = case(builder, *args)
    kw = dict(nbt=3, nbr=2) if conn.nelems == 0 else {}  # (no element to take the counts from)
    first = check_pattern(conn, ref, t, r, **kw)
    if conn.nelems == 0:
        assert len(first[1]) == 0 and len(first[2]) == 0 and not first[0].any()
    elif builder == 'ragged_mesh':
        assert (numpy.diff(first[0]) == 0).any()  # rows that no element touches
    second = check_pattern(conn, ref, t, r, **kw)
    for a, b in zip(first, second):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


# ---- d. many rows -------------------------------------------------------------------------------------------------------------------------------------

def test_chain_of_more_than_2_to_the_20_rows():
    '''k_row_unique walks the rows by grid stride (the grid is capped at 2^20 workgroups), the scans of 1 051 576 entries have two levels'''
    conn, ref = case('chain', 2 ** 20 + 3000)
    assert conn.nrows > 2 ** 20 and len(ref[1]) == 3154726
    check_pattern(conn, ref)


# ---- e. expansion -------------------------------------------------------------------------------------------------------------------------------------

EXPANSIONS = {
    '1x1': (1, 1, None), '3x2': (3, 2, None), '2x3': (2, 3, None), '1x8': (1, 8, None), '8x8': (8, 8, None),
    '3x3 mask with a zero row': (3, 3, [[1, 0, 1], [0, 0, 0], [1, 1, 0]]),
    '3x2 mask with a zero column': (3, 2, [[1, 0], [1, 0], [1, 0]]),
    '2x3 mask all zero': (2, 3, [[0, 0, 0], [0, 0, 0]]),
}
EXPANDED = {'random ragged mesh': ('ragged_mesh', (1, 300, 400), 'ragged'), 'hub(33,8)': ('hub', (33, 8), 'fixed')}


@pytest.fixture(scope='module')
def expandable():
    '''name -> (pattern, reference), each pattern built once for all its expansions and released with the module'''
    built = {}

    def get(name):
        if name not in built:
            builder, args, side = EXPANDED[name]
            conn, ref = case(builder, *args)
            built[name] = build(conn, side, side), ref
        return built[name]
    yield get
    built.clear()


@pytest.mark.parametrize('mask', EXPANSIONS)
@pytest.mark.parametrize('name', EXPANDED)
def test_expand(name, mask, expandable, marked_empty):
    '''k_expand and nh_pattern_expanded_nnz: nct != ncr, 8 x 8, masks with a zero row, a zero column and nothing but zeros, rows longer than the 64 lanes that
    walk them (hub(33,8): 232 columns) and empty rows (the ragged mesh)'''
    from nutils_amd import device
    nct, ncr, m = EXPANSIONS[mask]
    pat, ref = expandable(name)
    if name == 'hub(33,8)':
        assert numpy.diff(ref[0]).max() == 232
    rowptr, colidx = refs.ref_expand(ref[0], ref[1], nct, ncr, m)
    assert pat.expanded_nnz(nct, ncr, m) == len(colidx)
    got_rowptr, got_colidx = pat.expand(nct, ncr, m)
    same(device.to_host(got_rowptr), rowptr, 'rowptr')
    same(device.to_host(got_colidx), colidx, 'colidx')
    if m is not None and not numpy.any(m):
        assert len(colidx) == 0 and not rowptr.any()


# ---- f. union -----------------------------------------------------------------------------------------------------------------------------------------

def check_union(parts):
    from nutils_amd import device, kernels
    rowptr, colidx, pos = refs.ref_union(parts)
    got_rowptr, got_colidx, got_pos = kernels.pattern_union([(device.to_dev(rp, 'int64'), device.to_dev(ci, 'int64')) for rp, ci in parts])
    same(device.to_host(got_rowptr), rowptr, 'rowptr')
    cu = device.to_host(got_colidx)
    same(cu, colidx, 'colidx')
    assert len(got_pos) == len(parts)
    for i, ((rp, ci), p, g) in enumerate(zip(parts, pos, got_pos)):
        g = device.to_host(g)
        same(g, p, f'pos of part {i}')
        same(cu[g], ci, f'union[pos] of part {i}')


@pytest.mark.parametrize('nrows', [1, 127, 128, 129])
@pytest.mark.parametrize('nparts', [1, 2, 8, 9, 16])
def test_union_of_random_parts(nparts, nrows, marked_empty):
    '''1, 2 and 8 parts: one merge; 9: the fold 8 + 1; 16: 8 + 7 + 1, positions composed twice.  Rows either side of the workgroup of 128 threads (a thread per
    row); densities from empty to half full, one row empty in every part'''
    rng = numpy.random.default_rng(1000 * nparts + nrows)
    check_union([refs.random_csr(rng, nrows, 37, dens, empty_row=5) for dens in rng.random(nparts) * .5])


@pytest.mark.parametrize('nparts', [1, 8, 9])
def test_union_of_identical_parts(nparts, marked_empty):
    part = refs.random_csr(numpy.random.default_rng(3), 130, 37, .3, empty_row=5)
    check_union([part] * nparts)
    rowptr, colidx, pos = refs.ref_union([part] * nparts)
    assert numpy.array_equal(rowptr, part[0]) and numpy.array_equal(colidx, part[1]) and all(numpy.array_equal(p, numpy.arange(len(part[1]))) for p in pos)


@pytest.mark.parametrize('nparts,nrows', [(1, 0), (3, 0), (9, 0), (1, 130), (3, 130), (9, 130)])
def test_union_of_empty_parts(nparts, nrows, marked_empty):
    '''no rows at all, and rows without any entry'''
    check_union([(numpy.zeros(nrows + 1, dtype=numpy.int64), numpy.zeros(0, dtype=numpy.int64))] * nparts)


# ---- g. the scan ----------------------------------------------------------------------------------------------------------------------------------------

SCAN_MAX = 4194305


@pytest.fixture(scope='module')
def scan_part():
    '''one part of SCAN_MAX rows with 0 to 3 entries (columns 0 .. length-1), on the host and on the device; a prefix of its rows is a part as well'''
    from nutils_amd import device
    lens = numpy.random.default_rng(11).integers(0, 4, SCAN_MAX)
    rowptr = numpy.concatenate([[0], numpy.cumsum(lens)]).astype(numpy.int64)
    colidx = numpy.arange(rowptr[-1], dtype=numpy.int64) - numpy.repeat(rowptr[:-1], lens)
    return rowptr, device.to_dev(rowptr, 'int64'), device.to_dev(colidx, 'int64')


@pytest.mark.parametrize('nrows', [1, 2047, 2048, 2049, 4194304, SCAN_MAX])
def test_scan_through_the_union_count_of_a_single_part(nrows, scan_part):
    '''nh_scan_exclusive (256 threads x 8 entries per block, block totals scanned recursively) through nh_pattern_union_count with one part: the counts are the
    part's own row lengths, so the returned rowptr must be the part's rowptr and nnz its last entry.  One block up to 2048 rows, a second level up to
    2048^2 = 4 194 304, a third beyond.  Totals above 2^31 would need a column array of 17 GB: out of scope here.'''
    from nutils_amd import _lib, device
    rowptr, rowptr_dev, colidx_dev = scan_part
    out = device.empty(nrows + 1, 'int64').fill_(-1)
    nnz = ctypes.c_int64(-1)
    RP, CI = (ctypes.c_void_p * 1)(rowptr_dev.data_ptr()), (ctypes.c_void_p * 1)(colidx_dev.data_ptr())
    _lib.call('nh_pattern_union_count', 1, nrows, RP, CI, device.ptr(out), ctypes.byref(nnz), device.stream())
    assert nnz.value == rowptr[nrows]
    same(device.to_host(out), rowptr[:nrows + 1], 'rowptr')
