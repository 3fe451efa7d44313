'''bench.py: --dump-outputs (what the timed step computed, written for comparison between builds) and --full (the secondary figures).'''
import json
import os
import subprocess
import sys

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('values', 'rows', 'cols', 'summary')


def load(d, prefix=''):
    return {k: numpy.load(os.path.join(d, prefix + k + '.npy')) for k in NAMES}


def test_dump_samples_a_large_matrix(tmp_path):
    '''More entries than the budget: the same seeded positions on every call, each sampled entry with its row and column, float64 files
    of at most 64 MB in all; with several ranks the budget is split and every file carries the rank.'''
    import torch
    import bench
    rng = numpy.random.default_rng(5)
    lens = rng.integers(1, 20, 150_000)
    rowptr = numpy.r_[0, numpy.cumsum(lens)]
    nnz = int(rowptr[-1])
    assert nnz > bench.DUMP_ENTRIES

    class Workload:
        pass
    wl = Workload()
    wl.rowptr, wl.colidx = torch.from_numpy(rowptr), torch.from_numpy(rng.integers(0, 10 ** 6, nnz))
    wl.values = torch.arange(nnz, dtype=torch.float64) - nnz / 3  # (an entry's value tells its position)
    for world in (1, 2):
        for run in ('a', 'b'):
            for rank in range(world):
                bench.dump_outputs(wl, str(tmp_path / run / str(world)), rank, world)
        d = tmp_path / 'a' / str(world)
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
        for rank in range(world):
            prefix = f'rank{rank}_' if world > 1 else ''
            a, b = load(d, prefix), load(tmp_path / 'b' / str(world), prefix)
            assert all(a[k].dtype == numpy.float64 and numpy.array_equal(a[k], b[k]) for k in NAMES)
            assert len(a['values']) == bench.DUMP_ENTRIES // world
            rows, cols = a['rows'].astype(numpy.int64), a['cols'].astype(numpy.int64)
            assert (numpy.diff(rows) >= 0).all() and rows.min() >= 0 and rows.max() < len(lens)
            # distinct entries, each in its row and with its column
            pos = (a['values'] + nnz / 3).round().astype(numpy.int64)
            assert len(numpy.unique(pos)) == len(pos)
            assert ((rowptr[rows] <= pos) & (pos < rowptr[rows + 1])).all() and numpy.array_equal(cols, wl.colidx.numpy()[pos])
            v = wl.values.numpy()
            assert numpy.allclose(a['summary'], [len(lens), nnz, numpy.abs(v).sum(), numpy.abs(v).max(), numpy.linalg.norm(v)], rtol=1e-10)


@pytest.mark.gpu
def test_bench_dumps_the_timed_matrix(tmp_path):
    '''`bench.py --dump-outputs DIR` on an 8^3 mesh (fewer entries than the sample: all of them are written): the arrays are the CSR matrix of
    the timed step, equal to the oracle's C port on the same seeded vertices, and the line reports the --steps it timed.'''
    from oracle import assemble as oa, port
    from nutils_amd import workloads
    cmd = [sys.executable, 'bench.py', '--steps', '3', '--warmup', '1', '--settle', '0', '--elements-per-axis', '8', '--no-cpu', '--traffic', 'static',
           '--dump-outputs', str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{"metric"')][0])
    assert rec['steps'] == 3 and rec['n_gpus'] == 1
    wl = workloads.PoissonSlab(n=8, rank=0, world=1, variant='iso')
    wl.setup()
    pts, w = oa.gauss(2, 3)
    _, coeffs, _ = oa.structured_basis((1, 1, 1), 'std', 1)
    N, dN = oa.tabulate(coeffs[0], pts)
    T = numpy.concatenate([N.T[:, :, None], dN.transpose(1, 0, 2)], axis=2)
    v, rp, ci, _ = port.laplace3d((8, 8, 8), 1, T, T, w, wl.verts)
    d = load(tmp_path)
    assert all(d[k].dtype == numpy.float64 for k in NAMES)
    assert numpy.array_equal(d['rows'], numpy.repeat(numpy.arange(len(rp) - 1), numpy.diff(rp))) and numpy.array_equal(d['cols'], ci)
    assert numpy.abs(d['values'] - v).max() <= 1e-13 * numpy.abs(v).max()
    assert d['summary'][:2].tolist() == [len(rp) - 1, len(v)]


@pytest.mark.gpu
def test_full_option_carries_the_secondary_figures():
    '''A plain run prints the headline figure and its gate only; `--full` prints the same line with the figures that take runs of their own.'''
    secondary = ('roofline', 'first_assembly_ms', 'host_ready_ms', 'reassembly_host_ready_ms', 'variants')
    recs = {}
    for full in ([], ['--full', '--no-cpu', '--traffic', 'static']):  # (the plain leg without the options that switch secondary figures off)
        cmd = [sys.executable, 'bench.py', '--steps', '3', '--warmup', '1', '--settle', '0', '--elements-per-axis', '8'] + full
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = recs[bool(full)] = json.loads([l for l in out.stdout.splitlines() if l.startswith('{"metric"')][0])
        assert rec['steps'] == 3 and rec['value'] > 0 and rec['unit'] == 'elements/s' and rec['higher_is_better'] is True and rec['dtype'] == 'f64'
        assert abs(rec['value'] * rec['ms_per_step'] * 1e-3 / 8 ** 3 - 1) < 1e-9 and rec['checks']['owned_row_sums_rel'] < 1e-12 and rec['kernel_ms'] > 0
    assert not [k for k in secondary + ('cpu_baseline', 'speedup_vs_cpu_port') if k in recs[False]]
    assert not [k for k in secondary if k not in recs[True]]
    assert recs[True]['roofline']['kernel_ms'] > 0 and set(recs[True]['variants']) == {'uniform', 'generic_gather', 'generic_fused'}
