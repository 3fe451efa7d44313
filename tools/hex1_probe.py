#!/usr/bin/env python3
'''Steady re-assembly times of the trilinear 3-D write-once path (nh_hex1_matrix / nh_hex1_rows_uniform) against the generic path
(NUTILS_AMD_NO_FAST_PATH=1) in the same process, alternated: python tools/hex1_probe.py [case substrings].
One JSON line per case; algorithmic bytes = CSR values written once + the unique geometry vertices read once.'''
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nutils_amd import sample
from nutils_amd.workloads import hex1_form

HBM = 8e12
DEFAULT = sample.HEX1_ROUTED
CASES = [('96^3 iso elasticity', [96] * 3, 'elasticity', 'iso', 2), ('96^3 uniform elasticity', [96] * 3, 'elasticity', 'uniform', 2),
         ('96^3 graded elasticity', [96] * 3, 'elasticity', 'graded', 2), ('64^3 iso elasticity gauss3', [64] * 3, 'elasticity', 'iso', 4),
         ('128^3 iso anisotropic scalar', [128] * 3, 'aniso', 'iso', 2), ('128^3 uniform anisotropic scalar', [128] * 3, 'aniso', 'uniform', 2),
         ('128^3 graded anisotropic scalar', [128] * 3, 'aniso', 'graded', 2)]


def timed(plan, window=0.2):
    '''steady re-assembly: HIP events around batches, warmed up, over at least `window` seconds'''
    for _ in range(3):
        plan.run({})
    torch.cuda.synchronize()
    n, total = 0, 0.
    while total < window:
        k = max(1, n or 5)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            plan.run({})
        b.record()
        b.synchronize()
        total += a.elapsed_time(b) / 1e3
        n += k
    return 1e3 * total / n


only = sys.argv[1:]
for name, shape, kind, geometry, degree in CASES:
    if only and not any(o in name for o in only):
        continue
    os.environ.pop('NUTILS_AMD_NO_FAST_PATH', None)
    uniform = geometry == 'uniform'
    terms = hex1_form(shape, kind, uniform, degree, graded=geometry == 'graded')
    plan = sample._MatrixPlan(terms)
    setting = sample._hex1_form(plan)
    default = setting is not None
    # (a combination the front end keeps on the generic path by default is measured on the kernel all the same: the routing table is widened for this case only)
    sample.HEX1_ROUTED = sample.HEX1_ALL
    assert sample._hex1_form(plan) is not None
    v, rp, ci, _ = plan.run({})
    ms = timed(plan)
    os.environ['NUTILS_AMD_NO_FAST_PATH'] = '1'
    gplan = sample._MatrixPlan(terms)
    v0, rp0, ci0, _ = gplan.run({})
    ms_g = timed(gplan)
    os.environ.pop('NUTILS_AMD_NO_FAST_PATH')
    ms2 = timed(plan)  # (alternated: the fast path again after the generic one)
    sample.HEX1_ROUTED = DEFAULT
    same_idx = bool(torch.equal(rp, rp0) and torch.equal(ci, ci0))
    err = float((v - v0).abs().max() / v0.abs().max())
    # (uniform cells: no geometry array; graded cells: the three coordinate axes)
    ngeom = 0 if uniform else sum(n + 1 for n in shape) if geometry == 'graded' else 3 * (shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1)
    nbytes = 8 * v.numel() + 8 * ngeom
    ms = min(ms, ms2)
    print(json.dumps(dict(case=name, default=default, nnz=v.numel(), ms=round(ms, 4), ms_generic=round(ms_g, 4), speedup=round(ms_g / ms, 2),
                          algorithmic_bytes=nbytes, hbm_frac=round(nbytes / (ms * 1e-3) / HBM, 3), indices_equal=same_idx, max_rel_err=err)), flush=True)
    del plan, gplan, v, v0, rp, ci, rp0, ci0, terms
    torch.cuda.empty_cache()
