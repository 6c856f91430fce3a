"""Shape fuzz (run by hand on a GPU box: python tests/fuzz_shapes.py <seed> <cases>): random (ny, nx) pairs of built sides,
any even sides (embedded where not built) and sides above 1024 against short partners, random fields and component sets
(test_gpu_random.random_case), the fused back end against the fp64 oracle.  Round 4: 1420 cases, no mismatch (one ill-conditioned sum, within 2e-12 of the terms' magnitudes on both back ends).
The generator (`fuzz_cases`) and the bound (`fuzz_bound`) are shared with tests/test_gpu_fuzz.py."""
import sys, os
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (this file lives in tests/: test infrastructure, the only place beside smoke() and the bench baseline that may use the oracle)
for _p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tools')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import psfmc_oracle as orc
import test_gpu_random as tgr
from psfmc_amd import engine


def fuzz_cases(seed, n_cases):
    """(index, (ny, nx), case seed) of the fuzz's cases: `tgr.random_case(case seed, (ny, nx))` is the case.
    Shapes the fused back end does not take with the case's PSF are the caller's to skip."""
    rng = np.random.RandomState(seed)
    sides = [s for s in engine.FUSED_SIDES if s <= 900]
    big = [1152, 1280, 1536, 2048]
    for i in range(n_cases):
        if i % 10 == 9:
            shape = (int(rng.choice(big)), int(rng.choice([64, 96, 128, 200, 300, 336, 512])))
            if rng.rand() < 0.5: shape = shape[::-1]
        elif i % 10 == 8:
            shape = (int(rng.randint(40, 400)) * 2, int(rng.randint(40, 400)) * 2)       # any even side: embedded if not built
        else:
            shape = (int(rng.choice(sides)), int(rng.choice(sides)))
        yield i, shape, 5000 + i


def fuzz_bound(field, imgs, want):
    """Largest |got - want| accepted.  A log-likelihood near zero is a cancellation of terms thousands of times larger
    (case 137 of seed 21: 548 out of 232 434, both back ends 3e-7 from the oracle): the bound is relative to the sum of
    the terms' magnitudes as well."""
    g = ~field.bad_px
    ivm = imgs['composite_ivm'][g]
    cond = 0.5 * float(np.abs((field.sci - imgs['convolved_model'])[g] ** 2 * ivm).sum() + np.abs(np.log(0.5 / np.pi * ivm)).sum())
    return max(2e-10 * abs(want), 5e-12 * cond)


def main(seed, n_cases):
    bad = 0
    for i, shape, case_seed in fuzz_cases(seed, n_cases):
        case = tgr.random_case(case_seed, shape)
        if not engine.fused_supports(shape[0], shape[1], case['psfs'][0].shape):
            continue
        field = orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'], mag_zp=case['zp'])
        want, imgs = orc.evaluate(field, case['comps'], case['psf_index'], raw_dtype=np.float64)
        want = want if np.isfinite(want) else -np.inf
        # (the fixed-component form: psf_index is all that is free, so the two walkers are one vector; the
        # distinct-walker form runs in tests/test_gpu_fuzz.py)
        n_free = 1 if len(case['psfs']) > 1 else 0
        theta = np.zeros((2, n_free)) + float(case['psf_index'])
        model = tgr.build(case, 'fused')
        got = model.log_likelihood_batch(theta)
        ok = (got[0] == got[1]) and ((not np.isfinite(want) and got[0] == -np.inf) or (np.isfinite(want) and abs(got[0] - want) <= fuzz_bound(field, imgs, want)))
        print(shape, 'transform', (int(model.engine.get_option('transform_ny')), int(model.engine.get_option('transform_nx'))), 'ok' if ok else 'MISMATCH %r %r' % (got[0], want), flush=True)
        bad += 0 if ok else 1
        model.close()
    print('mismatches:', bad)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 0, int(sys.argv[2]) if len(sys.argv) > 2 else 60)
