"""The half-step API (psfmc_stretch_open / _half_eval / _half_accept / _accumulate / _close, psfmc_get / set_accumulated_sums)
driven as R ranks would drive it, inside ONE process on one GPU: R contexts of the same model, every one opened with
the same ensemble and random numbers, rank r evaluating block `shard_bounds(half, R, r)` of every half-step's proposals
into its slice of one device vector, every rank accepting from the whole vector (no subprocess, no torch.distributed).
Plus what tests/test_gpu_sharded_forms.py and tests/test_sharded_forms_inputs.py share: the lean model kinds (at most
ten free parameters: 20 walkers are an ensemble), their fields and start ensembles, the proposals of a run rebuilt
on the host, the contract's log-posterior of a vector, and the conditions a run has to meet for the tests to mean
anything (`conditions`)."""
import numpy as np

import extra_contract as xc
from psfmc_amd.distributions import Uniform
from psfmc_amd.parallel import shard_bounds

FREE = xc.FREE
SHAPE = (70, 96)            # 70 is no built side: embedded in y, rectangular, a window offset
WIDE = (64, 320)            # 320 pixels per row: the power-table rasteriser
WIDTH = 1e-2                # the start ball about the scene (tests/test_gpu_law_fields.py lean_model's)
KINDS = ('P', 'I', 'G', 'F', 'M', 'S', 'R', 'X')
N_ITER = 6
# (back end, kind, shape, ranks, walkers, seed): three ranks on 20 walkers -- half-ensemble blocks 4, 3, 3, accumulation
# blocks 7, 7, 6 --; four ranks on 6 walkers: half-ensemble blocks 1, 1, 1, 0, accumulation blocks 2, 2, 1, 1.  The
# seeds (start ball: seed, random numbers: seed + 100) are chosen on the host (tests/test_sharded_forms_inputs.py)
# (the hipFFT cases follow the fused ones of their kind: the contract's values of a kind are kept while it lasts)
CASES = [(b, k, SHAPE, 3, 20, 7) for k in KINDS for b in (('fused', 'hipfft') if k in 'SX' else ('fused',))] + \
        [('fused', 'X', SHAPE, 4, 6, 4), ('fused', 'X', WIDE, 3, 20, 7), ('fused', 'M', WIDE, 3, 20, 7)]


def case_id(v):
    return '%dx%d' % v if isinstance(v, tuple) else str(v)


def random_state(seed):
    return np.random.RandomState(seed + 100).get_state()


def lean_spec(kind, shape):
    """`make_model`'s (sersics, slope) of a kind, constants from walker 0 of `scene(shape)` until at most ten free
    parameters are left (with `lean=True`: Sky adu, PointSource mag, PSF_Index and seven more).  Fresh prior objects
    per call.  P plain; I a pixel-integrated Sersic; G a boxy Sersic (boxiness free) and a free tilted sky; F a boxy
    Sersic with modes 1 and 4; M modes + an integrated Sersic + a free tilted sky; S a boxy spiral; R a boxy Moffat, a
    boxy Ferrer (boxiness free) and a tilted sky; X a boxy Ferrer with a spiral and modes, an integrated Sersic, a
    Moffat and a tilted sky."""
    sky, _, s = xc.scene(shape)
    box = lambda: Uniform(loc=-1.5, scale=4.0)
    fix = lambda k, *names: {n: s[k][n] for n in names}
    arms = dict(r_in=2.0, r_out=9.0, winding=FREE, inclination=35.0, sky_angle=20.0)
    moffat = lambda k, *names: ('moffat', {{'moffat_beta': 'beta'}.get(n, n): s[k][n] for n in names})
    ferrer = lambda k, *names: ('ferrer', {{'ferrer_alpha': 'alpha', 'ferrer_beta': 'beta'}.get(n, n): s[k][n]
                                           for n in names})
    if kind == 'P':
        return dict(sersics=[{}], slope=xc.ABSENT)
    if kind == 'I':
        return dict(sersics=[dict(integrate=True)], slope=xc.ABSENT)
    if kind == 'G':
        return dict(sersics=[dict(boxiness=box(), fixed=fix(0, 'reff_b', 'index'))], slope=FREE)
    if kind == 'F':
        return dict(sersics=[dict(boxiness=FREE, fourier={1: (FREE, FREE), 4: (0.1, FREE)},
                                  fixed=fix(0, 'reff_b', 'index'))], slope=xc.ABSENT)
    if kind == 'M':
        return dict(sersics=[dict(boxiness=FREE, fourier={1: (FREE, 30.0), 4: (0.1, FREE)},
                                  fixed=fix(0, 'xy', 'reff_b', 'index')),
                             dict(integrate=True, fixed=fix(1, 'xy', 'reff', 'reff_b', 'index'))], slope=FREE)
    if kind == 'S':
        return dict(sersics=[dict(boxiness=box(), spiral=dict(arms, r_out=FREE), fixed=fix(0, 'reff_b', 'index', 'reff'))],
                    slope=xc.ABSENT)
    if kind == 'R':
        return dict(sersics=[dict(law=moffat(0, 'xy', 'fwhm_b'), boxiness=FREE),
                             dict(law=ferrer(1, 'xy', 'r_out_b', 'ferrer_beta'), boxiness=box())], slope=sky['slope'])
    if kind == 'X':
        return dict(sersics=[dict(law=ferrer(0, 'xy', 'r_out_b', 'ferrer_beta', 'ferrer_alpha'), boxiness=box(),
                                  spiral=dict(arms), fourier={1: (FREE, 30.0), 4: (0.1, -100.0)}),
                             dict(integrate=True, fixed=fix(1, 'xy', 'reff', 'reff_b', 'index')),
                             dict(law=moffat(2, 'xy', 'fwhm', 'fwhm_b', 'moffat_beta'))], slope=sky['slope'])
    raise KeyError(kind)


def field_of(kind, shape):
    """(case, oracle field): `extra_contract.law_case`'s of the kind (the plain model on G's, which plants nothing
    further) -- the lean kinds keep an integrated Sersic and a Ferrer in the slots of `extra_contract.KINDS`."""
    return xc.law_case(kind if kind in xc.KINDS else 'G', shape)


def make_models(kind, shape, n, backend='fused', max_walkers=24):
    case, _ = field_of(kind, shape)
    return [xc.make_model(case, backend=backend, max_walkers=max_walkers, lean=True, **lean_spec(kind, shape))
            for _ in range(n)]


def start_ensemble(model, shape, n_w, seed, width=WIDTH):
    """[n_w, P]: a ball about walker 0 of the scene, PSF_Index alternating over the walkers; every prior finite."""
    sky, ps, sersics = xc.scene(shape)
    n_s = sum(isinstance(c, xc.Sersic) for c in model.components)
    base = xc.theta_of(model, sky, ps, sersics[:n_s], psf=0.0)
    assert model.param_names[-1] == 'PSF_Index'
    p0 = base + np.random.RandomState(seed).normal(size=(n_w, len(base))) * width
    p0[:, -1] = np.arange(n_w) % 2
    assert np.all(np.isfinite(model.log_priors_batch(p0)))
    return p0


def draw(state, n_iter, n_w, dim, a=2.0):
    """(z, lz, partner, log_u), each [n_iter, 2, n_w / 2], from `state` in `DeviceEnsembleSampler._draw`'s order."""
    rs = np.random.RandomState()
    rs.set_state(state)
    half = n_w // 2
    z = np.empty((n_iter, 2, half))
    partner = np.empty((n_iter, 2, half), dtype=np.int32)
    log_u = np.empty((n_iter, 2, half))
    for it in range(n_iter):
        for h in range(2):
            z[it, h] = ((a - 1.0) * rs.rand(half) + 1) ** 2.0 / a
            partner[it, h] = rs.randint(half, size=(half,))
            log_u[it, h] = np.log(rs.rand(half))
    return z, (dim - 1.0) * np.log(z), partner, log_u


def replay(p0, chain, z, partner):
    """(proposals [n_iter, 2, half, P], accepted [n_iter, 2, half]) of a run from its chain [W, n_iter, P]: the
    proposal of walker j of half h is c - z (c - s) with c its partner in the other half as it stood then; a walker
    accepted where its position changed."""
    n_w, n_iter, dim = chain.shape
    half = n_w // 2
    q = np.empty((n_iter, 2, half, dim))
    acc = np.zeros((n_iter, 2, half), dtype=bool)
    prev = np.array(p0, dtype=np.float64)
    for it in range(n_iter):
        now = chain[:, it]
        for h in range(2):
            s = prev[:half] if h == 0 else prev[half:]
            c = (prev[half:] if h == 0 else now[:half])[partner[it, h]]
            q[it, h] = c - z[it, h][:, None] * (c - s)
            mine = now[:half] if h == 0 else now[half:]
            acc[it, h] = np.any(mine != s, axis=1)
            assert np.all(~acc[it, h] | np.all(np.abs(mine - q[it, h]) <= 1e-12 * np.abs(q[it, h]).max(), axis=1))
        prev = now
    return q, acc


_contract = {}


def contract_of(kind, shape, model, theta):
    """(log-posterior, log-likelihood, log-prior, smallest |1 - x| of the Ferrers, images) of one vector from the
    contract: `contract_with_state`'s log-likelihood + `log_priors_batch`; (-inf, -inf, prior, inf, None), nothing
    evaluated, where the prior is not finite.  Kept per vector: the runs of a case share their proposals."""
    key = (kind, shape, np.asarray(theta, dtype=np.float64).tobytes())
    if _contract and next(iter(_contract))[:2] != key[:2]:
        _contract.clear()                                            # (one kind's images at a time)
    if key not in _contract:
        prior = float(model.log_priors_batch(np.asarray(theta)[None])[0])
        if not np.isfinite(prior):
            _contract[key] = (-np.inf, -np.inf, prior, np.inf, None)
        else:
            ll, images, _, margin = xc.contract_with_state(model, field_of(kind, shape)[1], theta)
            _contract[key] = (ll + prior, ll, prior, margin, images)
    return _contract[key]


def conditions(q, prior, acc, ranks, n_psf=2):
    """What keeps a run from passing vacuously, counted: proposals with a non-finite prior in blocks with lo > 0,
    the fewest accepted moves of any non-empty block (half h, rank r), the fewest evaluated proposals of any PSF in
    blocks with lo > 0.  q [n_iter, 2, half, P], prior and acc [n_iter, 2, half]."""
    half = q.shape[2]
    bounds = [shard_bounds(half, ranks, r) for r in range(ranks)]
    behind = np.arange(half) >= bounds[0][1]                      # walkers of the blocks with lo > 0
    fin = np.isfinite(prior)
    psf = np.rint(q[..., -1])
    return dict(outside_behind=int((~fin[:, :, behind]).sum()),
                accepted_min=min(int(acc[:, h, lo:hi].sum()) for h in range(2) for lo, hi in bounds if hi > lo),
                accepted_rank_min=min(int(acc[:, :, lo:hi].sum()) for lo, hi in bounds if hi > lo),
                psf_min=min(int((fin & (psf == k))[:, :, behind].sum()) for k in range(n_psf)),
                blocks=[hi - lo for lo, hi in bounds])


def run_blocks(models, p0, lnp0, draws, accumulate=False, streams=False, intrude=None):
    """The run.  models: R models (their contexts on device 0), every one opened with the same arguments; per
    half-step rank r evaluates its block into its slice of that half-step's device vector, the device is
    synchronised (streams: rank r's own stream first), every rank accepts from the whole vector.  accumulate: rank r
    adds its block of `shard_bounds(W, R, r)` after every iteration; after `stretch_close` the ranks' sums are added
    on the host and the total written to every rank.  intrude(eng, it, h): called before every half-step of rank 0
    (the refusals).  Returns dict(chain, lnchain, pos, lnp, nacc: per rank; gathered [n_iter, 2, half]; own: each
    rank's count before the exchange; total)."""
    import torch
    ranks, n_w = len(models), len(p0)
    half, n_iter = n_w // 2, draws[0].shape[0]
    engines = [m.engine for m in models]
    nacc = [np.zeros(n_w, dtype=np.int64) for _ in engines]
    own = [torch.cuda.Stream() for _ in engines] if streams else None
    ptr = [s.cuda_stream if streams else None for s in (own or engines)]
    gathered = torch.full((n_iter, 2, half), float('nan'), dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    for r, eng in enumerate(engines):
        eng.stretch_open(p0, lnp0, *draws, nacc[r], store=True)
    for it in range(n_iter):
        for h in range(2):
            if intrude is not None:
                intrude(engines[0], it, h)
            row = gathered[it, h]
            for r, eng in enumerate(engines):
                lo, hi = shard_bounds(half, ranks, r)
                eng.stretch_half_eval(it, h, lo, hi - lo, row.data_ptr() + 8 * lo if hi > lo else 0, ptr[r])
                if streams:
                    own[r].synchronize()
            torch.cuda.synchronize()
            for r, eng in enumerate(engines):
                eng.stretch_half_accept(it, h, row.data_ptr(), ptr[r])
        if accumulate:
            for r, eng in enumerate(engines):
                lo, hi = shard_bounds(n_w, ranks, r)
                eng.stretch_accumulate(lo, hi - lo, ptr[r])
    torch.cuda.synchronize()
    out = [eng.stretch_close(nacc[r], ptr[r]) for r, eng in enumerate(engines)]
    res = dict(pos=[o[0] for o in out], lnp=[o[1] for o in out], chain=[o[2] for o in out],
               lnchain=[o[3] for o in out], nacc=nacc, gathered=gathered.cpu().numpy(), own=None, total=0)
    if accumulate:
        shares = [eng.accumulated_sums() for eng in engines]
        res['own'] = [n for _, n in shares]
        res['total'] = sum(res['own'])
        total = sum(s for s, _ in shares)
        for m, eng in zip(models, engines):
            eng.set_accumulated_sums(total, res['total'])
            m._device_samples = m.accumulated_samples = res['total']
    return res
