"""The half-step API that every multi-GPU fit goes through (psfmc_stretch_open / _half_eval / _half_accept /
_accumulate / _close, psfmc_get / set_accumulated_sums) on every model form, driven by tests/shard_driver.py as three
(and four) ranks inside one process.  `psfmc_stretch_half_eval` is the one caller of the likelihood pipeline with a
walker offset -- after the records of the whole half were derived at offset 0 -- and on the caller's stream: a wrong
offset of any per-walker array outside the prep record (auxiliary vectors, the general / Fourier / spiral / radial /
integrated constants, the extra images, the power tables, the skip flags) evaluates a walker with another walker's
values.

Per case (tests/shard_driver.py CASES; fields of 70 x 96 -- embedded in y, rectangular, a window offset -- and 64 x
320 -- the power-table rasteriser --, two PSFs with a free index alternating over the walkers, at most ten free
parameters, six iterations):
  (a) every rank's chain, log-probabilities, final positions and acceptance counts are bit-identical,
  (b) and bit-identical to ONE `DeviceEnsembleSampler` on one more context, run with `speculate` -1 and 0 (the header's
      promise "the result equals psfmc_stretch_run's chain bit for bit": no tolerance),
  (c) the gathered log-posterior of EVERY proposal and the log-posterior of every start position equal the contract's
      (tests/extra_contract.py + log_priors_batch) to `check_ll`'s 1e-9 |ll| -- -inf exactly where the prior is; with
      a Ferrer, no compared position within EDGE_MARGIN of its cut-off (asserted first); the stored log-probabilities
      are those values bit for bit,
  (d) the run is not vacuous (`shard_driver.conditions`; tests/test_sharded_forms_inputs.py holds the inputs to three
      times as much on the host): a proposal with a non-finite prior in a block with lo > 0, an accepted move in every
      non-empty block, both PSFs in blocks with lo > 0,
  (e) posterior sums under `linear_accumulation` 1 and 0 (hipFFT: 0): each rank's count before the exchange is its
      block x iterations, the total W x iterations; after the exchange every rank's images equal the one context's to
      1e-12 of the image's largest finite value (tests/test_gpu_multirank.py's bound) and the contract's means to
      `test_gpu_random.image_tol`,
  (f) with every rank on its own stream, (a) and (b) bit for bit.
Then the sums exchange alone on the embedded field, and the refusals."""
import numpy as np
import pytest

import extra_contract as xc
import shard_driver as sd
import test_gpu_random as tgr
from psfmc_amd.engine import NativeError
from psfmc_amd.parallel import shard_bounds
from test_gpu_extra_image_fields import check_ll

pytestmark = pytest.mark.gpu

EINVAL = -1                 # include/psfmc_hip.h PSFMC_EINVAL
POST_BOUND = 1e-12          # of the image's largest finite value (tests/test_gpu_multirank.py)


def one_context(model, p0, n_w, seed, speculate, linear):
    """The same ensemble on ONE context through `DeviceEnsembleSampler` (psfmc_stretch_run): (sampler, images)."""
    from psfmc_amd.sampler import DeviceEnsembleSampler
    eng = model.engine
    eng.set_option('speculate', speculate)
    if linear is not None:
        eng.set_option('linear_accumulation', linear)
        assert eng.get_option('linear_accumulation') == linear
    model.reset_images()
    before = eng.get_option('speculated_runs')
    samp = DeviceEnsembleSampler(n_w, model, accumulate=True, live_dangerously=n_w < 2 * model.num_params)
    samp.random_state = sd.random_state(seed)
    list(samp.sample(p0, iterations=sd.N_ITER))
    if model._backend == 'fused':
        assert eng.get_option('speculated_runs') - before == (1 if speculate < 0 else 0)
    assert model.accumulated_samples == n_w * sd.N_ITER
    return samp, {k: v.copy() for k, v in model.collect_posterior_images().items()}


def contract_means(kind, shape, model, p0, q, acc):
    """The contract's posterior means over every (walker, iteration) of the chain, and the images they are made of."""
    n_iter, _, half = acc.shape
    cur = [sd.contract_of(kind, shape, model, t)[4] for t in p0]
    seen, sums, n = {}, None, 0
    with np.errstate(all='ignore'):
        for it in range(n_iter):
            for h in range(2):
                for j in np.flatnonzero(acc[it, h]):
                    cur[h * half + j] = sd.contract_of(kind, shape, model, q[it, h, j])[4]
            for imgs in cur:
                seen[id(imgs)] = imgs
                add = {k: (1.0 / v if k == 'composite_ivm' else v) for k, v in imgs.items()}
                sums = add if sums is None else {k: sums[k] + add[k] for k in add}
                n += 1
        means = {k: (n / v if k == 'composite_ivm' else v / n) for k, v in sums.items()}
    return means, list(seen.values())


def check_means(post, means, refs, tag):
    """`test_gpu_random.check_posterior_sums`' comparison of images already collected."""
    worst = 0.0
    for kind, want in means.items():
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(post[kind]), fin), (tag, kind, 'posterior')
        scale = max(np.abs(want[fin]).max(), 1e-300)
        err = np.abs(post[kind][fin] - want[fin]).max() / scale
        assert err <= tgr.image_tol(kind, refs), (tag, kind, err)
        worst = max(worst, err / tgr.image_tol(kind, refs))
    return worst


def same_images(got, want, tag):
    worst = 0.0
    for kind, img in want.items():
        fin = np.isfinite(img)
        assert np.array_equal(np.isfinite(got[kind]), fin), (tag, kind)
        err = np.abs(got[kind][fin] - img[fin]).max() / np.abs(img[fin]).max()
        assert err <= POST_BOUND, (tag, kind, err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize('backend,kind,shape,ranks,n_w,seed', sd.CASES, ids=sd.case_id)
def test_blocks_equal_one_context_and_the_contract(backend, kind, shape, ranks, n_w, seed):
    tag = '%s %s %dx%d R=%d W=%d' % ((backend, kind) + shape + (ranks, n_w))
    models = sd.make_models(kind, shape, ranks + 1, backend, max_walkers=n_w)
    single, models = models[-1], models[:-1]
    dim, half = single.num_params, n_w // 2
    assert all(m._backend == backend for m in models) and (n_w >= 2 * dim or n_w == 6)
    p0 = sd.start_ensemble(single, shape, n_w, seed)
    draws = sd.draw(sd.random_state(seed), sd.N_ITER, n_w, dim)
    lnp0 = models[0].log_posterior_batch(p0)
    if backend == 'fused':
        if shape == sd.WIDE:
            assert all(m.engine.get_option('pow_tabs') == 1 for m in models + [single]), tag
        else:
            assert single.engine.get_option('transform_ny') > shape[0], tag                  # embedded in y
    # the two runs: (speculate of the one context, linear_accumulation, every rank on its own stream)
    runs = [(-1, 1, False), (0, 0, True), (-1, 1, True)] if backend == 'fused' else [(-1, None, False), (0, None, True)]
    first, worst_post, worst_mean = None, 0.0, 0.0
    for speculate, linear, streams in runs:
        samp, want_post = one_context(single, p0, n_w, seed, speculate, linear)
        for m in models:
            m.reset_images()
            if linear is not None:
                m.engine.set_option('linear_accumulation', linear)
                assert m.engine.get_option('linear_accumulation') == linear
        res = sd.run_blocks(models, p0, lnp0, draws, accumulate=True, streams=streams)
        for r in range(ranks):                                                      # (a), (b), (f)
            assert np.array_equal(res['chain'][r], samp.chain), (tag, r, streams)
            assert np.array_equal(res['lnchain'][r], samp.lnprobability), (tag, r, streams)
            assert np.array_equal(res['pos'][r], samp.chain[:, -1]), (tag, r, streams)
            assert np.array_equal(res['lnp'][r], samp.lnprobability[:, -1]), (tag, r, streams)
            assert np.array_equal(res['nacc'][r], samp.naccepted.astype(np.int64)), (tag, r, streams)
        if first is None:
            first = res
            q, acc = sd.replay(p0, res['chain'][0], draws[0], draws[2])
            means, refs = contract_means(kind, shape, single, p0, q, acc)
        else:
            assert np.array_equal(res['gathered'], first['gathered']), (tag, streams)
        # (e) the counts, then every rank's images after the exchange
        assert res['own'] == [(hi - lo) * sd.N_ITER for lo, hi in (shard_bounds(n_w, ranks, r) for r in range(ranks))]
        assert res['total'] == n_w * sd.N_ITER
        for r, m in enumerate(models):
            assert m.accumulated_samples == n_w * sd.N_ITER
            post = m.collect_posterior_images()
            worst_post = max(worst_post, same_images(post, want_post, (tag, r, linear)))
            worst_mean = max(worst_mean, check_means(post, means, refs, (tag, r, linear)))
        check_means(want_post, means, refs, (tag, 'one context', linear))
    # (c) every proposal and every start position against the contract; the stored log-probabilities are those values
    got = first['gathered']
    worst_ll, cur = 0.0, lnp0.copy()
    for w in range(n_w):
        lp, ll, prior, margin, _ = sd.contract_of(kind, shape, single, p0[w])
        assert margin >= xc.EDGE_MARGIN, (tag, 'start', w, margin)
        worst_ll = max(worst_ll, check_ll(lnp0[w], lp, ll, (tag, 'start', w)))
    prior_q = np.empty(acc.shape)
    for it in range(sd.N_ITER):
        for h in range(2):
            for j in range(half):
                lp, ll, prior, margin, _ = sd.contract_of(kind, shape, single, q[it, h, j])
                prior_q[it, h, j] = prior
                if not np.isfinite(prior):
                    assert prior == -np.inf and got[it, h, j] == -np.inf, (tag, it, h, j, got[it, h, j])
                    continue
                assert margin >= xc.EDGE_MARGIN, (tag, it, h, j, margin)
                worst_ll = max(worst_ll, check_ll(got[it, h, j], lp, ll, (tag, it, h, j)))
            mine = slice(0, half) if h == 0 else slice(half, n_w)
            cur[mine] = np.where(acc[it, h], got[it, h], cur[mine])
        assert np.array_equal(first['lnchain'][0][:, it], cur), (tag, it)
    # (d) the run is not vacuous
    cond = sd.conditions(q, prior_q, acc, ranks)
    assert cond['blocks'] == ([4, 3, 3] if n_w == 20 else [1, 1, 1, 0]), cond
    assert cond['outside_behind'] >= 1 and cond['psf_min'] >= 1, (tag, cond)
    assert cond['accepted_min' if n_w >= 20 else 'accepted_rank_min'] >= 1, (tag, cond)
    eng = models[1].engine
    print('%s: worst log-posterior relative error %.2e; posterior images: %.2e of the largest value from one context, '
          '%.1e of image_tol from the contract; pow_tabs %g, pow_tabs_built %g, raster_group %g; %s'
          % (tag, worst_ll, worst_post, worst_mean, eng.get_option('pow_tabs'), eng.get_option('pow_tabs_built'),
             eng.get_option('raster_group'), cond))
    for m in models + [single]:
        m.close()


# -- the sums exchange alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('linear', [1, 0])
def test_sums_exchange_on_an_embedded_field(linear):
    """Kind X on 70 x 96 (the transform is taller: the embedded branches of psfmc_get / set_accumulated_sums, which copy
    the image's window out of and into the transform).  `set(*get())` leaves the images bit-identical; a context that
    accumulated nothing returns all-zero sums and count 0; k samples accumulated after a `set` of n give count n + k
    and the means of one context that accumulated all n + k (1e-12 of the largest finite value); each of the four
    planes read back has the image's shape and equals the one context's plane pixel for pixel to the same bound --
    and the raw and convolved planes the contract's sums to `image_tol`, so that a window shifted by a row or a column
    in both calls alike fails too."""
    kind, shape, n, k = 'X', sd.SHAPE, 13, 7
    whole, part, rest = sd.make_models(kind, shape, 3, max_walkers=n + k)
    thetas = sd.start_ensemble(whole, shape, n + k, 7)
    for m in (whole, part, rest):
        m.engine.set_option('linear_accumulation', linear)
        assert m.engine.get_option('transform_ny') > shape[0] and m.engine.get_option('transform_nx') == shape[1]
    sums, count = rest.engine.accumulated_sums()
    assert count == 0 and sums.shape == (4,) + shape and not sums.any()
    whole.engine.accumulate_theta(thetas)
    want, n_want = whole.engine.accumulated()
    assert n_want == n + k
    sums_all, count = whole.engine.accumulated_sums()
    assert count == n + k and sums_all.shape == (4,) + shape and np.all(np.isfinite(sums_all))
    whole.engine.set_accumulated_sums(sums_all, count)
    again, n_again = whole.engine.accumulated()
    assert n_again == n + k
    for key in want:
        assert np.array_equal(again[key], want[key], equal_nan=True), key
    back, _ = whole.engine.accumulated_sums()
    assert np.array_equal(back, sums_all)
    # n samples on one context, handed to another, k more there
    part.engine.accumulate_theta(thetas[:n])
    sums_n, count = part.engine.accumulated_sums()
    assert count == n
    rest.engine.set_accumulated_sums(sums_n, count)
    rest.engine.accumulate_theta(thetas[n:])
    sums_got, count = rest.engine.accumulated_sums()
    assert count == n + k and sums_got.shape == (4,) + shape
    for plane in range(4):
        scale = np.abs(sums_all[plane]).max()
        assert scale > 0 and np.abs(sums_got[plane] - sums_all[plane]).max() <= POST_BOUND * scale, plane
        for shift in ((1, 0), (0, 1)):                                   # (the bound tells a shifted window apart)
            assert np.abs(np.roll(sums_all[plane], shift, (0, 1)) - sums_all[plane]).max() > 1e3 * POST_BOUND * scale
    got, n_got = rest.engine.accumulated()
    same_images(got, want, ('exchange', linear))
    refs = [sd.contract_of(kind, shape, whole, t)[4] for t in thetas]
    for plane, key in enumerate(('raw_model', 'convolved_model')):
        total = sum(r[key] for r in refs)
        assert np.abs(sums_got[plane] - total).max() <= tgr.image_tol(key, refs) * np.abs(total).max(), key
    # ... and through the model, as `MultiComponentModel.reduce_accumulated` leaves it
    rest._device_samples = rest.accumulated_samples = n_got
    post = rest.collect_posterior_images()
    for key in want:
        assert np.array_equal(post[key], got[key], equal_nan=True), key
    for m in (whole, part, rest):
        m.close()


# -- refusals --------------------------------------------------------------------------------------------------------
def refused(call, *args):
    with pytest.raises(NativeError) as err:
        call(*args)
    assert err.value.code == EINVAL, err.value


def test_refusals_leave_the_run_alone():
    """A half-step call before `stretch_open`, `it` or `h` out of range, a block reaching past the half-ensemble, an
    accumulation block reaching past the ensemble and a NULL output with n > 0 are each PSFMC_EINVAL; made before every
    half-step of rank 0, they leave the chain the one context's, bit for bit."""
    import torch
    kind, shape, ranks, n_w, seed = 'X', sd.SHAPE, 3, 20, 7
    models = sd.make_models(kind, shape, ranks + 1, max_walkers=n_w)
    single, models = models[-1], models[:-1]
    p0 = sd.start_ensemble(single, shape, n_w, seed)
    draws = sd.draw(sd.random_state(seed), sd.N_ITER, n_w, single.num_params)
    lnp0 = models[0].log_posterior_batch(p0)
    samp, _ = one_context(single, p0, n_w, seed, -1, 1)
    out = torch.zeros(n_w, dtype=torch.float64, device='cuda:0')
    eng, half = models[0].engine, n_w // 2
    refused(eng.stretch_half_eval, 0, 0, 0, 1, out.data_ptr())
    refused(eng.stretch_half_accept, 0, 0, out.data_ptr())
    refused(eng.stretch_accumulate, 0, 1)
    calls = []

    def intrude(eng, it, h):
        for bad_it, bad_h in ((sd.N_ITER, h), (-1, h), (it, 2), (it, -1)):
            refused(eng.stretch_half_eval, bad_it, bad_h, 0, 1, out.data_ptr())
            refused(eng.stretch_half_accept, bad_it, bad_h, out.data_ptr())
        refused(eng.stretch_half_eval, it, h, half - 1, 2, out.data_ptr())
        refused(eng.stretch_half_eval, it, h, -1, 2, out.data_ptr())
        refused(eng.stretch_half_eval, it, h, 0, half + 1, out.data_ptr())
        refused(eng.stretch_accumulate, n_w - 1, 2)
        refused(eng.stretch_accumulate, -1, 2)
        refused(eng.stretch_half_eval, it, h, 0, 1, 0)
        refused(eng.stretch_half_accept, it, h, 0)
        calls.append((it, h))
    res = sd.run_blocks(models, p0, lnp0, draws, accumulate=True, intrude=intrude)
    torch.cuda.synchronize()
    assert len(calls) == 2 * sd.N_ITER and not out.cpu().numpy().any()
    for r in range(ranks):
        assert np.array_equal(res['chain'][r], samp.chain), r
        assert np.array_equal(res['lnchain'][r], samp.lnprobability), r
        assert np.array_equal(res['nacc'][r], samp.naccepted.astype(np.int64)), r
    assert res['total'] == n_w * sd.N_ITER
    for m in models + [single]:
        m.close()
