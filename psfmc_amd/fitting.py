"""
`model_galaxy_mcmc`: the reference's entry point (psfMC/fitting.py:13-113) on the
batched GPU log-posterior.  Same arguments and outputs (trace database
`<output_name>_db.fits`, posterior images `<output_name>_<type>.fits`); every
half-ensemble proposal is one GPU batch, and the per-iteration image accumulation
(`fitting.py:83`) evaluates the walkers' current positions in one batch instead of
carrying five images back from every proposal.
"""
import os
from collections import OrderedDict
from warnings import warn

import numpy as np

from .analysis import check_convergence_autocorr, save_posterior_images, default_filetypes
from .database import Table, save_database, load_database
from .models import JointModel, MultiComponentModel
from .sampler import EnsembleSampler, DeviceEnsembleSampler, moves_label
from .utils import print_progress


def _rank_group(group, device):
    """The `parallel.RankGroup` of this run, or None for a single process.  'auto' looks for an
    initialised torch.distributed process group and quietly settles for one process when torch
    (or its distributed package) is not importable: the single-GPU entry point needs neither."""
    if group is None:
        return None
    auto = isinstance(group, str)
    try:
        from .parallel import RankGroup
        if isinstance(group, RankGroup):
            ranks = group
        else:
            if auto:
                import torch.distributed as dist
                if not (dist.is_available() and dist.is_initialized()):
                    return None
            ranks = RankGroup(None if auto else group, 'cuda:%d' % device)
    except ImportError:
        if auto:
            return None
        raise
    return None if ranks.single else ranks


def _takes_moves(cls):
    """Whether a sampler class's constructor has a `moves` keyword."""
    import inspect
    try:
        params = inspect.signature(cls.__init__).parameters
    except (TypeError, ValueError):
        return False
    return 'moves' in params


def _burn_and_sample(sampler, model, param_vec, burn, iterations, max_iterations, convergence_check,
                     host_acc, device_acc, quiet):
    """The reference's sampling flow (psfMC/fitting.py:56-86): burn-in, reset, sampling with posterior
    images accumulated (on the device inside the sampler if `device_acc`, else from the current positions
    after every iteration if `host_acc`), until `convergence_check` passes or `max_iterations` rounds.
    Returns whether it converged."""
    lnprob = None
    for step, result in enumerate(sampler.sample(param_vec, iterations=burn)):
        param_vec, lnprob = result[0], result[1]
        sampler.clear_blobs()
        if not quiet:
            print_progress(step, burn, 'Burning')
    sampler.reset()

    if device_acc:              # images are summed inside the device sampling loop
        sampler.accumulate = True
    for sampling_iter in range(max_iterations):
        for step, result in enumerate(sampler.sample(param_vec, lnprob0=lnprob,
                                                     iterations=iterations)):
            param_vec, lnprob = result[0], result[1]
            if host_acc and not device_acc:   # current positions, summed on the GPU
                model.accumulate_samples(param_vec)
            sampler.clear_blobs()
            if not quiet:
                print_progress(step, iterations, 'Sampling')
        if convergence_check(sampler):
            return True
        warn('Not yet converged after {:d} iterations:'.format((sampling_iter + 1) * iterations))
        convergence_check(sampler, verbose=0 if quiet else 1)
    return False


_NO_EVIDENCE = (float('nan'), float('nan'))


def _burn_and_sample_tempered(sampler, pos, burn, iterations, accumulate, quiet):
    """The tempered fits' flow: burn-in from `pos`, reset, `iterations` sampling iterations with the beta = 1
    rung's posterior images accumulated inside the sampler, then `log_evidence()` of the sampling iterations
    ((nan, nan) without a second rung or without iterations).  One text for a ladder and for a set of ladders
    (a sampler with `fields`): the set's yields and the returned evidences are lists over fields."""
    fields = getattr(sampler, 'fields', None)

    def run(n, label, *state):
        for step, result in enumerate(sampler.sample(*state, iterations=n)):
            state = (result[:3] if fields is None else
                     tuple(np.array([r[j] for r in result]) for j in range(3)))       # pos, lnL, lnpi
            if not quiet:
                print_progress(step, n, label)
        return state

    state = run(burn, 'Burning', pos, None, None)
    sampler.reset()
    sampler.accumulate = bool(accumulate)
    run(iterations, 'Sampling', *state)
    sampler.accumulate = False
    evidences = [m.log_evidence(fburnin=0.0) if m.ntemps > 1 and iterations > 0 else _NO_EVIDENCE
                 for m in ([sampler] if fields is None else fields)]
    return evidences[0] if fields is None else evidences


def _seed(sampler, state, default=None):
    """`random_state=` of an entry point into a sampler, or one of `random_states=` into a set's member: a
    RandomState state tuple, an int seed, or None -- then `default()`, or with no default the sampler keeps the
    fresh generator it was built with."""
    if state is None and default is not None:
        state = default()
    if state is None:
        return
    if isinstance(state, (int, np.integer)):
        state = np.random.RandomState(int(state)).get_state()
    sampler.random_state = state


def _check_start(start, start_positions=None):
    if start not in ('prior', 'mode'):
        raise ValueError("start must be 'prior' or 'mode' (got {!r})".format(start))
    if start == 'mode' and start_positions is not None:
        raise ValueError("start='mode' draws the walkers around the mode it finds: it cannot be combined with "
                         "start_positions")


def _start_from_mode(sampler, model, chains):
    """`start='mode'` of `model_galaxy_mcmc` and `model_joint_mcmc` (a `JointModel`: the joint mode): -> (start
    positions [chains, P], header keys).  The search's prior draws and the walkers' normal deviates come from the
    sampler's random stream, which moves on past them."""
    from .mode import find_mode
    random = np.random.RandomState()
    random.set_state(sampler.random_state)
    out = _walkers_about_mode(find_mode(model, rng=random), model, chains, random)
    sampler.random_state = random.get_state()
    return out


def _start_fields_from_modes(sampler, fieldset, chains):
    """`start='mode'` of `model_fields_mcmc`: one `find_modes` search for all fields, then `_start_from_mode`'s rule
    per field, each field's draws from its own sampler's random stream -> (start positions [F][chains, P], header
    keys per field)."""
    from .mode import find_modes
    randoms = []
    for sub in sampler.fields:
        randoms.append(np.random.RandomState())
        randoms[-1].set_state(sub.random_state)
    found = find_modes(fieldset, rng=randoms)
    outs = [_walkers_about_mode(res, m, chains, random) for res, m, random in zip(found, fieldset.models, randoms)]
    for sub, random in zip(sampler.fields, randoms):
        sub.random_state = random.get_state()
    return [o[0] for o in outs], [o[1] for o in outs]


def _walkers_about_mode(found, model, chains, random):
    """Walkers mode + L z around a `ModeResult` (discrete columns take prior draws; redrawn outside the support), or
    prior draws with a warning where the curvature at the mode is not positive definite; all from `random`."""
    from .mode import draw_about_mode, default_columns, _prior_draws
    if found.ok:
        others = None
        if len(default_columns(model)) < model.num_params:       # discrete columns take prior draws
            others = _prior_draws(model, chains, random)
        param_vec = draw_about_mode(found.theta, found.cov, found.columns, chains, random,
                                    log_prior=model.log_priors_batch, others=others)
        meta = OrderedDict([('MCSTART', 'mode'), ('MCMODELP', found.lnpost)])
    else:
        warn('the curvature at the mode found (log-posterior {:.6g}) is not positive definite: the walkers start '
             'from prior draws'.format(found.lnpost))
        param_vec, meta = _prior_draws(model, chains, random), OrderedDict()
    return param_vec, meta


def _seed_fields(sampler, random_states):
    """Every member of a set seeded from `random_states`; where there is none numpy's global generator seeds
    them, in field order."""
    for f, sub in enumerate(sampler.fields):
        _seed(sub, None if random_states is None else random_states[f],
              default=lambda: int(np.random.randint(0, 2 ** 31 - 1)))


def _check_chains(chains):
    if chains < 2 or chains % 2:
        raise ValueError('chains must be an even number >= 2 (got {}): the stretch move updates the ensemble in '
                         'two halves'.format(chains))


def _chain_meta(sampler, burn, chains, converged, moves, **extra):
    """The database header of a sampler's (or member's) chain: the common keys, then `extra` in the caller's
    order, then MCMOVES when moves were given.  The order is the order in the written file."""
    meta = OrderedDict([('MCITER', sampler.chain.shape[1]), ('MCBURN', burn), ('MCCHAINS', chains),
                        ('MCCONVRG', bool(converged)), ('MCACCEPT', float(sampler.acceptance_fraction.mean()))])
    meta.update(extra)
    if moves is not None:
        meta['MCMOVES'] = moves_label(moves)
    return meta


def _tempered_meta(sampler, n_t, evidence):
    """The header keys of a tempered chain, `extra` of `_chain_meta`."""
    return OrderedDict([('MCNTEMPS', n_t), ('MCLNZ', float(evidence[0])), ('MCLNZERR', float(evidence[1])),
                        ('MCTSWAP', float(sampler.tswap_acceptance_fraction.mean()) if n_t > 1 else 0.0)])


def _load_existing(db_names, quiet, fields=False):
    """The databases of an earlier run, which skip sampling, and the evidences in their headers."""
    if not quiet:
        print('Databases already contain sampled chains, skipping sampling' if fields else
              'Database already contains sampled chains, skipping sampling')
    databases = [load_database(d) for d in db_names]
    return databases, [(float(db.meta['MCLNZ']), float(db.meta['MCLNZERR'])) if 'MCLNZ' in db.meta
                       else _NO_EVIDENCE for db in databases]


def _fields_arguments(model_files, output_names, random_states, start_positions, chains, device, n_t=None):
    """The arguments of the two fields entry points, checked: -> (fieldset, output names with their '_{}',
    chains, database names, whether the databases exist).  `chains` defaults to 2 P + 2 of the first model;
    the set holds F x chains walkers, or F x n_t x chains for ladders of n_t rungs, whose start positions are
    [T, chains, P]."""
    from .models import FieldSet
    n_f = len(model_files)
    if output_names is None:
        output_names = ['out_' + str(f).replace('.py', '') for f in model_files]
    if len(output_names) != n_f:
        raise ValueError('one output name per field')
    output_names = [o + '_{}' for o in output_names]
    if chains is None:
        first = model_files[0]
        if not isinstance(first, MultiComponentModel):
            first = MultiComponentModel(first, device=device, backend='fused', max_walkers=1)
            model_files = [first] + list(model_files[1:])
        chains = 2 * first.num_params + 2
    _check_chains(chains)
    if random_states is not None and len(random_states) != n_f:
        raise ValueError('random_states: one per field ({} given for {} fields)'.format(len(random_states), n_f))
    if start_positions is not None and len(start_positions) != n_f:
        raise ValueError('start_positions: one [{}chains, P] array per field ({} given for {} fields)'.format(
            '' if n_t is None else 'T, ', len(start_positions), n_f))
    fieldset = FieldSet(model_files, max_walkers=n_f * (n_t or 1) * chains, device=device)
    shape = (() if n_t is None else (n_t,)) + (chains, fieldset.num_params)
    for f, p in enumerate(() if start_positions is None else start_positions):
        if np.shape(p) != shape:
            raise ValueError('start_positions[{}] must be [{}], got {}'.format(
                f, ', '.join(str(s) for s in shape), np.shape(p)))
    db_names = [o.format('db') + '.fits' for o in output_names]
    have = [os.path.exists(d) for d in db_names]
    if any(have) and not all(have):
        raise ValueError('some of the fields already have a database and some do not: {}'.format(
            [d for d, h in zip(db_names, have) if h]))
    return fieldset, output_names, chains, db_names, all(have)


def model_galaxy_mcmc(model_file, output_name=None, write_fits=default_filetypes, iterations=0,
                      burn=0, chains=None, max_iterations=1,
                      convergence_check=check_convergence_autocorr, sampler_class=None,
                      device=0, backend='auto', random_state=None, accumulate=True, quiet=False,
                      group='auto', moves=None, start='prior'):
    """Model a galaxy's surface brightness with MCMC.

    model_file, output_name, write_fits, iterations, burn, chains, max_iterations,
    convergence_check: as in the reference.  Extra keywords: `sampler_class` (an
    emcee-compatible EnsembleSampler; default the built-in one), `device`,
    `backend`, `random_state` (RandomState state tuple or seed for reproducible
    runs), `accumulate` (posterior images during sampling), `group`: with an initialised
    torch.distributed process group ('auto': the default group if there is one; or a group
    object) the walkers of every half-step are sharded over the ranks, one process per GPU
    (`device` should then be the rank's LOCAL_RANK); rank 0 draws the start positions and the
    sampler's random state and writes the outputs, every rank returns the same database.
    `moves`: the sampler's proposal moves (`sampler.StretchMove`, `sampler.DEMove`, or a list of (move, weight)
    pairs; None: the stretch move, outputs byte for byte as without the keyword).  The database header then
    records them as MCMOVES, e.g. 'stretch:0.5,de:0.5'.  A `sampler_class` that does not take a `moves` keyword
    raises ValueError.
    `start`: where the walkers begin.  'prior' (default): draws from the priors, the reference's flow; outputs byte
    for byte as without the keyword.  'mode': `mode.find_mode` searches the posterior mode first and the walkers are
    drawn as mode + L z, L L^T = the mode's covariance, z from the sampler's RandomState (`mode.draw_about_mode`;
    discrete columns take prior draws); the database header then records MCSTART = 'mode' and MCMODELP, the mode's
    log-posterior.  Where the curvature at the mode is not positive definite the walkers are prior draws, with a
    warning."""
    _check_start(start)
    if output_name is None:
        output_name = 'out_' + model_file.replace('.py', '')
    output_name += '_{}'

    mc_model = model_file if isinstance(model_file, MultiComponentModel) else None
    if mc_model is None:
        # room for batches beyond the ensemble: the posterior images are recomputed from the filtered database in
        # slices of max_walkers samples (152 k samples in slices of 64 were 2300 calls, a fifth of a default fit)
        n_hint = max(chains or 0, 1024)
        mc_model = MultiComponentModel(model_file, device=device, backend=backend,
                                       max_walkers=n_hint)
    ranks = _rank_group(group, mc_model._device)
    if chains is None:
        chains = 2 * mc_model.num_params + 2
    if chains > mc_model._max_walkers:
        raise ValueError('model was built for at most {} walkers'.format(mc_model._max_walkers))

    cls = sampler_class
    if cls is None:           # walkers resident on the GPU whenever every prior can be
        mc_model.engine
        cls = EnsembleSampler if mc_model._host_priors else DeviceEnsembleSampler
    device_acc = False
    extra = {} if moves is None else {'moves': moves}
    if extra and not _takes_moves(cls):
        raise ValueError('sampler_class {} does not take a `moves` keyword'.format(getattr(cls, '__name__', cls)))
    if cls is DeviceEnsembleSampler:
        sampler = cls(chains, mc_model, group=ranks, **extra)
        device_acc = accumulate
    elif cls is EnsembleSampler:
        if ranks:
            from .parallel import ShardedLogPosterior
            evaluate = ShardedLogPosterior(mc_model, group=ranks)
        else:
            evaluate = mc_model.log_posterior_batch
        sampler = cls(chains, mc_model.num_params, batch_lnpostfn=evaluate, **extra)
    else:                      # a real emcee: batch through its pool hook
        from .batch import BatchLogPosterior
        sampler = cls(chains, mc_model.num_params, mc_model.log_posterior,
                      kwargs={'model': mc_model}, pool=BatchLogPosterior(mc_model).as_pool(), **extra)
    _seed(sampler, random_state)
    writer = ranks is None or ranks.rank == 0
    if ranks is not None:                      # one random stream for all ranks
        sampler.random_state = ranks.broadcast_object(sampler.random_state)
        quiet = quiet or not writer

    db_name = output_name.format('db') + '.fits'
    have_db = os.path.exists(db_name)
    if ranks is not None:
        have_db = ranks.broadcast_object(have_db)
    if not have_db:
        start_meta = OrderedDict()
        if start == 'mode':
            # rank 0 searches and draws; the others take its walkers (and, below, its random state)
            param_vec, start_meta = _start_from_mode(sampler, mc_model, chains) if writer else (None, None)
            if ranks is not None:
                param_vec, start_meta = ranks.broadcast_object((param_vec, start_meta))
                sampler.random_state = ranks.broadcast_object(sampler.random_state)
        else:
            param_vec = mc_model.init_params_from_priors(chains)
            if ranks is not None:
                param_vec = ranks.broadcast_object(param_vec)
        converged = _burn_and_sample(sampler, mc_model, param_vec, burn, iterations, max_iterations,
                                     convergence_check, accumulate and writer, device_acc, quiet)
        if device_acc:
            mc_model.reduce_accumulated(ranks)
        meta = _chain_meta(sampler, burn, chains, converged, moves, **start_meta)
        database = save_database(sampler, mc_model, db_name, meta_dict=meta) if writer else None
        if ranks is not None:
            ranks.broadcast_object(True)          # the file is complete
            database = database if writer else load_database(db_name)
    else:                                         # (the writer says so, whatever `quiet`)
        (database,), _ = _load_existing([db_name], quiet=not writer)

    if writer:
        save_posterior_images(mc_model, database, output_name=output_name, filetypes=write_fits)
    if ranks is not None:
        ranks.broadcast_object(True)              # outputs written
    return mc_model, database


def model_fields_mcmc(model_files, output_names=None, write_fits=default_filetypes, iterations=0, burn=0,
                      chains=None, max_iterations=1, convergence_check=check_convergence_autocorr,
                      device=0, random_states=None, start_positions=None, accumulate=True, quiet=False, moves=None,
                      start='prior'):
    """`model_galaxy_mcmc` for SEVERAL fields of one model structure at once (their image and PSF sizes may
    differ: each field's database and posterior images have its own shape), in
    one GPU context (`models.FieldSet`): every field is fitted exactly as its own `model_galaxy_mcmc`
    run would fit it -- its own ensemble of `chains` walkers, its own random stream, burn-in, sampling
    with posterior images accumulated, convergence check, trace database `<output_name>_db.fits` and
    posterior images -- but all fields advance together and every half-step's proposals of all fields
    are evaluated as ONE batch.  For surveys of many small fields (BASELINE config 5: 64 fields of
    256 x 256 with 256 walkers each, 8 per GPU), where a fit per field is dominated by fixed costs.
    The reference has no counterpart: one field per process (psfMC/fitting.py:13-113).

    model_files      model files (or MultiComponentModel objects) with the same component lists
    output_names     one per field (default 'out_<model file>')
    random_states    one RandomState state tuple or seed per field (default: numpy's global generator
                     seeds them in field order)
    start_positions  optional [F][chains, P] start positions (default: drawn from each field's priors)
    moves            as `model_galaxy_mcmc`'s (`FieldSetSampler.set_moves`; recorded as MCMOVES)
    start            'prior' (default; outputs byte for byte as without the keyword) or 'mode': ONE `mode.find_modes`
                     search finds every field's posterior mode, and each field's walkers are drawn around its own as
                     `model_galaxy_mcmc(start='mode')` draws them, from that field's random stream; each field's
                     database header records MCSTART and MCMODELP.  Not together with `start_positions`.
    Returns a list of (model, database), one per field."""
    from .sampler import FieldSetSampler
    _check_start(start, start_positions)
    fieldset, output_names, chains, db_names, have_db = _fields_arguments(
        model_files, output_names, random_states, start_positions, chains, device)
    models = fieldset.models
    sampler = FieldSetSampler(chains, fieldset, accumulate=False)
    sampler.set_moves(moves)
    _seed_fields(sampler, random_states)

    if not have_db:
        start_meta = [OrderedDict() for _ in models]
        if start == 'mode':
            start_positions, start_meta = _start_fields_from_modes(sampler, fieldset, chains)
        elif start_positions is None:
            start_positions = [m.init_params_from_priors(chains) for m in models]
        pos = np.array([np.asarray(p, dtype=np.float64) for p in start_positions])
        lnprob = None
        for step, result in enumerate(sampler.sample(pos, iterations=burn)):
            pos = np.array([r[0] for r in result])
            lnprob = np.array([r[1] for r in result])
            if not quiet:
                print_progress(step, burn, 'Burning')
        sampler.reset()
        sampler.accumulate = bool(accumulate)
        converged = [False] * len(models)
        for sampling_iter in range(max_iterations):
            for step, result in enumerate(sampler.sample(pos, lnprob0=lnprob, iterations=iterations)):
                pos = np.array([r[0] for r in result])
                lnprob = np.array([r[1] for r in result])
                if not quiet:
                    print_progress(step, iterations, 'Sampling')
            converged = [bool(convergence_check(sub)) for sub in sampler.fields]
            if all(converged):
                break
            warn('Not yet converged after {:d} iterations: fields {}'.format(
                (sampling_iter + 1) * iterations, [f for f, ok in enumerate(converged) if not ok]))
        databases = [save_database(sub, m, name, meta_dict=_chain_meta(sub, burn, chains, ok, moves, **extra))
                     for sub, m, name, ok, extra in zip(sampler.fields, models, db_names, converged, start_meta)]
    else:
        databases, _ = _load_existing(db_names, quiet, fields=True)
    for m, db, out in zip(models, databases, output_names):
        save_posterior_images(m, db, output_name=out, filetypes=write_fits)
    return list(zip(models, databases))


def model_joint_mcmc(model_files, per_field=(), output_name=None, write_fits=default_filetypes, iterations=0,
                     burn=0, chains=None, max_iterations=1, convergence_check=check_convergence_autocorr,
                     device=0, random_state=None, accumulate=True, quiet=False, moves=None, start='prior'):
    """`model_galaxy_mcmc` for ONE model fitted jointly to several exposures of the same object
    (`models.JointModel`: each field its own data, PSFs, constants and zeropoint; the parameters not named
    in `per_field` shared).  The reference's flow -- burn-in, reset, sampling with posterior images
    accumulated, convergence loop, metadata -- on the device sampler, one ensemble of `chains` walkers
    (default 2 P_joint + 2) in the joint parameters.  The reference has no counterpart (one model file per
    process, psfMC/fitting.py:13-113).

    Outputs: ONE trace database `<output_name>_db.fits` with the joint columns (metadata MCFIELDS = number
    of fields), and each field's posterior images `<output_name>_f<k>_<type>.fits` at that field's shape
    (what `save_posterior_images` writes for the field's model and the database's rows mapped to the
    field's own parameter names).  An existing database skips sampling.  `moves`: as `model_galaxy_mcmc`'s
    (recorded as MCMOVES).  `start`: as `model_galaxy_mcmc`'s -- 'mode' searches the JOINT posterior mode
    (`mode.find_mode` on the `JointModel`) and draws the walkers around it; the header then records MCSTART and
    MCMODELP.  Returns (JointModel, database)."""
    _check_start(start)
    if output_name is None:
        output_name = 'out_joint_' + str(model_files[0]).replace('.py', '')
    joint = model_files if isinstance(model_files, JointModel) else None
    if joint is None:
        # room for the image recomputation's batches (as model_galaxy_mcmc), F field records per walker
        n_f = len(model_files)
        joint = JointModel(model_files, per_field=per_field, device=device,
                           max_walkers=n_f * max(chains or 0, 1024))
    n_f = len(joint.field_models)
    if chains is None:
        chains = 2 * joint.num_params + 2
    _check_chains(chains)
    if chains * n_f > joint._max_walkers:
        raise ValueError('{} fields x {} chains exceed max_walkers={}'.format(n_f, chains, joint._max_walkers))
    sampler = DeviceEnsembleSampler(chains, joint, moves=moves)
    _seed(sampler, random_state)

    db_name = output_name + '_db.fits'
    if not os.path.exists(db_name):
        start_meta = OrderedDict()
        if start == 'mode':
            param_vec, start_meta = _start_from_mode(sampler, joint, chains)
        else:
            param_vec = joint.init_params_from_priors(chains)
        converged = _burn_and_sample(sampler, joint, param_vec, burn, iterations, max_iterations,
                                     convergence_check, False, accumulate, quiet)
        meta = _chain_meta(sampler, burn, chains, converged, moves, MCFIELDS=n_f, **start_meta)
        database = save_database(sampler, joint, db_name, meta_dict=meta)
    else:
        (database,), _ = _load_existing([db_name], quiet)

    _save_joint_images(joint, database, output_name, write_fits)
    return joint, database


def _save_joint_images(joint, database, output_name, write_fits):
    """Each field's posterior images `<output_name>_f<k>_<type>.fits` from a joint database: the rows mapped to
    the field's own parameter names, then `save_posterior_images` for the field's model."""
    theta = database.param_matrix(joint.param_names)
    for f, m in enumerate(joint.field_models):
        own = joint.field_theta(theta, f)
        cols, pos = OrderedDict(), 0
        for name, width in zip(m.param_names, m.param_lens):
            cols[name] = own[:, pos:pos + width]
            pos += width
        for name in ('lnprobability', 'walker', 'sample'):
            cols[name] = database[name]
        save_posterior_images(m, Table(cols, database.meta), output_name='{}_f{}_{{}}'.format(output_name, f),
                              filetypes=write_fits)


def model_galaxy_ptmcmc(model_file, output_name=None, write_fits=default_filetypes, iterations=0, burn=0,
                        chains=None, ntemps=16, tmax=1e6, betas=None, device=0, backend='auto', random_state=None,
                        accumulate=True, quiet=False, moves=None):
    """`model_galaxy_mcmc` on the parallel-tempered device sampler (`sampler.DeviceTemperedSampler`), for the
    Bayesian evidence of the model: burn-in, reset and `iterations` sampling iterations as the reference runs
    them, then the beta = 1 rung's database and posterior images exactly as `model_galaxy_mcmc` writes them, with
    the header keys MCNTEMPS (rungs), MCLNZ / MCLNZERR (`log_evidence()` of the sampling iterations) and MCTSWAP
    (mean swap acceptance).  The ladder is `betas`, or `default_betas(ntemps, tmax)` (defaults: DESIGN.md
    section 13).  One-field models with every prior on the device.  `moves`: as `model_galaxy_mcmc`'s, the moves
    of every rung (`DeviceTemperedSampler.set_moves`; recorded as MCMOVES).  Returns (model, database, (lnZ, err))."""
    from .sampler import DeviceTemperedSampler, default_betas
    if output_name is None:
        output_name = 'out_' + model_file.replace('.py', '')
    output_name += '_{}'
    betas = default_betas(ntemps, tmax) if betas is None else np.asarray(betas, dtype=np.float64)
    n_t = len(betas)
    mc_model = model_file if isinstance(model_file, MultiComponentModel) else None
    if mc_model is None:
        n_hint = max(chains or 0, 1024)
        n_chains = chains if chains is not None else 0
        mc_model = MultiComponentModel(model_file, device=device, backend=backend,
                                       max_walkers=max(n_hint, n_t * n_chains))
    if chains is None:
        chains = 2 * mc_model.num_params + 2
    if n_t * chains > mc_model._max_walkers:
        if isinstance(model_file, MultiComponentModel):
            raise ValueError('model was built for at most {} walkers; {} temperatures x {} walkers need more'
                             .format(mc_model._max_walkers, n_t, chains))
        mc_model.close()
        mc_model = MultiComponentModel(model_file, device=device, backend=backend, max_walkers=n_t * chains)
    mc_model.engine
    sampler = DeviceTemperedSampler(chains, mc_model, betas=betas)
    sampler.set_moves(moves)
    _seed(sampler, random_state)

    db_name = output_name.format('db') + '.fits'
    if not os.path.exists(db_name):
        pos = np.stack([mc_model.init_params_from_priors(chains) for _ in range(n_t)])
        evidence = _burn_and_sample_tempered(sampler, pos, burn, iterations, accumulate, quiet)
        meta = _chain_meta(sampler, burn, chains, check_convergence_autocorr(sampler), moves,
                           **_tempered_meta(sampler, n_t, evidence))
        database = save_database(sampler, mc_model, db_name, meta_dict=meta)
    else:
        (database,), (evidence,) = _load_existing([db_name], quiet)
    save_posterior_images(mc_model, database, output_name=output_name, filetypes=write_fits)
    return mc_model, database, evidence


def model_joint_ptmcmc(model_files, per_field=(), output_name=None, write_fits=default_filetypes, iterations=0,
                       burn=0, chains=None, ntemps=16, tmax=1e6, betas=None, device=0, random_state=None,
                       accumulate=True, quiet=False, moves=None):
    """`model_galaxy_ptmcmc` for ONE model fitted jointly to several exposures (`models.JointModel`, as
    `model_joint_mcmc` builds it): the Bayesian evidence of the joint fit, every exposure counted.  Burn-in,
    reset and `iterations` sampling iterations on `sampler.DeviceTemperedSampler` with `chains` walkers per rung
    (default 2 P_joint + 2) on the ladder `betas`, or `default_betas(ntemps, tmax)`; then `log_evidence()` of the
    sampling iterations.  The model is sized so that `max_walkers` holds ntemps x chains x F field records.

    Outputs: ONE database `<output_name>_db.fits` with the joint columns and the beta = 1 rung's chain, the
    header keys MCFIELDS, MCNTEMPS, MCLNZ, MCLNZERR and MCTSWAP (mean swap acceptance), and each field's
    posterior images `<output_name>_f<k>_<type>.fits` at that field's shape.  An existing database skips
    sampling; the evidence is then read back from its header.  `moves`: as `model_galaxy_ptmcmc`'s (recorded as
    MCMOVES).  Returns (JointModel, database, (lnZ, err))."""
    from .sampler import DeviceTemperedSampler, check_betas, default_betas
    betas = default_betas(ntemps, tmax) if betas is None else check_betas(betas)
    n_t = len(betas)
    if chains is not None:
        _check_chains(chains)
    if output_name is None:
        output_name = 'out_joint_' + str(model_files[0]).replace('.py', '')
    given = isinstance(model_files, JointModel)
    joint = model_files if given else None
    if joint is None:
        # room for the image recomputation's batches (as model_joint_mcmc) and for every rung's walkers
        n_f = len(model_files)
        joint = JointModel(model_files, per_field=per_field, device=device,
                           max_walkers=n_f * max(n_t * (chains or 0), 1024))
    n_f = len(joint.field_models)
    if chains is None:
        chains = 2 * joint.num_params + 2
    if n_t * chains * n_f > joint._max_walkers:
        if given:
            raise ValueError('{} temperatures x {} chains x {} fields exceed max_walkers={}'.format(
                n_t, chains, n_f, joint._max_walkers))
        joint = JointModel(model_files, per_field=per_field, device=device, max_walkers=n_t * chains * n_f)
    sampler = DeviceTemperedSampler(chains, joint, betas=betas)
    sampler.set_moves(moves)
    _seed(sampler, random_state)

    db_name = output_name + '_db.fits'
    if not os.path.exists(db_name):
        pos = np.stack([joint.init_params_from_priors(chains) for _ in range(n_t)])
        evidence = _burn_and_sample_tempered(sampler, pos, burn, iterations, accumulate, quiet)
        meta = _chain_meta(sampler, burn, chains, check_convergence_autocorr(sampler), moves, MCFIELDS=n_f,
                           **_tempered_meta(sampler, n_t, evidence))
        database = save_database(sampler, joint, db_name, meta_dict=meta)
    else:
        (database,), (evidence,) = _load_existing([db_name], quiet)
    _save_joint_images(joint, database, output_name, write_fits)
    return joint, database, evidence


def model_fields_ptmcmc(model_files, output_names=None, write_fits=default_filetypes, iterations=0, burn=0,
                        chains=None, ntemps=16, tmax=1e6, betas=None, device=0, random_states=None,
                        start_positions=None, accumulate=True, quiet=False, moves=None):
    """`model_galaxy_ptmcmc` for SEVERAL fields of one model structure at once, in one GPU context
    (`models.FieldSet`, `sampler.FieldSetTemperedSampler`): the Bayesian evidence of every field's model from
    one run.  Every field is tempered exactly as its own `model_galaxy_ptmcmc` run would temper it -- its own
    ladder of `chains` walkers per rung on `betas` (or `default_betas(ntemps, tmax)`; one ladder for all), its
    own random stream, burn-in, reset, `iterations` sampling iterations with the beta = 1 rung's posterior
    images accumulated -- but all fields advance together, every half-step's proposals of all fields and rungs
    ONE batch.  For samples of many small cut-outs, where a ladder per field leaves the GPU idle (DESIGN.md
    section 24).  The set is sized so that `max_walkers` holds F x ntemps x chains.

    model_files      model files (or MultiComponentModel objects) with the same component lists
    output_names     one per field (default 'out_<model file>')
    random_states    one RandomState state tuple or seed per field (default: numpy's global generator
                     seeds them in field order)
    start_positions  optional [F][T, chains, P] start positions (default: every rung drawn from its field's priors)
    moves            as `model_galaxy_ptmcmc`'s (`FieldSetTemperedSampler.set_moves`; recorded as MCMOVES)
    Outputs per field: the beta = 1 database `<output_name>_db.fits` with the header keys MCNTEMPS, MCLNZ, MCLNZERR
    and MCTSWAP, and the posterior images, as `model_galaxy_ptmcmc` writes them.  Existing databases skip
    sampling; the evidences are then read back from their headers.
    Returns a list of (model, database, (lnZ, err)), one per field."""
    from .sampler import FieldSetTemperedSampler, check_betas, default_betas
    betas = default_betas(ntemps, tmax) if betas is None else check_betas(betas)
    n_t = len(betas)
    fieldset, output_names, chains, db_names, have_db = _fields_arguments(
        model_files, output_names, random_states, start_positions, chains, device, n_t=n_t)
    models = fieldset.models
    sampler = FieldSetTemperedSampler(chains, fieldset, betas=betas, accumulate=False)
    sampler.set_moves(moves)
    _seed_fields(sampler, random_states)

    if not have_db:
        if start_positions is None:
            start_positions = [np.stack([m.init_params_from_priors(chains) for _ in range(n_t)]) for m in models]
        pos = np.array([np.asarray(p, dtype=np.float64) for p in start_positions])
        evidences = _burn_and_sample_tempered(sampler, pos, burn, iterations, accumulate, quiet)
        databases = []
        for sub, m, name, ev in zip(sampler.fields, models, db_names, evidences):
            meta = _chain_meta(sub, burn, chains, check_convergence_autocorr(sub), moves,
                               **_tempered_meta(sub, n_t, ev))
            databases.append(save_database(sub, m, name, meta_dict=meta))
    else:
        databases, evidences = _load_existing(db_names, quiet, fields=True)
    for m, db, out in zip(models, databases, output_names):
        save_posterior_images(m, db, output_name=out, filetypes=write_fits)
    return [(m, db, ev) for m, db, ev in zip(models, databases, evidences)]

