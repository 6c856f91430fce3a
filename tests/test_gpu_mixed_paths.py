"""Mixed-shape field sets and joint fits on every kernel family of the fused back end.

tests/test_gpu_mixed_fields.py and tests/test_gpu_joint.py hold a set of fields of different sizes
(psfmc_ctx_create_fields_shaped) to the oracle at one 128^2 transform.  Here each set of MIXED_SETS lands on
another family -- the power-table rasteriser, k_cols3g / k_cols3f, the three-stage row kernels, row groups of 8,
a transform above 1024 -- with fields embedded on one axis, on both or not at all, some of them with the exact
wrap-around margin.  Every field carries a sky, Sersics and point sources at and beyond its own four edges
(`edge_components`), where a wrong per-field descriptor (`walker_wrap`) or a point-source window clipped to
another field's sides (k_theta_prep) changes the log-likelihood.

Per set: the report of the library; every walker against the fp64 oracle, bit for bit the same under every
segment order, pass size, stream count, table mode of the rasteriser and on the field's own context where it
has the set's transform; images and posterior sums; a joint fit of the same fields (every parameter per
field); the refusal of f32 storage.  At the two largest sets: the FieldSetSampler and a JointModel (shared
parameters) with its device sampler against the host sampler."""
import collections

import numpy as np
import pytest

import helpers
from test_gpu_joint import LAYOUT, _col, _joint_truth, _oracle_field, _thetas
from test_gpu_mixed_fields import _eval_segments
from test_gpu_random import (build, check_images, check_posterior_sums, check_walkers, edge_case, edge_components,
                             image_pair, oracle_walker)
from test_gpu_variants import K_COLS, K_COLS3F, K_COLS3G, assert_report, field_of
from test_joint_link import POS, make_field, make_model

pytestmark = pytest.mark.gpu

# fields [(ny, nx, PSF side)], PSFs per field, and what the library reports for the set: the transform
# (transform_ny, transform_nx), column_engine, rows3 (bit 0 forward, bit 1 inverse three-stage rows), row_group
MixedSet = collections.namedtuple('MixedSet', 'name fields n_psf transform column_engine rows3 row_group')
MIXED_SETS = [
    # field 0 embedded on x only, field 1 on y only, field 2 not at all; rows of 128 in groups of 8
    MixedSet('A', [(128, 100, 11), (96, 128, 21), (128, 128, 9)], 2, (128, 128), K_COLS, 0, 8),
    # rows of 64 in groups of 8 (160 rows: whole groups); field 1 embedded on y only, exact margin 150 + 11 - 1
    MixedSet('B', [(160, 64, 11), (150, 64, 11)], 1, (160, 64), K_COLS, 0, 8),
    # the last row length on log2 + exp2; exact margin 250 + 7 - 1 = 256
    MixedSet('C', [(256, 256, 21), (240, 250, 7)], 1, (256, 256), K_COLS, 0, 4),
    # the first row length on the power tables; exact margin 250 + 11 - 1 = 260
    MixedSet('D', [(260, 260, 21), (250, 250, 11)], 1, (260, 260), K_COLS, 0, 4),
    # a rectangular transform: general-side k_cols columns under power-table rows; exact margin 96 + 17 - 1 = 112
    MixedSet('E', [(96, 300, 17), (90, 288, 13)], 2, (112, 300), K_COLS, 0, 4),
    # k_cols3f under plain power-of-two rows
    MixedSet('F', [(512, 512, 33), (480, 470, 25), (300, 512, 41)], 1, (512, 512), K_COLS3F, 0, 4),
    # k_cols3g and the three-stage inverse rows (summing chi^2 per field); exact margin 690 + 31 - 1 = 720
    MixedSet('G', [(720, 720, 31), (680, 690, 31), (400, 720, 17)], 2, (720, 720), K_COLS3G, 2, 4),
    # above 1024: three-stage forward and inverse rows, k_cols3g (8, 8); exact margin 1100 + 53 - 1 = 1152
    MixedSet('H', [(1152, 1152, 33), (1000, 1100, 53)], 1, (1152, 1152), K_COLS3G, 3, 1),
]
SETS = {s.name: s for s in MIXED_SETS}
# psfmc_hip.hip kInWavePowTabWaves: batches of up to this many (row wave, Sersic) pairs form their power-table
# entries in the forward row waves, larger ones read k_pow_tables' output
IN_WAVE_POW_TAB_WAVES = 8192
N_SERSIC = 4                        # edge_components: a sky, four Sersics, four point sources


@pytest.fixture(scope='module', params=MIXED_SETS, ids=lambda s: s.name)
def mixed(request):
    """(set, cases, oracle fields, oracle log-likelihoods per field, FieldSet) -- five distinct walkers per field,
    one of them outside its priors; with two PSFs the walkers alternate between them."""
    from psfmc_amd import FieldSet
    s = request.param
    cases = []
    for f, (ny, nx, pk) in enumerate(s.fields):
        case = edge_case(21000 + 100 * ord(s.name) + f, (ny, nx), (pk, pk), edge_components(ny, nx), n_psf=s.n_psf)
        if s.n_psf > 1:
            case['theta'][:, -1] = np.arange(len(case['theta'])) % 2
        cases.append(case)
    fields = [field_of(c) for c in cases]
    want = [np.array([oracle_walker(fld, c, t)[0] for t in c['theta']]) for fld, c in zip(fields, cases)]
    fs = FieldSet([build(c, 'fused', max_walkers=1) for c in cases], max_walkers=64)
    yield s, cases, fields, want, fs
    fs.close()


def _interleaved(fs, thetas):
    """One psfmc_eval_theta_fields call on every field's walkers, in segments of 3 and 2 walkers with the fields
    in the order 0, F-1, ..., 1 each time (0 2 1 0 2 1 for three fields) -> [W_f] per field."""
    order = [0] + list(range(len(thetas) - 1, 0, -1))
    segs = [(f, thetas[f][lo:hi]) for lo, hi in ((0, 3), (3, None)) for f in order]
    parts = _eval_segments(fs, segs)
    return [np.concatenate([p for (g, _), p in zip(segs, parts) if g == f]) for f in range(len(thetas))]


def _alone(fs, f, theta):
    """Field f's walkers alone through the set."""
    thetas = [None] * len(fs.models)
    thetas[f] = theta
    return fs.log_posterior_batch(thetas)[f]


def test_set_reports_its_family(mixed):
    s, _, _, _, fs = mixed
    ctx = fs.context
    assert ctx.shapes == [(ny, nx) for ny, nx, _ in s.fields]
    for f, (ny, nx, _) in enumerate(s.fields):
        assert ctx.field_shape(f) == (ny, nx), (s.name, f)
    assert_report(ctx, s.name, column_engine=s.column_engine, rows3=s.rows3, row_group=s.row_group, storage_f32=0,
                  transform=s.transform)
    assert ctx.get_option('pow_tabs') == (s.transform[1] > 256), s.name


def test_log_posteriors_against_the_oracle(mixed):
    """The interleaved call in passes of at most two walkers (cutting across segments) against the oracle; the same
    bits alone, under every pass size and stream count, in both table modes of the rasteriser and on each field's
    own context where that has the set's transform."""
    s, cases, _, want, fs = mixed
    ctx = fs.context
    thetas = [c['theta'] for c in cases]
    n_f, n_total = len(cases), sum(len(t) for t in thetas)
    chunk0, streams0 = int(ctx.get_option('chunk_walkers')), int(ctx.get_option('streams'))
    ctx.set_option('chunk_walkers', 2)
    assert ctx._lib.psfmc_pass_size(ctx._ctx, n_total) == 2
    base = _interleaved(fs, thetas)
    for f, c in enumerate(cases):
        check_walkers(base[f], want[f], fs.models[f].log_priors_batch(c['theta']), c['outside'], (s.name, f))
    try:
        for streams in (1, 2):
            ctx.set_option('streams', streams)
            for chunk in (2, 3, chunk0):
                ctx.set_option('chunk_walkers', chunk)
                tag = (s.name, 'streams', streams, 'chunk', chunk)
                got = _interleaved(fs, thetas)
                assert all(np.array_equal(g, b) for g, b in zip(got, base)), tag
                for f in range(n_f):
                    assert np.array_equal(_alone(fs, f, thetas[f]), base[f]), tag + (f,)
    finally:
        ctx.set_option('streams', streams0)
        ctx.set_option('chunk_walkers', chunk0)
    if s.transform[1] > 256:
        # the largest batch whose row waves form the table entries themselves, and one walker more
        small = IN_WAVE_POW_TAB_WAVES // (N_SERSIC * int(ctx.get_option('partials_per_walker')))
        assert small >= 1
        for f, t in enumerate(thetas):
            tiled = np.concatenate([t] * (small // len(t) + 2))[:max(small + 1, len(t))]
            got = _alone(fs, f, tiled)
            assert ctx.get_option('pow_tabs_built') == 1, (s.name, f)
            assert np.array_equal(got[:len(t)], base[f]) and np.array_equal(got, base[f][np.arange(len(got)) % len(t)])
            for lo in range(0, len(t), small):
                assert np.array_equal(_alone(fs, f, t[lo:lo + small]), base[f][lo:lo + small]), (s.name, f, lo)
                assert ctx.get_option('pow_tabs_built') == 0, (s.name, f)
    shared = []
    for f, c in enumerate(cases):
        own = build(c, 'fused', max_walkers=8)
        if (own.engine.get_option('transform_ny'), own.engine.get_option('transform_nx')) == s.transform:
            shared.append(f)
            assert np.array_equal(own.log_posterior_batch(c['theta']), base[f]), (s.name, f)
        own.close()
    assert all(f in shared for f, fld in enumerate(s.fields) if fld[:2] == s.transform), (s.name, shared)


def test_joint_fit_of_the_edge_fields(mixed):
    """The set's fields as one JointModel with every parameter per field: F x 6 field records in one batch
    (k_theta_prep over every field at once, each with its own sides), in passes of two that cut through the
    field-major blocks, against the oracle's per-field log-likelihoods plus the joint prior.  Joint walkers 0 ... 4
    take walkers with finite values in every field, walker 5 field 1's walker outside its priors (-inf)."""
    from psfmc_amd import JointModel
    s, cases, _, want, _ = mixed
    models = [build(c, 'fused', max_walkers=1) for c in cases]
    joint = JointModel(models, per_field=models[0].param_names, max_walkers=64)
    picks = []
    for f, (m, c) in enumerate(zip(models, cases)):
        fin = np.flatnonzero(np.isfinite(want[f]) & np.isfinite(m.log_priors_batch(c['theta'])))
        assert len(fin) >= 2, (s.name, f)
        picks.append([fin[w % len(fin)] for w in range(5)] + [c['outside'] if f == 1 else fin[0]])
    theta = np.zeros((6, joint.num_params))
    for f, c in enumerate(cases):
        theta[:, joint.field_columns(f)] = c['theta'][picks[f]]
    joint.engine.set_option('chunk_walkers', 2)
    got = joint.log_posterior_batch(theta)
    prior = joint.log_priors_batch(theta)
    for w in range(5):
        lls = np.array([want[f][picks[f][w]] for f in range(len(cases))])
        total = prior[w] + lls.sum()
        assert abs(got[w] - total) <= 2e-10 * np.abs(lls).sum(), (s.name, w, got[w], total)
    assert not np.isfinite(prior[5]) and got[5] == -np.inf, (s.name, got[5])
    joint.close()


def test_images_and_posterior_sums(mixed):
    s, cases, fields, want, fs = mixed
    for f, c in enumerate(cases):
        ny, nx, _ = s.fields[f]
        pair = image_pair(want[f])
        assert len(pair) == 2, (s.name, f)
        refs = [oracle_walker(fields[f], c, c['theta'][i], images=True)[1] for i in pair]
        dev = fs.models[f].sample_images(c['theta'][pair])
        assert set(dev) == set(fs.context.IMAGE_KINDS)
        for kind, img in dev.items():
            assert img.shape == (2, ny, nx), (s.name, f, kind)
        check_images(dev, refs, (s.name, f))
        check_posterior_sums(fs.models[f], c['theta'][pair], refs, (s.name, f))
        post = fs.models[f].collect_posterior_images()
        assert all(img.shape == (ny, nx) for img in post.values()), (s.name, f)
        fs.models[f].reset_images()


def test_f32_storage_is_refused(mixed):
    from psfmc_amd.engine import NativeError
    s, cases, _, _, fs = mixed
    thetas = [c['theta'] for c in cases]
    before = _interleaved(fs, thetas)
    with pytest.raises(NativeError, match='storage_f32'):
        fs.context.set_option('storage_f32', 1)
    assert fs.context.get_option('storage_f32') == 0
    after = _interleaved(fs, thetas)
    assert all(np.array_equal(a, b) for a, b in zip(after, before)), s.name


# ---- the samplers and joint fits at the two largest sets (make_field / make_model: 11 parameters, 2 PSFs) ----
@pytest.mark.parametrize('name', ['G', 'H'])
def test_fieldset_sampler_at_large_transforms(name):
    """Every field's FieldSetSampler chain equals the host sampler's on that field's log-posterior, bit for bit."""
    from psfmc_amd import EnsembleSampler, FieldSet, FieldSetSampler
    s = SETS[name]
    n_f, n_w, n_iter = len(s.fields), 22, 3                     # (at least twice the 11 parameters)
    flds = [make_field(ny, nx, pk, seed=400 + f) for f, (ny, nx, pk) in enumerate(s.fields)]
    fs = FieldSet([make_model(fld) for fld in flds], max_walkers=n_f * n_w)
    assert_report(fs.context, name, column_engine=s.column_engine, rows3=s.rows3, row_group=s.row_group,
                  transform=s.transform)
    p0 = [flds[f]['truth'] + np.random.RandomState(70 + f).normal(size=(n_w, 11)) * 1e-3 for f in range(n_f)]
    for p in p0:
        p[:, 10] = np.arange(n_w) % 2
    samp = FieldSetSampler(n_w, fs, block=2)
    for f, sub in enumerate(samp.fields):
        sub.random_state = np.random.RandomState(600 + f).get_state()
    for _ in samp.sample(p0, iterations=n_iter):
        pass
    for f in range(n_f):
        host = EnsembleSampler(n_w, fs.num_params, batch_lnpostfn=fs.models[f].log_posterior_batch)
        host.random_state = np.random.RandomState(600 + f).get_state()
        for _ in host.sample(p0[f], iterations=n_iter):
            pass
        sub = samp.fields[f]
        assert np.array_equal(sub.chain, host.chain), (name, f)
        assert np.array_equal(sub.lnprobability, host.lnprobability), (name, f)
        assert np.array_equal(sub.naccepted, host.naccepted), (name, f)
        assert host.naccepted.sum() > 0
    fs.close()


@pytest.mark.parametrize('name', ['G', 'H'])
def test_joint_fit_at_large_transforms(name):
    """JointModel(per_field=POS): ten walkers' F x 10 field records in passes of 8 that cut through the field-major
    blocks, against the oracle plus the joint prior (with test_gpu_joint's -inf rows); then the joint device
    sampler against the host sampler, bit for bit, with every field's posterior sums at its own shape.  The joint
    sampler always takes two half-steps, even where a one-field context would take its single-pass route."""
    from psfmc_amd import DeviceEnsembleSampler, EnsembleSampler, JointModel
    s = SETS[name]
    n_f, n_w = len(s.fields), 10
    flds = [make_field(ny, nx, pk, seed=500 + f) for f, (ny, nx, pk) in enumerate(s.fields)]
    joint = JointModel([make_model(fld) for fld in flds], per_field=POS, max_walkers=n_f * 2 * n_w)
    eng = joint.engine
    assert_report(eng, name, column_engine=s.column_engine, rows3=s.rows3, row_group=s.row_group,
                  transform=s.transform)
    eng.set_option('chunk_walkers', 8)
    assert joint.context._lib.psfmc_pass_size(joint.context._ctx, n_f * n_w) == 8
    theta = _thetas(joint, flds, n_w, seed=15)
    ir, ib = _col(joint, '1_Sersic_reff'), _col(joint, '1_Sersic_reff_b')
    cs = _col(joint, '1_Sersic_xy_f1')
    theta[6, _col(joint, '1_Sersic_mag')] = 30.0                 # a shared parameter out of support
    theta[7, _col(joint, '0_PointSource_mag_f1')] = 10.0         # field 1's parameter out of support
    theta[8, ib] = theta[8, ir] + 0.5                            # reff_b > reff
    theta[9, cs:cs + 2] = np.floor(flds[1]['c'])                 # field 1's Sersic centre on a pixel centre
    got = joint.log_posterior_batch(theta)
    prior = joint.log_priors_batch(theta)
    fields = [_oracle_field(fld) for fld in flds]
    for w in range(n_w):
        if w in (6, 7, 8):
            assert not np.isfinite(prior[w]) and got[w] == -np.inf, (name, w)
            continue
        lls = [helpers.oracle_loglike(fields[f], LAYOUT, joint.field_theta(theta[w], f)[0], has_psf_index=True)
               for f in range(n_f)]
        if w == 9:
            assert np.isfinite(prior[w]) and not np.isfinite(lls[1]) and np.isfinite(np.delete(lls, 1)).all()
            assert got[w] == -np.inf
            continue
        want = prior[w] + sum(lls)
        assert abs(got[w] - want) <= 1e-11 * (abs(prior[w]) + sum(abs(v) for v in lls)), (name, w, got[w], want)

    # the device sampler: speculation allowed for ensembles of this size, still two half-steps per iteration
    n_iter = 6
    eng.set_option('speculate', n_w)
    speculated = eng.get_option('speculated_runs')
    p0 = _joint_truth(joint, flds) + np.random.RandomState(n_w).normal(size=(n_w, joint.num_params)) * 1e-3
    for f in range(n_f):
        p0[:, _col(joint, 'PSF_Index_f%d' % f)] = np.arange(n_w) % 2
    joint.reset_images()
    dev = DeviceEnsembleSampler(n_w, joint, live_dangerously=True, block=3, accumulate=True)
    dev.random_state = np.random.RandomState(800).get_state()
    for _ in dev.sample(p0, iterations=n_iter):
        pass
    assert eng.get_option('speculated_runs') == speculated
    host = EnsembleSampler(n_w, joint.num_params, batch_lnpostfn=joint.log_posterior_batch, live_dangerously=True)
    host.random_state = np.random.RandomState(800).get_state()
    for _ in host.sample(p0, iterations=n_iter):
        pass
    assert np.array_equal(dev.chain, host.chain), name
    assert np.array_equal(dev.lnprobability, host.lnprobability), name
    assert np.array_equal(dev.naccepted, host.naccepted), name
    assert host.naccepted.sum() > 0
    flat = dev.chain.transpose(1, 0, 2).reshape(-1, joint.num_params)
    for f, m in enumerate(joint.field_models):
        assert m.accumulated_samples == n_iter * n_w
        got = {k: v.copy() for k, v in m.collect_posterior_images().items()}
        m.reset_images()
        m.accumulate_samples(joint.field_theta(flat, f))
        want = m.collect_posterior_images()
        for kind, img in want.items():
            assert img.shape == got[kind].shape == s.fields[f][:2], (name, f, kind)
            fin = np.isfinite(img)
            assert np.array_equal(fin, np.isfinite(got[kind])), (name, f, kind)
            assert np.abs(got[kind][fin] - img[fin]).max() <= 1e-12 * np.abs(img[fin]).max(), (name, f, kind)
        m.reset_images()
    joint.close()
