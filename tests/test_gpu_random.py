"""Randomised GPU-vs-oracle parity: random image shapes (square and rectangular),
PSF shapes (odd and even), component sets, shift methods, angle units, bad pixels,
masks, several PSFs -- every draw evaluated by both GPU back ends and by the fp64
oracle on the same parameters."""
import numpy as np
import pytest

import helpers
import psfmc_oracle as orc
import synth_field

pytestmark = pytest.mark.gpu


def random_case(seed, shape=None, n_walkers=0):
    rng = np.random.RandomState(seed)
    ny, nx = rng.choice([64, 128, 256]), rng.choice([64, 128, 256])
    if shape is not None:
        ny, nx = shape
    n_psf = rng.choice([1, 1, 2, 3])
    py, px = rng.choice([9, 16, 21, 32, 33]), rng.choice([9, 16, 21, 32, 33])
    psfs, pivms = [], []
    for k in range(n_psf):
        yy, xx = np.mgrid[0:py, 0:px].astype(float)
        fw = 1.6 + 0.4 * k + rng.uniform(0, 0.5)
        core = (1 + ((xx - px // 2 - 0.2 * k) ** 2 + (yy - py // 2 + 0.1) ** 2) / fw ** 2) ** -2.5 * 300
        var = 0.01 + np.abs(core) / rng.uniform(20, 60)
        img = core + rng.normal(size=core.shape) * np.sqrt(var)
        iv = 1.0 / var
        if rng.rand() < 0.5:
            iv[rng.randint(py), rng.randint(px)] = 0.0
        psfs.append(img.astype(np.float32))
        pivms.append(iv.astype(np.float32))
    sci = (rng.normal(size=(ny, nx)) * 0.05).astype(np.float32)
    ivm = (1.0 / rng.uniform(0.02, 0.08, size=(ny, nx)) ** 2).astype(np.float32)
    for _ in range(rng.randint(0, 6)):
        ivm[rng.randint(ny), rng.randint(nx)] = rng.choice([0.0, -1.0, np.nan])
    for _ in range(rng.randint(0, 3)):
        sci[rng.randint(ny), rng.randint(nx)] = np.nan
    mask = None
    if rng.rand() < 0.5:
        mask = np.zeros((ny, nx), dtype=np.uint8)
        y0, x0 = rng.randint(ny - 8), rng.randint(nx - 8)
        mask[y0:y0 + rng.randint(1, 8), x0:x0 + rng.randint(1, 8)] = 1
    zp = rng.uniform(22, 27)
    comps = []
    if rng.rand() < 0.6:
        comps.append(dict(type='sky', adu=rng.normal() * 0.02))
    for _ in range(rng.randint(0, 3)):
        edge = rng.rand() < 0.3
        xy = (rng.uniform(-3, nx + 3), rng.uniform(-3, ny + 3)) if edge else \
            (rng.uniform(8, nx - 8), rng.uniform(8, ny - 8))
        if rng.rand() < 0.2:
            xy = (np.floor(xy[0]) + rng.choice([0.0, 0.5]), np.floor(xy[1]) + rng.choice([0.0, 0.5]))
        comps.append(dict(type='ps', xy=xy, mag=rng.uniform(16, 22), method=rng.choice(['lanczos3', 'bilinear'])))
    for _ in range(rng.randint(0, 4)):
        reff = rng.uniform(1.5, min(ny, nx) / 6)
        deg = bool(rng.rand() < 0.5)
        comps.append(dict(type='sersic', xy=(rng.uniform(10, nx - 10), rng.uniform(10, ny - 10)),
                          mag=rng.uniform(15, 23), reff=reff, reff_b=reff * rng.uniform(0.2, 1.0),
                          index=rng.choice([0.5, 1.0, 4.0, rng.uniform(0.3, 8.0)]),
                          angle=rng.uniform(0, 180) if deg else rng.uniform(-3.2, 3.2), angle_degrees=deg))
    if not comps:
        comps.append(dict(type='sky', adu=0.01))
    psf_index = rng.randint(n_psf)
    case = dict(sci=sci, ivm=ivm, psfs=psfs, pivms=pivms, mask=mask, zp=zp, comps=comps, psf_index=psf_index)
    if n_walkers:
        case.update(free_parameters(case, rng, n_walkers))
    return case


def free_parameters(case, rng, n_walkers):
    """The opt-in form of `random_case` (`n_walkers` > 0): every component parameter free, under a narrow
    Uniform window around its drawn value (`priors`: per component, name -> (low, high)); the PSF index free
    when there are several PSFs (the Configuration's DiscreteUniform, last).  Returns the layout
    `helpers.comps_from_theta` reads and `n_walkers` DISTINCT walkers: walker 0 is the drawn values
    themselves, the others inside the windows with reff_b <= reff, except walker `outside` (neither the
    first nor the last), which has one parameter beyond its window and must come back -inf."""
    assert n_walkers >= 3
    layout, priors, lo, hi = [], [], [], []

    def window(name, low, high):
        priors[-1][name] = (np.asarray(low, dtype=float), np.asarray(high, dtype=float))
        lo.extend(np.ravel(low)); hi.extend(np.ravel(high))
    for c in case['comps']:
        priors.append({})
        if c['type'] == 'sky':
            layout.append(('sky',))
            window('adu', c['adu'] - 0.005, c['adu'] + 0.005)
        elif c['type'] == 'ps':
            layout.append(('ps', c['method']))
            window('mag', c['mag'] - 0.25, c['mag'] + 0.25)
            window('xy', np.array(c['xy']) - 1.5, np.array(c['xy']) + 1.5)
        else:
            layout.append(('sersic', c['angle_degrees']))
            da = 8.0 if c['angle_degrees'] else 0.14
            # (packing order: alphabetical inside a component -- helpers.comps_from_theta)
            window('angle', c['angle'] - da, c['angle'] + da)
            window('index', c['index'] * 0.9, c['index'] * 1.1)
            window('mag', c['mag'] - 0.25, c['mag'] + 0.25)
            window('reff', c['reff'] * 0.85, c['reff'] * 1.15)
            window('reff_b', c['reff_b'] * 0.85, c['reff_b'] * 1.15)
            window('xy', np.array(c['xy']) - 1.5, np.array(c['xy']) + 1.5)
    lo, hi = np.array(lo), np.array(hi)
    n_cont = len(lo)
    has_psf_index = len(case['psfs']) > 1
    centre = []
    for c in case['comps']:
        centre += ([c['adu']] if c['type'] == 'sky' else [c['mag'], c['xy'][0], c['xy'][1]] if c['type'] == 'ps' else
                   [c['angle'], c['index'], c['mag'], c['reff'], c['reff_b'], c['xy'][0], c['xy'][1]])
    theta = np.empty((n_walkers, n_cont + has_psf_index))
    theta[0, :n_cont] = centre
    theta[1:, :n_cont] = rng.uniform(lo, hi, (n_walkers - 1, n_cont))
    pos = 0
    for item in layout:
        if item[0] == 'sersic':
            re, rb = pos + 3, pos + 4
            theta[1:, rb] = rng.uniform(lo[rb], np.minimum(hi[rb], theta[1:, re]))
        pos += {'sky': 1, 'ps': 3, 'sersic': 7}[item[0]]
    if has_psf_index:
        theta[0, -1] = case['psf_index']
        theta[1:, -1] = rng.randint(len(case['psfs']), size=n_walkers - 1)
    outside = rng.randint(1, n_walkers - 1)
    col = rng.randint(n_cont)
    theta[outside, col] = hi[col] + 0.5 * (hi[col] - lo[col]) if rng.rand() < 0.5 else lo[col] - 0.5 * (hi[col] - lo[col])
    return dict(layout=layout, priors=priors, has_psf_index=has_psf_index, theta=theta, outside=outside)


def build(case, backend, max_walkers=4):
    from psfmc_amd import MultiComponentModel
    from psfmc_amd.ModelComponents import Configuration, Sky, PointSource, Sersic
    from psfmc_amd.distributions import Uniform
    cfg = Configuration(case['sci'], case['ivm'], case['psfs'] if len(case['psfs']) > 1 else case['psfs'][0],
                        case['pivms'] if len(case['pivms']) > 1 else case['pivms'][0],
                        mask_file=case['mask'], mag_zeropoint=case['zp'])
    objs = [cfg]
    for k, c in enumerate(case['comps']):
        if 'priors' in case:
            v = {name: Uniform(loc=a, scale=b - a) for name, (a, b) in case['priors'][k].items()}
        else:
            v = {name: c[name] for name in ('adu', 'xy', 'mag', 'reff', 'reff_b', 'index', 'angle') if name in c}
        if c['type'] == 'sky':
            objs.append(Sky(adu=v['adu']))
        elif c['type'] == 'ps':
            objs.append(PointSource(xy=v['xy'], mag=v['mag'], shift_method=c['method']))
        else:
            objs.append(Sersic(xy=v['xy'], mag=v['mag'], reff=v['reff'], reff_b=v['reff_b'], index=v['index'],
                               angle=v['angle'], angle_degrees=c['angle_degrees']))
    return MultiComponentModel(objs, backend=backend, max_walkers=max_walkers)


def several_passes(model, n_w):
    """Run a batch of n_w walkers in several internal passes of at most 2 walkers (chunk_walkers 2 where the
    library's own pass is larger): pass offsets into the T buffers, partials and records are exercised, with a
    short last pass when n_w is odd.  Returns the pass size."""
    eng = model.engine
    if eng.pass_size(n_w) > 2:
        eng.set_option('chunk_walkers', 2)
    size = eng.pass_size(n_w)
    assert size <= 2 and size < n_w
    return size


def oracle_walker(field, case, t, images=False):
    """(log-likelihood, images or None) of one walker of a free-parameter case from the fp64 oracle."""
    comps, psf = helpers.comps_from_theta(case['layout'], t, case['has_psf_index'])
    ll, imgs = orc.evaluate(field, comps, psf, raw_dtype=np.float64, want_ps_sub=images)
    return (ll if np.isfinite(ll) else -np.inf), imgs


def check_walkers(got, want_ll, prior, outside, tag):
    """Log-posteriors of a distinct-walker batch: -inf outside the prior support or where the oracle's
    likelihood is not finite, else the oracle's likelihood + prior at the bound of the fixed-parameter tests;
    the finite values pairwise distinct (a swap of two walkers cannot pass by coincidence)."""
    assert not np.isfinite(prior[outside]) and np.isfinite(np.delete(prior, outside)).all(), tag
    for w in range(len(got)):
        if not (np.isfinite(prior[w]) and np.isfinite(want_ll[w])):
            assert got[w] == -np.inf, (tag, w, got[w])
        else:
            want = want_ll[w] + prior[w]
            assert abs(got[w] - want) <= 2e-10 * abs(want_ll[w]), (tag, w, got[w], want)
    fin = got[np.isfinite(got)]
    assert len(np.unique(fin)) == len(fin), (tag, got)


def image_tol(kind, imgs, general=True):
    """Bound of an image (relative to its largest value) -- test_random_model_matches_oracle's for the small
    random fields, test_general_sides_match_oracle's (the variance channel growing with the squared peak)
    for the rest."""
    if kind != 'composite_ivm':
        return 1e-11
    if not general:
        return 1e-9
    peak = max(np.nanmax(np.abs(im['raw_model'])) for im in imgs)
    return 5e-9 * max(1.0, (peak / 2e3) ** 2)


def check_images(dev, refs, tag, general=True):
    """dev: kind -> [n, ny, nx] of one call; refs: the oracle's images of those n walkers."""
    for i, ref_imgs in enumerate(refs):
        for kind, ref in ref_imgs.items():
            fin = np.isfinite(ref)
            assert dev[kind][i].shape == ref.shape, (tag, kind)
            assert np.array_equal(np.isfinite(dev[kind][i]), fin), (tag, i, kind)
            scale = max(np.abs(ref[fin]).max(), 1e-300)
            tol = image_tol(kind, [ref_imgs], general)
            assert np.abs(dev[kind][i][fin] - ref[fin]).max() <= tol * scale, (tag, i, kind)


def check_posterior_sums(model, theta, refs, tag):
    """The device posterior sums of these walkers against the running mean of the oracle's images (the
    weight map averaged as a variance: models.py accumulate_images)."""
    model.reset_images()
    model.accumulate_samples(theta)
    post = model.collect_posterior_images()
    with np.errstate(all='ignore'):
        for kind in refs[0]:
            if kind == 'composite_ivm':
                want = len(refs) / sum(1.0 / r[kind] for r in refs)
            else:
                want = sum(r[kind] for r in refs) / len(refs)
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(post[kind]), fin), (tag, kind, 'posterior')
            scale = max(np.abs(want[fin]).max(), 1e-300)
            tol = image_tol(kind, refs)
            assert np.abs(post[kind][fin] - want[fin]).max() <= tol * scale, (tag, kind, 'posterior')


def image_pair(want_ll):
    """Two distinct walkers with finite likelihoods for the image checks: the first and the last."""
    fin = np.flatnonzero(np.isfinite(want_ll))
    return [int(fin[0]), int(fin[-1])] if len(fin) >= 2 else []


@pytest.mark.parametrize('seed', range(24))
def test_random_model_matches_oracle(seed):
    """Seven distinct walkers (one outside the priors) in passes of two: every walker against the oracle on
    both back ends; on every fourth seed the images of two walkers from one call."""
    n_w = 7
    case = random_case(seed, n_walkers=n_w)
    theta = case['theta']
    field = orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'],
                           mag_zp=case['zp'])
    want_ll, refs = zip(*[oracle_walker(field, case, t, images=True) for t in theta])
    want_ll = np.array(want_ll)
    pair = image_pair(want_ll)
    for backend in ('fused', 'hipfft'):
        model = build(case, backend, max_walkers=8)
        assert model.num_params == theta.shape[1]
        assert several_passes(model, n_w) == 2
        got = model.log_posterior_batch(theta)
        check_walkers(got, want_ll, model.log_priors_batch(theta), case['outside'], (seed, backend))
        if seed % 4 == 0 and pair:
            dev = model.sample_images(theta[pair])
            check_images(dev, [refs[i] for i in pair], (seed, backend), general=False)
        model.close()


# every side the fused kernels are built for beyond the powers of two (psfmc_fft.h FftShape),
# each once as the row length and once as the column length, in rectangular pairs that also mix
# in power-of-two sides
GENERAL_SIDES = [96, 100, 120, 144, 150, 160, 180, 192, 200, 240, 250, 288, 300, 320, 360, 384, 400, 480,
                 500, 576, 600, 640, 720, 768, 800, 900, 960]


def general_shapes():
    from psfmc_amd import engine
    n = len(GENERAL_SIDES)
    shapes = [(GENERAL_SIDES[i], GENERAL_SIDES[(5 * i + 3) % n]) for i in range(n)]
    shapes += [(200, 200), (300, 300), (500, 500), (256, 200), (200, 256), (96, 512), (1024, 120), (160, 64), (150, 96),
               # a power-of-two nx whose unguarded row kernels do not divide ny: the guarded variant
               (150, 64), (100, 128), (150, 256), (250, 512), (500, 1024), (96, 1024)]
    # sides with a factor 7 (radix-7 codelet): every one of them once, paired with a side of another kind
    sevens = [84, 98, 112, 126, 140, 168, 196, 210, 224, 252, 280, 294, 336, 350, 392, 420, 448, 504, 560, 630,
              672, 700, 784, 840, 896]
    partners = [84, 256, 100, 126, 64, 150, 196, 128, 96, 252, 140, 120, 64, 350, 96, 210, 128, 84, 160, 98, 144,
                112, 168, 64, 224]
    shapes += list(zip(sevens, partners)) + [(140, 140), (64, 448), (200, 294)]
    # ... and once as the ROW length (round-2 advice: k_rows_fwd / k_rows_inv / k_raster_sums / k_pack_field of
    # these NX had only ever run for the few sides that happened to be a partner)
    shapes += [(p, s) for s, p in zip(sevens, partners) if (p, s) not in shapes]
    # sides with a factor 11 or 13 (the generic prime-radix codelet)
    primes = [88, 104, 110, 130, 132, 156, 176, 208, 220, 260, 264, 286, 308, 312, 330, 352, 364, 390, 416, 440, 484,
              520, 528, 572, 616, 624, 650, 660, 676, 704, 728, 780, 832]
    mates = [88, 64, 100, 130, 96, 128, 176, 84, 110, 64, 120, 104, 96, 156, 64, 88, 100, 130, 64, 132, 96,
             104, 64, 110, 88, 96, 64, 84, 100, 64, 104, 96, 64]
    shapes += list(zip(primes, mates)) + [(128, 286), (64, 676)]
    shapes += [(m, s) for s, m in zip(primes, mates) if (m, s) not in shapes]
    shapes += [(420, 420), (560, 560), (308, 308), (832, 832), (512, 100)]          # squares of the larger seven / prime sides
    # round 4: sides above 1024 (three-stage row and column kernels only), as the row and as the column length,
    # against two-stage, three-stage and power-of-two partners, and squares
    shapes += [(1152, 64), (96, 1152), (1280, 100), (128, 1280), (1536, 480), (250, 1536), (2048, 64), (84, 2048),
               (1152, 1152), (1280, 1536), (2048, 1152), (1536, 2048)]
    # round 4, second column survey: the seven sides that moved to the three-stage column kernel, against row lengths of
    # every layout (row groups of 8 -- where a side with 8 not dividing L falls back to the two-stage kernel --, 4, 2, 1)
    shapes += [(300, 128), (336, 128), (288, 64), (630, 128), (360, 1024), (280, 512), (350, 256), (300, 1152), (336, 2048)]
    assert all(engine.fused_supports(ny, nx) for ny, nx in shapes)
    # the claim above, enforced: every built side runs as the column length AND as the row length
    assert {ny for ny, _ in shapes} >= set(engine.FUSED_SIDES), sorted(set(engine.FUSED_SIDES) - {ny for ny, _ in shapes})
    assert {nx for _, nx in shapes} >= set(engine.FUSED_SIDES), sorted(set(engine.FUSED_SIDES) - {nx for _, nx in shapes})
    # a side with a prime factor > 13 (or factors the shapes cannot split into P, T <= 32) is not built ...
    assert not engine.fused_supports(170, 170) and not engine.fused_supports(256, 90) and not engine.fused_supports(490, 64)
    # ... but given the PSF's shape it is embedded in the next built side (test_embedded_sides_match_oracle)
    assert engine.fused_supports(170, 170, (33, 33)) and engine.fused_supports(490, 64, (16, 9))
    assert not engine.fused_supports(171, 170, (9, 9))
    # every even side up to 2048 - PSF side + 1 runs on the hand-written kernels
    assert all(engine.fused_supports(n, n, (64, 64)) for n in range(64, 1986, 2))
    assert not engine.fused_supports(1986, 1986, (64, 64)) and engine.fused_supports(2048, 2048, (64, 64))
    return shapes


@pytest.mark.parametrize('shape', general_shapes(), ids=lambda s: '%dx%d' % s)
def test_general_sides_match_oracle(shape):
    """Sides with factors 3, 5, 7, 11 and 13 (real cut-outs are rarely 2^k) on the fused kernels: five distinct
    walkers (one outside the priors) in passes of at most two, each against the fp64 oracle; all five images of
    two walkers from one call; above 1024 their posterior-image sums."""
    seed = 1000 + shape[0] * 7 + shape[1]
    n_w = 5
    case = random_case(seed, shape, n_walkers=n_w)
    theta = case['theta']
    field = orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'],
                           mag_zp=case['zp'])
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in theta])
    model = build(case, 'fused', max_walkers=8)
    assert model._backend == 'fused'
    several_passes(model, n_w)
    got = model.log_posterior_batch(theta)
    check_walkers(got, want_ll, model.log_priors_batch(theta), case['outside'], shape)
    pair = image_pair(want_ll)
    if pair:
        refs = [oracle_walker(field, case, theta[i], images=True)[1] for i in pair]
        dev = model.sample_images(theta[pair])
        check_images(dev, refs, shape)
        # (the variance channel: 1.8e-9 observed at 900 x 600.  Its rounding error is eps x the norm of raw^2
        # whatever transforms it -- 224 x 96 and 200 x 294 draw a 6e3-count peak and BOTH back ends, i.e. plain
        # rfft2 too, sit at 2.0e-8 from the oracle -- so the bound grows with the squared peak)
        ref, raw = refs[0]['composite_ivm'], refs[0]['raw_model']
        if np.nanmax(np.abs(raw)) > 2e3 and np.finfo(np.longdouble).nmant >= 63:
            # the evidence for that bound (tests/test_oracle_precision.py): against the weight map computed with
            # 80-bit transforms the GPU is no farther off than a few times the fp64 oracle itself
            fin = np.isfinite(ref)
            scale = max(np.abs(ref[fin]).max(), 1e-300)
            t = theta[pair[0]]
            exact = helpers.longdouble_weight_map(field, raw, t[-1] if case['has_psf_index'] else 0)
            e_orc = float(np.abs(ref[fin].astype(np.longdouble) - exact[fin]).max())
            e_gpu = float(np.abs(dev['composite_ivm'][0][fin].astype(np.longdouble) - exact[fin]).max())
            assert e_gpu <= 4.0 * e_orc + 1e-11 * scale, (shape, e_gpu / scale, e_orc / scale)
        if max(shape) > 1024:
            # sides above 1024: the posterior-image sums too (k_raster_sums with one row per wave, the forward row
            # kernel's from-image form and the inverse kernel's image outputs of the three-stage family)
            check_posterior_sums(model, theta[pair], refs, shape)
    # the device-computed PSF spectra of this shape against numpy
    psf_spec, var_spec = model.engine.spectra()
    for k in range(len(case['psfs'])):
        assert np.abs(psf_spec[k] - field.psf_spec[k]).max() <= 1e-13 * np.abs(field.psf_spec[k]).max()
        assert np.abs(var_spec[k] - field.var_spec[k]).max() <= 1e-13 * np.abs(field.var_spec[k]).max()
    model.close()


# (676 ... 840: sides whose inverse row kernel is the three-stage one; 1280 ... 2048: the three-stage row and column
# kernels, k_cols3f at 1536 and 2048)
@pytest.mark.parametrize('n_side', [96, 100, 120, 150, 180, 200, 250, 300, 384, 500, 640, 900,
                                    676, 720, 728, 780, 784, 840, 1280, 1536, 2048])
def test_general_sides_with_distinct_walkers(n_side):
    """A batch of DISTINCT walkers (prior draws and near-truth) on square general-side fields:
    the fused kernels against the hipFFT back end (independent arithmetic), the oracle on two
    walkers, and bitwise independence of batch order and composition -- the column kernel's
    kx-major work order, idle lanes and spare slots must not leak between walkers."""
    from test_gpu_fullsize import make_model
    n_sersic = 2 if n_side <= 300 else 1
    n_w = 24 if n_side <= 500 else 10 if n_side <= 1024 else 5
    model, fld = make_model(n_side, n_sersic, 'fused', max_walkers=n_w)
    ref, _ = make_model(n_side, n_sersic, 'hipfft', max_walkers=n_w)
    theta = np.vstack([synth_field.draw_walkers(n_side, n_sersic, n_w // 2, seed=n_side),
                       synth_field.draw_walkers(n_side, n_sersic, n_w - n_w // 2, seed=n_side + 1,
                                                near_truth=fld['truth'])])
    got = model.log_posterior_batch(theta)
    assert np.isfinite(got).all()
    assert helpers.rel_err(got, ref.log_posterior_batch(theta)) <= 1e-11
    field = orc.make_field(fld['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mag_zp=fld['mag_zp'])
    prior = model.log_priors_batch(theta[[0, n_w - 1]])
    for i, p in zip((0, n_w - 1), prior):
        want = helpers.oracle_loglike(field, helpers.synth_layout(n_sersic), theta[i]) + p
        assert abs(got[i] - want) <= 1e-10 * abs(want), (n_side, i)
    perm = np.random.RandomState(n_side).permutation(n_w)
    assert np.array_equal(model.log_posterior_batch(theta[perm]), got[perm])
    assert np.array_equal(model.log_posterior_batch(theta[2:5]), got[2:5])
    assert np.array_equal(model.log_posterior_batch(theta[-1:]), got[-1:])
    model.close()
    ref.close()


# even sides the transforms are NOT built for (prime factors above 13, or no P x T split with P, T <= 32):
# embedded in the next built side >= side + PSF side - 1 (psfmc_device.h WrapDesc), each axis on its own
EMBEDDED_SHAPES = [(170, 170), (256, 90), (490, 64), (64, 490), (74, 74), (134, 256), (200, 134), (166, 226),
                   (238, 340), (68, 1000), (958, 70), (290, 292), (990, 82), (94, 102), (502, 514), (686, 98),
                   (642, 70), (70, 642),        # (642: the smallest sides that fit -- 650, 660, 676 -- have slow kernels)
                   (1000, 1000), (1100, 1024), (66, 1030), (1300, 70), (1984, 64)]   # round 4: embedded above 1024


@pytest.mark.parametrize('shape', EMBEDDED_SHAPES, ids=lambda s: '%dx%d' % s)
def test_embedded_sides_match_oracle(shape):
    """Image sides outside the built list on the fused kernels (round-2 review: `backend='auto'` left them
    to hipFFT): five distinct walkers (one outside the priors) in passes of at most two against the fp64 oracle
    at the SAME tolerances as the built sides -- the circular convolution of the image's own size, not of a
    padded one (psfMC/utils.py:25-32) -- and against the hipFFT back end, which transforms at the image's size;
    all five images of two walkers from one call and their posterior-image sums."""
    from psfmc_amd import engine
    seed = 3000 + shape[0] * 7 + shape[1]
    n_w = 5
    case = random_case(seed, shape, n_walkers=n_w)
    theta = case['theta']
    psf_shape = case['psfs'][0].shape
    assert engine.fused_supports(shape[0], shape[1], psf_shape) and not engine.fused_supports(*shape)
    field = orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'],
                           mag_zp=case['zp'])
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in theta])
    model = build(case, 'auto', max_walkers=8)
    assert model._backend == 'fused'
    # the transform shape: built sides with room for the image and the wrap-around margin -- the smallest
    # such side or a larger one whose kernels are cheaper (psfmc_hip.hip choose_embedding)
    for axis, key in ((0, 'transform_ny'), (1, 'transform_nx')):
        side = int(model.engine.get_option(key))
        assert side in engine.FUSED_SIDES
        assert side == shape[axis] or side >= engine.embedding_side(shape[axis], psf_shape[axis])
    several_passes(model, n_w)
    got = model.log_posterior_batch(theta)
    prior = model.log_priors_batch(theta)
    check_walkers(got, want_ll, prior, case['outside'], shape)
    ref = build(case, 'hipfft', max_walkers=8)
    other = ref.log_posterior_batch(theta)
    assert np.array_equal(np.isfinite(other), np.isfinite(got)), shape
    fin = np.isfinite(got)
    assert np.all(np.abs(got[fin] - other[fin]) <= 2e-10 * np.abs(want_ll[fin])), shape
    pair = image_pair(want_ll)
    if pair:
        refs = [oracle_walker(field, case, theta[i], images=True)[1] for i in pair]
        check_images(model.sample_images(theta[pair]), refs, shape)
        # posterior-image sums (the linear-sum route rasterises with the wrapped coordinates too)
        check_posterior_sums(model, theta[pair], refs, shape)
    model.close()
    ref.close()


def test_embedded_side_with_distinct_walkers_and_priors():
    """170 x 170 (2 x 5 x 17) through the raw-vector path: priors, early-out, a batch of distinct walkers,
    the device sampler -- against the hipFFT back end and the oracle."""
    from test_gpu_fullsize import make_model
    n_side, n_sersic, n_w = 170, 1, 24
    model, fld = make_model(n_side, n_sersic, 'auto', max_walkers=n_w)
    assert model._backend == 'fused'
    ref, _ = make_model(n_side, n_sersic, 'hipfft', max_walkers=n_w)
    theta = np.vstack([synth_field.draw_walkers(n_side, n_sersic, n_w // 2, seed=n_side),
                       synth_field.draw_walkers(n_side, n_sersic, n_w - n_w // 2, seed=n_side + 1,
                                                near_truth=fld['truth'])])
    got = model.log_posterior_batch(theta)
    assert np.isfinite(got).all()
    assert helpers.rel_err(got, ref.log_posterior_batch(theta)) <= 1e-11
    field = orc.make_field(fld['sci'], fld['ivm'], [fld['psf']], [fld['psf_ivm']], mag_zp=fld['mag_zp'])
    prior = model.log_priors_batch(theta[[0, n_w - 1]])
    for i, p in zip((0, n_w - 1), prior):
        want = helpers.oracle_loglike(field, helpers.synth_layout(n_sersic), theta[i]) + p
        assert abs(got[i] - want) <= 1e-10 * abs(want), i
    perm = np.random.RandomState(n_side).permutation(n_w)
    assert np.array_equal(model.log_posterior_batch(theta[perm]), got[perm])
    from psfmc_amd import DeviceEnsembleSampler
    samp = DeviceEnsembleSampler(n_w, model, block=3)
    samp.random_state = np.random.RandomState(5).get_state()
    for res in samp.sample(theta, iterations=4):
        pass
    assert np.isfinite(res[1]).all() and samp.naccepted.sum() > 0
    assert np.array_equal(model.log_posterior_batch(res[0]), res[1])
    with pytest.raises(Exception):
        model.engine.spectra()
    model.close()
    ref.close()


# one rectangular shape per kernel family of the fused back end: (shape, column engine -- 0 k_cols, 2 k_cols3g,
# 3 k_cols3f --, rows3 -- bit 0 forward, bit 1 inverse three-stage row kernel --, row layout group, embedded)
SCHEDULE_PATHS = [((200, 256), 0, 0, 4, False),        # k_cols two-stage
                  ((150, 64), 0, 0, 4, False),         # the guarded row kernel (150 rows: no whole fast groups)
                  ((300, 128), 2, 0, 4, False),        # row-group fallback: 128's fast groups of 8 do not divide 300
                  ((384, 64), 2, 0, 8, False),         # k_cols3g with its load pipeline, fast row groups of 8
                  ((392, 96), 2, 0, 4, False),         # k_cols3g, load pipeline off
                  ((512, 96), 3, 0, 4, False),         # k_cols3f
                  ((1024, 100), 3, 0, 4, False),       # k_cols3f
                  ((96, 676), 0, 2, 4, False),         # three-stage inverse row kernel
                  ((84, 2048), 0, 3, 1, False),        # three-stage forward and inverse row kernels above 1024
                  ((1536, 96), 3, 0, 4, False),        # k_cols3f above 1024
                  ((166, 226), 0, 0, 4, True)]         # embedded


def test_schedule_paths_cover_every_family():
    assert {p[1] for p in SCHEDULE_PATHS} == {0, 2, 3}
    assert {b for p in SCHEDULE_PATHS for b in (1, 2) if p[2] & b} == {1, 2}
    assert any(p[4] for p in SCHEDULE_PATHS) and all(p[0][0] != p[0][1] for p in SCHEDULE_PATHS)


@pytest.mark.parametrize('path', SCHEDULE_PATHS, ids=lambda p: '%dx%d' % p[0])
def test_schedule_invariance_across_kernel_families(path):
    """A distinct-walker batch gives the same bits under every schedule: streams 1 ... 4, passes of 1, 3, 5
    walkers and the default, a single pass split over two streams (min_split), a permuted batch, single-walker and
    pass-straddling sub-batches, every `exclusive` chaining with and without `stagger`, and the device sampler with
    and without graph replay.  A missing event between
    lanes or a pass offset applied twice would change some walker's value."""
    from psfmc_amd import DeviceEnsembleSampler
    shape, col, rows3, group, embedded = path
    n_w = 7
    case = random_case(7000 + shape[0] * 3 + shape[1], shape, n_walkers=n_w)
    theta = case['theta']
    model = build(case, 'auto', max_walkers=8)
    assert model._backend == 'fused'
    eng = model.engine
    assert (eng.get_option('column_engine'), eng.get_option('rows3'), eng.get_option('row_group')) == \
        (col, rows3, group), shape
    transform = (int(eng.get_option('transform_ny')), int(eng.get_option('transform_nx')))
    assert (transform != shape) == embedded, transform
    default = int(eng.get_option('chunk_walkers'))
    default_stagger = int(eng.get_option('stagger'))
    base = model.log_posterior_batch(theta)
    inside = np.isfinite(model.log_priors_batch(theta))
    assert np.isfinite(base[inside]).all() and np.all(base[~inside] == -np.inf)
    assert len(np.unique(base[inside])) == inside.sum()

    def same(tag, sub=slice(None)):
        assert np.array_equal(model.log_posterior_batch(theta[sub]), base[sub]), (shape, tag)
    try:
        for streams in (1, 2, 3, 4):
            eng.set_option('streams', streams)
            assert eng.get_option('streams') == streams
            for chunk in (1, 3, 5, default):
                eng.set_option('chunk_walkers', chunk)
                same(('streams', streams, 'chunk', chunk))
                same(('single', streams, chunk), slice(3, 4))
                same(('straddling', streams, chunk), slice(1, 6))
        # passes of 5: seven walkers run as ONE pass (up to two passes' worth), or with min_split on as two
        # passes of 4 and 3 on the two streams
        eng.set_option('streams', 2)
        eng.set_option('chunk_walkers', 5)
        eng.set_option('min_split', 1)
        assert eng.pass_size(n_w) == 4
        same('min_split on')
        eng.set_option('min_split', 1 << 30)
        assert eng.pass_size(n_w) == n_w
        same('min_split off')
        # the measurement knobs (psfmc_hip.hip run_pipeline): kernels of the kinds in `exclusive` (bits 0 ... 2) of
        # one pass wait for those of the pass before, on two streams; `stagger` delays the second lane by one
        # forward-row kernel from 8 passes on -- eight walkers (walker 0 twice) in passes of one
        eight, want8 = np.vstack([theta, theta[:1]]), np.concatenate([base, base[:1]])
        for stagger in (0, 1):
            eng.set_option('stagger', stagger)
            for exclusive in range(8):
                eng.set_option('exclusive', exclusive)
                assert (eng.get_option('stagger'), eng.get_option('exclusive')) == (stagger, exclusive)
                for streams in (2, 4):
                    eng.set_option('streams', streams)
                    for chunk in (1, default):
                        eng.set_option('chunk_walkers', chunk)
                        same(('stagger', stagger, 'exclusive', exclusive, streams, chunk))
                        assert np.array_equal(model.log_posterior_batch(eight), want8), (shape, stagger, exclusive)
        eng.set_option('stagger', default_stagger)
        eng.set_option('exclusive', 0)
        eng.set_option('streams', 2)
        eng.set_option('chunk_walkers', default)
        perm = np.random.RandomState(shape[0]).permutation(n_w)
        assert np.array_equal(model.log_posterior_batch(theta[perm]), base[perm]), shape
        chains = []
        for graph in (0, 1):
            eng.set_option('graph', graph)
            launches = eng.get_option('graph_launches')
            samp = DeviceEnsembleSampler(int(inside.sum()), model, block=3, live_dangerously=True)
            samp.random_state = np.random.RandomState(1).get_state()
            for res in samp.sample(theta[inside], iterations=3):
                pass
            assert (eng.get_option('graph_launches') > launches) == bool(graph)
            chains.append((samp.chain.copy(), samp.lnprobability.copy()))
        assert np.array_equal(chains[0][0], chains[1][0]) and np.array_equal(chains[0][1], chains[1][1]), shape
    finally:
        eng.set_option('graph', 0)
        eng.set_option('min_split', 1 << 30)
        eng.set_option('streams', 2)
        eng.set_option('chunk_walkers', default)
        eng.set_option('stagger', default_stagger)
        eng.set_option('exclusive', 0)
    model.close()


def edge_case(seed, shape, psf_shape, comps=None, n_walkers=5, n_psf=1):
    """A random field (`random_case`) with n_psf PSFs of the given shape (each wider than the one before; with
    several, the PSF index is free) and, if given, these components; in the free-parameter form."""
    case = random_case(seed, shape)
    rng = np.random.RandomState(seed + 1)
    py, px = psf_shape
    yy, xx = np.mgrid[0:py, 0:px].astype(float)
    case['psfs'], case['pivms'] = [], []
    for k in range(n_psf):
        core = (1 + ((xx - px // 2) ** 2 + (yy - py // 2 + 0.1) ** 2) / (2.0 + 0.6 * k) ** 2) ** -2.5 * 300
        var = 0.01 + core / 40.0
        case['psfs'].append((core + rng.normal(size=core.shape) * np.sqrt(var)).astype(np.float32))
        case['pivms'].append((1.0 / var).astype(np.float32))
    case['psf_index'] = 0
    if comps is not None:
        case['comps'] = comps
    case.update(free_parameters(case, rng, n_walkers))
    return case


def edge_components(ny, nx):
    """Sersic and point-source centres a few pixels inside and just beyond each of the four edges (the wrapped
    rasteriser of an embedded image, the profile and the shift kernel across the wrap-around margin)."""
    comps = [dict(type='sky', adu=0.003)]
    spots = [(2.5, ny * 0.5), (-1.2, ny * 0.3), (nx - 3.0, ny * 0.6), (nx + 0.8, ny * 0.25),
             (nx * 0.5, 2.2), (nx * 0.3, -1.6), (nx * 0.6, ny - 2.7), (nx * 0.25, ny + 1.1)]
    for k, xy in enumerate(spots):
        if k % 2 == 0:
            comps.append(dict(type='sersic', xy=xy, mag=18.0 + 0.3 * k, reff=3.0 + 0.2 * k, reff_b=2.0, index=1.5,
                              angle=20.0 * k, angle_degrees=True))
        else:
            comps.append(dict(type='ps', xy=xy, mag=18.5 + 0.2 * k, method='lanczos3' if k % 4 == 1 else 'bilinear'))
    return comps


# (image shape, PSF shape, edge components): the PSF as large as the image on both axes and on one, an odd PSF one
# pixel smaller than the image, an embedded axis whose PSF side equals the image side (the widest wrap-around
# margin), and centres at every edge of embedded images
PSF_EDGES = [((64, 64), (64, 64), False), ((64, 128), (64, 64), False), ((96, 100), (96, 33), False),
             ((64, 64), (63, 63), False), ((100, 96), (99, 95), False), ((74, 74), (74, 9), False),
             ((74, 74), (74, 9), True), ((166, 226), (21, 17), True), ((170, 170), (33, 33), True)]


@pytest.mark.parametrize('shape,psf_shape,edges', PSF_EDGES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple)
                         else ('edges' if v else 'random'))
def test_psf_size_edges_match_oracle(shape, psf_shape, edges):
    """PSF-size and centre edges on both back ends: five distinct walkers against the oracle, two walkers'
    images from one call."""
    from psfmc_amd import engine
    seed = 9000 + shape[0] * 7 + shape[1] + psf_shape[1]
    case = edge_case(seed, shape, psf_shape, edge_components(*shape) if edges else None)
    theta = case['theta']
    field = orc.make_field(case['sci'], case['ivm'], case['psfs'], case['pivms'], mask=case['mask'],
                           mag_zp=case['zp'])
    want_ll = np.array([oracle_walker(field, case, t)[0] for t in theta])
    pair = image_pair(want_ll)
    refs = [oracle_walker(field, case, theta[i], images=True)[1] for i in pair]
    for backend in ('fused', 'hipfft'):
        model = build(case, backend, max_walkers=8)
        if backend == 'fused':
            embedded = not engine.fused_supports(*shape)
            transform = (int(model.engine.get_option('transform_ny')), int(model.engine.get_option('transform_nx')))
            assert embedded == (transform != shape)
            if embedded:
                assert all(t >= s + p - 1 for t, s, p in zip(transform, shape, psf_shape) if t != s), transform
        several_passes(model, len(theta))
        got = model.log_posterior_batch(theta)
        check_walkers(got, want_ll, model.log_priors_batch(theta), case['outside'], (shape, psf_shape, backend))
        if pair:
            check_images(model.sample_images(theta[pair]), refs, (shape, psf_shape, backend))
        model.close()
