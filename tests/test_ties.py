"""Ties, `Tied(source, ratio, offset)`, on the host: a model file with variables, the packing and the names, the numpy
definition `ratio * source + offset` in `tied_values`, `derived_rows`, `aux_rows`, `log_priors_batch` and the
single-vector path, the refusals, and the database header.  Every tied model has an UNTIED TWIN -- the same components
with a wide `Uniform` in place of each `Tied` -- and the tests expand the tied model's vectors into the twin's
themselves (`expand`: plain numpy from the table of ties written out beside each model), never through the product.
No GPU needed; the device is held to the same twins in tests/test_gpu_ties.py, which takes its models from here."""
import numpy as np
import pytest
import scipy.stats as st

import test_gpu_general_components as tgg
from psfmc_amd import JointModel, MultiComponentModel, Tied
from psfmc_amd.ModelComponents import Configuration, Moffat, PointSource, Sersic, Sky
from psfmc_amd.distributions import Normal, Uniform

make_field = tgg.make_field


def U(lo, hi):
    """Uniform on [lo, hi] (numbers or vectors) that remembers its scipy form for the tests' own prior sums."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    prior = Uniform(loc=lo, scale=hi - lo)
    prior.scipy = st.uniform(loc=lo, scale=hi - lo)
    return prior


def N(loc, scale):
    prior = Normal(loc=loc, scale=scale)
    prior.scipy = st.norm(loc=np.asarray(loc, dtype=np.float64), scale=np.asarray(scale, dtype=np.float64))
    return prior


def _config(fld):
    return Configuration(fld['sci'], fld['ivm'], fld['psf'], fld['psf_ivm'], mag_zeropoint=fld['mag_zp'])


# ---------------------------------------------------------------------------------------------------------------
# the quasar + host model: plain components.  Ties on xy with a vector offset prior, on reff_b with a ratio prior
# (which reaches 1.2: reff_b > reff is inside the ratio's prior and outside the support), on xy with neither term,
# on an angle to another component's angle with the constant offset 90.
# ---------------------------------------------------------------------------------------------------------------
QSO_TIES = {'2_Sersic_xy': ('1_PointSource_xy', 1.0, '2_Sersic_xy_offset'),
            '2_Sersic_reff_b': ('2_Sersic_reff', '2_Sersic_reff_b_ratio', 0.0),
            '3_Sersic_angle': ('2_Sersic_angle', 1.0, 90.0),
            '3_Sersic_xy': ('1_PointSource_xy', 1.0, 0.0)}


def qso_components(fld, tied):
    """The components of the tied model, or of its twin (tied=False: a wide Uniform where the other has a Tied)."""
    ny, nx = fld['shape']
    c = np.array((nx / 2.0, ny / 2.0))
    tie = (lambda wide, *a, **kw: Tied(*a, **kw)) if tied else (lambda wide, *a, **kw: wide)
    centre, size, ang = U(c - 4.0, c + 4.0), U(2.0, 22.0), U(-180.0, 180.0)
    wide_xy = lambda: U(c - 200.0, c + 200.0)
    return [_config(fld), Sky(adu=N(0.05, 0.05)),
            PointSource(xy=centre, mag=U(17.0, 21.0)),
            Sersic(xy=tie(wide_xy(), centre, offset=N((0.0, 0.0), (0.5, 0.5))), mag=U(16.0, 22.0), reff=size,
                   reff_b=tie(U(0.01, 60.0), size, ratio=U(0.1, 1.2)), index=U(0.5, 6.0), angle=ang, angle_degrees=True),
            Sersic(xy=tie(wide_xy(), centre), mag=U(16.0, 22.0), reff=U(1.0, 30.0), reff_b=U(0.5, 30.0), index=1.0,
                   angle=tie(U(-720.0, 720.0), ang, offset=90.0), angle_degrees=True)]


def qso_theta(model, fld, n_w, seed, spread=1.0):
    """[n_w, P] vectors of the tied QSO model inside every prior and support rule, by name."""
    ny, nx = fld['shape']
    rng = np.random.RandomState(seed)
    r = lambda lo, hi, size=None: rng.uniform(lo, hi, size=(n_w,) + (() if size is None else (size,)))
    mid = lambda lo, hi: (0.5 * (lo + hi) - 0.5 * spread * (hi - lo), 0.5 * (lo + hi) + 0.5 * spread * (hi - lo))
    vals = {'0_Sky_adu': r(*mid(0.03, 0.07)), '1_PointSource_mag': r(*mid(18.0, 20.0)),
            '1_PointSource_xy': np.array((nx / 2.0, ny / 2.0)) + r(*mid(-2.0, 2.0), size=2),
            '2_Sersic_angle': r(*mid(-60.0, 80.0)), '2_Sersic_index': r(*mid(1.0, 3.5)), '2_Sersic_mag': r(*mid(17.5, 19.5)),
            '2_Sersic_reff': r(*mid(5.0, 12.0)), '2_Sersic_reff_b_ratio': r(*mid(0.3, 0.9)),
            '2_Sersic_xy_offset': r(*mid(-0.6, 0.6), size=2),
            '3_Sersic_mag': r(*mid(18.0, 20.0)), '3_Sersic_reff': r(*mid(9.0, 14.0)), '3_Sersic_reff_b': r(*mid(3.0, 8.0))}
    return pack(model, vals, n_w)


# ---------------------------------------------------------------------------------------------------------------
# the general model: ties in the auxiliary table -- a Sky slope, a boxiness, a Fourier amplitude, a spiral r_out as
# a ratio of r_in's source, a truncation radius, a bending amplitude -- and on a Moffat's fwhm_b; pixel_mean on one
# ---------------------------------------------------------------------------------------------------------------
GEN_TIES = {'1_Sky_slope': ('0_Sky_slope', -0.5, 0.0),
            '4_Moffat_boxiness': ('3_Sersic_boxiness', -1.0, 0.25),
            '4_Moffat_f2_amp': ('3_Sersic_f2_amp', 0.5, 0.0),
            '4_Moffat_spiral_r_out': ('4_Moffat_spiral_r_in', 3.0, 1.0),
            '4_Moffat_trunc_out_lo': ('3_Sersic_trunc_out_lo', 1.0, 2.0),
            '4_Moffat_bend2': ('3_Sersic_bend2', '4_Moffat_bend2_ratio', 0.0),
            '4_Moffat_fwhm_b': ('4_Moffat_fwhm', '4_Moffat_fwhm_b_ratio', 0.0)}


def gen_components(fld, tied):
    ny, nx = fld['shape']
    c = np.array((nx / 2.0, ny / 2.0))
    tie = (lambda wide, *a, **kw: Tied(*a, **kw)) if tied else (lambda wide, *a, **kw: wide)
    slope, box, amp, r_in, t_lo, bend, fw = (U((-1e-3, -1e-3), (1e-3, 1e-3)), U(-1.0, 1.5), U(-0.6, 0.6), U(0.0, 8.0),
                                             U(6.0, 20.0), U(-0.5, 0.5), U(3.0, 20.0))
    return [_config(fld), Sky(adu=N(0.05, 0.05), slope=slope),
            Sky(adu=0.0, slope=tie(U((-1.0, -1.0), (1.0, 1.0)), slope, ratio=-0.5)),
            PointSource(xy=(nx / 2 + 1.3, ny / 2 - 0.8), mag=U(17.0, 21.0)),
            Sersic(xy=U(c - 4.0, c + 4.0), mag=U(16.0, 22.0), reff=U(2.0, 22.0), reff_b=U(1.0, 22.0), index=U(0.5, 4.0),
                   angle=30.0, angle_degrees=True, boxiness=box, fourier={2: (amp, 20.0)},
                   truncation={'outer': (t_lo, 40.0)}, bending={2: bend}, pixel_mean=True),
            Moffat(xy=U(c - 4.0, c + 4.0), mag=U(16.0, 22.0), fwhm=fw, fwhm_b=tie(U(0.01, 60.0), fw, ratio=U(0.2, 0.9)),
                   beta=U(1.5, 5.0), angle=70.0, angle_degrees=True, boxiness=tie(U(-3.0, 3.0), box, ratio=-1.0, offset=0.25),
                   fourier={2: (tie(U(-2.0, 2.0), amp, ratio=0.5), 10.0)},
                   spiral=dict(r_in=r_in, r_out=tie(U(-5.0, 100.0), r_in, ratio=3.0, offset=1.0), winding=100.0),
                   truncation={'outer': (tie(U(-5.0, 100.0), t_lo, offset=2.0), 45.0)},
                   bending={2: tie(U(-3.0, 3.0), bend, ratio=U(-1.0, 1.0))})]


def gen_theta(model, fld, n_w, seed):
    ny, nx = fld['shape']
    rng = np.random.RandomState(seed)
    r = lambda lo, hi, size=None: rng.uniform(lo, hi, size=(n_w,) + (() if size is None else (size,)))
    c = np.array((nx / 2.0, ny / 2.0))
    vals = {'0_Sky_adu': r(0.04, 0.06), '0_Sky_slope': r(1e-5, 2e-4, size=2), '2_PointSource_mag': r(18.5, 19.5),
            '3_Sersic_bend2': r(-0.2, 0.2), '3_Sersic_boxiness': r(-0.4, 0.6), '3_Sersic_f2_amp': r(-0.3, 0.3),
            '3_Sersic_index': r(1.0, 2.5), '3_Sersic_mag': r(17.5, 18.5), '3_Sersic_reff': r(8.0, 11.0),
            '3_Sersic_reff_b': r(4.0, 7.0), '3_Sersic_trunc_out_lo': r(12.0, 16.0), '3_Sersic_xy': c + r(-2.0, 2.0, size=2),
            '4_Moffat_bend2_ratio': r(-0.9, 0.9), '4_Moffat_beta': r(2.0, 3.5), '4_Moffat_fwhm': r(6.0, 10.0),
            '4_Moffat_fwhm_b_ratio': r(0.4, 0.8), '4_Moffat_mag': r(18.0, 19.0), '4_Moffat_spiral_r_in': r(1.0, 4.0),
            '4_Moffat_xy': c + r(-3.0, 3.0, size=2)}
    return pack(model, vals, n_w)


def pack(model, vals, n_w):
    out = np.zeros((n_w, model.num_params))
    left = dict(vals)
    pos = 0
    for name, width in zip(model.param_names, model.param_lens):
        out[:, pos:pos + width] = np.reshape(left.pop(name), (n_w, width))
        pos += width
    assert not left, sorted(left)
    return out


def build(components, fld, tied, **kw):
    return MultiComponentModel(components(fld, tied), **kw)


def columns_of(model, name):
    names = sum(([n] * w for n, w in zip(model.param_names, model.param_lens)), [])
    return [i for i, n in enumerate(names) if n == name]


def expand(tied, twin, ties, theta):
    """theta of the tied model [W, P_free] -> the twin's vectors [W, P_full]: a free parameter copied, a tied one
    ratio * source + offset in plain numpy, ratio / offset a number or the name of the column block that holds it.
    The twin has no column for a ratio / offset prior."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    get = lambda term: theta[:, columns_of(tied, term)] if isinstance(term, str) else term
    out = np.zeros((theta.shape[0], twin.num_params))
    for name in twin.param_names:
        if name in ties:
            src, ratio, offset = ties[name]
            out[:, columns_of(twin, name)] = get(ratio) * get(src) + get(offset)
        else:
            out[:, columns_of(twin, name)] = get(name)
    return out


def scipy_prior_sum(model, theta):
    """The sum of the free columns' priors of a model built from `U` / `N`, with scipy directly."""
    total = np.zeros(theta.shape[0])
    for comp, span in zip(model.components, model._spans):
        pos = span.start
        for attr, width in zip(comp.free_names(), comp.stochastic_lens()):
            total = total + np.sum(comp._priors[attr].scipy.logpdf(theta[:, pos:pos + width]), axis=1)
            pos += width
    return total


MODELS = [(qso_components, QSO_TIES, qso_theta), (gen_components, GEN_TIES, gen_theta)]


# -- 1. a model file ---------------------------------------------------------------------------------------------
MODEL_FILE = """
Configuration(obs_file='sci.fits', obsivm_file='ivm.fits', psf_files='psf.fits', psfivm_files='psf_ivm.fits',
              mag_zeropoint=25.0)
centre = Uniform(loc=(28, 28), scale=(8, 8))
size = Uniform(loc=2, scale=20)
Sky(adu=Normal(loc=0, scale=0.1))
PointSource(xy=centre, mag=Uniform(loc=17, scale=4))
Sersic(xy=Tied(centre, offset=Normal(loc=(0, 0), scale=(0.5, 0.5))),
       reff=size, reff_b=Tied(size, ratio=Uniform(loc=0.1, scale=0.8)),
       mag=Uniform(loc=17, scale=4), index=Uniform(loc=0.5, scale=5), angle=Uniform(loc=0, scale=180),
       angle_degrees=True)
"""


def test_a_model_file_with_variables_and_tied(tmp_path):
    from psfmc_amd import fits_io
    fld = make_field(64, 64, seed=1)
    for name in ('sci', 'ivm', 'psf', 'psf_ivm'):
        fits_io.write_image(str(tmp_path / (name + '.fits')), fld[name])
    path = tmp_path / 'model.py'
    path.write_text(MODEL_FILE)
    model = MultiComponentModel(str(path))
    assert model.param_names == ['0_Sky_adu', '1_PointSource_mag', '1_PointSource_xy', '2_Sersic_angle', '2_Sersic_index',
                                 '2_Sersic_mag', '2_Sersic_reff', '2_Sersic_reff_b_ratio', '2_Sersic_xy_offset']
    assert model.param_lens == [1, 1, 2, 1, 1, 1, 1, 1, 2] and model.num_params == 11
    assert model.param_fits_abbrs[-3:] == ['2SER_RE', '2SERREBR', '2SERxyO']
    assert all(len(n) <= 8 for n in model.param_fits_abbrs)
    theta = np.array([[0.01, 18.0, 30.5, 31.25, 40.0, 2.0, 19.0, 10.0, 0.3, 0.125, -0.25],
                      [0.02, 19.0, 29.0, 33.0, 50.0, 1.0, 18.0, 7.0, 0.7, 0.0, 0.4]])
    got = model.tied_values(theta)
    assert sorted(got) == ['2_Sersic_reff_b', '2_Sersic_xy']
    assert np.array_equal(got['2_Sersic_reff_b'], theta[:, 8] * theta[:, 7] + 0.0)
    assert np.array_equal(got['2_Sersic_xy'], 1.0 * theta[:, 2:4] + theta[:, 9:11])
    assert model.tie_records == [('2SER_REB', '2SER_RE', '2SERREBR', 0.0), ('2SER_xy', '1PS_xy', 1.0, '2SERxyO')]


def test_short_names_are_short_and_distinct():
    """Every column's and every tied attribute's FITS name over both models: at most 8 characters and no two alike --
    the ratio / offset columns of the long attributes (`trunc_out_lo`, `spiral_r_out`, `bend2`, `f2_amp`, `fwhm_b`)
    among them, and, beside the general model's, ratio and offset priors on every one of its tied attributes."""
    fld = make_field(64, 64, seed=1)
    comps = gen_components(fld, True)
    for comp in comps[1:]:
        for attr, tie in list(comp._ties.items()):
            width = comp.attr_width(attr)
            setattr(comp, attr, Tied(tie.source, ratio=U(0.1, 0.9),
                                     offset=N((0.0,) * width, (1.0,) * width) if width > 1 else N(0.0, 1.0)))
    for model in (build(qso_components, fld, True), build(gen_components, fld, True), MultiComponentModel(comps)):
        names = model.param_fits_abbrs + [r[0] for r in model.tie_records]
        assert len(names) == len(set(names)), sorted(names)
        assert all(0 < len(n) <= 8 for n in names), [n for n in names if len(n) > 8]
    assert {'4MOFTOLR', '4MOFTOLO', '4MOFSROR', '4MOFBD2R', '4MOFF2AO', '4MOFFWBR', '1SkySLPO'} <= set(names)


# -- 2. rows and auxiliary rows against the twin --------------------------------------------------------------------
@pytest.mark.parametrize('components,ties,draw', MODELS, ids=['qso', 'general'])
def test_rows_and_aux_rows_equal_the_twins(components, ties, draw):
    fld = make_field(64, 64, seed=2)
    tied, twin = build(components, fld, True), build(components, fld, False)
    assert tied.num_params == twin.num_params - sum(len(columns_of(twin, n)) for n in ties) + sum(
        len(columns_of(tied, t)) for v in ties.values() for t in v[1:] if isinstance(t, str))
    theta = draw(tied, fld, 9, seed=3)
    full = expand(tied, twin, ties, theta)
    assert np.array_equal(tied.derived_rows(theta), twin.derived_rows(full))
    a, b = tied.aux_rows(theta), twin.aux_rows(full)
    assert (a is None and b is None) or np.array_equal(a, b)
    if components is gen_components:
        assert a.shape == (9, 2 * 2 + 29 * 2)
    resolved = tied.tied_values(theta)
    assert sorted(resolved) == sorted(ties)
    for name, vals in resolved.items():
        assert np.array_equal(np.reshape(vals, (9, -1)), full[:, columns_of(twin, name)]), name


# -- 3. priors -----------------------------------------------------------------------------------------------------
def test_log_priors_are_the_free_columns_and_the_resolved_support():
    fld = make_field(64, 64, seed=2)
    tied, twin = build(qso_components, fld, True), build(qso_components, fld, False)
    theta = qso_theta(tied, fld, 12, seed=4)
    col = lambda name: columns_of(tied, name)[0]
    theta[3, col('2_Sersic_reff_b_ratio')] = 1.15          # inside the ratio's prior, reff_b > reff
    theta[5, col('2_Sersic_reff_b_ratio')] = 1.0           # reff_b == reff: inside
    theta[7, col('1_PointSource_mag')] = 30.0              # outside a free column's prior
    want = scipy_prior_sum(tied, theta)
    assert np.isfinite(want[3]) and np.isfinite(want[5]) and want[7] == -np.inf
    inside = np.isfinite(twin.log_priors_batch(expand(tied, twin, QSO_TIES, theta)))
    assert list(np.flatnonzero(~inside)) == [3, 7]
    got = tied.log_priors_batch(theta)
    assert np.array_equal(np.isfinite(got), inside)
    assert np.allclose(got[inside], want[inside], rtol=1e-14, atol=0)
    # the general model: a resolved boxiness <= -2, sum |a_m| >= 1 of a resolved amplitude, a resolved r_out <= r_in,
    # a resolved truncation lo >= hi, a resolved bending amplitude that is not finite, a resolved beta is not there
    tied, twin = build(gen_components, fld, True), build(gen_components, fld, False)
    theta = gen_theta(tied, fld, 8, seed=5)
    col = lambda name: columns_of(tied, name)[0]
    theta[1, col('3_Sersic_boxiness')] = 1.4               # the Moffat's: -1.4 + 0.25 > -2: inside
    theta[2, col('4_Moffat_fwhm_b_ratio')] = 0.9           # on the ratio prior's edge: inside
    theta[4, col('4_Moffat_spiral_r_in')] = -0.25          # outside its own prior (and r_in < 0)
    theta[6, col('3_Sersic_trunc_out_lo')] = 19.9          # the Sersic's 19.9 < 40 inside; the Moffat's 21.9 < 45 inside
    want = scipy_prior_sum(tied, theta)
    inside = np.isfinite(twin.log_priors_batch(expand(tied, twin, GEN_TIES, theta)))
    assert list(np.flatnonzero(~inside)) == [4]
    got = tied.log_priors_batch(theta)
    assert np.array_equal(np.isfinite(got), inside) and np.allclose(got[inside], want[inside], rtol=1e-14, atol=0)
    # a support rule that only the RESOLVED value breaks: a truncation radius tied past its partner
    bad = theta[:1].copy()
    bad[0, col('3_Sersic_trunc_out_lo')] = 19.0
    wider = gen_components(fld, True)
    wider[5].trunc_out_lo = Tied(wider[4]._priors['trunc_out_lo'], offset=30.0)        # 49 >= 45
    model = MultiComponentModel(wider)
    assert np.isfinite(scipy_prior_sum(model, bad)[0]) and model.log_priors_batch(bad)[0] == -np.inf


# -- 4. refusals -----------------------------------------------------------------------------------------------------
def _with(fld, **sersic_kw):
    ny, nx = fld['shape']
    kw = dict(xy=U((20.0, 20.0), (40.0, 40.0)), mag=U(16.0, 22.0), reff=U(2.0, 22.0), reff_b=U(1.0, 22.0), index=2.0,
              angle=0.0)
    kw.update(sersic_kw)
    return kw


def test_refusals_name_the_attribute():
    fld = make_field(64, 64, seed=2)
    centre, size = U((28.0, 28.0), (36.0, 36.0)), U(2.0, 22.0)
    ps = lambda: PointSource(xy=centre, mag=U(17.0, 21.0))
    model = lambda *comps: MultiComponentModel([_config(fld), Sky(adu=0.0)] + list(comps))
    with pytest.raises(ValueError, match=r'Sersic\.xy.*itself tied'):
        model(ps(), Sersic(**_with(fld, xy=Tied(Tied(centre)))))
    with pytest.raises(ValueError, match=r'Sersic\.reff_b.*not a free parameter of a component of this model'):
        model(ps(), Sersic(**_with(fld, reff_b=Tied(size))))                # `size` is given to no attribute
    with pytest.raises(ValueError, match=r'Sersic\.reff_b.*not a free parameter'):
        model(ps(), Sersic(**_with(fld, reff_b=Tied(3.0))))
    with pytest.raises(ValueError, match=r'Sersic\.reff_b.*1-element attribute tied to a source of 2'):
        model(ps(), Sersic(**_with(fld, reff_b=Tied(centre))))
    with pytest.raises(ValueError, match=r'Sersic\.xy.*2-element attribute tied to a source of 1'):
        model(ps(), Sersic(**_with(fld, reff=size, xy=Tied(size))))
    with pytest.raises(ValueError, match=r'Sersic\.reff_b.*ratio has 2 elements'):
        model(ps(), Sersic(**_with(fld, reff=size, reff_b=Tied(size, ratio=(0.5, 0.6)))))
    with pytest.raises(ValueError, match=r'Sersic\.reff_b.*offset has 2 elements'):
        model(ps(), Sersic(**_with(fld, reff=size, reff_b=Tied(size, offset=N((0.0, 0.0), (1.0, 1.0))))))
    # one prior object given bare to two attributes (it made two columns until now): refused, pointing to Tied
    with pytest.raises(ValueError, match=r'Sersic\.xy: the prior object is also given to PointSource\.xy.*Tied\('):
        model(ps(), Sersic(**_with(fld, xy=centre)))
    with pytest.raises(ValueError, match=r'Sersic\.reff_b.*also given to Sersic\.reff.*Tied\('):
        model(ps(), Sersic(**_with(fld, reff=size, reff_b=size)))
    # ... two separate but equal prior objects are two parameters, as ever; so is a model with a PSF index
    same = lambda: U((28.0, 28.0), (36.0, 36.0))
    both = model(PointSource(xy=same(), mag=U(17.0, 21.0)), Sersic(**_with(fld, xy=same())))
    assert both.num_params == 8 and '1_PointSource_xy' in both.param_names and '2_Sersic_xy' in both.param_names
    psfs = Configuration(fld['sci'], fld['ivm'], [fld['psf'], fld['psf']], [fld['psf_ivm'], fld['psf_ivm']],
                         mag_zeropoint=25.0)
    assert MultiComponentModel([psfs, Sky(adu=0.0), ps(), Sersic(**_with(fld, xy=Tied(centre)))]).param_names[-1] == \
        'PSF_Index'
    # the PSF index: not tied, not a source
    two = Configuration(fld['sci'], fld['ivm'], [fld['psf'], fld['psf']], [fld['psf_ivm'], fld['psf_ivm']],
                        mag_zeropoint=25.0)
    index = two.psf_selector._priors['psf_index']
    with pytest.raises(ValueError, match=r'Sersic\.index.*PSF index cannot be the source'):
        MultiComponentModel([two, Sky(adu=0.0), ps(), Sersic(**_with(fld, index=Tied(index, offset=1.0)))])
    two.psf_selector.psf_index = Tied(size)
    with pytest.raises(ValueError, match=r'PSFSelector\.psf_index.*cannot be tied'):
        MultiComponentModel([two, Sky(adu=0.0), ps(), Sersic(**_with(fld, reff=size))])
    # a joint fit: a tied attribute is no per_field name; the ties are the same in every exposure
    fa, fb = make_field(64, 64, seed=3), make_field(64, 64, seed=4)
    a, b = build(qso_components, fa, True), build(qso_components, fb, True)
    with pytest.raises(ValueError, match=r"2_Sersic_reff_b.*tied attribute"):
        JointModel([a, b], per_field=['2_Sersic_reff_b'])
    other = qso_components(fb, True)
    other[4].angle = Tied(other[3]._priors['angle'], offset=45.0)
    with pytest.raises(ValueError, match='the ties of a joint fit are the same in every field'):
        JointModel([a, MultiComponentModel(other)])
    untied = qso_components(fb, True)
    untied[4].xy = Tied(untied[3]._priors['xy_offset'])
    with pytest.raises(ValueError, match=r'Sersic\.xy.*ratio / offset of another tie'):
        MultiComponentModel(untied)
    JointModel([a, b], per_field=['1_PointSource_xy'])                      # the SOURCE may be per field


# -- 5. database header ---------------------------------------------------------------------------------------------
class _Chain(object):
    def __init__(self, n_w, n_it, p, seed):
        rng = np.random.RandomState(seed)
        self.chain = rng.normal(size=(n_w, n_it, p))
        self.lnprobability = rng.normal(size=(n_w, n_it))


def test_database_header_records_the_ties(tmp_path):
    from psfmc_amd.database import database_ties, load_database, save_database
    fld = make_field(64, 64, seed=2)
    tied, twin = build(qso_components, fld, True), build(qso_components, fld, False)
    db = save_database(_Chain(4, 3, tied.num_params, 1), tied, str(tmp_path / 'tied_db.fits'))
    assert [n for n in db.colnames if n not in ('lnprobability', 'walker', 'sample')] == tied.param_names
    db = load_database(str(tmp_path / 'tied_db.fits'))
    assert db.meta['MCTIES'] == 4
    assert db.meta['MCTIE0'] == '2SER_REB 2SER_RE' and db.meta['MCTIR0'] == '2SERREBR'
    assert db.meta['MCTIO0'] == 0.0 and not isinstance(db.meta['MCTIO0'], str)    # a number is a FITS number
    assert db.meta['MCTIO2'] == 90.0 and db.meta['MCTIR2'] == 1.0 and db.meta['MCTIO1'] == '2SERxyO'
    assert database_ties(db) == [('2SER_REB', '2SER_RE', '2SERREBR', 0.0), ('2SER_xy', '1PS_xy', 1.0, '2SERxyO'),
                                 ('3SER_ANG', '2SER_ANG', 1.0, 90.0), ('3SER_xy', '1PS_xy', 1.0, 0.0)]
    # a vector constant: its numbers in one string, read back as a tuple
    gen = build(gen_components, fld, True)
    vec = gen_components(fld, True)
    vec[2].slope = Tied(vec[1]._priors['slope'], ratio=(-0.5, 0.25), offset=(0.0, 1e-5))
    vec = MultiComponentModel(vec)
    db = save_database(_Chain(4, 3, vec.num_params, 1), vec, str(tmp_path / 'vec_db.fits'))
    assert db.meta['MCTIES'] == len(GEN_TIES) and database_ties(db) == vec.tie_records
    assert database_ties(db)[0] == ('1Sky_SLP', '0Sky_SLP', (-0.5, 0.25), (0.0, 1e-5))
    assert database_ties(save_database(_Chain(4, 3, gen.num_params, 1), gen, str(tmp_path / 'gen_db.fits'))) == \
        gen.tie_records
    plain = save_database(_Chain(4, 3, twin.num_params, 1), twin, str(tmp_path / 'twin_db.fits'))
    assert not [k for k in plain.meta if k.startswith('MCTI')] and database_ties(plain) == []


# -- 6. the single-vector path ----------------------------------------------------------------------------------------
def test_param_values_resolve_the_tied_attributes():
    fld = make_field(64, 64, seed=2)
    tied, twin = build(qso_components, fld, True), build(qso_components, fld, False)
    theta = qso_theta(tied, fld, 2, seed=6)
    full = expand(tied, twin, QSO_TIES, theta)
    for t, f in zip(theta, full):
        tied.param_values = t
        twin.param_values = f
        for a, b in zip(tied.components, twin.components):
            for attr in b._declared:
                if attr in b._priors or attr in b._constants:
                    assert np.array_equal(np.ravel(getattr(a, attr)), np.ravel(getattr(b, attr))), attr
        assert tied.log_priors() == scipy_prior_sum(tied, t[None])[0] or np.isclose(
            tied.log_priors(), scipy_prior_sum(tied, t[None])[0], rtol=1e-14, atol=0)
    bad = theta[0].copy()
    bad[columns_of(tied, '2_Sersic_reff_b_ratio')[0]] = 1.1
    tied.param_values = bad
    assert tied.log_priors() == -np.inf
