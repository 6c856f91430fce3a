"""psfmc_fisher_rows on every instantiation of its Gram kernel and on its slab tail, held to the long-double
definition of the device's own images at rounding level (`mode_helpers.fisher_reference_longdouble`,
`mode_helpers.fisher_rounding_bound`; their teeth: tests/test_fisher_reference.py), and the two behaviours
psfmc_fisher.h documents without a test: aux rows across a pass boundary, and a stencil image that is not finite.

Which test runs which k_fisher_gram<T, Src> (T tile rows of the K + 1 extended vectors):
    T   K        <T, FisherVectors>: test_gpu_fisher.py              <T, FisherStencil>: this file
                 test_gram_kernel_is_exact_on_small_integers         test_entry_on_every_tile_count
    1   1..15    K = 1, 3, 15                                        K = 15
    2   16..31   K = 16, 17, 31                                      K = 16, 31
    3   32..47   K = 32, 33, 47                                      K = 32, 47 (and two stencils at K = 32)
    4   48..63   K = 48, 63                                          K = 48, 63
(test_gpu_fisher.py's entry cases, K = 10, 11, 14, 18, run <1, FisherStencil> and <2, FisherStencil> as well.)
K = 63 is ten tiles and the finish kernel's triangle walk at T = 4; K = 64 is refused.

The model is sky + point source + nine Sersic components, 67 free columns, of which the first K are differentiated:
the sky's is always among them, and its derivative is the only one that does not vanish at the last pixels of the
image.  The 62 x 66 field has 4092 = 63 * 64 + 60 pixels, so the last wave's slab is padded (`on ? p : 0` of the
FisherStencil path); 64 x 64 is whole slabs, for contrast.  The library takes even image sides only, so a field's
pixel count is a multiple of 4 and a tail that is not can only reach the kernel through the hook (n_pix = 3, 65,
257, 4099 there).  No oracle here: the image passes do not depend on the stencil's form and are held to the oracle
in tests/test_gpu_fisher.py; what is checked is the entry against the definition on the same images."""
import numpy as np
import pytest

import mode_helpers as mh
import test_gpu_fisher as tgf
from psfmc_amd import mode

pytestmark = pytest.mark.gpu

SHAPES = [(62, 66), (64, 64)]
TILE_K = [15, 16, 31, 32, 47, 48, 63]
N_SERSIC = 9
MAX_WALKERS = 128                # the context takes half as many again: two stencils of K = 32 (130 walkers) fit


def _components(ny, nx):
    comps = [dict(type='sky', adu=0.004), tgf._ps(nx, ny)]
    for k in range(N_SERSIC):                    # a 3 x 3 grid of centres, every shape parameter different
        gx, gy = k % 3, k // 3
        comps.append(dict(type='sersic', xy=(nx * (0.25 + 0.25 * gx) + 0.3, ny * (0.25 + 0.25 * gy) - 0.2),
                          mag=18.0 + 0.25 * k, reff=3.0 + 0.3 * k, reff_b=2.0 + 0.2 * k, index=0.8 + 0.4 * k,
                          angle=15.0 + 19.0 * k, angle_degrees=True))
    return comps


_MODELS = {}


@pytest.fixture(scope='module')
def models():
    """(shape, back end) -> (case, model), built on first use and closed with the module."""
    def get(shape, backend):
        if (shape, backend) not in _MODELS:
            case = _MODELS.get(shape) or tgf._edge_case(shape, _components(*shape), max_walkers=MAX_WALKERS)
            _MODELS[shape] = case
            _MODELS[(shape, backend)] = (case, case['build'](backend))
        return _MODELS[(shape, backend)]
    yield get
    for key in [k for k in _MODELS if isinstance(k[1], str)]:
        _MODELS.pop(key)[1].close()


def cases_meet_their_conditions():
    """On the host alone (tests/test_fisher_reference.py runs it without a GPU too)."""
    assert (62 * 66) % 64 == 60 and (64 * 64) % 64 == 0
    for shape in SHAPES:
        case = tgf._edge_case(shape, _components(*shape), max_walkers=MAX_WALKERS)
        assert case['layout'][0] == ('sky',) and case['n_columns'] == 67 and not case['has_psf_index']
        assert not case['field'].bad_px[-1, -1]              # the last pixel counts
    assert min(TILE_K) >= 1                                  # column 0, the sky, is in every slice


def test_cases_meet_their_conditions():
    cases_meet_their_conditions()


@pytest.mark.parametrize('backend', tgf.BACKENDS)
@pytest.mark.parametrize('k', TILE_K)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_entry_on_every_tile_count(models, shape, k, backend):
    case, model = models(shape, backend)
    columns = np.arange(k)
    out = model.fisher(case['theta'], columns=columns)
    assert out['F'].shape == (k, k) and np.array_equal(out['F'], out['F'].T)
    assert np.all(np.isfinite(out['F'])) and np.all(np.isfinite(out['grad']))
    vecs = mode.stencil(case['theta'], out['step'], columns)[0]
    assert len(vecs) == 2 * k + 1 <= 127
    tgf.held_to_own_images(model, vecs, out, 0.5 / out['step'], '%dx%d %s' % (shape + (backend,)))
    assert out['loglike'] == model.log_likelihood_batch(case['theta'])[0]


@pytest.mark.parametrize('backend', tgf.BACKENDS)
def test_two_stencils_of_three_tile_rows_do_not_mix(models, backend):
    """K = 32, two stencils in one call: partial[base][u][tile] with base > 0 and tile > 0, on the padded field."""
    case, model = models(SHAPES[0], backend)
    columns = np.arange(32)
    assert model.engine.max_walkers >= 2 * 65                # both stencils go in ONE psfmc_fisher_rows call
    other = case['theta'].copy()
    other[:32] += 3.0 * mode.default_steps(model, case['theta'], columns)[0]
    thetas = np.vstack([case['theta'], other])
    both = model.fisher(thetas, columns=columns)
    for i in range(2):
        alone = model.fisher(thetas[i], columns=columns)
        for key in ('F', 'grad', 'loglike'):
            assert np.array_equal(both[key][i], alone[key]), (i, key)
    assert not np.array_equal(both['F'][0], both['F'][1])


def test_sixty_four_columns_are_refused(models):
    _, model = models(SHAPES[1], 'fused')
    eng = model.engine
    with pytest.raises(ValueError, match='63'):
        eng.fisher_rows(np.zeros((1, 129, eng.row_len)), np.ones((1, 64)))
    with pytest.raises(ValueError):
        model.fisher(np.zeros(model.num_params), columns=np.arange(64))


# ---------------------------------------------------------------------------
# aux rows across a pass boundary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('backend', tgf.BACKENDS)
def test_a_stencil_with_aux_rows_does_not_depend_on_the_batch(backend):
    """Three stencils of the general-component model (K = 14: 29 walkers each, 87 in all, every one with aux rows) in
    passes of 40 walkers: the first boundary falls inside the middle stencil (29 < 40 < 58), the second inside the
    third."""
    case = tgf.CASES['boxy-moffat-truncated']()
    model = case['build'](backend)
    theta = case['theta']
    assert len(mode.default_columns(model)) == 14 and model.aux_rows(theta).shape[1] > 0
    model.engine.set_option('chunk_walkers', 40)
    step = mode.default_steps(model, theta, mode.default_columns(model))[0]
    thetas = np.vstack([theta, theta + 5.0 * step, theta - 7.0 * step])
    tgf._three_stencils(model, thetas)
    model.close()


# ---------------------------------------------------------------------------
# a stencil image that is not finite
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('backend', tgf.BACKENDS)
def test_a_non_finite_stencil_image_stays_in_its_stencil(backend):
    """Three stencils through `Context.fisher_rows`; in the second, the point source's flux of one +- row is NaN.  A
    point source's flux only scales pixel values: build_prep folds it into the x weights of the source's window,
    whose place and size come from the position alone, and takes it into the peak estimate through fmax and a range
    test, both of which a NaN falls out of; no address, table index or loop count depends on it (psfmc_device.h
    prep_ps_axis, prep_head, ps_pixel, raster_row).  That stencil's F and grad come back non-finite (`model.fisher`
    would blank them to NaN), its log-likelihood -- the base row's -- and the other two stencils are what they are
    without the NaN, bit for bit, and nothing is raised."""
    fld, _ = mh.synth_field_64()
    model = tgf._synth_model(fld, backend)
    columns = mode.default_columns(model)
    k = len(columns)
    step = mode.default_steps(model, fld['truth'], columns)[0]
    thetas = np.vstack([fld['truth'], fld['truth'] + 4.0 * np.r_[step], fld['truth'] - 6.0 * np.r_[step]])
    steps = np.tile(step, (3, 1))
    vecs = mode.stencil(thetas, steps, columns)
    rows = model.derived_rows(vecs.reshape(-1, model.num_params)).reshape(3, 2 * k + 1, -1)
    eng = model.engine
    assert rows.shape[2] == eng.row_len and 3 * (2 * k + 1) <= eng.max_walkers
    clean = eng.fisher_rows(rows, 0.5 / steps)
    assert all(np.all(np.isfinite(v)) for v in clean)
    flux = 1                                     # a row is the sky, then per point source flux, x, y, method
    assert np.all(rows[:, :, flux] > 0)          # ... and column 0 of the vector is the point source's magnitude
    assert rows[1, 1, flux] != rows[1, 0, flux] and np.array_equal(rows[1, 3:, flux], np.full(2 * k - 2, rows[1, 0, flux]))
    spoilt = rows.copy()
    spoilt[1, 6, flux] = np.nan                  # the - row of column 2
    got = eng.fisher_rows(spoilt, 0.5 / steps)
    for i in (0, 2):
        alone = eng.fisher_rows(rows[i:i + 1], 0.5 / steps[i:i + 1])
        for j in range(3):
            assert np.array_equal(got[j][i], alone[j][0]), (i, j)
            assert np.array_equal(got[j][i], clean[j][i]), (i, j)
    assert np.isnan(got[0][1][2, 2]) and np.isnan(got[1][1][2])
    assert not np.all(np.isfinite(got[0][1])) and not np.all(np.isfinite(got[1][1]))
    assert got[2][1] == clean[2][1]
    model.close()
