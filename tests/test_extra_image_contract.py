"""tests/extra_contract.py pinned on the CPU before it judges kernels: without the keywords it IS the oracle; every
case tests/test_gpu_extra_image_fields.py and tests/test_gpu_law_fields.py use tells the PSFs and the flag rows apart by orders more than the GPU
tests' bound; every field has the features it claims."""
import numpy as np
import pytest

import extra_contract as xc
import psfmc_oracle as orc


@pytest.mark.parametrize('shape,n_psf', [((70, 96), 2), ((96, 150), 3), ((64, 320), 2)], ids=xc.case_id)
def test_contract_without_keywords_is_the_oracle(shape, n_psf):
    """A model without `integrate`, `boxiness`, `fourier` or `slope` on a masked field with several PSFs: the helper's
    log-likelihood (relative to itself) and five images (finite masks equal, then relative to the image's largest
    value) equal `orc.evaluate`'s for every PSF index to 1e-13; an index outside the support is -inf."""
    case = xc.field_case(shape, 40 + shape[1], n_psf)
    field = xc.oracle_field(case)
    xc.field_features(case, field)
    assert len(field.psf_spec) == n_psf
    model = xc.make_model(case, [{}, {}])
    assert model.param_names[-1] == 'PSF_Index' and not model.has_aux and not any(model.sersic_integrate)
    worst = 0.0
    for k in range(n_psf):
        for i, psf in enumerate((float(k), k + 0.3)):
            sky, ps, sersics = xc.scene(shape, i)
            theta = xc.theta_of(model, sky, ps, sersics[:2], psf=psf)
            comps = [dict(type='sky', adu=sky['adu']), dict(type='ps', xy=ps['xy'], mag=ps['mag'], method='lanczos3')]
            comps += [dict(type='sersic', angle_degrees=True, **{n: s[n] for n in ('xy', 'mag', 'reff', 'reff_b', 'index',
                                                                                   'angle')}) for s in sersics[:2]]
            want_ll, want = orc.evaluate(field, comps, psf, raw_dtype=np.float64, want_ps_sub=True)
            got_ll, got = xc.contract_evaluate(model, field, theta)
            assert np.isfinite(want_ll) and xc.rel(got_ll, want_ll) <= 1e-13, (k, got_ll, want_ll)
            worst = max(worst, xc.rel(got_ll, want_ll))
            assert set(got) == set(want)
            for kind in want:
                fin = np.isfinite(want[kind])
                assert np.array_equal(np.isfinite(got[kind]), fin), (k, kind)
                err = np.abs(got[kind][fin] - want[kind][fin]).max() / np.abs(want[kind][fin]).max()
                worst = max(worst, err)
                assert err <= 1e-13, (k, kind, err)
    print('%dx%d: worst relative difference from the oracle %.2e' % (shape + (worst,)))
    for psf in (-0.6, n_psf - 0.4, float(n_psf)):
        theta = xc.theta_of(model, *xc.scene(shape)[:2], xc.scene(shape)[2][:2], psf=psf)
        assert xc.contract_evaluate(model, field, theta) == (-np.inf, None)
    assert np.isfinite(xc.contract_evaluate(model, field, xc.theta_of(model, sky, ps, sersics[:2], psf=n_psf - 0.6))[0])


def test_model_builder_packs_by_name():
    """Sky + slope, PointSource, one Sersic with boxiness and modes 1 and 4, one integrated Sersic on a two-PSF field:
    3 + 3 + (7 + 1 + 4) + 7 + 1 = 26 free parameters, `PSF_Index` last; values go in by name."""
    case = xc.field_case((70, 96), 3, 2)
    model = xc.make_model(case, [dict(boxiness=xc.FREE, fourier=xc.MODES_1_4), dict(integrate=True)], slope=xc.FREE)
    assert model.num_params == 26 and model.param_names[-1] == 'PSF_Index'
    assert model.sersic_integrate == [False, True] and model.sersic_general_flags == [True, False]
    assert model.sersic_fourier_masks == [0b1001, 0]
    sky, ps, sersics = xc.scene((70, 96))
    theta = xc.theta_of(model, sky, ps, sersics[:2], psf=1.0)
    model.param_values = theta
    values = dict(zip(model.param_names, np.split(theta, np.cumsum(model.param_lens)[:-1])))
    assert values['2_Sersic_f4_phase'][0] == sersics[0]['f4_phase'] and values['0_Sky_slope'][1] == sky['slope'][1]
    assert tuple(values['3_Sersic_xy']) == sersics[1]['xy'] and values['PSF_Index'][0] == 1.0
    assert np.isfinite(model.log_priors_batch(theta)[0])


@pytest.mark.parametrize('backend,kind,shape', xc.CASES, ids=xc.case_id)
def test_cases_discriminate_and_have_their_features(backend, kind, shape):
    """Every parametrised case of the GPU file: the field has the features it claims; the contract log-likelihoods of
    PSF 0 and PSF 1 differ by more than 1e-6 relative, and so do the model's and the one with the keywords moved to
    the next Sersic -- three orders above the GPU tests' 1e-9, so a walker evaluated with the wrong PSF or the wrong
    flag row cannot pass; the six walkers are distinct, finite inside the support and -inf outside; the raw model's
    peak stays below 2e3 counts."""
    case, field = xc.several_psf_case(kind, shape)
    xc.field_features(case, field, xc.integrated_centre(kind, shape))
    n_psf = xc.N_PSF[shape]
    assert len(field.psf_spec) == n_psf >= 2
    model = xc.make_model(case, **xc.KINDS[kind])
    other = xc.make_model(case, **xc.moved(kind))
    assert model.num_params == other.num_params and model.param_names[-1] == 'PSF_Index'
    assert (model.sersic_integrate, model.sersic_general_flags) != (other.sersic_integrate, other.sersic_general_flags)
    n_s = len(xc.KINDS[kind]['sersics'])
    for i in (0, 3):
        sky, ps, sersics = xc.scene(shape, i)
        ll = [xc.contract_evaluate(model, field, xc.theta_of(model, sky, ps, sersics[:n_s], psf=float(k)))
              for k in range(n_psf)]
        assert all(np.isfinite(v[0]) for v in ll)
        assert max(np.abs(v[1]['raw_model']).max() for v in ll) < 2e3
        assert xc.rel(ll[1][0], ll[0][0]) > 1e-6, (ll[0][0], ll[1][0])
        # the keywords' VALUES move with the keywords: the ordinary parameters stay where they are
        extras = [{n: v for n, v in s.items() if n == 'boxiness' or n[0] == 'f'} for s in sersics[:n_s]]
        plain = [{n: v for n, v in s.items() if n not in e} for s, e in zip(sersics, extras)]
        shifted = [dict(plain[k], **extras[k - 1]) for k in range(n_s)]
        ll_moved = xc.contract_evaluate(other, field, xc.theta_of(other, sky, ps, shifted, psf=0.0))[0]
        assert np.isfinite(ll_moved) and xc.rel(ll_moved, ll[0][0]) > 1e-6, (ll[0][0], ll_moved)
        print('%s %dx%d walker %d: PSF 0 %.6g, PSF 1 %.6g, keywords moved %.6g' % ((kind,) + shape + (i, ll[0][0], ll[1][0],
                                                                                                ll_moved)))
    thetas = xc.several_psf_thetas(model, shape)
    want = np.array([xc.contract_evaluate(model, field, t)[0] for t in thetas])
    inside = np.array([0 <= np.rint(p) < n_psf for p in xc.psf_indices(n_psf)])
    assert len(thetas) == 6 and 1 <= (~inside).sum() <= 2
    assert np.all(np.isfinite(want[inside])) and np.all(want[~inside] == -np.inf)
    assert len(np.unique(want[inside])) == inside.sum()
    prior = model.log_priors_batch(thetas)
    assert np.all(np.isfinite(prior[inside])) and np.all(prior[~inside] == -np.inf)
    assert {int(np.rint(p)) for p, ok in zip(xc.psf_indices(n_psf), inside) if ok} == set(range(n_psf))


KEYWORD_VALUES = ('boxiness', 'spiral_', 'moffat_', 'ferrer_')


def keyword_values(sersic):
    """The entries of a `scene` Sersic that belong to its keywords (they move with them): the boxiness, the modes,
    the spiral's values and the laws' own parameters.  The position, magnitude, angle and radii stay."""
    return {n: v for n, v in sersic.items() if n.startswith(KEYWORD_VALUES) or (n[0] == 'f' and n[1].isdigit())}


@pytest.mark.parametrize('backend,kind,shape', xc.LAW_CASES, ids=xc.case_id)
def test_law_cases_discriminate_and_have_their_features(backend, kind, shape):
    """`test_cases_discriminate_and_have_their_features` for every parametrised case of tests/test_gpu_law_fields.py:
    the field's features (X: a bad pixel in the integrated box); PSF 0 against PSF 1 and the model against the one
    with its keywords -- spiral and law included: the models' spiral flags / radial kinds differ -- moved to the next
    Sersic by more than 1e-6 of the log-likelihood; six distinct walkers, finite inside the support and -inf outside;
    the peak below 2e3.  With a Ferrer: every walker's |1 - x| is at least EDGE_MARGIN on every pixel, the rho = 1
    contour of at least one walker lies inside the image (no pixel of the outermost rows and columns is inside the
    cut-off), and of the field's bad pixels at least one lies inside every walker's support and one outside."""
    case, field = xc.law_case(kind, shape)
    xc.field_features(case, field, xc.integrated_centre(kind, shape))
    n_psf = xc.N_PSF[shape]
    assert len(field.psf_spec) == n_psf >= 2
    model = xc.make_model(case, **xc.KINDS[kind])
    other = xc.make_model(case, **xc.moved(kind))
    assert model.num_params == other.num_params and model.param_names[-1] == 'PSF_Index'
    assert (model.sersic_spiral_flags, model.sersic_radial_kinds) != (other.sersic_spiral_flags, other.sersic_radial_kinds)
    assert any(model.sersic_spiral_flags) or any(model.sersic_radial_kinds)
    assert any(model.sersic_integrate) == (kind == 'X') and xc.has_ferrer(model) == (kind in 'RX')
    n_s = len(xc.KINDS[kind]['sersics'])
    for i in (0, 3):
        sky, ps, sersics = xc.scene(shape, i)
        ll = [xc.contract_evaluate(model, field, xc.theta_of(model, sky, ps, sersics[:n_s], psf=float(k)))
              for k in range(n_psf)]
        assert all(np.isfinite(v[0]) for v in ll)
        peak = max(np.abs(v[1]['raw_model']).max() for v in ll)
        assert peak < 2e3
        assert xc.rel(ll[1][0], ll[0][0]) > 1e-6, (ll[0][0], ll[1][0])
        extras = [keyword_values(s) for s in sersics[:n_s]]
        plain = [{n: v for n, v in s.items() if n not in e} for s, e in zip(sersics, extras)]
        shifted = [dict(plain[k], **extras[k - 1]) for k in range(n_s)]
        ll_moved = xc.contract_evaluate(other, field, xc.theta_of(other, sky, ps, shifted, psf=0.0))[0]
        assert np.isfinite(ll_moved) and xc.rel(ll_moved, ll[0][0]) > 1e-6, (ll[0][0], ll_moved)
        print('%s %dx%d walker %d: peak %.1f, PSF 0 %.6g, PSF 1 %.6g (%.1e), keywords moved %.6g (%.1e)'
              % ((kind,) + shape + (i, peak, ll[0][0], ll[1][0], xc.rel(ll[1][0], ll[0][0]), ll_moved,
                                    xc.rel(ll_moved, ll[0][0]))))
    thetas = xc.several_psf_thetas(model, shape)
    state = [xc.contract_with_state(model, field, np.append(t[:-1], 0.0)) for t in thetas]
    want = np.array([xc.contract_evaluate(model, field, t)[0] for t in thetas])
    inside = np.array([0 <= np.rint(p) < n_psf for p in xc.psf_indices(n_psf)])
    assert len(thetas) == 6 and 1 <= (~inside).sum() <= 2
    assert np.all(np.isfinite(want[inside])) and np.all(want[~inside] == -np.inf)
    assert len(np.unique(want[inside])) == inside.sum()
    prior = model.log_priors_batch(thetas)
    assert np.all(np.isfinite(prior[inside])) and np.all(prior[~inside] == -np.inf)
    assert {int(np.rint(p)) for p, ok in zip(xc.psf_indices(n_psf), inside) if ok} == set(range(n_psf))
    if not xc.has_ferrer(model):
        return
    contained = 0
    for w, t in enumerate(thetas):
        assert state[w][3] >= xc.EDGE_MARGIN, (kind, shape, w, state[w][3])
        model.param_values = t
        for comp in model.components:
            if getattr(comp, 'radial_law', None) != 'ferrer':
                continue
            support = xc.ferrer_x(model, comp)[0] < 1.0
            rim = np.ones(shape, dtype=bool)
            rim[1:-1, 1:-1] = False
            contained += int(not (support & rim).any())
            assert (field.bad_px & support).any() and (field.bad_px & ~support).any(), (kind, shape, w)
            assert 20 < support.sum() < support.size // 2, (kind, shape, w, support.sum())
    print('%s %dx%d: the rho = 1 contour of %d of 6 walkers lies inside the image, smallest |1 - x| %.2e'
          % ((kind,) + shape + (contained, min(s[3] for s in state))))
    assert contained >= 1


def test_a_field_without_keywords_gets_zero_aux_rows_in_a_shared_context(monkeypatch):
    """The host side of what test_field_set_with_two_psfs_per_field found on the GPU: a field whose model has no
    auxiliary vectors, in a shared context where another field registered some, sends zero rows of the context's
    width with its row-based calls (the library refuses such a call without rows); its own rows, and a context
    without any auxiliary layout, are left alone."""
    from psfmc_amd import engine

    class Shared(object):
        """The width is the library's (`get_option('aux_stride')`): the stand-in answers for it."""
        _field_aux = engine.FieldSetContext._field_aux
        _aux_width = engine.FieldSetContext._aux_width
        stride = 0.0

        def get_option(self, key):
            assert key == 'aux_stride'
            return self.stride
    ctx = Shared()
    assert ctx._aux_width() == 0 and ctx._field_aux(None, 3) is None
    ctx.stride = 4.0
    rows = ctx._field_aux(None, 3)
    assert rows.shape == (3, 4) and not rows.any()
    ctx.stride = 28.0
    assert ctx._field_aux(None, 2).shape == (2, 28)
    own = np.ones((2, 4))
    assert ctx._field_aux(own, 2) is own
    # a context where fields registered spirals and laws as well: what reaches the library after `_send_aux_rows`'
    # padding has the context's full width, for a plain field's zero rows and for a modes-only field's own rows
    assert ctx._aux_width() == 28
    ctx.stride = 4.0 + 24 + 12 + 4
    assert ctx._aux_width() == 44 and isinstance(ctx._aux_width(), int)
    sent = []

    class Library(object):
        @staticmethod
        def psfmc_set_aux_rows(handle, n_w, rows):
            sent.append((n_w, rows))
            return 0
    monkeypatch.setattr(engine, '_dp', lambda a: a)
    for rows in (None, np.ones((3, 28))):
        engine._send_aux_rows(Library, None, lambda rc: None, ctx._field_aux(rows, 3), 3, ctx._aux_width())
        n_w, got = sent.pop()
        assert n_w == 3 and got.shape == (3, 44) and got.flags.c_contiguous and got.dtype == np.float64
        assert not got[:, 28:].any() and np.all(got[:, :28] == (0.0 if rows is None else 1.0))
    assert not sent
