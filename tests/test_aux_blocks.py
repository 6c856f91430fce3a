"""The four blocks behind a field's auxiliary entries -- Fourier modes, spiral arms, radial laws, truncations -- from
a model to the layout calls, the auxiliary rows and the table the library composes.  No GPU needed.

Two models, a recording stub in place of the engine:
  (a) a `Sersic` with modes 1 and 3 and an outer truncation, and a `Moffat` with a spiral and a free beta: every block
      is registered;
  (b) a single `Sersic` with a spiral only: the Fourier block is padding in front of the spiral's.
EXPECTED holds the tags, columns and constants of every block call in order, and the auxiliary rows of three fixed
parameter vectors.  The literals were PRODUCED BY RUNNING THE PARENT COMMIT of the one that introduced this file (the
hand-written stanzas per block in `models.py`), through `observed` below: they pin what a model sends, entry for
entry, against any rewrite of how the blocks are walked."""
import numpy as np
import pytest

import test_general_components as tg
import test_radial_laws as tr
import test_truncation as tt
from psfmc_amd import MultiComponentModel, engine

BLOCKS = ('fourier', 'spiral', 'radial', 'truncation')
SERSIC_A = (', fourier={1: (Uniform(loc=-0.5, scale=1), Uniform(loc=-180, scale=360)), 3: (0.1, Normal(loc=0, scale=30))}'
            ", truncation={'outer': (14.0, Uniform(loc=15.0, scale=20.0))}")
MOFFAT_A = ('Moffat(xy=Uniform(loc=c - ms, scale=2 * ms), mag=Uniform(loc=19.0, scale=5.0), '
            'fwhm=Uniform(loc=1.0, scale=6.0), fwhm_b=2.0, beta=Uniform(loc=1.1, scale=8), angle=30.0, '
            "angle_degrees=True, spiral={'r_in': 2.0, 'r_out': Uniform(loc=5, scale=20), "
            "'winding': Normal(loc=0, scale=200), 'inclination': Uniform(loc=0, scale=70)})\n")
SERSIC_B = ", spiral={'r_in': 1.5, 'r_out': Uniform(loc=5, scale=20), 'winding': 120.0, 'alpha': Uniform(loc=0, scale=2)}"


def model_of(directory, which):
    directory.mkdir()
    if which == 'a':
        path, _ = tr.write_field(directory, MOFFAT_A, sky_text=tg.SKY_PLAIN, sersic_text=SERSIC_A)
    else:
        path, _ = tg.write_field(directory, sky_text=tg.SKY_PLAIN, sersic_text=SERSIC_B)
    return MultiComponentModel(path)


def thetas(model):
    """Three fixed parameter vectors, every value a short binary fraction."""
    return 1.0 + 0.25 * np.arange(model.num_params)[None, :] + 0.125 * np.arange(3)[:, None]


def observed(model):
    rec = tt.RecordingLayout()
    model._register_layout(rec)
    return {'n_params': model.num_params,
            'order': [c[0] for c in rec.calls],
            'aux': [list(map(int, rec.calls[1][1][0])), list(map(float, rec.calls[1][1][1]))],
            'blocks': [(name, [int(t) for t in args[0]], [int(c) for c in args[1]], [float(k) for k in args[2]])
                       for name, args in rec.calls if name in BLOCKS],
            'aux_rows': model.aux_rows(thetas(model)).tolist()}


EXPECTED = {'a': {'aux': [[-1, -1, -1, -1], [0.0, 0.0, 0.0, 0.0]],
       'aux_rows': [[0.0, 0.0, 0.0, 0.0, 2.25, 2.5, 0.0, 0.0, 0.1, 2.75, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                     0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 5.75, 6.0, 0.0,
                     5.5, 0.0, 0.0, 0.0, 4.75, 0.0, 0.0, 1.0, 14.0, 4.0, 0.0, 1.0, 0.0, 1.0],
                    [0.0, 0.0, 0.0, 0.0, 2.375, 2.625, 0.0, 0.0, 0.1, 2.875, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                     0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 5.875,
                     6.125, 0.0, 5.625, 0.0, 0.0, 0.0, 4.875, 0.0, 0.0, 1.0, 14.0, 4.125, 0.0, 1.0, 0.0, 1.0],
                    [0.0, 0.0, 0.0, 0.0, 2.5, 2.75, 0.0, 0.0, 0.1, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                     0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 6.0, 6.25, 0.0,
                     5.75, 0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 1.0, 14.0, 4.25, 0.0, 1.0, 0.0, 1.0]],
       'blocks': [('fourier', [5, 0],
                   [5, 6, -1, -1, -1, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1],
                   [0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                    0.0, 0.0, 0.0, 0.0, 0.0]),
                  ('spiral', [0, 1], [-1, -1, -1, -1, -1, -1, -1, 19, 20, -1, 18, -1],
                   [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
                  ('radial', [0, 1], [-1, -1, 15, -1], [0.0, 0.0, 0.0, 0.0]),
                  ('truncation', [2, 0], [-1, -1, -1, 12, -1, -1, -1, -1],
                   [0.0, 1.0, 14.0, 0.0, 0.0, 1.0, 0.0, 1.0])],
       'n_params': 23,
       'order': ['layout', 'aux', 'fourier', 'spiral', 'radial', 'truncation']},
 'b': {'aux': [[-1, -1, -1], [0.0, 0.0, 0.0]],
       'aux_rows': [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5, 3.5, 120.0, 3.25,
                     0.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5, 3.625, 120.0,
                     3.375, 0.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5, 3.75, 120.0, 3.5,
                     0.0, 0.0]],
       'blocks': [('spiral', [1], [-1, 10, -1, 9, -1, -1], [1.5, 0.0, 120.0, 0.0, 0.0, 0.0])],
       'n_params': 13,
       'order': ['layout', 'aux', 'spiral']}}


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    root = tmp_path_factory.mktemp('aux_blocks')
    return {which: model_of(root / which, which) for which in 'ab'}


@pytest.mark.parametrize('which', ['a', 'b'])
def test_the_calls_and_the_rows_are_the_parents(models, which):
    got, want = observed(models[which]), EXPECTED[which]
    assert got['n_params'] == want['n_params'] and got['order'] == want['order']
    assert got['aux'] == want['aux']
    assert got['blocks'] == want['blocks']                     # tags, col and const of every block call, in order
    rows = np.array(got['aux_rows'])
    assert rows.shape == np.array(want['aux_rows']).shape and rows.dtype == np.float64
    assert got['aux_rows'] == want['aux_rows']                 # exact: the entries are theta's values or constants


def test_what_the_models_pin():
    """(a) registers every block behind the aux layout; (b) only the spiral's, its rows carry the twelve zeros of the
    Fourier block in front of the six spiral entries."""
    assert EXPECTED['a']['order'] == ['layout', 'aux', 'fourier', 'spiral', 'radial', 'truncation']
    assert EXPECTED['b']['order'] == ['layout', 'aux', 'spiral']
    rows = np.array(EXPECTED['b']['aux_rows'])
    assert rows.shape == (3, 2 + 1 + 12 + 6) and not rows[:, :15].any() and rows[:, 15:19].all()
    assert np.array(EXPECTED['a']['aux_rows']).shape == (3, 2 + 25 * 2)


@pytest.mark.parametrize('which', ['a', 'b'])
def test_the_library_composes_the_concatenation(models, which):
    """`engine.debug_aux_table` on what the model sent: the base entries, then every block up to the last one sent --
    the block as sent, or its padding (column -1, constant 0, r_out = 1 in an absent spiral block)."""
    want = EXPECTED[which]
    sent = {name: (tags, col, const) for name, tags, col, const in want['blocks']}
    n_ser = len(want['blocks'][0][1])
    const, col, kinds, sides, counts = engine.debug_aux_table(1, n_ser, base=want['aux'], **dict(
        sent, truncation=sent.get('truncation', ([0] * n_ser, [-1] * 4 * n_ser, [0.0] * 4 * n_ser))))
    per = {'fourier': 12, 'spiral': 6, 'radial': 2, 'truncation': 4}
    pad = {'fourier': [0.0] * 12, 'spiral': [0.0, 1.0, 0.0, 0.0, 0.0, 0.0], 'radial': [0.0] * 2}
    last = max(BLOCKS.index(name) for name in sent)
    exp_col, exp_const = list(want['aux'][0]), list(want['aux'][1])
    for name in BLOCKS[:last + 1]:
        exp_col += sent[name][1] if name in sent else [-1] * per[name] * n_ser
        exp_const += sent[name][2] if name in sent else pad[name] * n_ser
    assert list(col) == exp_col and list(const) == exp_const
    assert counts == (len(exp_col),) + tuple(per[n] * n_ser if i <= last else 0 for i, n in enumerate(BLOCKS))
    assert list(kinds) == (sent['radial'][0] if 'radial' in sent else [0] * n_ser if last >= 2 else [])
    assert list(sides) == (sent['truncation'][0] if 'truncation' in sent else [])
    # ... and without the truncation argument the same table in the four-count form
    if 'truncation' not in sent:
        const4, col4, kinds4, counts4 = engine.debug_aux_table(1, n_ser, base=want['aux'], **sent)
        assert (list(const4), list(col4), list(kinds4), counts4) == (list(const), list(col), list(kinds), counts[:4])
    if which == 'b':                                           # the padded Fourier block of a spiral alone
        assert counts == (21, 12, 6, 0, 0) and col[3:15].tolist() == [-1] * 12 and not const[3:15].any()
    else:
        # the same field without its spiral: the absent spiral block is padded with r_out = 1
        fewer = {k: v for k, v in sent.items() if k != 'spiral'}
        const, col, kinds, sides, counts = engine.debug_aux_table(1, n_ser, base=want['aux'], **fewer)
        at = len(want['aux'][0]) + 12 * n_ser
        assert counts == (2 + 25 * n_ser, 12 * n_ser, 6 * n_ser, 2 * n_ser, 4 * n_ser)
        assert col[at:at + 6 * n_ser].tolist() == [-1] * 6 * n_ser
        assert const[at:at + 6 * n_ser].tolist() == pad['spiral'] * n_ser
        assert const[:at].tolist() == exp_const[:at] and const[at + 6 * n_ser:].tolist() == exp_const[at + 6 * n_ser:]
