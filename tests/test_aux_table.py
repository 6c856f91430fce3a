"""The auxiliary table the library composes for a field from what the field registered (csrc/psfmc_aux_table.h),
through psfmc_debug_aux_table: host code only, no context and no device.  n_sky = 1, n_sersic = 2: 4 base entries,
then 24 Fourier, 12 spiral and 4 radial ones -- the spiral entries of Sersic k at 2 n_sky + 13 n_sersic + 6 k, the
laws' at 2 n_sky + 19 n_sersic + 2 k (include/psfmc_hip.h).  Every entry is compared, not only the counts."""
import numpy as np

from psfmc_amd import engine

N_SKY, N_SER = 1, 2
BASE = ([3, -1, 5, -1], [0.0, 0.5, 0.0, 0.25])
FOURIER = ([0, 0b101], list(range(10, 34)), [0.01 * j for j in range(24)])            # modes on Sersic 1
SPIRAL = ([True, False], [-1, 7, 8, -1, 9, -1] + [-1] * 6, [2.0, 0.0, 0.0, 1.5, 0.0, 20.0] + [0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
RADIAL = ([0, 2], [-1, -1, 6, -1], [0.0, 0.0, 0.0, 0.5])                              # a Ferrer in slot 1
PAD_FOURIER = ([-1] * 24, [0.0] * 24)
PAD_SPIRAL = ([-1] * 12, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] * 2)                          # r_out = 1 at 28 + 1 and 28 + 7


def table(**blocks):
    const, col, kinds, counts = engine.debug_aux_table(N_SKY, N_SER, base=BASE, **blocks)
    assert const.dtype == np.float64 and len(const) == len(col) == counts[0]
    return list(col), list(const), list(kinds), counts


def joined(*parts):
    return sum((list(p[0]) for p in parts), []), sum((list(p[1]) for p in parts), [])


def test_base_only():
    assert table() == (BASE[0], BASE[1], [], (4, 0, 0, 0))
    assert engine.debug_aux_table(N_SKY, N_SER)[3] == (0, 0, 0, 0)                    # no aux layout, no table


def test_modes_on_one_component():
    col, const, kinds, counts = table(fourier=FOURIER)
    assert counts == (28, 24, 0, 0) and kinds == []
    assert (col, const) == joined(BASE, FOURIER[1:])
    assert col[4:] == FOURIER[1] and const[4:] == FOURIER[2]


def test_a_spiral_alone_gets_the_empty_fourier_block():
    col, const, kinds, counts = table(spiral=SPIRAL)
    assert counts == (40, 24, 12, 0) and kinds == []
    assert all(c == -1 and k == 0.0 for c, k in zip(col[4:28], const[4:28]))
    assert col[28:] == SPIRAL[1] and const[28:] == SPIRAL[2]
    assert (col[:4], const[:4]) == (BASE[0], BASE[1])


def test_a_law_alone_gets_both_blocks():
    col, const, kinds, counts = table(radial=RADIAL)
    assert counts == (44, 24, 12, 4)
    assert (col, const) == joined(BASE, PAD_FOURIER, PAD_SPIRAL, RADIAL[1:])
    assert col[28:40] == [-1] * 12 and [j for j in range(28, 40) if const[j] != 0.0] == [29, 35]
    assert const[29] == const[35] == 1.0
    assert col[40:] == RADIAL[1] and const[40:] == RADIAL[2]
    assert kinds == RADIAL[0]


def test_all_four():
    col, const, kinds, counts = table(fourier=FOURIER, spiral=SPIRAL, radial=RADIAL)
    assert counts == (44, 24, 12, 4) and kinds == RADIAL[0]
    assert (col, const) == joined(BASE, FOURIER[1:], SPIRAL[1:], RADIAL[1:])
    # a law behind modes alone: only the spiral block is padded
    col, const, kinds, counts = table(fourier=FOURIER, radial=RADIAL)
    assert counts == (44, 24, 12, 4) and kinds == RADIAL[0]
    assert (col, const) == joined(BASE, FOURIER[1:], PAD_SPIRAL, RADIAL[1:])


def test_all_zero_tags_are_no_registration():
    zero = lambda block: ([0] * N_SER,) + tuple(block[1:])
    assert table(fourier=zero(FOURIER), spiral=zero(SPIRAL), radial=zero(RADIAL)) == table()
    assert table(fourier=FOURIER, spiral=zero(SPIRAL), radial=zero(RADIAL)) == table(fourier=FOURIER)
    assert table(fourier=zero(FOURIER), spiral=SPIRAL) == table(spiral=SPIRAL)
