"""Argument checks of psfmc_ctx_create_fields_shaped (fields of different image and PSF sizes in one
context): every refusal happens before a device is touched, names the field and leaves *out NULL."""
import ctypes

import numpy as np
import pytest

from psfmc_amd import engine

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def _create(sides, psf_sides, n_psf):
    """rc, error text and handle of a create call for fields of sides [(ny, nx)], PSF sides [(py, px)] and
    n_psf [k] PSFs per field; the pixel arrays are zeros of the right total length."""
    lib = engine.load_library()
    n_f = len(sides)
    n_px = sum(y * x for y, x in sides)
    n_pk = sum(k * y * x for k, (y, x) in zip(n_psf, psf_sides))
    img, bad = np.zeros(n_px), np.zeros(n_px, dtype=np.uint8)
    psf = np.zeros(max(n_pk, 1))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    ny, nx = i32([s[0] for s in sides]), i32([s[1] for s in sides])
    py, px = i32([s[0] for s in psf_sides]), i32([s[1] for s in psf_sides])
    kn = i32(n_psf)
    handle = ctypes.c_void_p(12345)                 # must come back NULL
    rc = lib.psfmc_ctx_create_fields_shaped(
        ctypes.byref(handle), 0, n_f, ny.ctypes.data_as(_ip), nx.ctypes.data_as(_ip), img.ctypes.data_as(_dp),
        img.ctypes.data_as(_dp), bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), kn.ctypes.data_as(_ip),
        py.ctypes.data_as(_ip), px.ctypes.data_as(_ip), psf.ctypes.data_as(_dp), psf.ctypes.data_as(_dp), 1, 1, 64)
    return rc, lib.psfmc_last_error().decode(), handle.value


@pytest.mark.parametrize('sides, psf_sides, n_psf, words', [
    # an odd side (field 1)
    ([(118, 118), (100, 113), (128, 128)], [(11, 11), (17, 17), (21, 21)], [2, 2, 2], ('field 1', 'even')),
    # a PSF larger than its own field (field 2; it would fit field 0)
    ([(128, 128), (100, 112), (20, 20)], [(21, 21), (17, 17), (21, 21)], [2, 2, 2], ('field 2', 'PSF larger')),
    # unequal numbers of PSFs
    ([(118, 118), (100, 112), (128, 128)], [(11, 11), (17, 17), (21, 21)], [2, 2, 1], ('field 2', 'PSFs')),
    # each field alone fits a built side, together no side up to 2048 serves both: 1536 is built but too small
    # for 1530 + 11 - 1, and 2048 is less than 1536 + 601 - 1
    ([(1536, 1536), (1530, 1530)], [(601, 601), (11, 11)], [1, 1], ('field 0', 'exceeds the largest built side')),
    # one field beyond the largest side
    ([(64, 64), (2040, 2040)], [(5, 5), (25, 25)], [1, 1], ('field 1', 'exceeds the largest built side')),
])
def test_shaped_create_refuses_before_the_device(sides, psf_sides, n_psf, words):
    rc, msg, handle = _create(sides, psf_sides, n_psf)
    assert rc == -1, (rc, msg)
    for w in words:
        assert w in msg, msg
    assert handle is None


def test_shaped_entry_point_is_declared_and_exported():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'psfmc_hip.h')) as f:
        declared = set(re.findall(r'\b(psfmc_[a-z_]+)\s*\(', f.read()))
    lib = engine.load_library()
    for sym in ('psfmc_ctx_create_fields_shaped', 'psfmc_field_shape'):
        assert sym in declared and hasattr(lib, sym)
    assert lib.psfmc_abi_version() == 1


def test_fieldset_context_refuses_unequal_psf_counts():
    z = np.zeros((64, 64))
    fields = [(z, z + 1, z, np.zeros((2, 9, 9)), np.zeros((2, 9, 9))),
              (np.zeros((96, 96)), np.ones((96, 96)), np.zeros((96, 96)), np.zeros((1, 9, 9)), np.zeros((1, 9, 9)))]
    with pytest.raises(ValueError, match='same number of PSFs'):
        engine.FieldSetContext(fields, n_ps=1, n_sersic=1, max_walkers=8)


def test_fieldset_context_refuses_odd_side_naming_the_field():
    # mixed shapes reach the library (no np.stack across fields); its refusal names the field
    good = np.zeros((96, 96))
    odd = np.zeros((64, 63))
    fields = [(good, good + 1, good, np.zeros((1, 9, 9)), np.zeros((1, 9, 9))),
              (odd, odd + 1, odd, np.zeros((1, 9, 9)), np.zeros((1, 9, 9)))]
    with pytest.raises(engine.NativeError) as err:
        engine.FieldSetContext(fields, n_ps=1, n_sersic=1, max_walkers=8)
    assert err.value.code == -1 and 'field 1' in str(err.value) and 'even' in str(err.value)


def test_mixed_sets_cover_the_issue():
    """tests/test_gpu_mixed_paths.py's sets reach every kernel family a mixed set can land on (each set's test
    asserts the family the library reports)."""
    from test_gpu_mixed_paths import MIXED_SETS
    from test_gpu_variants import K_COLS, K_COLS3F, K_COLS3G, ROWS3_SIDES
    code = {'k_cols': K_COLS, 'k_cols3g': K_COLS3G, 'k_cols3f': K_COLS3F}
    for s in MIXED_SETS:
        ty, tx = s.transform
        assert code[engine.column_engine(ty)[0]] == s.column_engine, s.name
        assert ty in engine.FUSED_SIDES and tx in engine.FUSED_SIDES, s.name
        for ly, lx, pk in s.fields:
            # an embedded axis holds the image and its wrap-around margin
            assert all(t == l or t >= l + pk - 1 for t, l in ((ty, ly), (tx, lx))), (s.name, ly, lx, pk)
    assert {s.column_engine for s in MIXED_SETS} == {K_COLS, K_COLS3G, K_COLS3F}
    assert any(s.rows3 & 2 and s.transform[1] in ROWS3_SIDES for s in MIXED_SETS)
    assert any(s.rows3 == 3 and min(s.transform) > 1024 for s in MIXED_SETS)
    rows = {s.transform[1] for s in MIXED_SETS}
    assert 256 in rows and any(256 < n <= 300 for n in rows) and min(rows) <= 64
    assert any(s.row_group == 8 for s in MIXED_SETS) and any(s.row_group == 1 for s in MIXED_SETS)
    assert any(s.transform[0] != s.transform[1] for s in MIXED_SETS)
    fields = [(s, fld) for s in MIXED_SETS for fld in s.fields]
    embedded = [((fld[0] != s.transform[0]), (fld[1] != s.transform[1])) for s, fld in fields]
    assert (True, False) in embedded and (False, True) in embedded and (True, True) in embedded
    assert any(fld[:2] == s.transform for s, fld in fields)
    exact = [(s.name, axis) for s, fld in fields for axis in (0, 1)
             if fld[axis] != s.transform[axis] and fld[axis] + fld[2] - 1 == s.transform[axis]]
    assert {name for name, _ in exact} >= {'B', 'C', 'D', 'G', 'H'}
    assert {axis for _, axis in exact} == {0, 1}
    assert any(s.n_psf > 1 for s in MIXED_SETS) and {len(s.fields) for s in MIXED_SETS} == {2, 3}
