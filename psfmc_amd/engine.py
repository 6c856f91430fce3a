"""
ctypes binding of libpsfmc_hip.so (include/psfmc_hip.h) -- the only way the
Python host reaches the GPU.  There is deliberately no CPU fallback: if the
library is missing or no gfx950 device is present, construction raises.
"""
import ctypes
import os

import numpy as np

BACKEND_FUSED = 0
BACKEND_HIPFFT = 1
BACKENDS = {'fused': BACKEND_FUSED, 'hipfft': BACKEND_HIPFFT}

ROW_SKY, ROW_PS, ROW_SERSIC = 1, 4, 9

# sides the fused kernels are built for: the rows of psfmc_amd/csrc/psfmc_sides.h (tests/test_host_glue.py compares)
FUSED_SIDES = (64, 84, 88, 96, 98, 100, 104, 110, 112, 120, 126, 128, 130, 132, 140, 144, 150, 156,
               160, 168, 176, 180, 192, 196, 200, 208, 210, 220, 224, 240, 250, 252, 256, 260, 264,
               280, 286, 288, 294, 300, 308, 312, 320, 330, 336, 350, 352, 360, 364, 384, 390, 392,
               400, 416, 420, 440, 448, 480, 484, 500, 504, 512, 520, 528, 560, 572, 576, 600, 616,
               624, 630, 640, 650, 660, 672, 676, 700, 704, 720, 728, 768, 780, 784, 800, 832, 840,
               896, 900, 960, 1024,
               # round 4: sides above 1024 (three-stage row AND column kernels only: R1 x 8 x 8, R1 = 18 ... 32)
               1152, 1280, 1536, 2048)


def nearest_fused_sides(n):
    """The supported sides around `n`: (largest side <= n or None, smallest side >= n or None) --
    for choosing a cut-out size that stays on the fused kernels."""
    below = [v for v in FUSED_SIDES if v <= n]
    above = [v for v in FUSED_SIDES if v >= n]
    return (below[-1] if below else None), (above[0] if above else None)


# psfmc_fft.h fft3g_pick: the sides whose columns run on the general wave-wide three-stage engine, with
# their (R2, R3) split of the wave's lanes
_COLS3G_SHAPES = {}
for _sides, _shape in (((264, 308, 352, 484), (4, 11)), ((528, 576), (4, 12)),
                       ((312, 364, 416, 520, 572, 624, 676), (4, 13)),
                       ((560, 616, 672, 840, 896), (4, 14)), ((900,), (4, 15)),
                       ((640, 704), (4, 16)), ((330, 440), (5, 11)), ((250, 500), (5, 10)), ((294,), (7, 7)),
                       ((660, 720), (5, 12)),
                       # round 4: the re-surveyed shapes and the second survey's new sides (csrc/psfmc_fft.h fft3g_pick)
                       ((480, 600, 780), (6, 10)), ((392, 504, 728, 784), (7, 8)), ((448,), (8, 7)),
                       ((280, 336), (7, 8)), ((288,), (6, 8)), ((300,), (5, 12)), ((350,), (5, 10)), ((360,), (6, 10)),
                       ((630,), (7, 9)),
                       ((384, 768, 832, 960, 1152, 1280, 1536, 2048), (8, 8))):
    for _n in _sides:
        _COLS3G_SHAPES[_n] = _shape


def column_engine(ny):
    """Which column kernel the fused back end launches for transform side `ny` (decided in one place,
    psfmc_hip.hip col_engine, which launch_cols switches on): 'k_cols3f' (512, 1024, 1536, 2048: the general
    three-stage engine run forward both ways; round 3's power-of-two kernel 'k_cols3' remains behind option
    cols3 = 3 and for storage='f32'), 'k_cols3g' (the sides psfmc_fft.h fft3g_pick lists: ny = R1 * R2 * R3 on
    R2 * R3 <= 64 lanes) or 'k_cols' (the two-stage engine).  Returns (kernel name, (R1, R2, R3) or None).  This is the default (option cols3 = 1) at row
    groups of 4; a context with rows in groups of 8 whose k_cols3g column length L = R2 * R3 is a multiple of 4 but
    not of 8 (psfmc_fused_path.h cols3g_layout_ok) runs 'k_cols' instead, and option cols3 or storage='f32' select
    others.  `Context.get_option('column_engine')` reports what a context runs -- the answer of that same col_engine:
    0 k_cols, 1 k_cols3, 2 k_cols3g, 3 k_cols3f."""
    if ny in (512, 1024, 1536, 2048):
        return 'k_cols3f', (ny // 64, 8, 8)
    if ny in _COLS3G_SHAPES:
        r2, r3 = _COLS3G_SHAPES[ny]
        return 'k_cols3g', (ny // (r2 * r3), r2, r3)
    return 'k_cols', None


def embedding_side(side, psf_side):
    """The smallest transform side an image side the kernels are not built for can be EMBEDDED in: the
    smallest built side >= side + psf_side - 1 (the image, a wrap-around margin of psf_side - 1 pixels,
    zeros: the circular convolution of that length equals the image's own on the image's pixels --
    csrc/psfmc_device.h WrapDesc), or None when there is none (side + psf_side - 1 > 2048).  The library
    may pick a LARGER built side whose kernels are cheaper per walker (psfmc_hip.hip choose_embedding,
    measured table csrc/psfmc_side_costs.h); `Context.get_option('transform_ny' / 'transform_nx')` tells."""
    need = side + psf_side - 1
    fits = [v for v in FUSED_SIDES if v >= need]
    return fits[0] if fits else None


def fused_supports(ny, nx, psf_shape=None):
    """Whether psfmc_ctx_create accepts this image shape for the fused back end: both sides from
    FUSED_SIDES in any combination -- or, with the PSF's (py, px) given, any even side that can be
    embedded in a built one (`embedding_side`)."""
    if ny in FUSED_SIDES and nx in FUSED_SIDES:
        return True
    if psf_shape is None or ny % 2 or nx % 2:
        return False
    return all(side in FUSED_SIDES or embedding_side(side, pk) is not None
               for side, pk in ((ny, psf_shape[0]), (nx, psf_shape[1])))


_LIB_NAME = 'libpsfmc_hip.so'
_lib = None

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_u8_p = ctypes.POINTER(ctypes.c_uint8)


class NativeError(RuntimeError):
    """A libpsfmc_hip call failed (code + message of psfmc_last_error)."""

    def __init__(self, code, message):
        super(NativeError, self).__init__('libpsfmc_hip error {}: {}'.format(code, message))
        self.code = code


def library_path():
    """The in-tree extension; PSFMC_LIB may name another build of it (A/B runs)."""
    override = os.environ.get('PSFMC_LIB')
    if override:
        return override
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def load_library():
    """Load (once) and type the C ABI.  Raises ImportError when the extension
    has not been built -- the product never runs without it."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            '{} not found: build it with `make -C psfmc_amd/csrc` (or '
            '`python -c "import __graft_entry__ as g; g.build()"`). psfmc_amd has no '
            'CPU fallback.'.format(path))
    # torch (device memory / streams / torch.distributed plumbing) ships its own
    # libamdhip64 with the same SONAME; importing it first makes this process use
    # ONE HIP runtime for both.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.psfmc_abi_version.restype = ci
    lib.psfmc_abi_version.argtypes = []
    lib.psfmc_last_error.restype = ctypes.c_char_p
    lib.psfmc_last_error.argtypes = []
    lib.psfmc_ctx_create.restype = ci
    lib.psfmc_ctx_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, _c_double_p, _c_double_p,
                                     _c_u8_p, ci, ci, ci, _c_double_p, _c_double_p, ci, ci, ci, ci]
    lib.psfmc_ctx_destroy.restype = ci
    lib.psfmc_ctx_destroy.argtypes = [vp]
    lib.psfmc_row_len.restype = ci
    lib.psfmc_row_len.argtypes = [vp]
    lib.psfmc_pass_size.restype = ci
    lib.psfmc_pass_size.argtypes = [vp, ci]
    lib.psfmc_eval_batch.restype = ci
    lib.psfmc_eval_batch.argtypes = [vp, ci, _c_double_p, _c_u8_p, _c_double_p]
    lib.psfmc_eval_batch_field.restype = ci
    lib.psfmc_eval_batch_field.argtypes = [vp, ci, ci, _c_double_p, _c_u8_p, _c_double_p]
    lib.psfmc_eval_batch_device.restype = ci
    lib.psfmc_eval_batch_device.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.psfmc_eval_images.restype = ci
    lib.psfmc_eval_images.argtypes = [vp, ci, _c_double_p] + [_c_double_p] * 5
    lib.psfmc_get_spectra.restype = ci
    lib.psfmc_get_spectra.argtypes = [vp, _c_double_p, _c_double_p]
    lib.psfmc_set_option.restype = ci
    lib.psfmc_set_option.argtypes = [vp, ctypes.c_char_p, cd]
    lib.psfmc_get_option.restype = cd
    lib.psfmc_get_option.argtypes = [vp, ctypes.c_char_p]
    ip = ctypes.POINTER(ctypes.c_int)
    lib.psfmc_set_layout.restype = ci
    lib.psfmc_set_layout.argtypes = [vp, ci, ci, ip, _c_double_p, ip, ip, cd, ip, _c_double_p,
                                     _c_double_p, _c_double_p]
    lib.psfmc_set_priors.restype = ci
    lib.psfmc_set_priors.argtypes = [vp, ci, ci, ip, _c_double_p]
    lib.psfmc_eval_theta.restype = ci
    lib.psfmc_eval_theta.argtypes = [vp, ci, _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_eval_theta_device.restype = ci
    lib.psfmc_eval_theta_device.argtypes = [vp, ci, vp, vp, vp, vp]
    ip = ctypes.POINTER(ctypes.c_int)
    lib.psfmc_ctx_create_fields.restype = ci
    lib.psfmc_ctx_create_fields.argtypes = [ctypes.POINTER(vp), ci, ci, ci, ci, _c_double_p, _c_double_p, _c_u8_p,
                                            ci, ci, ci, _c_double_p, _c_double_p, ci, ci, ci]
    lib.psfmc_ctx_create_fields_shaped.restype = ci
    lib.psfmc_ctx_create_fields_shaped.argtypes = [ctypes.POINTER(vp), ci, ci, ip, ip, _c_double_p, _c_double_p,
                                                   _c_u8_p, ip, ip, ip, _c_double_p, _c_double_p, ci, ci, ci]
    lib.psfmc_field_shape.restype = ci
    lib.psfmc_field_shape.argtypes = [vp, ci, ip, ip]
    lib.psfmc_set_layout_field.restype = ci
    lib.psfmc_set_layout_field.argtypes = [vp, ci, ci, ci, ip, _c_double_p, ip, ip, ctypes.c_double, ip,
                                           _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_eval_theta_fields.restype = ci
    lib.psfmc_eval_theta_fields.argtypes = [vp, ci, ip, ip, _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_eval_theta_device_fields.restype = ci
    lib.psfmc_eval_theta_device_fields.argtypes = [vp, ci, ip, ip, vp, vp, vp, vp]
    lib.psfmc_accumulate_theta.restype = ci
    lib.psfmc_accumulate_theta.argtypes = [vp, ci, _c_double_p]
    lib.psfmc_debug_theta_rows.restype = ci
    lib.psfmc_debug_theta_rows.argtypes = [vp, ci, _c_double_p, _c_double_p, _c_double_p, _c_u8_p]
    lib.psfmc_stretch_run.restype = ci
    lib.psfmc_stretch_run.argtypes = [vp, ci, ci, _c_double_p, _c_double_p, ci, _c_double_p, _c_double_p,
                                      ip, _c_double_p, _c_double_p, _c_double_p,
                                      ctypes.POINTER(ctypes.c_longlong), ci]
    llp = ctypes.POINTER(ctypes.c_longlong)
    lib.psfmc_stretch_run_fields.restype = ci
    lib.psfmc_stretch_run_fields.argtypes = lib.psfmc_stretch_run.argtypes
    lib.psfmc_eval_theta_split.restype = ci
    lib.psfmc_eval_theta_split.argtypes = [vp, ci, _c_double_p, _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_pt_run.restype = ci
    lib.psfmc_pt_run.argtypes = [vp, ci, ci, ci, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ci,
                                 _c_double_p, _c_double_p, ip, _c_double_p, ip, ip, _c_double_p,
                                 _c_double_p, _c_double_p, _c_double_p, _c_double_p, llp, llp, ci]
    lib.psfmc_set_joint_priors.restype = ci
    lib.psfmc_set_joint_priors.argtypes = [vp, ci, ip, _c_double_p]
    lib.psfmc_eval_theta_joint.restype = ci
    lib.psfmc_eval_theta_joint.argtypes = [vp, ci, _c_double_p, _c_double_p]
    lib.psfmc_eval_theta_joint_device.restype = ci
    lib.psfmc_eval_theta_joint_device.argtypes = [vp, ci, vp, vp, vp]
    lib.psfmc_stretch_run_joint.restype = ci
    lib.psfmc_stretch_run_joint.argtypes = lib.psfmc_stretch_run.argtypes
    lib.psfmc_eval_theta_joint_split.restype = ci
    lib.psfmc_eval_theta_joint_split.argtypes = [vp, ci, _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_pt_run_joint.restype = ci
    lib.psfmc_pt_run_joint.argtypes = lib.psfmc_pt_run.argtypes
    lib.psfmc_eval_theta_split_fields.restype = ci
    lib.psfmc_eval_theta_split_fields.argtypes = [vp, ci, ip, ip, _c_double_p, _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_pt_run_fields.restype = ci
    lib.psfmc_pt_run_fields.argtypes = lib.psfmc_pt_run.argtypes
    for fn in (lib.psfmc_pt_move_run, lib.psfmc_pt_move_run_joint, lib.psfmc_pt_move_run_fields):
        fn.restype = ci                         # (the twin's arguments with kind and partner_b behind log_u)
        fn.argtypes = lib.psfmc_pt_run.argtypes[:13] + [ip, ip] + lib.psfmc_pt_run.argtypes[13:]
    lib.psfmc_accumulate_theta_field.restype = ci
    lib.psfmc_accumulate_theta_field.argtypes = [vp, ci, ci, _c_double_p]
    lib.psfmc_reset_accumulated_field.restype = ci
    lib.psfmc_reset_accumulated_field.argtypes = [vp, ci]
    lib.psfmc_get_accumulated_field.restype = ci
    lib.psfmc_get_accumulated_field.argtypes = [vp, ci] + [_c_double_p] * 5 + [llp]
    lib.psfmc_eval_images_field.restype = ci
    lib.psfmc_eval_images_field.argtypes = [vp, ci, ci, _c_double_p] + [_c_double_p] * 5
    lib.psfmc_stretch_open.restype = ci
    lib.psfmc_stretch_open.argtypes = [vp, ci, ci, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ip,
                                       _c_double_p, llp, ci]
    lib.psfmc_move_run.restype = ci
    lib.psfmc_move_run.argtypes = [vp, ci, ci, _c_double_p, _c_double_p, ci, _c_double_p, _c_double_p,
                                   ip, _c_double_p, ip, ip, _c_double_p, _c_double_p, llp, ci]
    lib.psfmc_move_run_joint.restype = ci
    lib.psfmc_move_run_joint.argtypes = lib.psfmc_move_run.argtypes
    lib.psfmc_stretch_set_moves.restype = ci
    lib.psfmc_stretch_set_moves.argtypes = [vp, ip, ip]
    lib.psfmc_stretch_half_eval.restype = ci
    lib.psfmc_stretch_half_eval.argtypes = [vp, ci, ci, ci, ci, vp, vp]
    lib.psfmc_stretch_half_accept.restype = ci
    lib.psfmc_stretch_half_accept.argtypes = [vp, ci, ci, vp, vp]
    lib.psfmc_stretch_accumulate.restype = ci
    lib.psfmc_stretch_accumulate.argtypes = [vp, ci, ci, vp]
    lib.psfmc_stretch_close.restype = ci
    lib.psfmc_stretch_close.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p, llp, vp]
    lib.psfmc_get_accumulated_sums.restype = ci
    lib.psfmc_get_accumulated_sums.argtypes = [vp, _c_double_p, llp]
    lib.psfmc_set_accumulated_sums.restype = ci
    lib.psfmc_set_accumulated_sums.argtypes = [vp, _c_double_p, ctypes.c_longlong]
    lib.psfmc_accumulate_images.restype = ci
    lib.psfmc_accumulate_images.argtypes = [vp, ci, _c_double_p]
    lib.psfmc_get_accumulated.restype = ci
    lib.psfmc_get_accumulated.argtypes = [vp] + [_c_double_p] * 5 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.psfmc_reset_accumulated.restype = ci
    lib.psfmc_reset_accumulated.argtypes = [vp]
    lib.psfmc_group_create.restype = ci
    lib.psfmc_group_create.argtypes = [ctypes.POINTER(vp), ci, ip, ci, ci, _c_double_p, _c_double_p,
                                       _c_u8_p, ci, ci, ci, _c_double_p, _c_double_p, ci, ci, ci, ci]
    lib.psfmc_group_destroy.restype = ci
    lib.psfmc_group_destroy.argtypes = [vp]
    lib.psfmc_group_size.restype = ci
    lib.psfmc_group_size.argtypes = [vp]
    lib.psfmc_group_set_layout.restype = ci
    lib.psfmc_group_set_layout.argtypes = [vp, ci, ci, ip, _c_double_p, ip, ip, cd, ip, _c_double_p,
                                           _c_double_p, _c_double_p]
    lib.psfmc_set_sersic_integrate.restype = ci
    lib.psfmc_set_sersic_integrate.argtypes = [vp, ci, ci, ip]
    lib.psfmc_group_set_sersic_integrate.restype = ci
    lib.psfmc_group_set_sersic_integrate.argtypes = [vp, ci, ip]
    lib.psfmc_set_aux_layout.restype = ci
    lib.psfmc_set_aux_layout.argtypes = [vp, ci, ci, ip, _c_double_p, ip, ip]
    lib.psfmc_set_aux_rows.restype = ci
    lib.psfmc_set_aux_rows.argtypes = [vp, ci, _c_double_p]
    lib.psfmc_set_ties.restype = ci
    lib.psfmc_set_ties.argtypes = [vp, ci, ci, ip, ip, _c_double_p, ip, _c_double_p]
    lib.psfmc_group_set_ties.restype = ci
    lib.psfmc_group_set_ties.argtypes = [vp, ci, ip, ip, _c_double_p, ip, _c_double_p]
    lib.psfmc_group_set_aux_layout.restype = ci
    lib.psfmc_group_set_aux_layout.argtypes = [vp, ci, ip, _c_double_p, ip, ip]
    lib.psfmc_set_fourier_layout.restype = ci
    lib.psfmc_set_fourier_layout.argtypes = [vp, ci, ci, ip, ip, _c_double_p]
    lib.psfmc_group_set_fourier_layout.restype = ci
    lib.psfmc_group_set_fourier_layout.argtypes = [vp, ci, ip, ip, _c_double_p]
    lib.psfmc_set_spiral_layout.restype = ci
    lib.psfmc_set_spiral_layout.argtypes = [vp, ci, ci, ip, ip, _c_double_p]
    lib.psfmc_group_set_spiral_layout.restype = ci
    lib.psfmc_group_set_spiral_layout.argtypes = [vp, ci, ip, ip, _c_double_p]
    lib.psfmc_set_radial_layout.restype = ci
    lib.psfmc_set_radial_layout.argtypes = [vp, ci, ci, ip, ip, _c_double_p]
    lib.psfmc_group_set_radial_layout.restype = ci
    lib.psfmc_group_set_radial_layout.argtypes = [vp, ci, ip, ip, _c_double_p]
    lib.psfmc_set_truncation_layout.restype = ci
    lib.psfmc_set_truncation_layout.argtypes = [vp, ci, ci, ip, ip, _c_double_p]
    lib.psfmc_group_set_truncation_layout.restype = ci
    lib.psfmc_group_set_truncation_layout.argtypes = [vp, ci, ip, ip, _c_double_p]
    lib.psfmc_set_bending_layout.restype = ci
    lib.psfmc_set_bending_layout.argtypes = [vp, ci, ci, ip, ip, _c_double_p]
    lib.psfmc_group_set_bending_layout.restype = ci
    lib.psfmc_group_set_bending_layout.argtypes = [vp, ci, ip, ip, _c_double_p]
    lib.psfmc_set_general_mean.restype = ci
    lib.psfmc_set_general_mean.argtypes = [vp, ci, ci, ip]
    lib.psfmc_group_set_general_mean.restype = ci
    lib.psfmc_group_set_general_mean.argtypes = [vp, ci, ip]
    lib.psfmc_group_set_priors.restype = ci
    lib.psfmc_group_set_priors.argtypes = [vp, ci, ip, _c_double_p]
    lib.psfmc_group_eval_batch.restype = ci
    lib.psfmc_group_eval_batch.argtypes = [vp, ci, _c_double_p, _c_u8_p, _c_double_p]
    lib.psfmc_group_eval_theta.restype = ci
    lib.psfmc_group_eval_theta.argtypes = [vp, ci, _c_double_p, _c_double_p, _c_double_p]
    lib.psfmc_debug_math.restype = ci
    lib.psfmc_debug_math.argtypes = [ci, ci, ci, _c_double_p, _c_double_p]
    lib.psfmc_debug_aux_table.restype = ci
    lib.psfmc_debug_aux_table.argtypes = [ci, ci, ip, _c_double_p] + 3 * [ip, ip, _c_double_p] + [_c_double_p, ip, ip, ip]
    lib.psfmc_debug_aux_table_blocks.restype = ci
    lib.psfmc_debug_aux_table_blocks.argtypes = ([ci, ci, ip, _c_double_p] + 4 * [ip, ip, _c_double_p] +
                                                 [_c_double_p, ip, ip, ip, ip])
    lib.psfmc_debug_aux_table_bending.restype = ci
    lib.psfmc_debug_aux_table_bending.argtypes = ([ci, ci, ip, _c_double_p] + 5 * [ip, ip, _c_double_p] +
                                                  [_c_double_p, ip, ip, ip, ip, ip])
    lib.psfmc_fisher_rows.restype = ci
    lib.psfmc_fisher_rows.argtypes = [vp, ci, ci, ci] + [_c_double_p] * 5
    lib.psfmc_fisher_rows_fields.restype = ci
    lib.psfmc_fisher_rows_fields.argtypes = [vp, ci, ci, ip] + [_c_double_p] * 5
    lib.psfmc_fisher_rows_joint.restype = ci
    lib.psfmc_fisher_rows_joint.argtypes = [vp, ci, ci, ci, ip] + [_c_double_p] * 5
    lib.psfmc_debug_fisher_gram.restype = ci
    lib.psfmc_debug_fisher_gram.argtypes = [ci, ci, ci] + [_c_double_p] * 6
    lib.psfmc_debug_sweep.restype = ci
    lib.psfmc_debug_sweep.argtypes = [ci, ci, ctypes.c_size_t, ci, _c_double_p]
    lib.psfmc_debug_valu_rate.restype = ci
    lib.psfmc_debug_valu_rate.argtypes = [ci, ci, ci, _c_double_p]
    if lib.psfmc_abi_version() != 1:
        raise ImportError('libpsfmc_hip ABI version mismatch')
    _lib = lib
    return lib


def _dp(arr):
    return arr.ctypes.data_as(_c_double_p)


PRIOR_NPAR = 4          # include/psfmc_hip.h PSFMC_PRIOR_NPAR


def _prior_table(family, params):
    """(family [P] int32, params [P, PRIOR_NPAR] float64) for psfmc_set_priors; `params` may have fewer
    columns (the rest is 0)."""
    family = np.ascontiguousarray(family, dtype=np.int32).ravel()
    params = np.asarray(params, dtype=np.float64).reshape(len(family), -1)
    if params.shape[1] > PRIOR_NPAR:
        raise ValueError('at most {} parameters per prior'.format(PRIOR_NPAR))
    table = np.zeros((len(family), PRIOR_NPAR))
    table[:, :params.shape[1]] = params
    return family, table, family.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(table)


def _f64(arr):
    return np.ascontiguousarray(arr, dtype=np.float64)


MOVE_STRETCH, MOVE_DE = 0, 1          # include/psfmc_hip.h PSFMC_MOVE_*


def _move_run(fn, ctx, pos, lnprob, scal, lz, partner, log_u, kind, partner_b, naccepted, store, accumulate):
    """The arrays of a psfmc_stretch_run* or psfmc_move_run* call (`fn`) shaped and the call made.  The leading
    dimensions of pos, `lead` = [W] or [F, W], lead every per-walker array; the random arrays are lead[:-1] +
    [n_iter, 2, W/2].  kind int32 [n_iter] and partner_b: the arrays a move run adds, None for the stretch
    entry points (scal is then z).  Returns (rc, (pos, lnprob, chain lead + [n_iter, P] | None, lnprob_chain
    lead + [n_iter] | None)); naccepted, a contiguous int64 array of shape `lead`, is updated."""
    pos = np.array(pos, dtype=np.float64, order='C')
    lead, n_p = pos.shape[:-1], pos.shape[-1]
    if len(lead) not in (1, 2):
        raise ValueError('pos must be [W, P] or [F, W, P]')
    n_w = lead[-1]
    n_iter = int(np.shape(scal)[len(lead) - 1])
    rand = lead[:-1] + (n_iter, 2, n_w // 2)
    have = lnprob is not None
    lnp = np.array(lnprob, dtype=np.float64).reshape(lead) if have else np.empty(lead)
    scal, lz, log_u = (_f64(a).reshape(rand) for a in (scal, lz, log_u))
    ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    partner = np.ascontiguousarray(partner, dtype=np.int32).reshape(rand)
    moves = ()
    if kind is not None:
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(n_iter)
        partner_b = np.ascontiguousarray(partner_b, dtype=np.int32).reshape(rand)
        moves = (ipt(kind), ipt(partner_b))
    if naccepted.dtype != np.int64 or naccepted.shape != lead or not naccepted.flags.c_contiguous:
        raise ValueError('naccepted must be a contiguous int64 {}'.format(list(lead)))
    chain = np.empty(lead + (n_iter, n_p)) if store and n_iter else None
    lnchain = np.empty(lead + (n_iter,)) if store and n_iter else None
    rc = fn(ctx, n_w, n_iter, _dp(pos), _dp(lnp), int(have), _dp(scal), _dp(lz), ipt(partner), _dp(log_u), *moves,
            _dp(chain) if chain is not None else None, _dp(lnchain) if lnchain is not None else None,
            naccepted.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), int(bool(accumulate)))
    return rc, (pos, lnp, chain, lnchain)


def _pt_run(fn, ctx, betas, pos, lnlike, lnprior, z, lz, partner, log_u, swap_i, swap_j, swap_log_u, naccepted,
            nswap, store, accumulate, kind=None, partner_b=None):
    """The arrays of psfmc_pt_run / psfmc_pt_run_joint / psfmc_pt_run_fields or, with kind int32 [n_iter] + lead
    and partner_b shaped as partner, of their psfmc_pt_move_run* twins (`fn`) shaped and the call made;
    betas [T] and pos [T, W, P] -- or, for the fields of a set, [F, T, W, P]: `lead` = () or (F,) then leads every
    per-walker array and follows the iteration (and half-step) in the random ones -- are contiguous float64
    already.  Returns (rc, (pos, lnlike, lnprior, chain, lnprob_chain, lnlike_chain, lnprior_chain)); naccepted
    and nswap are updated."""
    lead, (n_t, n_w, n_p) = pos.shape[:-3], pos.shape[-3:]
    n_iter = int(np.shape(z)[0])
    have = lnlike is not None and lnprior is not None
    ll = np.array(lnlike, dtype=np.float64).reshape(lead + (n_t, n_w)) if have else np.empty(lead + (n_t, n_w))
    lp = np.array(lnprior, dtype=np.float64).reshape(lead + (n_t, n_w)) if have else np.empty(lead + (n_t, n_w))
    rand = (n_iter, 2) + lead + (n_t, n_w // 2)
    z, lz, log_u = (_f64(a).reshape(rand) for a in (z, lz, log_u))
    partner = np.ascontiguousarray(partner, dtype=np.int32).reshape(rand)
    n_sw = max(n_t - 1, 0)
    srand = (n_iter,) + lead + (n_sw, n_w)
    swap_i, swap_j = (np.ascontiguousarray(a, dtype=np.int32).reshape(srand) for a in (swap_i, swap_j))
    swap_log_u = _f64(swap_log_u).reshape(srand)
    names = ''.join('F, ' for _ in lead)
    if naccepted.dtype != np.int64 or naccepted.shape != lead + (n_t, n_w) or not naccepted.flags.c_contiguous:
        raise ValueError('naccepted must be int64 [{}T, W]'.format(names))
    if nswap.dtype != np.int64 or nswap.shape != lead + (n_sw,) or not nswap.flags.c_contiguous:
        raise ValueError('nswap must be int64 [{}T-1]'.format(names))
    store = store and n_iter > 0
    chain = np.empty(lead + (n_t, n_w, n_iter, n_p)) if store else None
    lnchain = np.empty(lead + (n_w, n_iter)) if store else None
    llchain = np.empty(lead + (n_t, n_w, n_iter)) if store else None
    lpchain = np.empty(lead + (n_t, n_w, n_iter)) if store else None
    ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    lpt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    opt = lambda a: _dp(a) if a is not None else None
    moves = ()
    if kind is not None:
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape((n_iter,) + lead)
        partner_b = np.ascontiguousarray(partner_b, dtype=np.int32).reshape(rand)
        moves = (ipt(kind), ipt(partner_b))
    rc = fn(ctx, n_t, n_w, n_iter, _dp(betas), _dp(pos), _dp(ll), _dp(lp), int(have), _dp(z), _dp(lz),
            ipt(partner), _dp(log_u), *moves, ipt(swap_i), ipt(swap_j), _dp(swap_log_u), opt(chain), opt(lnchain),
            opt(llchain), opt(lpchain), lpt(naccepted), lpt(nswap) if n_sw else None, int(bool(accumulate)))
    return rc, (pos, ll, lp, chain, lnchain, llchain, lpchain)


def _aux_layout_args(aux_col, aux_const, sky_flags, sersic_flags):
    """The arrays of psfmc_set_aux_layout (kept alive by the caller's tuple) and their ctypes pointers."""
    i32 = lambda a: np.ascontiguousarray(np.asarray(a).astype(np.int32), dtype=np.int32).ravel()
    col, sky, ser = i32(aux_col), i32(np.asarray(sky_flags, dtype=bool)), i32(np.asarray(sersic_flags, dtype=bool))
    const = _f64(aux_const).ravel()
    if len(col) != len(const) or len(col) != 2 * len(sky) + len(ser):
        raise ValueError('aux layout: 2 values per Sky and 1 per Sersic, got {} for {} + {}'.format(
            len(col), len(sky), len(ser)))
    ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    return (col, const, sky, ser), (len(col), ipt(col), _dp(const), ipt(sky), ipt(ser))


MAX_TIES = 64              # PSFMC_MAX_TIES: tied values per field (a tied `xy` is two)


def _tie_args(src_col, ratio_col, ratio_const, offset_col, offset_const):
    """The arrays of psfmc_set_ties (kept alive by the caller's tuple) and their ctypes pointers: per tie the source
    column, the ratio's column or -1 and constant, the offset's column or -1 and constant."""
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int32), dtype=np.int32).ravel()
    src, rcol, ocol = i32(src_col), i32(ratio_col), i32(offset_col)
    rconst, oconst = _f64(ratio_const).ravel(), _f64(offset_const).ravel()
    if not (len(src) == len(rcol) == len(ocol) == len(rconst) == len(oconst)):
        raise ValueError('ties: five arrays of one length')
    ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    return (src, rcol, ocol, rconst, oconst), (len(src), ipt(src), ipt(rcol), _dp(rconst), ipt(ocol), _dp(oconst))


FOURIER_MODES = 6          # PSFMC_FOURIER_MODES: modes 1 ... 6, an amplitude and a phase entry each
SPIRAL_PARAMS = 6          # PSFMC_SPIRAL_PARAMS: r_in, r_out, winding, alpha, inclination, sky angle
RADIAL_PARAMS = 2          # PSFMC_RADIAL_PARAMS: (beta, unused) of a Moffat slot, (alpha, beta) of a Ferrer slot
TRUNC_PARAMS = 4           # PSFMC_TRUNC_PARAMS: in_lo, in_hi, out_lo, out_hi of a slot (flag bit 0 inner, bit 1 outer)
BEND_MODES = 4             # PSFMC_BEND_MODES: bending modes 1 ... 4, an amplitude entry each (mask bit m - 1)
# the blocks behind the aux entries, in table order: name -> (entries per Sersic, the per-Sersic tags are flags)
_BLOCKS = {'fourier': (2 * FOURIER_MODES, False), 'spiral': (SPIRAL_PARAMS, True), 'radial': (RADIAL_PARAMS, False),
           'truncation': (TRUNC_PARAMS, False), 'bending': (BEND_MODES, False)}


def _block_args(name, tags, col, const):
    """The arrays of psfmc_set_<name>_layout (kept alive by the caller's tuple) and their ctypes pointers: per
    Sersic a tag -- mode mask, spiral flag, radial kind, truncation sides, bending mask -- and the block's entries."""
    per_sersic, tags_are_flags = _BLOCKS[name]
    i32 = lambda a: np.ascontiguousarray(np.asarray(a).astype(np.int32), dtype=np.int32).ravel()
    tags = i32(np.asarray(tags, dtype=bool) if tags_are_flags else tags)
    col, const = i32(col), _f64(const).ravel()
    if len(col) != len(const) or len(col) != per_sersic * len(tags):
        raise ValueError('{} layout: {} entries per Sersic, got {} for {}'.format(name, per_sersic, len(col), len(tags)))
    ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    return (tags, col, const), (len(tags), ipt(tags), ipt(col), _dp(const))


class _BlockLayouts(object):
    """The five block layout calls of a context, a field of a set and a group: each class has
    `_set_block(name, tags, col, const)`, psfmc_[group_]set_<name>_layout on what it stands for."""

    def set_fourier_layout(self, mode_masks, col, const):
        """Azimuthal Fourier modes (psfmc_set_fourier_layout; after `set_aux_layout`): per Sersic a mask of its
        modes (bit m - 1: mode m) and, per Sersic and mode 1 ... 6, an amplitude and a phase entry -- column of theta
        or -1 and a constant.  A context that never gets the call is what it was without it."""
        self._set_block('fourier', mode_masks, col, const)

    def set_spiral_layout(self, flags, col, const):
        """Spiral arms (psfmc_set_spiral_layout; after `set_aux_layout` and `set_fourier_layout`): per Sersic a flag
        and six entries -- r_in, r_out, winding, alpha, inclination, sky angle; column of theta or -1 and a
        constant.  A context that never gets the call is what it was without it."""
        self._set_block('spiral', flags, col, const)

    def set_radial_layout(self, kinds, col, const):
        """Radial laws (psfmc_set_radial_layout; behind the spiral layout): per Sersic slot a kind -- 0 Sersic,
        1 Moffat, 2 Ferrer -- and two entries, (beta, unused) or (alpha, beta); column of theta or -1 and a
        constant.  A context that never gets the call is what it was without it."""
        self._set_block('radial', kinds, col, const)

    def set_truncation_layout(self, flags, col, const):
        """Truncations (psfmc_set_truncation_layout; behind the radial layout): per Sersic slot the sides -- bit 0
        inner, bit 1 outer -- and four entries, in_lo, in_hi, out_lo, out_hi; column of theta or -1 and a constant.
        A context that never gets the call is what it was without it."""
        self._set_block('truncation', flags, col, const)

    def set_bending_layout(self, mode_masks, col, const):
        """Bending modes (psfmc_set_bending_layout; behind the truncation layout, the last block): per Sersic slot a
        mask of its modes (bit m - 1: mode m) and four entries, a_1 ... a_4; column of theta or -1 and a constant.  A
        context that never gets the call is what it was without it."""
        self._set_block('bending', mode_masks, col, const)


def _send_aux_rows(lib, ctx, check, aux, n_w, width=None):
    """psfmc_set_aux_rows for the next row-based call of n_w walkers (aux None: nothing to send).  width: the
    context's values per walker where a field's rows may be shorter (a field without Fourier modes in a context
    that has some): the rows are padded with zeros."""
    if aux is None:
        return
    aux = _f64(aux)
    if aux.ndim != 2 or aux.shape[0] != n_w:
        raise ValueError('aux rows must be [W, n_aux] with the rows\' W')
    if width is not None and aux.shape[1] < width:
        aux = np.ascontiguousarray(np.pad(aux, ((0, 0), (0, width - aux.shape[1]))))
    check(lib.psfmc_set_aux_rows(ctx, int(n_w), _dp(aux)))


FISHER_MAX_COLUMNS = 63         # psfmc_fisher_rows: K + 1 vectors in four 16-row tiles of the matrix unit


def _fisher_rows(lib, ctx, check, field, rows, inv2h, row_len, max_walkers, send_aux):
    """psfmc_fisher_rows for one context: rows [n_base, 2K+1, row_len], inv2h [n_base, K] ->
    (F [n_base, K, K], g [n_base, K], lnlike [n_base])."""
    rows, inv2h = _f64(rows), _f64(inv2h)
    if rows.ndim != 3 or rows.shape[2] != row_len:
        raise ValueError('rows must be [n_base, 2K+1, {}], got {}'.format(row_len, rows.shape))
    n_base, n_st = rows.shape[:2]
    k = (n_st - 1) // 2
    if n_base < 1 or k < 1 or n_st != 2 * k + 1 or inv2h.shape != (n_base, k):
        raise ValueError('rows [n_base, 2K+1, row_len] need inv2h [n_base, K] with K >= 1; got {} and {}'.format(
            rows.shape, inv2h.shape))
    if k > FISHER_MAX_COLUMNS:
        raise ValueError('K={} differentiated columns exceed {}'.format(k, FISHER_MAX_COLUMNS))
    if n_base * n_st > max_walkers:
        raise ValueError('n_base (2K+1) = {} exceeds max_walkers={}'.format(n_base * n_st, max_walkers))
    f_out, g_out, ll = np.empty((n_base, k, k)), np.empty((n_base, k)), np.empty(n_base)
    send_aux(n_base * n_st)
    check(lib.psfmc_fisher_rows(ctx, int(field), n_base, k, _dp(rows), _dp(inv2h), _dp(f_out), _dp(g_out), _dp(ll)))
    return f_out, g_out, ll


def debug_fisher_gram(a, b, c, d, device=0):
    """The Gram and finish kernels of psfmc_fisher_rows alone (psfmc_debug_fisher_gram): a, b [K, n_pix], c, d [n_pix]
    -> (F [K, K] = sum_pix (a a^T + b b^T), g [K] = sum_pix (a c + b d)).  Test hook for the matrix unit's lane map."""
    lib = load_library()
    a, b, c, d = (_f64(v) for v in (a, b, c, d))
    if a.ndim != 2 or b.shape != a.shape or c.shape != a.shape[1:] or d.shape != c.shape:
        raise ValueError('a, b must be [K, n_pix] and c, d [n_pix]')
    k, n_pix = a.shape
    f_out, g_out = np.empty((k, k)), np.empty(k)
    rc = lib.psfmc_debug_fisher_gram(int(device), k, n_pix, _dp(a), _dp(b), _dp(c), _dp(d), _dp(f_out), _dp(g_out))
    if rc != 0:
        raise NativeError(rc, lib.psfmc_last_error().decode('utf-8', 'replace'))
    return f_out, g_out


def debug_math(op, values, device=0):
    """Evaluate a device elementary function ('log2', 'exp2', 'rcp', 'rcp1',
    'exp2_noclamp', 'log2_tab', 'exp2_floor') on an array (test hook for the rasteriser's hand-written fp64 math)."""
    lib = load_library()
    code = {'log2': 0, 'exp2': 1, 'rcp': 2, 'rcp1': 3, 'exp2_noclamp': 4, 'log2_tab': 5, 'exp2_floor': 6}[op]
    x = _f64(np.ravel(values))
    out = np.empty_like(x)
    rc = lib.psfmc_debug_math(int(device), code, x.size, _dp(x), _dp(out))
    if rc != 0:
        raise NativeError(rc, lib.psfmc_last_error().decode('utf-8', 'replace'))
    return out.reshape(np.shape(values))


def debug_pow_tab(values, p, device=0):
    """values ** p through the rasteriser's power tables (k_pow_tables' builder + `fast_pow_tab`, the
    function that replaced log2 + exp2 per Sersic pixel): test hook."""
    lib = load_library()
    x = _f64(np.ravel(values))
    buf = np.concatenate([x, [float(p)]])
    out = np.empty_like(x)
    rc = lib.psfmc_debug_math(int(device), 100, x.size, _dp(buf), _dp(out))
    if rc != 0:
        raise NativeError(rc, lib.psfmc_last_error().decode('utf-8', 'replace'))
    return out.reshape(np.shape(values))


def debug_aux_table(n_sky, n_sersic, base=None, fourier=None, spiral=None, radial=None, truncation=None, bending=None):
    """The auxiliary table the library composes for one field (psfmc_debug_aux_table; host only, no device): base =
    (col, const) of the aux layout, each block (tags, col, const) as its layout call takes them, None where the
    field registered none -> (const, col, kinds, (n_aux, n_fou, n_spi, n_rad)).  With `truncation`
    (psfmc_debug_aux_table_blocks) -> (const, col, kinds, sides, (n_aux, n_fou, n_spi, n_rad, n_tru)).  With `bending`
    (psfmc_debug_aux_table_bending; with or without `truncation`) -> (const, col, kinds, sides, bends, (n_aux, n_fou,
    n_spi, n_rad, n_tru, n_bnd))."""
    lib = load_library()
    keep, args = [], [None, None]
    if base is not None:
        keep.append(_aux_layout_args(base[0], base[1], np.zeros(n_sky), np.zeros(n_sersic)))
        args = list(keep[-1][1][1:3])
    for name, block in zip(_BLOCKS, (fourier, spiral, radial, truncation) + ((bending,) if bending is not None else ())):
        if block is not None:
            keep.append(_block_args(name, *block))
        args += [None, None, None] if block is None else list(keep[-1][1][1:])
    n_max = 2 * n_sky + (1 + sum(per for per, _ in _BLOCKS.values())) * n_sersic
    const, col = np.full(n_max, np.nan), np.full(n_max, -2, dtype=np.int32)
    kinds, sides = np.full(n_sersic, -2, dtype=np.int32), np.full(n_sersic, -2, dtype=np.int32)
    bends, counts = np.full(n_sersic, -2, dtype=np.int32), np.zeros(5 if bending is None else 6, dtype=np.int32)
    ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    if bending is None:
        rc = lib.psfmc_debug_aux_table_blocks(int(n_sky), int(n_sersic), *(
            args + [_dp(const), ipt(col), ipt(kinds), ipt(sides), ipt(counts)]))
    else:
        rc = lib.psfmc_debug_aux_table_bending(int(n_sky), int(n_sersic), *(
            args + [_dp(const), ipt(col), ipt(kinds), ipt(sides), ipt(bends), ipt(counts)]))
    if rc != 0:
        raise NativeError(rc, lib.psfmc_last_error().decode('utf-8', 'replace'))
    n_aux = int(counts[0])
    out = (const[:n_aux], col[:n_aux], kinds[:n_sersic if counts[3] else 0])
    if bending is not None:
        return out + (sides[:n_sersic if counts[4] else 0], bends[:n_sersic if counts[5] else 0],
                      tuple(int(n) for n in counts))
    if truncation is None:
        return out + (tuple(int(n) for n in counts[:4]),)
    return out + (sides[:n_sersic if counts[4] else 0], tuple(int(n) for n in counts))


def debug_sweep(mode, nbytes, reps=20, device=0):
    """Average microseconds of a plain memory sweep over `nbytes` of scratch ('write', 'read_write',
    'read'): the traffic of the three kernels of a pass without their arithmetic (measurement hook)."""
    lib = load_library()
    us = ctypes.c_double(0.0)
    rc = lib.psfmc_debug_sweep(int(device), {'write': 0, 'read_write': 1, 'read': 2}[mode], int(nbytes), int(reps),
                               ctypes.byref(us))
    if rc != 0:
        raise NativeError(rc, lib.psfmc_last_error().decode('utf-8', 'replace'))
    return us.value


def debug_valu_rate(waves_per_simd=2, iters=20000, device=0):
    """Nanoseconds per fp64 vector wave-instruction per SIMD with every SIMD of the chip busy
    (psfmc_debug_valu_rate): the VALU ceiling of the path on this GPU, measured."""
    lib = load_library()
    out = ctypes.c_double(0.0)
    rc = lib.psfmc_debug_valu_rate(int(device), int(waves_per_simd), int(iters), ctypes.byref(out))
    if rc != 0:
        raise NativeError(rc, lib.psfmc_last_error().decode('utf-8', 'replace'))
    return float(out.value)


class Context(_BlockLayouts):
    """One observed field resident on one GPU (wraps `psfmc_ctx`)."""

    has_ties = False                  # does the registered layout have ties (`set_ties`)?

    IMAGE_KINDS = ('raw_model', 'convolved_model', 'residual', 'composite_ivm',
                   'point_source_subtracted')

    def __init__(self, sci, obs_var, bad_px, psfs, psf_vars, n_ps, n_sersic,
                 max_walkers=4096, device=0, backend='fused'):
        self._lib = load_library()
        self._ctx = None
        sci = _f64(sci)
        obs_var = _f64(obs_var)
        if sci.ndim != 2 or obs_var.shape != sci.shape:
            raise ValueError('sci / obs_var must be 2-D arrays of one shape')
        bad = np.ascontiguousarray(np.asarray(bad_px).astype(bool), dtype=np.uint8)
        psfs = _f64(psfs)
        psf_vars = _f64(psf_vars)
        if psfs.ndim != 3 or psf_vars.shape != psfs.shape:
            raise ValueError('psfs / psf_vars must be [n_psf, py, px]')
        self.shape = sci.shape
        self.n_psf = psfs.shape[0]
        self.n_ps, self.n_sersic = int(n_ps), int(n_sersic)
        self.max_walkers = int(max_walkers)
        self.device = int(device)
        self.backend = backend
        handle = ctypes.c_void_p()
        rc = self._lib.psfmc_ctx_create(
            ctypes.byref(handle), self.device, sci.shape[0], sci.shape[1], _dp(sci),
            _dp(obs_var), bad.ctypes.data_as(_c_u8_p), self.n_psf, psfs.shape[1],
            psfs.shape[2], _dp(psfs), _dp(psf_vars), self.n_ps, self.n_sersic,
            self.max_walkers, BACKENDS[backend] if isinstance(backend, str) else int(backend))
        self._check(rc)
        self._ctx = handle
        self.row_len = self._lib.psfmc_row_len(self._ctx)

    def _check(self, rc):
        if rc != 0:
            raise NativeError(rc, self._lib.psfmc_last_error().decode('utf-8', 'replace'))

    def close(self):
        if self._ctx is not None:
            self._lib.psfmc_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------
    def _rows(self, rows):
        rows = _f64(rows)
        if rows.ndim != 2 or rows.shape[1] != self.row_len:
            raise ValueError('rows must be [W, {}], got {}'.format(self.row_len, rows.shape))
        if rows.shape[0] > self.max_walkers:
            raise ValueError('W={} exceeds max_walkers={}'.format(rows.shape[0], self.max_walkers))
        return rows

    def pass_size(self, n_w):
        """Walkers per internal pass for a batch of n_w (psfmc_pass_size)."""
        rc = self._lib.psfmc_pass_size(self._ctx, int(n_w))
        if rc < 0:
            self._check(rc)
        return rc

    def loglike(self, rows, skip=None, aux=None):
        """[W, row_len] derived rows -> [W] log-likelihoods (NaN/inf preserved;
        skipped walkers -inf).  aux: the walkers' [W, n_aux] auxiliary vectors, for a context with an aux
        layout (`set_aux_layout`)."""
        rows = self._rows(rows)
        n_w = rows.shape[0]
        out = np.empty(n_w, dtype=np.float64)
        if n_w == 0:
            return out
        skip_p = None
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip).astype(bool), dtype=np.uint8)
            if skip.shape != (n_w,):
                raise ValueError('skip must be [W]')
            skip_p = skip.ctypes.data_as(_c_u8_p)
        _send_aux_rows(self._lib, self._ctx, self._check, aux, n_w)
        self._check(self._lib.psfmc_eval_batch(self._ctx, n_w, _dp(rows), skip_p, _dp(out)))
        return out

    def loglike_device(self, n_w, d_rows, d_skip, d_out, stream=None):
        """Enqueue on a HIP stream with raw device pointers (ints); no sync."""
        self._check(self._lib.psfmc_eval_batch_device(
            self._ctx, int(n_w), ctypes.c_void_p(d_rows),
            ctypes.c_void_p(d_skip) if d_skip else None, ctypes.c_void_p(d_out),
            ctypes.c_void_p(stream) if stream else None))

    def images(self, rows, kinds=None, aux=None):
        """dict kind -> [W, ny, nx] for the requested image kinds (aux: as for `loglike`)."""
        rows = self._rows(rows)
        kinds = self.IMAGE_KINDS if kinds is None else tuple(kinds)
        n_w = rows.shape[0]
        bufs, args = {}, []
        for k in self.IMAGE_KINDS:
            if k in kinds:
                bufs[k] = np.empty((n_w,) + self.shape, dtype=np.float64)
                args.append(_dp(bufs[k]))
            else:
                args.append(None)
        unknown = set(kinds) - set(self.IMAGE_KINDS)
        if unknown:
            raise ValueError('unknown image kinds: {}'.format(sorted(unknown)))
        if n_w:
            _send_aux_rows(self._lib, self._ctx, self._check, aux, n_w)
            self._check(self._lib.psfmc_eval_images(self._ctx, n_w, _dp(rows), *args))
        return bufs

    def fisher_rows(self, rows, inv2h, aux=None):
        """Fisher matrix, gradient and base log-likelihood of n_base central-difference stencils
        (psfmc_fisher_rows): rows [n_base, 2K+1, row_len] -- the base, then +h_k, -h_k per differentiated column --
        inv2h [n_base, K] = 1 / (2 h_k), aux [n_base (2K+1), n_aux] as for `loglike` ->
        (F [n_base, K, K], g [n_base, K], lnlike [n_base])."""
        return _fisher_rows(self._lib, self._ctx, self._check, 0, rows, inv2h, self.row_len, self.max_walkers,
                            lambda n_w: _send_aux_rows(self._lib, self._ctx, self._check, aux, n_w))

    # -- raw emcee vectors (device-side priors and derivation) ---------------
    def set_ties(self, src_col, ratio_col, ratio_const, offset_col, offset_const):
        """Ties (psfmc_set_ties; BEFORE `set_layout`, which they take effect with): tie t is
        ratio * theta[src_col[t]] + offset, ratio / offset each a column of theta or -1 and a constant; an entry
        -2 - t of a column table names it.  Empty arrays clear the ties.  A context that never gets the call is what
        it was without it."""
        keep, args = _tie_args(src_col, ratio_col, ratio_const, offset_col, offset_const)
        self._check(self._lib.psfmc_set_ties(self._ctx, 0, *args))
        self.has_ties = args[0] > 0

    def set_layout(self, n_sky, n_params, slot_col, slot_const, ps_method, sersic_degrees,
                   mag_zeropoint, family, p0, p1, p2):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        slot_col, ps_method, sersic_degrees, family = map(i32, (slot_col, ps_method, sersic_degrees,
                                                                family))
        slot_const, p0, p1, p2 = map(_f64, (slot_const, p0, p1, p2))
        self._check(self._lib.psfmc_set_layout(
            self._ctx, int(n_sky), int(n_params), ipt(slot_col), _dp(slot_const), ipt(ps_method),
            ipt(sersic_degrees), float(mag_zeropoint), ipt(family), _dp(p0), _dp(p1), _dp(p2)))
        self.n_params = int(n_params)

    def set_priors(self, family, params):
        """Replace the prior table of the layout (after `set_layout`): family [P] codes of
        include/psfmc_hip.h (0 = host), params [P, <= 4] their scipy.stats arguments in order."""
        fam, tab, fp, tp = _prior_table(family, params)
        self._check(self._lib.psfmc_set_priors(self._ctx, 0, len(fam), fp, tp))

    def set_sersic_integrate(self, flags):
        """Which Sersic components (model-file order) are the pixel-integrated profile
        (psfmc_set_sersic_integrate).  A context that never gets a true flag is what it was without the call."""
        flags = np.ascontiguousarray(np.asarray(flags, dtype=bool), dtype=np.int32)
        self._check(self._lib.psfmc_set_sersic_integrate(
            self._ctx, 0, len(flags), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def set_aux_layout(self, aux_col, aux_const, sky_flags, sersic_flags):
        """Auxiliary parameters (psfmc_set_aux_layout; after `set_layout`): per Sky two slope entries, per Sersic
        one boxiness entry -- column of theta or -1 and a constant -- and which components read them.  A context
        that never gets the call is what it was without it."""
        keep, args = _aux_layout_args(aux_col, aux_const, sky_flags, sersic_flags)
        self._check(self._lib.psfmc_set_aux_layout(self._ctx, 0, *args))

    def _set_block(self, name, tags, col, const):
        keep, args = _block_args(name, tags, col, const)
        self._check(getattr(self._lib, 'psfmc_set_%s_layout' % name)(self._ctx, 0, *args))

    def set_general_mean(self, flags):
        """Which general Sersic slots (model-file order) are rendered as the mean of their law over each pixel
        (psfmc_set_general_mean; after the aux and block layouts, which keep the flags -- a new layout or aux layout
        drops them).  A context that never gets a true flag is what it was without the call."""
        flags = np.ascontiguousarray(np.asarray(flags, dtype=bool), dtype=np.int32)
        self._check(self._lib.psfmc_set_general_mean(
            self._ctx, 0, len(flags), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def _theta(self, theta):
        theta = _f64(theta)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError('theta must be [W, {}], got {}'.format(self.n_params, theta.shape))
        if theta.shape[0] > self.max_walkers:
            raise ValueError('W={} exceeds max_walkers={}'.format(theta.shape[0], self.max_walkers))
        return theta

    def logpost_theta(self, theta, extra_lnprior=None):
        """[W, P] raw parameter vectors -> [W] log-posteriors, all on the device
        (never NaN; outside the priors or non-finite likelihood -> -inf)."""
        theta = self._theta(theta)
        n_w = theta.shape[0]
        out = np.empty(n_w)
        if n_w == 0:
            return out
        extra = None
        if extra_lnprior is not None:
            extra = _f64(extra_lnprior)
            if extra.shape != (n_w,):
                raise ValueError('extra_lnprior must be [W]')
        self._check(self._lib.psfmc_eval_theta(self._ctx, n_w, _dp(theta),
                                               _dp(extra) if extra is not None else None, _dp(out)))
        return out

    def logpost_theta_device(self, n_w, d_theta, d_extra, d_out, stream=None):
        self._check(self._lib.psfmc_eval_theta_device(
            self._ctx, int(n_w), ctypes.c_void_p(d_theta), ctypes.c_void_p(d_extra) if d_extra else None,
            ctypes.c_void_p(d_out), ctypes.c_void_p(stream) if stream else None))

    def debug_theta_rows(self, theta):
        """(rows [W, row_len], lnprior [W], skip [W]) as derived on the device."""
        theta = self._theta(theta)
        n_w = theta.shape[0]
        rows = np.zeros((n_w, self.row_len))
        lnprior = np.zeros(n_w)
        skip = np.zeros(n_w, dtype=np.uint8)
        if n_w:
            self._check(self._lib.psfmc_debug_theta_rows(self._ctx, n_w, _dp(theta), _dp(rows),
                                                         _dp(lnprior), skip.ctypes.data_as(_c_u8_p)))
        return rows, lnprior, skip.astype(bool)

    def stretch_run(self, pos, lnprob, z, lz, partner, log_u, naccepted, store=True,
                    accumulate=False):
        """Run z.shape[0] stretch-move iterations on the device (include/psfmc_hip.h
        psfmc_stretch_run).  pos [W,P], lnprob [W] or None, z/lz/log_u/partner
        [n_iter, 2, W/2], naccepted int64 [W].  Returns (pos, lnprob, chain
        [W,n_iter,P] | None, lnprob_chain [W,n_iter] | None); naccepted is updated."""
        rc, out = _move_run(self._lib.psfmc_stretch_run, self._ctx, pos, lnprob, z, lz, partner, log_u, None,
                            None, naccepted, store, accumulate)
        self._check(rc)
        return out

    def move_run(self, pos, lnprob, scal, lz, partner, log_u, kind, partner_b, naccepted, store=True,
                 accumulate=False):
        """`stretch_run` with the move of every iteration named (include/psfmc_hip.h psfmc_move_run): kind int32
        [n_iter] (MOVE_STRETCH / MOVE_DE), partner_b [n_iter, 2, W/2] the DE moves' second partner; scal is z
        for a stretch iteration and g for a DE one, lz its Hastings term (0 for DE).  Returns what `stretch_run`
        returns."""
        rc, out = _move_run(self._lib.psfmc_move_run, self._ctx, pos, lnprob, scal, lz, partner, log_u, kind,
                            partner_b, naccepted, store, accumulate)
        self._check(rc)
        return out

    def loglike_prior_theta(self, theta, extra_lnprior=None):
        """[W, P] raw parameter vectors -> (lnlike [W], lnprior [W]) as the device computes them
        (psfmc_eval_theta_split): lnlike -inf outside the priors or where it is not finite."""
        theta = self._theta(theta)
        n_w = theta.shape[0]
        ll, lp = np.empty(n_w), np.empty(n_w)
        if n_w == 0:
            return ll, lp
        extra = None
        if extra_lnprior is not None:
            extra = _f64(extra_lnprior)
            if extra.shape != (n_w,):
                raise ValueError('extra_lnprior must be [W]')
        self._check(self._lib.psfmc_eval_theta_split(self._ctx, n_w, _dp(theta),
                                                     _dp(extra) if extra is not None else None, _dp(ll), _dp(lp)))
        return ll, lp

    def pt_run(self, betas, pos, lnlike, lnprior, z, lz, partner, log_u, swap_i, swap_j, swap_log_u,
               naccepted, nswap, store=True, accumulate=False, kind=None, partner_b=None):
        """Run z.shape[0] parallel-tempered iterations on the device (include/psfmc_hip.h psfmc_pt_run).
        betas [T], pos [T,W,P], lnlike / lnprior [T,W] or None (then evaluated first), z/lz/log_u/partner
        [n_iter,2,T,W/2], swap_i/swap_j/swap_log_u [n_iter,T-1,W], naccepted int64 [T,W], nswap int64 [T-1].
        Returns (pos, lnlike, lnprior, chain [T,W,n_iter,P] (every rung, beta = 1 first), lnprob_chain [W,n_iter]
        (beta = 1), lnlike_chain [T,W,n_iter], lnprior_chain [T,W,n_iter]) -- the chains None unless `store`;
        naccepted and nswap are updated."""
        betas = _f64(betas)
        pos = np.array(pos, dtype=np.float64, order='C')
        if pos.ndim != 3 or betas.shape != (pos.shape[0],):
            raise ValueError('pos must be [T, W, P] with betas [T]')
        n_t, n_w, n_p = pos.shape
        if n_p != self.n_params:
            raise ValueError('pos must have {} parameters'.format(self.n_params))
        if n_t * n_w > self.max_walkers:
            raise ValueError('T x W = {} exceeds max_walkers={}'.format(n_t * n_w, self.max_walkers))
        fn = self._lib.psfmc_pt_run if kind is None else self._lib.psfmc_pt_move_run
        rc, out = _pt_run(fn, self._ctx, betas, pos, lnlike, lnprior, z, lz, partner, log_u,
                          swap_i, swap_j, swap_log_u, naccepted, nswap, store, accumulate, kind, partner_b)
        self._check(rc)
        return out

    def pt_move_run(self, betas, pos, lnlike, lnprior, scal, lz, partner, log_u, kind, partner_b, swap_i, swap_j,
                    swap_log_u, naccepted, nswap, store=True, accumulate=False):
        """`pt_run` with the move of every iteration named (include/psfmc_hip.h psfmc_pt_move_run): kind int32
        [n_iter] (MOVE_STRETCH / MOVE_DE, the move of both half-steps of every rung), partner_b
        [n_iter,2,T,W/2] the DE moves' second partner; scal is z for a stretch iteration and g for a DE one, lz
        its Hastings term (0 for DE).  Returns what `pt_run` returns."""
        return self.pt_run(betas, pos, lnlike, lnprior, scal, lz, partner, log_u, swap_i, swap_j, swap_log_u,
                           naccepted, nswap, store=store, accumulate=accumulate, kind=kind, partner_b=partner_b)

    # -- the sampler one half-step at a time (walkers sharded over ranks) -----
    def stretch_open(self, pos, lnprob, z, lz, partner, log_u, naccepted, store=True):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        n_w, n_iter = pos.shape[0], int(np.shape(z)[0])
        lnp = np.ascontiguousarray(lnprob, dtype=np.float64)
        z, lz, log_u = (_f64(a).reshape(n_iter, 2, n_w // 2) for a in (z, lz, log_u))
        partner = np.ascontiguousarray(partner, dtype=np.int32).reshape(n_iter, 2, n_w // 2)
        if naccepted.dtype != np.int64 or naccepted.shape != (n_w,):
            raise ValueError('naccepted must be int64 [W]')
        self._check(self._lib.psfmc_stretch_open(
            self._ctx, n_w, n_iter, _dp(pos), _dp(lnp), _dp(z), _dp(lz),
            partner.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(log_u),
            naccepted.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), int(bool(store))))
        self._stretch_shape = (n_w, n_iter, pos.shape[1], bool(store))

    def stretch_set_moves(self, kind, partner_b):
        """After `stretch_open`, before the first `stretch_half_eval`: the open run proposes by kind
        (psfmc_stretch_set_moves; the arrays `move_run` adds to `stretch_run`'s)."""
        n_w, n_iter = self._stretch_shape[:2]
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(n_iter)
        partner_b = np.ascontiguousarray(partner_b, dtype=np.int32).reshape(n_iter, 2, n_w // 2)
        ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self._check(self._lib.psfmc_stretch_set_moves(self._ctx, ipt(kind), ipt(partner_b)))

    def stretch_half_eval(self, it, h, lo, n, d_out, stream=None):
        self._check(self._lib.psfmc_stretch_half_eval(
            self._ctx, int(it), int(h), int(lo), int(n), ctypes.c_void_p(d_out) if d_out else None,
            ctypes.c_void_p(stream) if stream else None))

    def stretch_half_accept(self, it, h, d_newlnp, stream=None):
        self._check(self._lib.psfmc_stretch_half_accept(
            self._ctx, int(it), int(h), ctypes.c_void_p(d_newlnp), ctypes.c_void_p(stream) if stream else None))

    def stretch_accumulate(self, lo, n, stream=None):
        self._check(self._lib.psfmc_stretch_accumulate(self._ctx, int(lo), int(n),
                                                       ctypes.c_void_p(stream) if stream else None))

    def stretch_close(self, naccepted, stream=None):
        n_w, n_iter, n_p, store = self._stretch_shape
        pos, lnp = np.empty((n_w, n_p)), np.empty(n_w)
        chain = np.empty((n_w, n_iter, n_p)) if store else None
        lnchain = np.empty((n_w, n_iter)) if store else None
        self._check(self._lib.psfmc_stretch_close(
            self._ctx, _dp(pos), _dp(lnp), _dp(chain) if store else None, _dp(lnchain) if store else None,
            naccepted.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
            ctypes.c_void_p(stream) if stream else None))
        return pos, lnp, chain, lnchain

    def accumulated_sums(self):
        """(sums [4, ny, nx], count): the raw posterior-image sums of this context."""
        sums = np.empty((4,) + self.shape)
        count = ctypes.c_longlong(0)
        self._check(self._lib.psfmc_get_accumulated_sums(self._ctx, _dp(sums), ctypes.byref(count)))
        return sums, int(count.value)

    def set_accumulated_sums(self, sums, count):
        sums = _f64(sums)
        if sums.shape != (4,) + self.shape:
            raise ValueError('sums must be [4, ny, nx]')
        self._check(self._lib.psfmc_set_accumulated_sums(self._ctx, _dp(sums), int(count)))

    def accumulate(self, rows, aux=None):
        """Add the five images of every row's walker to the device-resident
        posterior sums (aux: as for `loglike`)."""
        rows = self._rows(rows)
        if len(rows):
            _send_aux_rows(self._lib, self._ctx, self._check, aux, len(rows))
            self._check(self._lib.psfmc_accumulate_images(self._ctx, len(rows), _dp(rows)))

    def accumulate_theta(self, theta):
        """Add the images of [W, P] raw parameter vectors to the device-resident sums (records derived
        on the device)."""
        theta = self._theta(theta)
        if len(theta):
            self._check(self._lib.psfmc_accumulate_theta(self._ctx, len(theta), _dp(theta)))

    def accumulated(self):
        """(dict kind -> mean image, sample count) of the device sums."""
        bufs = {k: np.empty(self.shape, dtype=np.float64) for k in self.IMAGE_KINDS}
        count = ctypes.c_longlong(0)
        self._check(self._lib.psfmc_get_accumulated(
            self._ctx, *[_dp(bufs[k]) for k in self.IMAGE_KINDS], ctypes.byref(count)))
        return bufs, int(count.value)

    def reset_accumulated(self):
        self._check(self._lib.psfmc_reset_accumulated(self._ctx))

    def spectra(self):
        """(psf_spec, var_spec) complex128 [n_psf, ny, nx//2+1] as computed on
        the device (== numpy.fft.rfft2 of the centre-padded images)."""
        shp = (self.n_psf, self.shape[0], self.shape[1] // 2 + 1, 2)
        a = np.empty(shp)
        b = np.empty(shp)
        self._check(self._lib.psfmc_get_spectra(self._ctx, _dp(a), _dp(b)))
        return a[..., 0] + 1j * a[..., 1], b[..., 0] + 1j * b[..., 1]

    def set_option(self, key, value):
        self._check(self._lib.psfmc_set_option(self._ctx, key.encode(), float(value)))

    def get_option(self, key):
        return self._lib.psfmc_get_option(self._ctx, key.encode())


class FieldSetContext(object):
    """Several observed fields resident on one GPU in one context (wraps `psfmc_ctx_create_fields_shaped`):
    their walkers share the batches, so many small ensembles run at the rate of one large one --
    log-posteriors, the device-resident sampler (every field's ensemble stepped together), posterior-image
    sums and per-sample images.  The fields may differ in image and PSF size.  They share one transform
    shape (`get_option('transform_ny' / 'transform_nx')`), and every field costs what a walker of that
    shape costs: a 96 x 96 field in a set with a 256 x 256 one costs a 256 x 256 walker.  Fields of very
    different sizes are cheaper in separate sets.

    fields: sequence of (sci, obs_var, bad_px, psfs [n_psf, py, px], psf_vars), every field with its own
    image and PSF shape and the same number of PSFs.  `shapes[f]` is field f's image shape."""

    def __init__(self, fields, n_ps, n_sersic, max_walkers=4096, device=0):
        self._lib = load_library()
        self._ctx = None
        fields = list(fields)
        if not fields:
            raise ValueError('no field')
        sci, var, bad, psfs, pvar = [], [], [], [], []
        for f, fld in enumerate(fields):
            sci.append(_f64(fld[0]))
            var.append(_f64(fld[1]))
            bad.append(np.ascontiguousarray(np.asarray(fld[2]).astype(bool), dtype=np.uint8))
            psfs.append(_f64(fld[3]))
            pvar.append(_f64(fld[4]))
            if sci[f].ndim != 2 or var[f].shape != sci[f].shape or bad[f].shape != sci[f].shape:
                raise ValueError('field {}: sci / obs_var / bad_px need one 2-D shape'.format(f))
            if psfs[f].ndim != 3 or pvar[f].shape != psfs[f].shape:
                raise ValueError('field {}: psfs / psf_vars need one [n_psf, py, px] shape'.format(f))
            if len(psfs[f]) != len(psfs[0]):
                raise ValueError('field {} has {} PSFs and field 0 has {}: every field of a set needs the same '
                                 'number of PSFs'.format(f, len(psfs[f]), len(psfs[0])))
        self.n_fields, self.n_psf = len(fields), psfs[0].shape[0]
        self.shapes = [tuple(a.shape) for a in sci]
        # the one image shape of a set whose fields all have it; None for a mixed set (see `shapes`)
        self.shape = self.shapes[0] if len(set(self.shapes)) == 1 else None
        self.n_ps, self.n_sersic = int(n_ps), int(n_sersic)
        self.max_walkers, self.device = int(max_walkers), int(device)
        self.n_params = None
        self._tied_fields = set()                     # the fields whose registered layout has ties
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        ny, nx = i32([sh[0] for sh in self.shapes]), i32([sh[1] for sh in self.shapes])
        kn = i32([len(p) for p in psfs])
        py, px = i32([p.shape[1] for p in psfs]), i32([p.shape[2] for p in psfs])
        cat = lambda arrs: np.ascontiguousarray(np.concatenate([a.ravel() for a in arrs]))
        sci, var, bad, psfs, pvar = cat(sci), cat(var), cat(bad), cat(psfs), cat(pvar)
        handle = ctypes.c_void_p()
        rc = self._lib.psfmc_ctx_create_fields_shaped(
            ctypes.byref(handle), self.device, self.n_fields, ipt(ny), ipt(nx), _dp(sci), _dp(var),
            bad.ctypes.data_as(_c_u8_p), ipt(kn), ipt(py), ipt(px), _dp(psfs), _dp(pvar),
            self.n_ps, self.n_sersic, self.max_walkers)
        self._check(rc)
        self._ctx = handle

    def field_shape(self, field):
        """Field `field`'s image shape as the library reports it (the shape of its images and sums)."""
        ny, nx = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.psfmc_field_shape(self._ctx, int(field), ctypes.byref(ny), ctypes.byref(nx)))
        return ny.value, nx.value

    def _check(self, rc):
        if rc != 0:
            raise NativeError(rc, self._lib.psfmc_last_error().decode('utf-8', 'replace'))

    def close(self):
        if self._ctx is not None:
            self._lib.psfmc_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._check(self._lib.psfmc_set_option(self._ctx, key.encode(), float(value)))

    def get_option(self, key):
        return self._lib.psfmc_get_option(self._ctx, key.encode())

    def layout_of(self, field):
        """An object with the `set_layout` of a Context that registers field `field`'s layout."""
        owner = self

        class _Proxy(_BlockLayouts):
            @property
            def has_ties(self):
                return field in owner._tied_fields

            def set_ties(self, src_col, ratio_col, ratio_const, offset_col, offset_const):
                keep, args = _tie_args(src_col, ratio_col, ratio_const, offset_col, offset_const)
                owner._check(owner._lib.psfmc_set_ties(owner._ctx, int(field), *args))
                (owner._tied_fields.add if args[0] else owner._tied_fields.discard)(field)

            def set_layout(self, n_sky, n_params, slot_col, slot_const, ps_method, sersic_degrees,
                           mag_zeropoint, family, p0, p1, p2):
                i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
                ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
                sc, pm, sd, fam = map(i32, (slot_col, ps_method, sersic_degrees, family))
                cst, a0, a1, a2 = map(_f64, (slot_const, p0, p1, p2))
                owner._check(owner._lib.psfmc_set_layout_field(
                    owner._ctx, int(field), int(n_sky), int(n_params), ipt(sc), _dp(cst), ipt(pm), ipt(sd),
                    float(mag_zeropoint), ipt(fam), _dp(a0), _dp(a1), _dp(a2)))
                if owner.n_params not in (None, int(n_params)):
                    raise ValueError('every field must have the same number of free parameters')
                owner.n_params = int(n_params)

            def set_priors(self, family, params):
                fam, tab, fp, tp = _prior_table(family, params)
                owner._check(owner._lib.psfmc_set_priors(owner._ctx, int(field), len(fam), fp, tp))

            def set_sersic_integrate(self, flags):
                flags = np.ascontiguousarray(np.asarray(flags, dtype=bool), dtype=np.int32)
                owner._check(owner._lib.psfmc_set_sersic_integrate(
                    owner._ctx, int(field), len(flags), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

            def set_aux_layout(self, aux_col, aux_const, sky_flags, sersic_flags):
                keep, args = _aux_layout_args(aux_col, aux_const, sky_flags, sersic_flags)
                owner._check(owner._lib.psfmc_set_aux_layout(owner._ctx, int(field), *args))

            def _set_block(self, name, tags, col, const):
                keep, args = _block_args(name, tags, col, const)
                owner._check(getattr(owner._lib, 'psfmc_set_%s_layout' % name)(owner._ctx, int(field), *args))

            def set_general_mean(self, flags):
                flags = np.ascontiguousarray(np.asarray(flags, dtype=bool), dtype=np.int32)
                owner._check(owner._lib.psfmc_set_general_mean(
                    owner._ctx, int(field), len(flags), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return _Proxy()

    @staticmethod
    def _segments(seg_field, seg_count):
        f = np.ascontiguousarray(seg_field, dtype=np.int32)
        n = np.ascontiguousarray(seg_count, dtype=np.int32)
        if f.shape != n.shape or f.ndim != 1:
            raise ValueError('seg_field / seg_count must be 1-D arrays of one length')
        ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        return f, n, ipt(f), ipt(n)

    def logpost_theta(self, thetas):
        """thetas: one [W_f, P] array per field (None or empty to leave a field out) -> list of [W_f]
        log-posteriors (empty arrays for the fields left out)."""
        if len(thetas) != self.n_fields:
            raise ValueError('one parameter array per field')
        parts = [(f, _f64(t)) for f, t in enumerate(thetas) if t is not None and len(t)]
        outs = [np.empty(0) for _ in range(self.n_fields)]
        if not parts:
            return outs
        for _, t in parts:
            if t.ndim != 2 or t.shape[1] != self.n_params:
                raise ValueError('theta must be [W, {}]'.format(self.n_params))
        theta = _f64(np.concatenate([t for _, t in parts]))
        if len(theta) > self.max_walkers:
            raise ValueError('W={} exceeds max_walkers={}'.format(len(theta), self.max_walkers))
        f, n, fp, np_ = self._segments([f for f, _ in parts], [len(t) for _, t in parts])
        out = np.empty(len(theta))
        self._check(self._lib.psfmc_eval_theta_fields(self._ctx, len(f), fp, np_, _dp(theta), None, _dp(out)))
        off = 0
        for fld, t in parts:
            outs[fld] = out[off:off + len(t)].copy()
            off += len(t)
        return outs

    def logpost_theta_device(self, seg_field, seg_count, d_theta, d_out, stream=None):
        f, n, fp, np_ = self._segments(seg_field, seg_count)
        self._check(self._lib.psfmc_eval_theta_device_fields(
            self._ctx, len(f), fp, np_, ctypes.c_void_p(d_theta), None, ctypes.c_void_p(d_out),
            ctypes.c_void_p(stream) if stream else None))

    IMAGE_KINDS = Context.IMAGE_KINDS

    def stretch_run(self, pos, lnprob, z, lz, partner, log_u, naccepted, store=True, accumulate=False):
        """Every field's ensemble stepped together on the device (psfmc_stretch_run_fields).
        pos [F, W, P], lnprob [F, W] or None, z / lz / log_u / partner [F, n_iter, 2, W/2], naccepted
        int64 [F, W] (updated).  Returns (pos, lnprob, chain [F, W, n_iter, P] | None, lnprob_chain
        [F, W, n_iter] | None)."""
        if np.ndim(pos) != 3 or np.shape(pos)[0] != self.n_fields:
            raise ValueError('pos must be [n_fields, W, P]')
        rc, out = _move_run(self._lib.psfmc_stretch_run_fields, self._ctx, pos, lnprob, z, lz, partner, log_u, None,
                            None, naccepted, store, accumulate)
        self._check(rc)
        return out

    # -- every field tempered together (include/psfmc_hip.h psfmc_eval_theta_split_fields, psfmc_pt_run_fields) --
    def eval_split(self, thetas):
        """`logpost_theta` with the two terms apart (psfmc_eval_theta_split_fields): thetas one [W_f, P] array per
        field (None or empty to leave a field out) -> list of (lnlike [W_f], lnprior [W_f]); lnlike -inf outside
        the priors or where it is not finite."""
        if len(thetas) != self.n_fields:
            raise ValueError('one parameter array per field')
        parts = [(f, _f64(t)) for f, t in enumerate(thetas) if t is not None and len(t)]
        outs = [(np.empty(0), np.empty(0)) for _ in range(self.n_fields)]
        if not parts:
            return outs
        for _, t in parts:
            if t.ndim != 2 or t.shape[1] != self.n_params:
                raise ValueError('theta must be [W, {}]'.format(self.n_params))
        theta = _f64(np.concatenate([t for _, t in parts]))
        if len(theta) > self.max_walkers:
            raise ValueError('W={} exceeds max_walkers={}'.format(len(theta), self.max_walkers))
        f, n, fp, np_ = self._segments([f for f, _ in parts], [len(t) for _, t in parts])
        ll, lp = np.empty(len(theta)), np.empty(len(theta))
        self._check(self._lib.psfmc_eval_theta_split_fields(self._ctx, len(f), fp, np_, _dp(theta), None, _dp(ll),
                                                            _dp(lp)))
        off = 0
        for fld, t in parts:
            outs[fld] = (ll[off:off + len(t)].copy(), lp[off:off + len(t)].copy())
            off += len(t)
        return outs

    def pt_run_fields(self, betas, pos, lnlike, lnprior, z, lz, partner, log_u, swap_i, swap_j, swap_log_u,
                      naccepted, nswap, store=True, accumulate=False, kind=None, partner_b=None):
        """`Context.pt_run` for every field's own ladder at once (psfmc_pt_run_fields): betas [T] for all, pos
        [F,T,W,P], lnlike / lnprior [F,T,W] or None, z/lz/log_u/partner [n_iter,2,F,T,W/2], swap_i/swap_j/
        swap_log_u [n_iter,F,T-1,W], naccepted int64 [F,T,W], nswap int64 [F,T-1].  Returns `Context.pt_run`'s
        values with the field in front: (pos, lnlike, lnprior, chain [F,T,W,n_iter,P], lnprob_chain
        [F,W,n_iter], lnlike_chain, lnprior_chain [F,T,W,n_iter]).  F x T x W <= max_walkers (the library checks
        it).  accumulate: field f's posterior sums get its beta = 1 rung's positions after every iteration."""
        betas = _f64(betas)
        pos = np.array(pos, dtype=np.float64, order='C')
        if pos.ndim != 4 or pos.shape[0] != self.n_fields or betas.shape != (pos.shape[1],):
            raise ValueError('pos must be [n_fields, T, W, P] with betas [T]')
        if pos.shape[3] != self.n_params:
            raise ValueError('pos must have {} parameters'.format(self.n_params))
        fn = self._lib.psfmc_pt_run_fields if kind is None else self._lib.psfmc_pt_move_run_fields
        rc, out = _pt_run(fn, self._ctx, betas, pos, lnlike, lnprior, z, lz, partner,
                          log_u, swap_i, swap_j, swap_log_u, naccepted, nswap, store, accumulate, kind, partner_b)
        self._check(rc)
        return out

    def pt_move_run_fields(self, betas, pos, lnlike, lnprior, scal, lz, partner, log_u, kind, partner_b, swap_i,
                           swap_j, swap_log_u, naccepted, nswap, store=True, accumulate=False):
        """`pt_run_fields` with every ladder's move named (psfmc_pt_move_run_fields): kind int32 [n_iter, F],
        partner_b [n_iter,2,F,T,W/2]; scal and lz as `Context.pt_move_run`.  With T = 1 and betas (1,) it is the
        moves run of the set's plain ensembles."""
        return self.pt_run_fields(betas, pos, lnlike, lnprior, scal, lz, partner, log_u, swap_i, swap_j, swap_log_u,
                                  naccepted, nswap, store=store, accumulate=accumulate, kind=kind,
                                  partner_b=partner_b)

    # -- joint fits: one parameter vector per walker for every field (include/psfmc_hip.h psfmc_*_joint) --
    def set_joint_priors(self, family, params):
        """The joint prior table (every field's layout registered first, with n_params joint columns)."""
        fam, tab, fp, tp = _prior_table(family, params)
        self._check(self._lib.psfmc_set_joint_priors(self._ctx, len(fam), fp, tp))

    def logpost_theta_joint(self, theta):
        """[W, n_params] joint vectors -> [W] joint log-posteriors; n_fields x W <= max_walkers."""
        theta = _f64(theta)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError('theta must be [W, {}]'.format(self.n_params))
        out = np.empty(len(theta))
        if len(theta):
            self._check(self._lib.psfmc_eval_theta_joint(self._ctx, len(theta), _dp(theta), _dp(out)))
        return out

    def logpost_theta_joint_device(self, n_w, d_theta, d_out, stream=None):
        self._check(self._lib.psfmc_eval_theta_joint_device(
            self._ctx, int(n_w), ctypes.c_void_p(d_theta), ctypes.c_void_p(d_out),
            ctypes.c_void_p(stream) if stream else None))

    def stretch_run_joint(self, pos, lnprob, z, lz, partner, log_u, naccepted, store=True, accumulate=False):
        """`Context.stretch_run` for ONE ensemble of joint walkers (psfmc_stretch_run_joint): pos [W, P],
        lnprob [W] or None, z / lz / log_u / partner [n_iter, 2, W/2], naccepted int64 [W] (updated).
        accumulate: every field's posterior sums get the positions after every iteration."""
        rc, out = _move_run(self._lib.psfmc_stretch_run_joint, self._ctx, pos, lnprob, z, lz, partner, log_u, None,
                            None, naccepted, store, accumulate)
        self._check(rc)
        return out

    def move_run_joint(self, pos, lnprob, scal, lz, partner, log_u, kind, partner_b, naccepted, store=True,
                       accumulate=False):
        """`Context.move_run` for ONE ensemble of joint walkers (psfmc_move_run_joint)."""
        rc, out = _move_run(self._lib.psfmc_move_run_joint, self._ctx, pos, lnprob, scal, lz, partner, log_u,
                            kind, partner_b, naccepted, store, accumulate)
        self._check(rc)
        return out

    def eval_joint_split(self, theta):
        """[W, n_params] joint vectors -> (lnlike [W], lnprior [W]), the two terms of `logpost_theta_joint`
        apart (psfmc_eval_theta_joint_split): lnlike the fields' sum, -inf where a field's record is skipped
        or the sum is not finite; lnprior the joint log-prior.  n_fields x W <= max_walkers."""
        theta = _f64(theta)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError('theta must be [W, {}]'.format(self.n_params))
        ll, lp = np.empty(len(theta)), np.empty(len(theta))
        if len(theta):
            self._check(self._lib.psfmc_eval_theta_joint_split(self._ctx, len(theta), _dp(theta), _dp(ll), _dp(lp)))
        return ll, lp

    def pt_run_joint(self, betas, pos, lnlike, lnprior, z, lz, partner, log_u, swap_i, swap_j, swap_log_u,
                     naccepted, nswap, store=True, accumulate=False, kind=None, partner_b=None):
        """`Context.pt_run` for T ensembles of joint walkers (psfmc_pt_run_joint): the same arrays and return
        values, P the joint column count; T x W x n_fields <= max_walkers (the library checks it).
        accumulate: every field's posterior sums get the beta = 1 rung's positions after every iteration."""
        betas = _f64(betas)
        pos = np.array(pos, dtype=np.float64, order='C')
        if pos.ndim != 3 or betas.shape != (pos.shape[0],):
            raise ValueError('pos must be [T, W, P] with betas [T]')
        if pos.shape[2] != self.n_params:
            raise ValueError('pos must have {} parameters'.format(self.n_params))
        # (kind, partner_b: psfmc_pt_move_run_joint, `JointView.pt_move_run`)
        fn = self._lib.psfmc_pt_run_joint if kind is None else self._lib.psfmc_pt_move_run_joint
        rc, out = _pt_run(fn, self._ctx, betas, pos, lnlike, lnprior, z, lz, partner,
                          log_u, swap_i, swap_j, swap_log_u, naccepted, nswap, store, accumulate, kind, partner_b)
        self._check(rc)
        return out

    def joint_view(self):
        """The interface a `JointModel` and `DeviceEnsembleSampler` use: `JointView`."""
        return JointView(self)

    def accumulate_theta(self, field, theta):
        """Add the images of [W, P] raw parameter vectors of one field to its posterior sums."""
        theta = _f64(theta)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError('theta must be [W, {}]'.format(self.n_params))
        for lo in range(0, len(theta), self.max_walkers):
            part = _f64(theta[lo:lo + self.max_walkers])
            self._check(self._lib.psfmc_accumulate_theta_field(self._ctx, int(field), len(part), _dp(part)))

    def accumulated(self, field):
        """(dict kind -> mean image, sample count) of one field's posterior sums, at the field's own shape."""
        bufs = {k: np.empty(self.shapes[field], dtype=np.float64) for k in self.IMAGE_KINDS}
        count = ctypes.c_longlong(0)
        self._check(self._lib.psfmc_get_accumulated_field(
            self._ctx, int(field), *[_dp(bufs[k]) for k in self.IMAGE_KINDS], ctypes.byref(count)))
        return bufs, int(count.value)

    def reset_accumulated(self, field=None):
        """Clear the posterior sums of one field, or (None) of every field."""
        if field is None:
            self._check(self._lib.psfmc_reset_accumulated(self._ctx))
        else:
            self._check(self._lib.psfmc_reset_accumulated_field(self._ctx, int(field)))

    def view(self, field, columns=None):
        """The part of `Context`'s interface a `MultiComponentModel` uses, for ONE field of this context.
        columns (joint fits): the joint column of each of the field's own columns -- the view takes the
        field's own vectors and places them there."""
        return FieldView(self, field, columns)

    def _aux_width(self):
        """Values per walker of the context's auxiliary vectors, as the library keeps it (0: no field has an aux
        layout yet): a field's shorter rows are padded to it."""
        return int(self.get_option('aux_stride'))

    def _field_aux(self, aux, n_w):
        """The auxiliary rows of a row-based call of one field: the field's own, or -- for a field WITHOUT the keywords
        in a context where another field has them, whose model has no auxiliary vectors (`aux_rows` is None) -- zero
        rows of the context's width: the library wants rows for every row-based call of such a context, and nothing
        reads them for a field whose flags are all clear."""
        if aux is None and self._aux_width():
            return np.zeros((n_w, self._aux_width()))
        return aux

    def loglike(self, field, rows, skip=None, aux=None):
        """[W] log-likelihoods of derived rows of one field (`Context.loglike` for a field of this context)."""
        rows = _f64(rows)
        n_w = rows.shape[0]
        if n_w > self.max_walkers:
            raise ValueError('W={} exceeds max_walkers={}'.format(n_w, self.max_walkers))
        out = np.empty(n_w, dtype=np.float64)
        skip_p = None
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip).astype(bool), dtype=np.uint8)
            skip_p = skip.ctypes.data_as(_c_u8_p)
        if n_w:
            _send_aux_rows(self._lib, self._ctx, self._check, self._field_aux(aux, n_w), n_w,
                           self._aux_width())
            self._check(self._lib.psfmc_eval_batch_field(self._ctx, int(field), n_w, _dp(rows), skip_p, _dp(out)))
        return out

    def images(self, field, rows, kinds=None, aux=None):
        """dict kind -> [W, ny, nx] of the requested per-sample images for derived rows of one field."""
        rows = _f64(rows)
        kinds = self.IMAGE_KINDS if kinds is None else tuple(kinds)
        n_w = rows.shape[0]
        bufs, args = {}, []
        for k in self.IMAGE_KINDS:
            if k in kinds:
                bufs[k] = np.empty((n_w,) + tuple(self.shapes[field]), dtype=np.float64)
                args.append(_dp(bufs[k]))
            else:
                args.append(None)
        if n_w:
            _send_aux_rows(self._lib, self._ctx, self._check, self._field_aux(aux, n_w), n_w,
                           self._aux_width())
            self._check(self._lib.psfmc_eval_images_field(self._ctx, int(field), n_w, _dp(rows), *args))
        return bufs

    def fisher_rows(self, field, rows, inv2h, aux=None):
        """`Context.fisher_rows` for stencils of one field of this context."""
        return _fisher_rows(self._lib, self._ctx, self._check, field, rows, inv2h,
                            self._lib.psfmc_row_len(self._ctx), self.max_walkers,
                            lambda n_w: _send_aux_rows(self._lib, self._ctx, self._check, self._field_aux(aux, n_w),
                                                       n_w, self._aux_width()))

    def _stencil_rows(self, rows, inv2h, lead):
        """The checked arrays of a several-stencil Fisher call: rows [*lead, 2K+1, row_len], inv2h [*lead, K] -> (rows,
        inv2h, K); the walkers must fit max_walkers."""
        rows, inv2h = _f64(rows), _f64(inv2h)
        row_len = self._lib.psfmc_row_len(self._ctx)
        if rows.ndim != len(lead) + 2 or rows.shape[:len(lead)] != tuple(lead) or rows.shape[-1] != row_len:
            raise ValueError('rows must be [{}, 2K+1, {}], got {}'.format(
                ', '.join(str(n) for n in lead), row_len, rows.shape))
        n_st = rows.shape[-2]
        k = (n_st - 1) // 2
        if min(lead) < 1 or k < 1 or n_st != 2 * k + 1 or inv2h.shape != tuple(lead) + (k,):
            raise ValueError('rows [..., 2K+1, row_len] need inv2h [..., K] with K >= 1; got {} and {}'.format(
                rows.shape, inv2h.shape))
        if k > FISHER_MAX_COLUMNS:
            raise ValueError('K={} differentiated columns of a field exceed {}'.format(k, FISHER_MAX_COLUMNS))
        n_w = int(np.prod(lead)) * n_st
        if n_w > self.max_walkers:
            raise ValueError('{} stencils of {} walkers exceed max_walkers={}'.format(
                int(np.prod(lead)), n_st, self.max_walkers))
        return rows, inv2h, k

    def fisher_rows_fields(self, fields, rows, inv2h, aux=None):
        """Stencils of several fields in ONE call (psfmc_fisher_rows_fields): fields [n] the stencils' fields (any
        order, repeats allowed), rows [n, 2K+1, row_len], inv2h [n, K], aux [n (2K+1), n_aux] or None ->
        (F [n, K, K], g [n, K], lnlike [n]); stencil s's values are the bits `fisher_rows(fields[s], ...)` gives for
        it alone."""
        fields = np.ascontiguousarray(fields, dtype=np.int32)
        if fields.ndim != 1 or len(fields) < 1 or fields.min() < 0 or fields.max() >= self.n_fields:
            raise ValueError('fields must be a non-empty list of fields of the context')
        n = len(fields)
        rows, inv2h, k = self._stencil_rows(rows, inv2h, (n,))
        f_out, g_out, ll = np.empty((n, k, k)), np.empty((n, k)), np.empty(n)
        n_w = n * (2 * k + 1)
        _send_aux_rows(self._lib, self._ctx, self._check, self._field_aux(aux, n_w), n_w, self._aux_width())
        self._check(self._lib.psfmc_fisher_rows_fields(
            self._ctx, n, k, fields.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(rows), _dp(inv2h), _dp(f_out),
            _dp(g_out), _dp(ll)))
        return f_out, g_out, ll

    def fisher_rows_joint(self, col_of, rows, inv2h, k_joint, aux=None):
        """Fisher matrix and gradient of a joint fit (psfmc_fisher_rows_joint): col_of [n_fields, K_field] the joint
        column of each field's differentiated columns, rows [n_base, n_fields, 2 K_field + 1, row_len], inv2h
        [n_base, n_fields, K_field], aux [n_base n_fields (2 K_field + 1), n_aux] or None ->
        (F [n_base, k_joint, k_joint], g [n_base, k_joint], lnlike [n_base])."""
        col_of = np.ascontiguousarray(col_of, dtype=np.int32)
        if col_of.ndim != 2 or col_of.shape[0] != self.n_fields:
            raise ValueError('col_of must be [{}, K_field], got {}'.format(self.n_fields, col_of.shape))
        k_joint = int(k_joint)
        n_base = np.shape(rows)[0] if np.ndim(rows) else 0
        rows, inv2h, k = self._stencil_rows(rows, inv2h, (n_base, self.n_fields))
        if col_of.shape[1] != k or k_joint < k:
            raise ValueError('col_of [n_fields, {}] must name K_field = {} of {} joint columns'.format(
                col_of.shape[1], k, k_joint))
        f_out, g_out, ll = np.empty((n_base, k_joint, k_joint)), np.empty((n_base, k_joint)), np.empty(n_base)
        n_w = n_base * self.n_fields * (2 * k + 1)
        _send_aux_rows(self._lib, self._ctx, self._check, self._field_aux(aux, n_w), n_w, self._aux_width())
        self._check(self._lib.psfmc_fisher_rows_joint(
            self._ctx, n_base, k_joint, k, col_of.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(rows), _dp(inv2h),
            _dp(f_out), _dp(g_out), _dp(ll)))
        return f_out, g_out, ll


class FieldView(object):
    """One field of a `FieldSetContext` behind the interface of a one-field `Context`, so that a
    `MultiComponentModel` of a `FieldSet` (images, posterior sums, log-posteriors) works on the shared
    context instead of creating its own."""

    IMAGE_KINDS = Context.IMAGE_KINDS

    def __init__(self, owner, field, columns=None):
        self.owner, self.field = owner, int(field)
        self.shape, self.n_psf = tuple(owner.shapes[self.field]), owner.n_psf
        self.max_walkers, self.device = owner.max_walkers, owner.device
        self.columns = None if columns is None else np.asarray(columns, dtype=np.int64)

    def _own_to_layout(self, theta):
        """The field's own [W, P_f] vectors as the [W, n_params] vectors its layout reads."""
        if self.columns is None:
            return theta
        theta = _f64(theta)
        full = np.zeros((theta.shape[0], self.owner.n_params))
        full[:, self.columns] = theta
        return full

    def close(self):                       # the FieldSet owns the context
        pass

    def set_option(self, key, value):
        self.owner.set_option(key, value)

    def get_option(self, key):
        return self.owner.get_option(key)

    def logpost_theta(self, theta, extra_lnprior=None):
        if self.columns is not None:
            raise NotImplementedError('field {} is part of a joint fit: its log-posterior is the JointModel\'s '
                                      '(log_posterior_batch)'.format(self.field))
        if extra_lnprior is not None:
            raise ValueError('a FieldSet evaluates priors on the GPU only')
        thetas = [None] * self.owner.n_fields
        thetas[self.field] = theta
        return self.owner.logpost_theta(thetas)[self.field]

    def loglike_prior_theta(self, theta, extra_lnprior=None):
        if self.columns is not None:
            raise NotImplementedError('field {} is part of a joint fit: its likelihood and prior are the '
                                      'JointModel\'s (log_likelihood_and_prior_batch)'.format(self.field))
        if extra_lnprior is not None:
            raise ValueError('a FieldSet evaluates priors on the GPU only')
        thetas = [None] * self.owner.n_fields
        thetas[self.field] = theta
        return self.owner.eval_split(thetas)[self.field]

    def images(self, rows, kinds=None, aux=None):
        return self.owner.images(self.field, rows, kinds, aux=aux)

    def loglike(self, rows, skip=None, aux=None):
        return self.owner.loglike(self.field, rows, skip, aux=aux)

    def fisher_rows(self, rows, inv2h, aux=None):
        return self.owner.fisher_rows(self.field, rows, inv2h, aux=aux)

    def __getattr__(self, name):
        # the rest of Context's interface (device-resident sampler, raw-sum exchange, device pointers, ...) has
        # no per-field form on a shared context: say so instead of an AttributeError deep inside a caller
        if callable(getattr(Context, name, None)):
            field = self.__dict__.get('field')

            def _unsupported(*args, **kwargs):
                raise NotImplementedError(
                    "'{}' is not available for field {} of a FieldSet (its context is shared by the set's "
                    "fields): use FieldSet / FieldSetSampler / fitting.model_fields_mcmc, or a "
                    "MultiComponentModel with a context of its own".format(name, field))
            return _unsupported
        raise AttributeError(name)

    def accumulate_theta(self, theta):
        self.owner.accumulate_theta(self.field, self._own_to_layout(theta))

    def accumulated(self):
        return self.owner.accumulated(self.field)

    def reset_accumulated(self):
        self.owner.reset_accumulated(self.field)


class JointView(object):
    """A `FieldSetContext` whose fields are fitted jointly (`models.JointModel`), behind the part of a
    one-field `Context`'s interface that `DeviceEnsembleSampler` uses: `stretch_run` is the joint run
    (psfmc_stretch_run_joint), `logpost_theta` the joint log-posterior; and of the part that
    `DeviceTemperedSampler` uses: `pt_run` (psfmc_pt_run_joint) and `loglike_prior_theta`."""

    IMAGE_KINDS = Context.IMAGE_KINDS

    def __init__(self, owner):
        self.owner = owner
        self.max_walkers, self.device = owner.max_walkers, owner.device

    def close(self):                       # the JointModel owns the context
        pass

    def set_option(self, key, value):
        self.owner.set_option(key, value)

    def get_option(self, key):
        return self.owner.get_option(key)

    def logpost_theta(self, theta, extra_lnprior=None):
        if extra_lnprior is not None:
            raise ValueError('a joint fit evaluates priors on the GPU only')
        return self.owner.logpost_theta_joint(theta)

    def stretch_run(self, pos, lnprob, z, lz, partner, log_u, naccepted, store=True, accumulate=False):
        return self.owner.stretch_run_joint(pos, lnprob, z, lz, partner, log_u, naccepted, store=store,
                                            accumulate=accumulate)

    def move_run(self, pos, lnprob, scal, lz, partner, log_u, kind, partner_b, naccepted, store=True,
                 accumulate=False):
        return self.owner.move_run_joint(pos, lnprob, scal, lz, partner, log_u, kind, partner_b, naccepted,
                                         store=store, accumulate=accumulate)

    def loglike_prior_theta(self, theta, extra_lnprior=None):
        if extra_lnprior is not None:
            raise ValueError('a joint fit evaluates priors on the GPU only')
        return self.owner.eval_joint_split(theta)

    def pt_run(self, betas, pos, lnlike, lnprior, z, lz, partner, log_u, swap_i, swap_j, swap_log_u,
               naccepted, nswap, store=True, accumulate=False):
        return self.owner.pt_run_joint(betas, pos, lnlike, lnprior, z, lz, partner, log_u, swap_i, swap_j,
                                       swap_log_u, naccepted, nswap, store=store, accumulate=accumulate)

    def pt_move_run(self, betas, pos, lnlike, lnprior, scal, lz, partner, log_u, kind, partner_b, swap_i, swap_j,
                    swap_log_u, naccepted, nswap, store=True, accumulate=False):
        return self.owner.pt_run_joint(betas, pos, lnlike, lnprior, scal, lz, partner, log_u, swap_i, swap_j,
                                       swap_log_u, naccepted, nswap, store=store, accumulate=accumulate, kind=kind,
                                       partner_b=partner_b)

    def fisher_rows(self, col_of, rows, inv2h, k_joint, aux=None):
        """`FieldSetContext.fisher_rows_joint`: the joint fit's Fisher matrix, gradient and log-likelihood."""
        return self.owner.fisher_rows_joint(col_of, rows, inv2h, k_joint, aux=aux)

    def accumulated(self, field):
        return self.owner.accumulated(field)

    def reset_accumulated(self, field=None):
        self.owner.reset_accumulated(field)

    def __getattr__(self, name):
        # the half-step API of sharded runs and the one-field raw-sum exchange have no joint form
        if callable(getattr(Context, name, None)):
            def _unsupported(*args, **kwargs):
                raise NotImplementedError(
                    "'{}' is not available for a joint fit: it runs on one GPU (no sharding over ranks) "
                    "and its images are per field (JointModel.field_models)".format(name))
            return _unsupported
        raise AttributeError(name)


class ContextGroup(_BlockLayouts):
    """One observed field replicated on several GPUs driven by THIS process (wraps
    `psfmc_group`): walkers are split into contiguous blocks, one per listed device.
    The one-process-per-GPU form (torch.distributed / RCCL) is `psfmc_amd.parallel`."""

    has_ties = False                  # as `Context.has_ties`

    def __init__(self, devices, sci, obs_var, bad_px, psfs, psf_vars, n_ps, n_sersic,
                 max_walkers=4096, backend='fused'):
        self._lib = load_library()
        self._grp = None
        sci, obs_var = _f64(sci), _f64(obs_var)
        bad = np.ascontiguousarray(np.asarray(bad_px).astype(bool), dtype=np.uint8)
        psfs, psf_vars = _f64(psfs), _f64(psf_vars)
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        handle = ctypes.c_void_p()
        rc = self._lib.psfmc_group_create(
            ctypes.byref(handle), len(devs), devs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            sci.shape[0], sci.shape[1], _dp(sci), _dp(obs_var), bad.ctypes.data_as(_c_u8_p),
            psfs.shape[0], psfs.shape[1], psfs.shape[2], _dp(psfs), _dp(psf_vars), int(n_ps),
            int(n_sersic), int(max_walkers), BACKENDS[backend] if isinstance(backend, str) else int(backend))
        self._check(rc)
        self._grp = handle
        self.devices = [int(d) for d in devs]
        self.max_walkers = int(max_walkers)
        self.row_len = ROW_SKY + ROW_PS * int(n_ps) + ROW_SERSIC * int(n_sersic) + 1
        self.n_params = None

    def _check(self, rc):
        if rc != 0:
            raise NativeError(rc, self._lib.psfmc_last_error().decode('utf-8', 'replace'))

    def close(self):
        if self._grp is not None:
            self._lib.psfmc_group_destroy(self._grp)
            self._grp = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_layout(self, n_sky, n_params, slot_col, slot_const, ps_method, sersic_degrees,
                   mag_zeropoint, family, p0, p1, p2):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        ipt = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        slot_col, ps_method, sersic_degrees, family = map(i32, (slot_col, ps_method, sersic_degrees, family))
        slot_const, p0, p1, p2 = map(_f64, (slot_const, p0, p1, p2))
        self._check(self._lib.psfmc_group_set_layout(
            self._grp, int(n_sky), int(n_params), ipt(slot_col), _dp(slot_const), ipt(ps_method),
            ipt(sersic_degrees), float(mag_zeropoint), ipt(family), _dp(p0), _dp(p1), _dp(p2)))
        self.n_params = int(n_params)

    def set_ties(self, src_col, ratio_col, ratio_const, offset_col, offset_const):
        """`Context.set_ties` on every device of the group."""
        keep, args = _tie_args(src_col, ratio_col, ratio_const, offset_col, offset_const)
        self._check(self._lib.psfmc_group_set_ties(self._grp, *args))
        self.has_ties = args[0] > 0

    def set_priors(self, family, params):
        """`Context.set_priors` on every device of the group."""
        fam, tab, fp, tp = _prior_table(family, params)
        self._check(self._lib.psfmc_group_set_priors(self._grp, len(fam), fp, tp))

    def set_sersic_integrate(self, flags):
        """`Context.set_sersic_integrate` on every device of the group."""
        flags = np.ascontiguousarray(np.asarray(flags, dtype=bool), dtype=np.int32)
        self._check(self._lib.psfmc_group_set_sersic_integrate(
            self._grp, len(flags), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def set_aux_layout(self, aux_col, aux_const, sky_flags, sersic_flags):
        """`Context.set_aux_layout` on every device of the group."""
        keep, args = _aux_layout_args(aux_col, aux_const, sky_flags, sersic_flags)
        self._check(self._lib.psfmc_group_set_aux_layout(self._grp, *args))

    def _set_block(self, name, tags, col, const):
        """The block's layout call (`_BlockLayouts`) on every device of the group."""
        keep, args = _block_args(name, tags, col, const)
        self._check(getattr(self._lib, 'psfmc_group_set_%s_layout' % name)(self._grp, *args))

    def set_general_mean(self, flags):
        """`Context.set_general_mean` on every device of the group."""
        flags = np.ascontiguousarray(np.asarray(flags, dtype=bool), dtype=np.int32)
        self._check(self._lib.psfmc_group_set_general_mean(
            self._grp, len(flags), flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def loglike(self, rows, skip=None, aux=None):
        if aux is not None:
            raise NotImplementedError('derived rows of a model with a Sky `slope` or a Sersic `boxiness`, `fourier` or `spiral` are not '
                                      'split over a ContextGroup: use logpost_theta (raw vectors)')
        rows = _f64(rows)
        if rows.ndim != 2 or rows.shape[1] != self.row_len:
            raise ValueError('rows must be [W, {}]'.format(self.row_len))
        out = np.empty(rows.shape[0])
        skip_p = None
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip).astype(bool), dtype=np.uint8)
            skip_p = skip.ctypes.data_as(_c_u8_p)
        if len(rows):
            self._check(self._lib.psfmc_group_eval_batch(self._grp, len(rows), _dp(rows), skip_p, _dp(out)))
        return out

    def logpost_theta(self, theta, extra_lnprior=None):
        theta = _f64(theta)
        if theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError('theta must be [W, {}]'.format(self.n_params))
        out = np.empty(theta.shape[0])
        extra = _f64(extra_lnprior) if extra_lnprior is not None else None
        if len(theta):
            self._check(self._lib.psfmc_group_eval_theta(self._grp, len(theta), _dp(theta),
                                                         _dp(extra) if extra is not None else None, _dp(out)))
        return out
