"""CPU-only checks of the host-side argument checks of the UNet glue kernels (vaw_conv3x3_wgrad_small, vaw_subsample2,
vaw_rowvec_add, vaw_rowvec_sum): a bad call returns VAW_ERR_INVALID and sets the message, nothing is launched.  The kernels
themselves are checked on the GPU in test_gpu_unet_glue.py."""
import ctypes as C

import vaw_amd
from vaw_amd import _lib as L


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, (C.addressof(buf) + 15) // 16 * 16


def _refused(rc, prefix):
    assert rc == -1
    assert vaw_amd.lib().vaw_last_error_string().decode().startswith(prefix)


def test_entry_points_are_exported_with_their_signatures():
    names = vaw_amd.exported_symbols()
    lib = vaw_amd.lib()
    _i, _p, _l, _f = C.c_int, C.c_void_p, C.c_int64, C.c_float
    want = {"vaw_conv3x3_wgrad_small": [_i, _p, _p, _p, _f, _i, _i, _i, _i, _i, _p, _l, _p],
            "vaw_subsample2": [_i, _p, _p, _i, _i, _i, _i, _i, _p],
            "vaw_rowvec_add": [_i, _p, _p, _l, _i, _i, _i, _p],
            "vaw_rowvec_sum": [_i, _p, _p, _l, _i, _i, _i, _f, _p]}
    for name, args in want.items():
        assert name in names and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is _i
    assert "vaw_conv3x3_wgrad_small_workspace_floats" in names


def test_wgrad_small_workspace_floats():
    """One slab of 9 * Ci * Co floats per chunk of 256 pixels, the last chunk ragged."""
    f = vaw_amd.lib().vaw_conv3x3_wgrad_small_workspace_floats
    assert f(3, 5, 7, 3, 64) == 1 * 9 * 3 * 64                 # M = 105
    assert f(1, 16, 16, 3, 8) == 1 * 9 * 3 * 8                 # M = 256: exactly one chunk
    assert f(1, 257, 1, 3, 8) == 2 * 9 * 3 * 8                 # M = 257
    assert f(2, 19, 21, 264, 3) == 4 * 9 * 264 * 3             # M = 798
    assert f(5, 24, 20, 1, 8) == 10 * 9 * 1 * 8                # M = 2400
    assert f(128, 64, 64, 3, 192) == 2048 * 9 * 3 * 192        # the benchmark's stem


def test_wgrad_small_refusals():
    lib = vaw_amd.lib()
    keep, a = _aligned(256)
    B, H, W = 2, 6, 6
    for dt in (L.F32, L.BF16):
        need = lib.vaw_conv3x3_wgrad_small_workspace_floats(B, H, W, 8, 8)
        _refused(lib.vaw_conv3x3_wgrad_small(dt, a, a, a, 0.0, B, H, W, 8, 8, a, need, None), "conv3x3_wgrad_small:")   # neither side <= 4
        for Ci, Co in ((3, 64), (64, 3), (4, 2)):
            need = lib.vaw_conv3x3_wgrad_small_workspace_floats(B, H, W, Ci, Co)
            assert need == 9 * Ci * Co
            _refused(lib.vaw_conv3x3_wgrad_small(dt, a, a, a, 0.0, B, H, W, Ci, Co, a, need - 1, None), "conv3x3_wgrad_small: workspace")
            _refused(lib.vaw_conv3x3_wgrad_small(dt, a, a, a, 0.0, B, H, W, Ci, Co, None, need, None), "conv3x3_wgrad_small: workspace")
        _refused(lib.vaw_conv3x3_wgrad_small(dt, a, a, a, 0.0, 0, H, W, 3, 8, a, 1 << 20, None), "conv3x3_wgrad_small:")
    del keep


def test_subsample2_and_rowvec_refusals():
    lib = vaw_amd.lib()
    keep, a = _aligned(256)
    for dt in (L.F32, L.BF16):
        for mode in (0, 1):
            for C_ in (2, 6, 35):                                                           # C % 4 != 0
                _refused(lib.vaw_subsample2(dt, a, a, 1, 2, 2, C_, mode, None), "subsample2:")
        _refused(lib.vaw_subsample2(dt, a, a, 1, 3, 4, 4, 1, None), "subsample2:")          # odd Ho in the transpose
        _refused(lib.vaw_subsample2(dt, a, a, 1, 4, 3, 4, 1, None), "subsample2:")          # odd Wo in the transpose
        _refused(lib.vaw_subsample2(dt, a, a, 1, 2, 2, 4, 2, None), "subsample2:")          # no such mode
        _refused(lib.vaw_subsample2(dt, None, a, 1, 2, 2, 4, 0, None), "subsample2:")
        _refused(lib.vaw_subsample2(dt, a, None, 1, 2, 2, 4, 0, None), "subsample2:")

        for C_ in (2, 6, 35):
            _refused(lib.vaw_rowvec_add(dt, a, a, 64, 1, 2, C_, None), "rowvec_add:")       # C % 4 != 0
        for ld in (6, 13, 66):
            _refused(lib.vaw_rowvec_add(dt, a, a, ld, 1, 2, 4, None), "rowvec_add:")        # ld % 4 != 0
        for off in (4, 8, 12):
            _refused(lib.vaw_rowvec_add(dt, a, a + off, 64, 1, 2, 4, None), "rowvec_add:")  # e off the 16-byte grid
        _refused(lib.vaw_rowvec_add(dt, None, a, 64, 1, 2, 4, None), "rowvec_add:")
        _refused(lib.vaw_rowvec_add(dt, a, None, 64, 1, 2, 4, None), "rowvec_add:")
        _refused(lib.vaw_rowvec_add(dt, a, a, 64, 0, 2, 4, None), "rowvec_add:")

        for B in (65536, 65537, 1 << 20):                                                   # B rides in gridDim.y
            _refused(lib.vaw_rowvec_sum(dt, a, a, 64, B, 2, 4, 0.0, None), "rowvec_sum:")
        _refused(lib.vaw_rowvec_sum(dt, None, a, 64, 1, 2, 4, 0.0, None), "rowvec_sum:")
        _refused(lib.vaw_rowvec_sum(dt, a, None, 64, 1, 2, 4, 0.0, None), "rowvec_sum:")
        _refused(lib.vaw_rowvec_sum(dt, a, a, 64, 1, 0, 4, 0.0, None), "rowvec_sum:")
    del keep
