"""CPU-only checks of the UNet's activation-recomputation surface (use_checkpoint / activation_checkpointing) and of the host-side
argument checks of the entry points it adds (vaw_groupnorm_apply, vaw_dropout_pack, vaw_dropout_bits_fwd / _bwd): a bad call
returns the status and sets the message, nothing is launched."""
import ctypes as C
import inspect

import pytest
import torch

import vaw_amd
from vaw_amd import _lib as L

from conftest import base_args

KW = dict(image_size=16, num_channels=32, num_res_blocks=1, channel_mult="1,2", attention_resolutions="8", num_heads=2)


def test_flag_surface():
    m = vaw_amd.create_unet_model(**KW)
    assert m.activation_checkpointing is False and m.use_checkpoint is False               # the default stays off
    m = vaw_amd.create_unet_model(**KW, use_checkpoint=True)
    assert m.activation_checkpointing is True and m.use_checkpoint is True
    m.set_activation_checkpointing(False)
    assert m.activation_checkpointing is False and m.use_checkpoint is False
    m.set_activation_checkpointing(1)
    assert m.activation_checkpointing is True
    u = vaw_amd.UNetModel(16, 3, 32, 3, 1, attention_resolutions=(2,), channel_mult=(1, 2), use_checkpoint=True)
    assert u.activation_checkpointing is True
    assert vaw_amd.UNetModel(16, 3, 32, 3, 1, attention_resolutions=(2,), channel_mult=(1, 2)).activation_checkpointing is False
    assert inspect.signature(vaw_amd.UNetModel.__init__).parameters["use_checkpoint"].default is False
    # every preset factory hands the keyword on
    assert vaw_amd.UNet_32(use_checkpoint=True).activation_checkpointing is True
    assert vaw_amd.UNet_32().activation_checkpointing is False
    # the flag is no parameter and no buffer: state_dict keys are those of the reference
    assert set(u.state_dict()) == set(vaw_amd.UNetModel(16, 3, 32, 3, 1, attention_resolutions=(2,), channel_mult=(1, 2)).state_dict())


def test_trainer_applies_the_args_field_to_the_unet():
    class Wrap(torch.nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module

    def trainer(model, **extra):
        args = base_args(image_size=16, **extra)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: 1.0)
        return vaw_amd.Trainer(args, torch.device("cpu"), model, None, opt, sched, None, [])

    m = vaw_amd.create_unet_model(**KW, class_cond=False)
    trainer(Wrap(m), activation_checkpointing=True)
    assert m.activation_checkpointing is True
    trainer(m)                                           # no such field: the model stays as it is
    assert m.activation_checkpointing is True
    trainer(m, activation_checkpointing=False)
    assert m.activation_checkpointing is False and m.use_checkpoint is False


def test_new_entry_points_are_exported_with_their_signatures():
    names = vaw_amd.exported_symbols()
    lib = vaw_amd.lib()
    _i, _p, _l, _f = C.c_int, C.c_void_p, C.c_int64, C.c_float
    want = {"vaw_groupnorm_apply": [_i, _p, _p, _p, _p, _p, _p, _p, _l, _i, _p, _i, _i, _i, _i, _p],
            "vaw_dropout_pack": [_i, _p, _p, _l, _i, _p],
            "vaw_dropout_bits_fwd": [_i, _p, _p, _f, _p, _l, _p],
            "vaw_dropout_bits_bwd": [_i, _p, _p, _f, _p, _l, _p]}
    for name, args in want.items():
        assert name in names and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is _i
    assert "vaw_dropout_bits_words" in names
    assert [lib.vaw_dropout_bits_words(n) for n in (0, 8, 32, 40, 264, 1 << 20)] == [0, 1, 1, 2, 9, 1 << 15]


def _aligned(nbytes):
    buf = C.create_string_buffer(nbytes + 16)
    return buf, (C.addressof(buf) + 15) // 16 * 16


def test_argument_checks_return_the_status():
    """Bad arguments: VAW_ERR_INVALID (-1) and a message that names the entry point, before anything is launched (no GPU here)."""
    lib = vaw_amd.lib()
    keep, a = _aligned(256)

    def refused(rc, prefix):
        assert rc == -1
        assert lib.vaw_last_error_string().decode().startswith(prefix)

    for dt in (L.F32, L.BF16):
        refused(lib.vaw_dropout_pack(dt, None, a, 4, 8, None), "dropout_pack:")
        refused(lib.vaw_dropout_pack(dt, a, None, 4, 8, None), "dropout_pack:")
        for C_ in (4, 12, 0, -8):                                      # the packer wants whole mask bytes per pixel row
            refused(lib.vaw_dropout_pack(dt, a, a, 4, C_, None), "dropout_pack:")
        refused(lib.vaw_dropout_pack(dt, a, a, 0, 8, None), "dropout_pack:")
        refused(lib.vaw_dropout_pack(dt, a + 2, a, 4, 8, None), "dropout_pack:")
        for fn, name in ((lib.vaw_dropout_bits_fwd, "dropout_bits_fwd:"), (lib.vaw_dropout_bits_bwd, "dropout_bits_bwd:")):
            refused(fn(dt, None, a, 2.0, a, 8, None), name)
            refused(fn(dt, a, None, 2.0, a, 8, None), name)
            refused(fn(dt, a, a, 2.0, None, 8, None), name)
            refused(fn(dt, a, a, 2.0, a, 12, None), name)
            refused(fn(dt, a, a, 2.0, a, 0, None), name)
            refused(fn(dt, a + 8, a, 2.0, a, 8, None), name)
        ok = (dt, a, a, a, a, a, None, None, 0, 1, a, 1, 4, 32, 32, None)
        for i in (1, 2, 3, 4, 5, 10):                                   # x, mean, rstd, gamma, beta, y
            refused(lib.vaw_groupnorm_apply(*[None if j == i else v for j, v in enumerate(ok)]), "groupnorm_apply:")
        refused(lib.vaw_groupnorm_apply(dt, a, a, a, a, a, a, None, 64, 1, a, 1, 4, 32, 32, None), "groupnorm_apply:")      # scale without shift
        refused(lib.vaw_groupnorm_apply(dt, a, a, a, a, a, a, a, 66, 1, a, 1, 4, 32, 32, None), "groupnorm_apply:")        # film_ld % 4
        refused(lib.vaw_groupnorm_apply(dt, a, a, a, a, a, None, None, 0, 1, a, 1, 4, 48, 32, None), "groupnorm_apply:")   # C % G
        refused(lib.vaw_groupnorm_apply(dt, a, a, a, a, a, None, None, 0, 1, a, 0, 4, 32, 32, None), "groupnorm_apply:")   # B = 0
    refused(lib.vaw_dropout_pack(L.FP8, a, a, 4, 8, None), "dropout_pack:")
    refused(lib.vaw_groupnorm_apply(L.FP8, a, a, a, a, a, None, None, 0, 1, a, 1, 4, 32, 32, None), "groupnorm_apply:")
    del keep
