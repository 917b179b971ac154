"""CPU-only checks of the DiT activation-workspace plan (vaw_dit_ws_plan: host arithmetic) and of the
activation_checkpointing flag's surface.  Every expected size is written out here, not taken from the library."""
import ctypes as C

import pytest

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import ops


def p_heads(D):
    return 2 if D < 256 else 16


def _plan(dt, B, T, D, depth, defer, ckpt, Dm=None, heads=None, Kp=16, No=16):
    Dm = 4 * D if Dm is None else Dm
    heads = p_heads(D) if heads is None else heads
    return ops.dit_ws_plan(dt, B, T, D, Dm, depth, heads, Kp, No, defer, ckpt)


def _expected(dt, B, T, D, Dm, depth, heads, Kp, No, defer, ckpt):
    """The buffers of dit.py's _Workspace, in bytes, by hand."""
    es = 2 if dt == L.BF16 else 4
    M = B * T
    Bk = -(-B // 64) * 64 if dt == L.BF16 else B
    mc = (6 * depth + 2) * D
    own_dy = bool(defer) and dt == L.BF16 and M % 64 == 0
    lse = 4 * B * heads * T
    rec_rows = es * M * (D + 3 * D + D + D + D + Dm + Dm + D)           # xm qkv ao y1 xm2 hpre a y2
    rec_stats = lse + 4 * 4 * M
    rec_dy = es * M * (D + Dm + D + 3 * D) if own_dy else 0                 # dy2 dDm dy1 dqkv
    row = 4 * M * D
    cp_set = 4 * (B * D + B * D + -(-M // 64) * Dm + max(B, M // 64) * 3 * D)
    scratch_dy = 0 if (ckpt and own_dy) else es * M * (Dm + 3 * D + D)       # dDm dqkv dyb
    scratch = (es * M * (No + D + D) + scratch_dy + row + 4 * M * Kp + lse + 4 * B * mc + es * Bk * mc + 4 * 4 * B * D
               + 2 * es * Bk * D)
    cond = es * Bk * (256 + 2 * D) + 3 * 4 * B * D + 4 * B * mc + es * M * Kp + es * M * D + 2 * 4 * M + 4 * M * No + row
    if ckpt:
        block, stat, shared, sets = row, 0, rec_rows + rec_stats + rec_dy + 2 * row, 1
    else:
        block, stat, shared, sets = rec_rows + rec_dy + 2 * row, rec_stats, 0, depth
    total = depth * (block + stat) + shared + sets * cp_set + scratch + cond
    return dict(records=1 if ckpt else depth, colsum_sets=sets, own_dy=int(own_dy), Bk=Bk, block_bytes=block, block_stat_bytes=stat,
                shared_bytes=shared, colsum_bytes=sets * cp_set, scratch_bytes=scratch, cond_bytes=cond, total=total)


def _as_dict(p):
    return {name: getattr(p, name) for name, _ in p._fields_}


def test_plan_off_is_58_D_bytes_per_token_per_block():
    """Every block keeps 16 D act elements, two f32 residual rows and (bf16, deferred weight gradients) 9 D dy elements:
    58 D bytes per token in bf16; 40 D without the deferred operands; 72 D in f32 (which never defers)."""
    for B, T, D in ((4, 16, 64), (128, 256, 1152), (256, 64, 768)):
        M = B * T
        assert _plan(L.BF16, B, T, D, 3, True, False).block_bytes == 58 * D * M == (32 + 8 + 18) * D * M
        assert _plan(L.BF16, B, T, D, 3, False, False).block_bytes == 40 * D * M
        assert _plan(L.F32, B, T, D, 3, True, False).block_bytes == 72 * D * M == _plan(L.F32, B, T, D, 3, False, False).block_bytes
        for dt in (L.BF16, L.F32):
            p = _plan(dt, B, T, D, 3, True, False)
            assert (p.records, p.colsum_sets, p.shared_bytes) == (3, 3, 0)
            assert p.own_dy == (dt == L.BF16) and p.block_stat_bytes == 4 * M * (p_heads(D) + 4)
    # bf16 rows off the 64-row tile of the grouped launch: no deferred operands either
    assert _plan(L.BF16, 3, 16, 64, 3, True, False).block_bytes == 40 * 64 * 48
    assert _plan(L.BF16, 3, 16, 64, 3, True, False).own_dy == 0


def test_plan_checkpoint_keeps_4_D_bytes_per_token_per_block():
    for dt in (L.BF16, L.F32):
        for defer in (False, True):
            for B, T, D in ((4, 16, 64), (3, 16, 64), (128, 1024, 1152)):
                p = _plan(dt, B, T, D, 5, defer, True)
                assert p.block_bytes == 4 * D * B * T and p.block_stat_bytes == 0
                assert (p.records, p.colsum_sets) == (1, 1)
                # the one shared record is as large as ONE block of the flag-off layout: the same record, and two f32 rows --
                # there the block's two residual rows, here xres_mid and the scratch row fc2's residual output goes to when a
                # block is recomputed
                off = _plan(dt, B, T, D, 5, defer, False)
                assert p.shared_bytes == off.block_bytes + off.block_stat_bytes


def test_plan_pins_the_dit_xl2_table():
    """DiT-XL/2 (D 1152, 28 blocks, 16 heads), bf16 with deferred weight gradients: block activations of the resident layout,
    and what recomputation keeps instead."""
    GB = 1e9
    for B, T, want in ((128, 256, 61), (256, 256, 123), (128, 1024, 245)):
        p = _plan(L.BF16, B, T, 1152, 28, True, False, heads=16)
        assert round(28 * p.block_bytes / GB) == want
        assert p.block_bytes == 58 * 1152 * B * T
    p = _plan(L.BF16, 128, 1024, 1152, 28, True, True, heads=16)
    per_token = (28 * p.block_bytes + p.shared_bytes) / (128 * 1024)
    # 4 D L + 58 D (32 D record, 18 D dy operands, xres_mid and the scratch row) + 4 (heads + 4) bytes of lse / statistics
    assert per_token == 4 * 1152 * 28 + 58 * 1152 + 4 * (16 + 4) == 195920
    assert 25.0 < (28 * p.block_bytes + p.shared_bytes) / GB < 26.0
    off = _plan(L.BF16, 128, 1024, 1152, 28, True, False, heads=16)
    assert off.total > 245 * GB and p.total < 30 * GB


def test_plan_sweep_matches_hand_count_and_checkpoint_is_smaller():
    n = 0
    for dt in (L.BF16, L.F32):
        for defer in (0, 1):
            for B in (1, 3, 4, 64):
                for T in (16, 64, 256):
                    for D in (64, 384, 1152, 1280):
                        heads, Dm, Kp, No = p_heads(D), 4 * D, 16, 32
                        M = B * T
                        Bk = -(-B // 64) * 64 if dt == L.BF16 else B
                        es = 2 if dt == L.BF16 else 4
                        for depth in (1, 4, 28):
                            args = (dt, B, T, D, Dm, depth, heads, Kp, No, defer)
                            on, off = ops.dit_ws_plan(*args, True), ops.dit_ws_plan(*args, False)
                            assert _as_dict(on) == _expected(*args, True), args
                            assert _as_dict(off) == _expected(*args, False), args
                            if depth >= 2:
                                assert on.total < off.total, args
                            # one more block: its input row, 4 D bytes per token -- and nothing else in the block-resident,
                            # shared and colsum parts; the conditioning path's modulation rows (mod, dmod: f32 [B, 6 D] each,
                            # dmod_a: act dtype [Bk, 6 D]) grow with the depth in either mode
                            more = ops.dit_ws_plan(dt, B, T, D, Dm, depth + 1, heads, Kp, No, defer, True)
                            resident = lambda p, d: d * p.block_bytes + p.shared_bytes + p.colsum_bytes
                            assert resident(more, depth + 1) - resident(on, depth) == 4 * D * B * T, args
                            assert more.total - on.total == 4 * D * B * T + 6 * D * (2 * 4 * B + es * Bk), args
                            n += 1
    assert n == 2 * 2 * 4 * 3 * 4 * 3


def test_plan_refuses_bad_arguments_with_a_message():
    lib = vaw_amd.lib()
    good = [L.BF16, 4, 16, 64, 256, 3, 2, 16, 16, 1, 1]
    out = L.DitWsPlan()
    assert lib.vaw_dit_ws_plan(*good, C.byref(out)) == 0
    bad = {0: (L.FP8, 7, -1), 1: (0, -4), 2: (0,), 3: (0, -64), 4: (0,), 5: (0, -1), 6: (0, 5), 7: (0,), 8: (0,), 9: (2, -1), 10: (2, -1)}
    for i, values in bad.items():
        for v in values:
            a = list(good)
            a[i] = v
            assert lib.vaw_dit_ws_plan(*a, C.byref(out)) == -1, (i, v)
            msg = lib.vaw_last_error_string().decode()
            assert msg.startswith("dit_ws_plan:") and len(msg) > 20, msg
            with pytest.raises(vaw_amd.VawError, match="dit_ws_plan"):
                ops.dit_ws_plan(*a)
    assert lib.vaw_dit_ws_plan(*good, None) == -1


def test_flag_surface_defaults_and_fp8_refusal():
    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, class_dropout_prob=0.0,
              num_classes=10, learn_sigma=False)
    with pytest.raises(ValueError, match="fp8"):
        vaw_amd.DiT(**kw, compute_dtype="fp8", activation_checkpointing=True)
    m = vaw_amd.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False)
    assert m.activation_checkpointing is False
    assert vaw_amd.DiT_S(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False,
                         activation_checkpointing=True).activation_checkpointing is True
    m = vaw_amd.DiT(**kw)
    assert m.activation_checkpointing is False
    m._ws["stale"] = object()
    m.set_activation_checkpointing(True)
    assert m.activation_checkpointing is True and m._ws == {}           # the setter drops the workspaces
    with pytest.raises(ValueError, match="fp8"):
        m.set_compute_dtype("fp8")
    assert m.compute_dtype == "bf16"
    m.set_activation_checkpointing(False)
    m.set_compute_dtype("fp8")
    with pytest.raises(ValueError, match="fp8"):
        m.set_activation_checkpointing(True)
    assert m.activation_checkpointing is False
    # last keyword of the signature
    import inspect
    assert list(inspect.signature(vaw_amd.DiT.__init__).parameters)[-1] == "activation_checkpointing"


def test_trainer_applies_the_args_field_to_the_wrapped_module():
    """args.activation_checkpointing reaches the DiT behind a `.module` wrapper (DDP-style); absent: the model stays as built."""
    import torch
    from conftest import base_args

    class Wrap(torch.nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module

    kw = dict(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, class_dropout_prob=0.0,
              num_classes=10, learn_sigma=False)

    def trainer(model, **extra):
        args = base_args(in_chans=4, class_cond=True, dataset="Latent", image_size=8, amp=True, **extra)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: 1.0)
        return vaw_amd.Trainer(args, torch.device("cpu"), model, None, opt, sched, None, [])

    m = vaw_amd.DiT(**kw)
    trainer(Wrap(m), activation_checkpointing=True)
    assert m.activation_checkpointing is True
    trainer(Wrap(m))                                     # no such field: untouched
    assert m.activation_checkpointing is True
    trainer(m, activation_checkpointing=False)
    assert m.activation_checkpointing is False
    with pytest.raises(ValueError, match="activation_checkpointing"):
        trainer(torch.nn.Linear(2, 2), activation_checkpointing=True)
    m8 = vaw_amd.DiT(**dict(kw, hidden_size=128), compute_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        trainer(m8, activation_checkpointing=True)
