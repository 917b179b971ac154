"""The DiT engine's host-side layout tables (no GPU): the named slots of the packed adaLN buffer, the table of a block's Linear
sites, and the one epilogue builder every GEMM launch and its plan share."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd import dit as vdit
from vaw_amd import ops

CHUNK6 = ("shift_msa", "scale_msa", "gate_msa", "shift_mlp", "scale_mlp", "gate_mlp")      # reference: adaLN_modulation(c).chunk(6, dim=1)


def _tiny(**kw):
    return vaw_amd.DiT(**dict(dict(hidden_size=8, depth=3, num_heads=2, image_size=4, patch_size=2), **kw))


# ---- slots ---------------------------------------------------------------------------------------------------------------------
def test_slot_names_follow_chunk6():
    assert [getattr(vdit, n.upper()) for n in CHUNK6] == list(range(6))
    assert (vdit.FINAL_SHIFT, vdit.FINAL_SCALE) == (0, 1)


def test_slot_addresses():
    m = _tiny()
    D, Lyr = m.D, m.depth
    assert m.mod_cols == (6 * Lyr + 2) * D
    ws = SimpleNamespace(mod=torch.zeros(2, m.mod_cols), dmod=torch.zeros(2, m.mod_cols), D=D)
    for buf, at in ((ws.mod, vdit._Workspace.mod_at), (ws.dmod, vdit._Workspace.dmod_at)):
        base = buf.data_ptr()
        for l in range(Lyr):
            for j, name in enumerate(CHUNK6):
                assert vdit.mod_offset(l, getattr(vdit, name.upper()), D) == (6 * l + j) * D
                assert at(ws, l, getattr(vdit, name.upper())) == base + 4 * ((6 * l + j) * D), (l, name)
        assert at(ws, Lyr, vdit.FINAL_SHIFT) == base + 4 * (6 * Lyr * D)
        assert at(ws, Lyr, vdit.FINAL_SCALE) == base + 4 * (6 * Lyr * D + D)
    assert vdit.mod_offset(Lyr, vdit.FINAL_SCALE, D) + D == m.mod_cols


def test_slots_line_up_with_the_packed_adaln_matrix():
    """column c of the modulation buffer is the output of row c of the packed adaLN weight (and of element c of the packed bias)"""
    m = _tiny()
    m.ensure_flat()
    D, Lyr, off = m.D, m.depth, m._flat_offsets
    ada_w, ada_b = m._flat_groups()
    w0, b0 = off[ada_w[0]][0], off[ada_b[0]][0]
    for l in range(Lyr):
        assert ada_w[l] == f"blocks.{l}.adaLN_modulation.1.weight" and ada_b[l] == f"blocks.{l}.adaLN_modulation.1.bias"
        assert off[ada_w[l]] == (w0 + vdit.mod_offset(l, vdit.SHIFT_MSA, D) * D, 6 * D * D)
        assert off[ada_b[l]] == (b0 + vdit.mod_offset(l, vdit.SHIFT_MSA, D), 6 * D)
    assert off[ada_w[Lyr]] == (w0 + vdit.mod_offset(Lyr, vdit.FINAL_SHIFT, D) * D, 2 * D * D)
    assert off[ada_b[Lyr]] == (b0 + vdit.mod_offset(Lyr, vdit.FINAL_SHIFT, D), 2 * D)
    packed = m._flat[w0:w0 + m.mod_cols * D].view(m.mod_cols, D)
    blk = m.blocks[1].adaLN_modulation[1].weight
    assert blk.data_ptr() == packed[vdit.mod_offset(1, vdit.SHIFT_MSA, D)].data_ptr() and blk.shape == (6 * D, D)


# ---- site table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mlp_ratio", [4, 2])
def test_site_shapes_are_the_modules(mlp_ratio):
    m = _tiny(depth=1, mlp_ratio=mlp_ratio)
    assert m.Dm == mlp_ratio * m.D
    params = dict(m.named_parameters())
    for s in vdit.SITES:
        N, K = s.shape(m.D, m.Dm)
        assert tuple(params[f"blocks.0.{s.prefix}weight"].shape) == (N, K), s.key
        assert tuple(params[f"blocks.0.{s.prefix}bias"].shape) == (N,), s.key


def test_site_orders():
    assert [s.key for s in vdit.SITES] == ["qkv", "proj", "fc1", "fc2"]                  # weights and their scaling-state rows
    assert [s.key for s in vdit.SITES_BWD] == ["fc2", "fc1", "proj", "qkv"]              # grouped problems and the bias fold
    assert (vdit.QKV, vdit.PROJ, vdit.FC1, vdit.FC2) == vdit.SITES
    states = sorted([(s.s_x, s.f_x) for s in vdit.SITES] + [(s.s_dy, s.f_dy) for s in vdit.SITES])
    assert [i for i, _ in states] == list(range(8))
    assert [k for _, k in states] == ["f_xm", "f_ao", "f_xm2", "f_a", "f_dy2", "f_dhid", "f_dy1", "f_dqkv"]
    assert [(s.x, s.dy, s.cp) for s in vdit.SITES] == [("xm", "dqkv", "qkv"), ("ao", "dy1", "proj"), ("xm2", "dDm", "fc1"), ("a", "dy2", "fc2")]
    assert [(s.gate, s.y) for s in vdit.SITES] == [(None, None), (vdit.GATE_MSA, "y1"), (None, None), (vdit.GATE_MLP, "y2")]


# ---- epilogue builder --------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(bias=None, act=0, aux_in=None, aux_out=None, gate=None, gate_ld=0, resid=None, rowadd=None, rows_per_batch=0, alpha=1.0,
                beta=0.0, out_f32=0, colsum_out=None, colsum_beta=0.0, resid_is_act=0, rowsum_a_out=None, rowsum_a_beta=0.0,
                colsum_partial_out=None)
A = 1 << 20
EPILOGUES = [
    ("plain", {}, {}),
    ("gated residual", dict(bias=A, aux_out=2 * A, gate=3 * A, gate_ld=160, resid=4 * A, rows_per_batch=16, out_f32=True),
     dict(bias=A, aux_out=2 * A, gate=3 * A, gate_ld=160, resid=4 * A, rows_per_batch=16, out_f32=1)),
    ("gelu", dict(bias=A, act=1, aux_out=2 * A), dict(bias=A, act=1, aux_out=2 * A)),
    ("gelu backward", dict(act=2, aux_in=A, colsum_partial=5), dict(act=2, aux_in=A, colsum_partial_out=16)),
    ("weight gradient", dict(beta=1.0, out_f32=True, rowsum_a_out=A, rowsum_a_beta=1.0), dict(beta=1.0, out_f32=1, rowsum_a_out=A, rowsum_a_beta=1.0)),
    ("weight gradient, bias elsewhere", dict(beta=0.0, out_f32=True, rowsum_a_out=None, rowsum_a_beta=0.0), dict(out_f32=1)),
    ("null addresses as 0", dict(bias=0, aux_in=0, aux_out=0, gate=0, resid=0, rowadd=0, colsum_out=0, rowsum_a_out=0), {}),
]


@pytest.mark.parametrize("what,kw,want", EPILOGUES, ids=[e[0] for e in EPILOGUES])
def test_epilogue_fields(what, kw, want):
    e = ops.epilogue(**kw)
    assert isinstance(e, L.Epilogue) and [n for n, _ in L.Epilogue._fields_][:-1] == list(DEFAULTS)
    for name, default in DEFAULTS.items():
        assert getattr(e, name) == want.get(name, default), (what, name)
    if "colsum_partial" in kw:
        assert e.colsum_rows_out.contents.value == kw["colsum_partial"]
    else:
        assert not e.colsum_rows_out


def test_epilogue_colsum_partial_object():
    cp = ops.ColsumPartial(7, 24, "cpu")
    cp.rows.value = 3                                       # left over from the launch before
    e = ops.epilogue(act=2, aux_in=A, colsum_partial=cp)
    assert e.colsum_partial_out == cp.buf.data_ptr() and cp.rows.value == 7       # in: the capacity
    assert C.addressof(e.colsum_rows_out.contents) == C.addressof(cp.rows)        # out: the kernel's count lands in cp.rows
    assert ops.epilogue(colsum_partial=4, colsum_partial_out=A).colsum_partial_out == A


def test_launches_and_plans_share_the_builder(monkeypatch):
    class Reached(Exception):
        pass

    seen = []

    def spy(**kw):
        seen.append(kw)
        raise Reached

    monkeypatch.setattr(ops, "epilogue", spy)
    kw = dict(bias=A, gate=A, gate_ld=96, resid=A, rows_per_batch=16, out_f32=True)
    for call in (lambda: ops.gemm(L.BF16, 1, 1, 64, 64, 64, A, 64, A, 64, A, 64, **kw),
                 lambda: ops.gemm_plan(L.BF16, 1, 1, 64, 64, 64, A, 64, A, 64, A, 64, **kw),
                 lambda: ops.gemm_fp8(128, 128, 128, A, 128, A, A, 128, A, A, 128, **kw),
                 lambda: ops.gemm_fp8_plan(128, 128, 128, A, 128, A, A, 128, A, A, 128, **kw),
                 lambda: ops.conv3x3(L.BF16, 0, A, 0, A, A, 2, 8, 8, 64, 64, bias=A, resid=A),
                 lambda: ops.conv3x3_plan(L.BF16, 0, A, 0, A, A, 2, 8, 8, 64, 64, bias=A, resid=A)):
        with pytest.raises(Reached):
            call()
    launch, plan, launch8, plan8, conv, conv_plan = ({k: v for k, v in s.items() if v not in (None, 0, 0.0, False) and (k, v) != ("alpha", 1.0)} for s in seen)
    assert launch == plan == launch8 == plan8 == kw                  # (defaults dropped: each twin sees its launch's keywords)
    assert conv == conv_plan == dict(bias=A, resid=A, resid_is_act=True)
