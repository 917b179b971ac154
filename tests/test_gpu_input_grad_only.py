"""FlatModule.input_grad_only() on the GPU: inside the context a forward plus backward of DiT / UNetModel yields dx -- bitwise the
full backward's -- and touches nothing else: no gradient buffer appears where none was, an existing one keeps its bits, an
accumulation is not disturbed by an evaluation in its middle, no hook fires, nothing is queued.  Tiny models of the golden
fixtures, every mode the context promises to work in.  Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

from conftest import load_pt, perturb_

pytestmark = pytest.mark.gpu

import vaw_amd

DEV = "cuda"


def _dit(tag, dtype, ckpt):
    g = load_pt("dit_tiny.pt")
    torch.manual_seed(11)
    m = vaw_amd.DiT(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, compute_dtype=dtype,
                    activation_checkpointing=ckpt, **g[f"{tag}/kw"]).to(DEV).train()
    perturb_(m, 99)
    x, t, y, gout = (g[f"{tag}/{k}"].to(DEV) for k in ("x", "t", "y", "gout"))
    return m, x, gout, (lambda xr: m(xr, t, y)[0])


def _unet(dtype, ckpt):
    g = load_pt("unet_tiny.pt")
    torch.manual_seed(21)
    m = vaw_amd.UNetModel(compute_dtype=dtype, **g["new/kw"])
    m.set_activation_checkpointing(ckpt)
    m = m.to(DEV).train()
    perturb_(m, 77, std=0.03)
    x, t, gout = (g[f"new/{k}"].to(DEV) for k in ("x", "t", "gout"))
    y = g["new/y"].to(DEV) if g["new/y"].numel() else None
    return m, x, gout, (lambda xr: m(xr, t, y=y) if y is not None else m(xr, t))


def _dx(fwd, x, gout, scale=1.0):
    xr = (x * scale).clone().requires_grad_(True)
    (fwd(xr) * gout).sum().backward()
    return xr.grad.clone()


def _check(m, x, gout, fwd):
    hooks = []
    m.grad_ready_hook = hooks.append
    # a model that never had a gradient buffer still has none
    with m.input_grad_only():
        dx_only = _dx(fwd, x, gout)
    assert m._flat_grad is None and all(p.grad is None for p in m.parameters()) and hooks == []
    assert getattr(m, "_pend_wgrad", {}) == {}
    m.grad_ready_hook = None
    dx_full = _dx(fwd, x, gout)
    assert torch.isfinite(dx_full).all() and float(dx_full.abs().max()) > 0
    assert torch.equal(dx_only, dx_full), float((dx_only - dx_full).abs().max())
    assert m._flat_grad is not None and m.grads_live()
    # a pre-filled gradient buffer keeps its bits
    flat = m.flat_grads()
    flat.copy_(torch.arange(flat.numel(), device=DEV, dtype=torch.float32).mul_(0.37).sin_())
    before, addr = flat.clone(), flat.data_ptr()
    with m.input_grad_only():
        again = _dx(fwd, x, gout)
    assert torch.equal(again, dx_full) and m.flat_grads().data_ptr() == addr and torch.equal(m.flat_grads(), before)
    # two accumulation micro-steps with an evaluation between them
    m.zero_grad_flat()
    _dx(fwd, x, gout), _dx(fwd, x, gout, 0.5)
    ref = m.flat_grads().clone()
    m.zero_grad_flat()
    _dx(fwd, x, gout)
    with m.input_grad_only():
        _dx(fwd, x, gout, -0.8)
    _dx(fwd, x, gout, 0.5)
    assert float(ref.abs().max()) > 0 and torch.equal(m.flat_grads(), ref)
    # the flag is recorded at forward and checked at backward
    xr = x.clone().requires_grad_(True)
    loss = (fwd(xr) * gout).sum()
    with m.input_grad_only():
        with pytest.raises(vaw_amd.VawError, match="input_grad_only"):
            loss.backward()
    with m.input_grad_only():
        xr = x.clone().requires_grad_(True)
        loss = (fwd(xr) * gout).sum()
    with pytest.raises(vaw_amd.VawError, match="input_grad_only"):
        loss.backward()
    assert torch.equal(m.flat_grads(), ref)


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["p2", "p4"])
def test_dit_input_grad_only(tag, dtype, ckpt):
    _check(*_dit(tag, dtype, ckpt))


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_unet_input_grad_only(dtype, ckpt):
    _check(*_unet(dtype, ckpt))


def test_dit_per_layer_weight_gradients_mode():
    """defer_wgrad off: the per-layer weight-gradient launches sit between the input-gradient ones; they go, dx stays."""
    m, x, gout, fwd = _dit("p2", "bf16", False)
    m.defer_wgrad = False
    _check(m, x, gout, fwd)


def test_fp8_is_refused():
    m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=1, num_heads=2, num_classes=10,
                    compute_dtype="fp8").to(DEV)
    with pytest.raises(ValueError, match="fp8"):
        with m.input_grad_only():
            pass
    bf = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=1, num_heads=2, num_classes=10).to(DEV)
    with bf.input_grad_only():
        with pytest.raises(ValueError):          # switching inside the context: the forward refuses
            bf.set_compute_dtype("fp8")
            bf(torch.zeros(8, 4, 8, 8, device=DEV), torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.long, device=DEV))
