"""The two engines of the bf16 grouped weight gradient (vaw_wgrad_grouped, 256-column tiles) give the same bits.

Engine 0 is the 8-wave persistent kernel (gemm_p8_kernel<..., GRP>), engine 1 the 4-wave kernel (gemm_g4_kernel: one wave per
SIMD, 128 x 128 wave tiles).  They share the tile, the MFMA instruction, the K order, the K-split points, the slab layout and
the epilogue arithmetic, so every output element sees the same sequence of accumulations: on RANDOM data (where any other
order shows in the last bits) every dW must be torch.equal.  Outputs sit inside larger canary-filled buffers (one row above
and below, columns left and right, a leading dimension beyond N) that must come back untouched."""
import pytest
import torch

from conftest import perturb_

pytestmark = pytest.mark.gpu

import vaw_amd
from vaw_amd import ops
from vaw_amd._lib import BF16, lib, ptr

DEV = "cuda"
CANARY = -7.25
PAD_TOP, PAD_LEFT, PAD_RIGHT = 1, 4, 4       # ld_dw = N + 8: a multiple of 4, and the first element stays 16-byte aligned

CASES = {
    # name: (shapes, K, beta, alphas)
    "k256": ([(256, 256), (512, 256)], 256, 0.0, None),                                    # 4 K tiles: the shortest loop that fills the ring
    "k320_edges_beta1": ([(200, 264), (520, 72), (136, 1000)], 320, 1.0, None),            # odd K-tile count; edge tiles in M and N
    "k512_split": ([(256, 512)], 512, 0.0, None),                                          # 2 tiles in 2 K ranges of 4 K tiles, the least a split keeps
    "k1024_mixed": ([(512, 512)] * 66, 1024, 0.0, None),                                   # 264 tiles: 256 whole + 8 K-split on 256 CUs
    "k1024_all_split": ([(768, 768), (2304, 768), (256, 512)], 1024, 0.0, None),           # 38 tiles, t_full == 0: slab path alone, operand
                                                                                           # bases switch between problems inside the stream
    "k1024_all_split_beta1_alpha": ([(768, 768), (2304, 768), (256, 512)], 1024, 1.0, (0.5, -1.75, 3.0)),
    "k320_edges_alpha": ([(200, 264), (520, 72), (136, 1000)], 320, 1.0, (0.5, -1.75, 3.0)),
}


def _inputs(name):
    shapes, K, beta, alphas = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    out = []
    for (M, N) in shapes:
        dy = torch.randn(K, M, generator=g).bfloat16()
        x = torch.randn(K, N, generator=g).bfloat16()
        dw0 = torch.randn(M, N, generator=g) if beta != 0.0 else torch.full((M, N), float("nan"))     # beta = 0 must not read dW
        out.append((dy, x, dw0))
    return out


def _launch(name, inputs, engine, launches=1):
    """One vaw_wgrad_grouped under `engine`; returns the canary-framed dW buffers."""
    shapes, K, beta, alphas = CASES[name]
    probs, keep, bigs = [], [], []
    for i, ((M, N), (dy, x, dw0)) in enumerate(zip(shapes, inputs)):
        ld = PAD_LEFT + N + PAD_RIGHT
        big = torch.full((PAD_TOP + M + 1, ld), CANARY, device=DEV)
        big[PAD_TOP:PAD_TOP + M, PAD_LEFT:PAD_LEFT + N] = dw0.to(DEV)
        dyd, xd = dy.to(DEV), x.to(DEV)
        keep += [dyd, xd]
        bigs.append(big)
        p = (ptr(dyd), ptr(xd), ptr(big) + 4 * (PAD_TOP * ld + PAD_LEFT), M, N, M, N, ld)
        probs.append(p + (alphas[i],) if alphas else p)
    lib().vaw_debug_wgrad_engine(engine)
    try:
        grp = ops.WgradGroup(probs, K, torch.device(DEV))
        for _ in range(launches):
            grp.launch(BF16, beta)
        torch.cuda.synchronize()
    finally:
        lib().vaw_debug_wgrad_engine(-1)
    return bigs


def _check_frame(name, bigs):
    for (M, N), big in zip(CASES[name][0], bigs):
        frame = big.clone()
        inner = frame[PAD_TOP:PAD_TOP + M, PAD_LEFT:PAD_LEFT + N]
        assert not bool(torch.isnan(inner).any()), (name, M, N)
        inner.fill_(CANARY)
        assert bool((frame == CANARY).all()), (name, M, N, "canary rows / columns written")


@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_engines_bitwise_equal(name):
    inputs = _inputs(name)
    old = _launch(name, inputs, 0)
    new = _launch(name, inputs, 1)
    _check_frame(name, old)
    _check_frame(name, new)
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), (name, i, CASES[name][0][i], float((a - b).abs().max()))


@pytest.mark.parametrize("name", ["k1024_mixed", "k1024_all_split"])
def test_wgrad_g4_repeat_launch_same_bits(name):
    """A second launch on the uploaded table (beta = 0) reproduces the first, slabs and fixup included."""
    inputs = _inputs(name)
    once = _launch(name, inputs, 1)
    twice = _launch(name, inputs, 1, launches=2)
    _check_frame(name, twice)
    for a, b in zip(once, twice):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["few_tiles_split", "full_rounds_plus_split", "edges_accumulate"])
def test_wgrad_g4_exact_integers(case):
    """The form of test_wgrad_grouped_exact_integers with engine 1 forced: small integers are exact in bf16 / f32, so every tile
    of every problem must match the float64 product bit for bit."""
    g = torch.Generator().manual_seed(11)
    shapes, K, beta = {
        "few_tiles_split": ([(768, 768), (2304, 768), (256, 512)], 1024, 0.0),
        "full_rounds_plus_split": ([(512, 512)] * 70, 2560, 0.0),
        "edges_accumulate": ([(200, 264), (520, 72), (136, 1000)], 320, 1.0),
    }[case]
    probs, keep, refs = [], [], []
    for (M, N) in shapes:
        dy = torch.randint(-2, 3, (K, M), generator=g).float()
        x = torch.randint(-2, 3, (K, N), generator=g).float()
        dw0 = torch.randint(-5, 6, (M, N), generator=g).float()
        dyd, xd, dwd = dy.to(DEV).bfloat16(), x.to(DEV).bfloat16(), dw0.to(DEV).clone()
        keep += [dyd, xd, dwd]
        probs.append((ptr(dyd), ptr(xd), ptr(dwd), M, N, M, N, N))
        refs.append((dwd, beta * dw0.double() + dy.double().t() @ x.double()))
    lib().vaw_debug_wgrad_engine(1)
    try:
        grp = ops.WgradGroup(probs, K, torch.device(DEV))
        grp.launch(BF16, beta)
        torch.cuda.synchronize()
    finally:
        lib().vaw_debug_wgrad_engine(-1)
    for i, (got, ref) in enumerate(refs):
        assert torch.equal(got.cpu().double(), ref), (case, i, shapes[i], float((got.cpu().double() - ref).abs().max()))


def test_dit_backward_bitwise_equal_under_both_engines():
    """A tiny bf16 DiT with deferred (grouped) weight gradients: one forward and backward under each engine, the whole flat
    gradient buffer bit for bit.  16 x 16 tokens = 256 rows = 4 K tiles; every Linear of a block is one 256-column-tile problem."""
    def make():
        torch.manual_seed(5)
        m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, num_classes=10,
                        class_dropout_prob=0.0, learn_sigma=False, compute_dtype="bf16").to(DEV).train()
        perturb_(m, 3, 0.05)
        m.ensure_flat()
        return m

    g = torch.Generator().manual_seed(9)
    x = torch.randn(16, 4, 8, 8, generator=g).to(DEV)
    t = (torch.rand(16, generator=g) * 999).to(DEV)
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)
    gout = torch.randn(16, 4, 8, 8, generator=g).to(DEV)

    def backward(engine):
        m = make()
        assert m.defer_wgrad
        lib().vaw_debug_wgrad_engine(engine)
        try:
            m.zero_grad_flat()
            out, _ = m(x, t, y)
            (out * gout).sum().backward()
            torch.cuda.synchronize()
            return m.flat_grads().clone()
        finally:
            lib().vaw_debug_wgrad_engine(-1)

    a, b = backward(0), backward(1)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0
    assert torch.equal(a, b), float((a - b).abs().max())
