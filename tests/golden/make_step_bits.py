#!/usr/bin/env python3
"""Generate tests/golden/step_bits.json: sha256 of the bytes that the reverse-step, likelihood, guidance and solver-step
kernels write, recorded on the MI355X from the commit BEFORE they were folded onto one table, one per-element body and one
loop each.  tests/test_gpu_step_bits.py recomputes the same cases at head and compares the hashes.

    python tests/golden/make_step_bits.py --tree <checkout of the commit to record, built in place> [--out FILE]

Only entry points that exist on both sides of that change are called: ops.sample_step, ops.guided_sample_step,
ops.ddim_reverse_step, ops.bpd_terms, ops.cfg_combine, ops.edm_input, ops.edm_step, ops.flow_step and
GaussianDiffusion._vb_terms_bpd (forward and backward).  Every input comes from a seeded CPU generator; the EDM and flow
coefficient tables are seeded numbers too (the kernels only do arithmetic on them), so nothing but the kernels under test
computes on the device.  No tensor is stored: a case is a name and one hash per output, taken over the bytes of that output
across the case's inner sweep (modes, kinds, clipping, guidance), in a fixed order.

B = 3 rows throughout.  per_sample 192: vector path; 193: scalar path; 16385: scalar path with a second grid-stride trip
(more than 64 x 256 items a row); 65540: vector path with a second trip; 192 on a base one float past a 16-byte boundary
(`shifted`) and with rows 2 floats further apart than their length (`ld_odd`): scalar path by layout.  bpd_terms runs one
1024-thread workgroup a row: 4100 (vector) and 1025 (scalar) give its second trip."""
import hashlib
import itertools
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
N = 3
SIZES = {"n192": (3, 8, 8), "n193": (193,), "n16385": (16385,), "n65540": (65540,)}
PLACES = [(k, "plain") for k in SIZES] + [("n192", "shifted"), ("n192", "ld_odd")]
MODES = [(mt, vt) for mt in ("EPSILON", "PREVIOUS_X") for vt in ("FIXED_SMALL", "LEARNED", "LEARNED_RANGE")]
VB_MODES = [(mt, vt) for mt in ("EPSILON", "START_X", "PREVIOUS_X") for vt in ("LEARNED_RANGE", "LEARNED", "FIXED_LARGE", "FIXED_SMALL")]
T_ROWS = [0, 99, 37]          # a t = 0 row among the others
SCALE = 2.5
GROUPS = ["step", "sample_step", "ddim_reverse", "bpd_terms", "cfg_combine", "vb", "edm_input", "edm_step", "flow_step"]


class Hashes:
    """case name -> output name -> running sha256 over the bytes of every tensor added under that name."""

    def __init__(self):
        self.h = {}

    def add(self, case, outputs):
        for k, t in outputs.items():
            if t is not None:
                self.h.setdefault(case, {}).setdefault(k, hashlib.sha256()).update(t.detach().contiguous().cpu().numpy().tobytes())

    def result(self):
        return {c: {k: h.hexdigest() for k, h in sorted(o.items())} for c, o in sorted(self.h.items())}


def place(vals, layout):
    """`vals` ([rows, ...] on the CPU) on the device: plain | shifted (base one float past a 16-byte boundary) | ld_odd (rows
    2 floats further apart than their length)."""
    row = vals[0].numel()
    if layout == "shifted":
        out = torch.empty(vals.numel() + 1, device=DEV)[1:].view(vals.shape)
        assert out.data_ptr() % 16 == 4
    elif layout == "ld_odd":
        out = torch.empty(vals.shape[0], row + 2, device=DEV)[:, :row].view(vals.shape)
        assert out.stride(0) % 4 == 2
    else:
        out = torch.empty(vals.shape, device=DEV)
    out.copy_(vals)
    return out


def step_inputs(shape, learned, seed, layout="plain"):
    """x, noise and one stacked [2N, (2)C, ...] model output on the device, as step_inputs of tests/test_gpu_sampler.py."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn((2 * N, (2 if learned else 1) * shape[0], *shape[1:]), generator=g) * 0.7
    if learned:
        vals[:, shape[0]:] = torch.rand((2 * N, *shape), generator=g) * 2 - 1
    x = torch.randn((N, *shape), generator=g).to(DEV)
    nz = torch.randn((N, *shape), generator=g).to(DEV)
    return place(vals, layout), x, nz


def quarters(out, C, learned):
    cond, uncond = out[:N], out[N:]
    return cond[:, :C], uncond[:, :C], (cond[:, C:] if learned else None), (uncond[:, C:] if learned else None)


def diffusion(pkg, mt, vt, loss="MSE"):
    args = SimpleNamespace(weight_type="constant" if mt == "PREVIOUS_X" else "lambda", gamma=0.0, learn_sigma=vt.startswith("LEARNED"),
                           p2_gamma=1, p2_k=1, time_dist=["uniform"], learn_align=False, cpu_rng=True)
    return pkg.GaussianDiffusion(args=args, betas=pkg.get_named_beta_schedule("linear", 100), model_mean_type=pkg.ModelMeanType[mt],
                                 model_var_type=pkg.ModelVarType[vt], loss_type=pkg.LossType[loss], rescale_timesteps=False)


def modes_of(mt, vt):
    return int(mt == "PREVIOUS_X"), {"LEARNED": 1, "LEARNED_RANGE": 2}.get(vt, 0)


def rows(d):
    return d._sample_rows(torch.tensor(T_ROWS, device=DEV))


# ---- the reverse step, guided and not ----------------------------------------------------------------------------------
def group_step(pkg, H):
    ops = pkg.ops
    for size, layout in PLACES:
        shape = SIZES[size]
        full = (size, layout) == ("n192", "plain")          # every mode / clip / scale here, one learned-range sweep elsewhere
        for i, (mt, vt) in enumerate(MODES if full else [("EPSILON", "LEARNED_RANGE")]):
            d, learned = diffusion(pkg, mt, vt), vt.startswith("LEARNED")
            mean_mode, var_mode = modes_of(mt, vt)
            out, x, nz = step_inputs(shape, learned, 40 + i, layout)
            coef, q = rows(d), quarters(out, shape[0], learned)
            for (kind, eta), clip, guided in itertools.product(((0, 0.0), (1, 0.0), (2, 0.7)), (True, False) if full else (True,), (True, False)):
                got = ops.guided_sample_step(kind, q[0], q[1] if guided else None, q[2], q[3] if guided else None, SCALE, x,
                                             nz if kind else None, coef, mean_mode, var_mode, clip, eta, want_all=True)
                H.add(f"step/{size}/{layout}/{mt}/{vt}", got)


def group_sample_step(pkg, H):
    """ops.sample_step on the halves of one [N, 2C, ...] output read in place, on contiguous copies of them, and with a fixed
    variance on a contiguous mean output."""
    ops = pkg.ops
    d, df = diffusion(pkg, "EPSILON", "LEARNED_RANGE"), diffusion(pkg, "EPSILON", "FIXED_SMALL")
    for size, shape in SIZES.items():
        out, x, nz = step_inputs(shape, True, 11)
        m, v = torch.split(out[:N], shape[0], dim=1)
        for (kind, vm), clip in itertools.product(((0, 2), (1, 1), (2, 2)), (True, False)):
            a = nz if kind else None
            H.add(f"sample_step/{size}/in_place", ops.sample_step(kind, m, v, x, a, rows(d), 0, vm, clip, 0.3, want_all=True))
            H.add(f"sample_step/{size}/dense", ops.sample_step(kind, m.contiguous(), v.contiguous(), x, a, rows(d), 0, vm, clip, 0.3, want_all=True))
            H.add(f"sample_step/{size}/fixed", ops.sample_step(kind, m.contiguous(), None, x, a, rows(df), 0, 0, clip, 0.3, want_all=True))


def group_ddim_reverse(pkg, H):
    ops = pkg.ops
    for size, layout in PLACES:
        shape = SIZES[size]
        for i, mt in enumerate(("EPSILON", "PREVIOUS_X")):
            out, x, _ = step_inputs(shape, True, 60 + i, layout)
            coef = rows(diffusion(pkg, mt, "LEARNED_RANGE"))
            m = out[:N, :shape[0]]
            for clip in (True, False):
                H.add(f"ddim_reverse/{size}/{layout}/{mt}", ops.ddim_reverse_step(m, x, coef, clip))
                if layout == "plain":
                    H.add(f"ddim_reverse/{size}/dense/{mt}", ops.ddim_reverse_step(m.contiguous(), x, coef, clip))


def group_bpd_terms(pkg, H):
    ops = pkg.ops
    places = [("n192", (3, 8, 8), "plain"), ("n193", (193,), "plain"), ("n4100", (4100,), "plain"), ("n1025", (1025,), "plain"),
              ("n192", (3, 8, 8), "shifted"), ("n192", (3, 8, 8), "ld_odd")]
    for size, shape, layout in places:
        for i, (mt, vt) in enumerate(MODES):
            learned = vt.startswith("LEARNED")
            mean_mode, var_mode = modes_of(mt, vt)
            out, x_t, nz = step_inputs(shape, learned, 80 + i, layout)
            g = torch.Generator().manual_seed(90 + i)
            x0 = (torch.randn((N, *shape), generator=g) * 0.8).clamp(-1, 1).to(DEV)          # some values in the open-ended bins
            m, _, v, _ = quarters(out, shape[0], learned)
            coef = rows(diffusion(pkg, mt, vt))
            for clip in (True, False):
                vb, xm, ms = ops.bpd_terms(m, v, x0, x_t, nz, coef, mean_mode, var_mode, clip)
                H.add(f"bpd_terms/{size}/{layout}/{mt}/{vt}", {"vb": vb, "xstart_mse": xm, "mse": ms})


def group_cfg_combine(pkg, H):
    for size, layout in PLACES:
        out, _, _ = step_inputs(SIZES[size], False, 100, layout)
        for scale in (SCALE, 1.0, -0.7):
            H.add(f"cfg_combine/{size}/{layout}", {"out": pkg.ops.cfg_combine(out[:N], out[N:], scale)})


# ---- the variational-bound term of the training loss, forward and backward ------------------------------------------------
def group_vb(pkg, H):
    t = torch.tensor(T_ROWS, device=DEV)
    for size in ("n192", "n16385"):          # 16385: the backward's second grid-stride trip
        shape = SIZES[size]
        for i, (mt, vt) in enumerate(VB_MODES):
            learned = vt.startswith("LEARNED")
            d = diffusion(pkg, mt, vt, "KL")
            out, x_t, _ = step_inputs(shape, learned, 120 + i)
            g = torch.Generator().manual_seed(140 + i)
            x0 = (torch.randn((N, *shape), generator=g) * 0.8).clamp(-1, 1).to(DEV)
            gvb = torch.tensor([1.0, -0.5, 2.25], device=DEV)
            m = out[:N, :shape[0]].contiguous().requires_grad_(True)
            v = out[:N, shape[0]:].contiguous().requires_grad_(True) if learned else None
            for scale in (1.0, 100.0):
                m.grad = None
                if v is not None:
                    v.grad = None
                vb = d._vb_terms_bpd(m, v, x0, x_t, t, scale)
                vb.backward(gvb)
                H.add(f"vb/{size}/{mt}/{vt}", {"vb": vb, "d_mean": m.grad, "d_var": None if v is None else v.grad})


# ---- solver steps -------------------------------------------------------------------------------------------------------
def seeded_table(cols, dtype, seed):
    """Four rows of generic coefficients in [0.5, 1.5): every divisor of the kernels is non-zero and every result finite."""
    return (torch.rand(4, cols, generator=torch.Generator().manual_seed(seed), dtype=dtype) + 0.5).to(DEV)


def solver_output(shape, layout, seed):
    """A stacked [2N, ...] float32 network output: plain | slice (the [:, :C] part of a [2N, 2C, ...] output) | shifted | ld_odd."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn((2 * N, *shape), generator=g) * 0.7
    if layout == "slice":
        out = torch.empty((2 * N, 2 * shape[0], *shape[1:]), device=DEV)[:, :shape[0]]
        out.copy_(vals)
        return out
    return place(vals, layout)


SOLVER_PLACES = PLACES + [("n192", "slice")]


def group_edm_input(pkg, H):
    ops, coef = pkg.ops, seeded_table(pkg.ops.EDM_COLS, torch.float64, 200)
    for size, shape in SIZES.items():
        g = torch.Generator().manual_seed(201)
        x = (torch.randn((N, *shape), generator=g, dtype=torch.float64) * 30).to(DEV)
        nz = torch.randn((N, *shape), generator=g, dtype=torch.float64).to(DEV)
        for noise, stacked in itertools.product((True, False), (True, False)):
            buf = torch.full((2 * N if stacked else N, *shape), 7.0, device=DEV)
            x_hat = ops.edm_input(x, nz if noise else None, coef, 1, torch.empty_like(x), buf[:N], buf[N:] if stacked else None)
            H.add(f"edm_input/{size}", {"x_hat": x_hat, "model_in": buf})
        shifted = torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape)
        H.add(f"edm_input/{size}", {"x_hat": ops.edm_input(x, nz, coef, 2, torch.empty_like(x), shifted), "model_in": shifted})


def group_edm_step(pkg, H):
    ops, coef = pkg.ops, seeded_table(pkg.ops.EDM_COLS, torch.float64, 210)
    for size, layout in SOLVER_PLACES:
        shape = SIZES[size]
        g = torch.Generator().manual_seed(211)
        x_hat = (torch.randn((N, *shape), generator=g, dtype=torch.float64) * 20).to(DEV)
        d_prev = torch.randn((N, *shape), generator=g, dtype=torch.float64).to(DEV)
        out = solver_output(shape, layout, 212)
        for pred_type, guided in itertools.product(ops.EDM_PRED, (True, False)):
            cond, uncond = out[:N], (out[N:] if guided else None)
            case = f"edm_step/{size}/{layout}/{pred_type}"
            H.add(case, {"euler": ops.edm_step(ops.STEP_EULER, pred_type, cond, uncond, SCALE, x_hat, None, coef, 1, x_out=torch.empty_like(x_hat))})
            buf = torch.full((2 * N, *shape), 7.0, device=DEV)
            d_cur = ops.edm_step(ops.STEP_PREDICT, pred_type, cond, uncond, SCALE, x_hat, torch.empty_like(x_hat), coef, 1, model_in=buf[:N],
                                 model_in_dup=buf[N:])
            H.add(case, {"d_cur": d_cur, "model_in": buf})
            H.add(case, {"correct": ops.edm_step(ops.STEP_CORRECT, pred_type, cond, uncond, SCALE, x_hat, d_prev, coef, 1,
                                                 x_out=torch.empty_like(x_hat))})


def group_flow_step(pkg, H):
    ops, coef = pkg.ops, seeded_table(pkg.ops.FLOW_COLS, torch.float32, 220)
    for size, layout in SOLVER_PLACES:
        shape = SIZES[size]
        g = torch.Generator().manual_seed(221)
        x, nz, f_prev, x_pred = (torch.randn((N, *shape), generator=g).to(DEV) for _ in range(4))
        kick_prev = (torch.randn((N, *shape), generator=g) * 0.3).to(DEV)
        out = solver_output(shape, layout, 222)
        new = lambda r=N: torch.full((r, *shape), 7.0, device=DEV)
        for mean_type, sde, guided in itertools.product(ops.FLOW_MEAN, (True, False), (True, False)):
            cond, uncond = out[:N], (out[N:] if guided else None)
            case = f"flow_step/{size}/{layout}/{mean_type}"
            H.add(case, {"euler": ops.flow_step(ops.STEP_EULER, sde, mean_type, cond, uncond, SCALE, x, nz if sde else None, None, None, None, coef,
                                                1, 1, new())})
            if sde:          # the noise-free last step
                H.add(case, {"euler": ops.flow_step(ops.STEP_EULER, True, mean_type, cond, uncond, SCALE, x, None, None, None, None, coef, 1, 1, new())})
            buf, f0, kick = new(2 * N), new(), (new() if sde else None)
            ops.flow_step(ops.STEP_PREDICT, sde, mean_type, cond, uncond, SCALE, x, nz if sde else None, None, f0, kick, coef, 1, 2, buf[:N], buf[N:])
            H.add(case, {"predict": buf, "f0": f0, "kick": kick})
            H.add(case, {"correct": ops.flow_step(ops.STEP_CORRECT, sde, mean_type, cond, uncond, SCALE, x, None, x_pred, f_prev,
                                                  kick_prev if sde else None, coef, 1, 2, new())})


def compute(pkg, group):
    """{case name: {output name: sha256}} of one of GROUPS with the package `pkg` (vaw_amd of the tree under test)."""
    H = Hashes()
    globals()["group_" + group](pkg, H)
    torch.cuda.synchronize()
    return H.result()


def main():
    tree = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--tree" or a.startswith("--tree=")]
    out = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--out" or a.startswith("--out=")]
    sys.path.insert(0, os.path.abspath(tree[0]) if tree else os.path.dirname(os.path.dirname(HERE)))
    import vaw_amd
    print("package:", os.path.dirname(os.path.abspath(vaw_amd.__file__)), flush=True)
    bits = {}
    for group in GROUPS:
        bits.update(compute(vaw_amd, group))
        print(f"  {group}: {sum(1 for c in bits if c.startswith(group + '/'))} cases", flush=True)
    path = out[0] if out else os.path.join(HERE, "step_bits.json")
    with open(path, "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(bits)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
