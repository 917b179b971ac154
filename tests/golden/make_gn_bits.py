#!/usr/bin/env python3
"""Generate tests/golden/gn_bits.json: sha256 of the bytes that vaw_groupnorm_fwd, vaw_groupnorm_apply and vaw_groupnorm_bwd
write, recorded on the MI355X from the commit BEFORE GroupNorm moved into csrc/groupnorm.hip behind vaw_gn_plan (and lost the dead
fold mode of its group kernel, its dispatch macros and the three copies of the per-octet coefficients).
tests/test_gpu_gn_bits.py recomputes the same cases at head and compares the hashes.

    python tests/golden/make_gn_bits.py --tree <checkout of the commit to record, built in place> [--out FILE]

Only what exists on both sides of that change is called: the three entry points, vaw_groupnorm_workspace_floats and the
vaw_debug_gn_flat switch.  Every input comes from a seeded CPU generator, the workspace is NaN-filled before every call and
allocated before the switch is set.  No tensor is stored: a case is a name and one hash per output -- y, mean, rstd, the y of
vaw_groupnorm_apply on those statistics, dx, dgamma and dbeta with grad_beta 0 and 1, and the FiLM gradient rows.  Every case is
computed twice and nothing is written if the two runs differ (the kernels sum in a fixed order, so they should not).

Cases (B, HW, C, G), the smallest that reach each way the kernels can go wrong:
  f32_quad      64 ch x 64 px, 96 ch x 25 px (half-filled second channel block, odd rows), 1600 px = four 512-row chunks with a
                ragged tail, 40 channels in 10 groups
  bf16_quad     C = 100, G = 25: C % 8 == 4 keeps bf16 off the flat kernels whatever the switch
  bf16_switch0 / bf16_switch1   the nine shapes of test_groupnorm_flat_mapping_kernels on the quad and on the flat kernels: several
                chunks with ragged tails, 216 / 240 / 192 live lanes, groups straddling a lane's channel octet
  bf16_default  by shape: 128 x 512 px -> flat on 128-row chunks, 1024 px -> 256 rows, 2048 px -> 512 rows; 3 x 64 px -> quad
One shape of f32_quad, bf16_switch0 and bf16_switch1 runs all eight film / silu / add combinations, the others their listed one."""
import hashlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
F32, BF16 = 0, 1
ALL = list(itertools.product((True, False), repeat=3))
FLAT_SHAPES = [((3, 576, 192, 32), (True, True, True)), ((2, 256, 576, 32), (False, True, False)), ((2, 64, 1536, 32), (True, False, True)),
               ((5, 400, 96, 32), (True, True, False)), ((2, 529, 384, 32), (False, False, True)), ((1, 1089, 128, 32), (True, True, True)),
               ((3, 1024, 192, 32), (True, True, True)), ((2, 576, 384, 32), (False, False, True)), ((40, 144, 64, 32), (True, True, True))]
# group -> (dtype, switch, [(shape, [flags, ...])])
GROUPS = {
    "f32_quad": (F32, -1, [((2, 64, 64, 32), ALL), ((3, 25, 96, 32), [(False, True, True)]), ((2, 1600, 64, 32), [(True, True, True)]),
                           ((2, 36, 40, 10), [(True, True, True)])]),
    "bf16_quad": (BF16, -1, [((2, 36, 100, 25), [(True, True, True)])]),
    "bf16_switch0": (BF16, 0, [(s, ALL if s == (5, 400, 96, 32) else [f]) for s, f in FLAT_SHAPES]),
    "bf16_switch1": (BF16, 1, [(s, ALL if s == (5, 400, 96, 32) else [f]) for s, f in FLAT_SHAPES]),
    "bf16_default": (BF16, -1, [((B, HW, 32, 32), [(True, True, True)]) for B, HW in ((128, 512), (128, 1024), (128, 2048), (3, 64))]),
}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(L, dt, switch, shape, film, silu, add, seed):
    """{output name: sha256} of one forward, one apply and two backwards (grad_beta 0 and 1) on seeded inputs."""
    lib, ptr, stream = L.lib(), L.ptr, L.stream_ptr
    B, HW, C, G = shape
    td = torch.float32 if dt == F32 else torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B * HW, C, generator=g) * 1.5 + 0.3).to(DEV, td)
    dout, dadd = torch.randn(B * HW, C, generator=g).to(DEV, td), torch.randn(B * HW, C, generator=g).to(DEV, td)
    gam, bet = (torch.randn(C, generator=g) * 0.5 + 1).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    emb = (torch.randn(B, 3 * C, generator=g) * 0.3).to(DEV)          # FiLM rows with a stride wider than 2 C, as in the engine
    old_g, old_b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    sc, sh = (ptr(emb) + 4 * C, ptr(emb) + 8 * C) if film else (None, None)
    ws = torch.empty(lib.vaw_groupnorm_workspace_floats(B, HW, C), device=DEV)
    lib.vaw_debug_gn_flat(switch)          # after the workspace was sized, as callers meet it
    y, ya = torch.full((B * HW, C), 7.0, device=DEV, dtype=td), torch.full((B * HW, C), 7.0, device=DEV, dtype=td)
    mean, rstd = torch.full((B * G,), 7.0, device=DEV), torch.full((B * G,), 7.0, device=DEV)
    ws.fill_(float("nan"))
    assert lib.vaw_groupnorm_fwd(dt, ptr(x), ptr(gam), ptr(bet), sc, sh, 3 * C, int(silu), ptr(y), ptr(mean), ptr(rstd), B, HW, C, G, 1e-5,
                                 ptr(ws), stream()) == 0
    ws.fill_(float("nan"))
    assert lib.vaw_groupnorm_apply(dt, ptr(x), ptr(mean), ptr(rstd), ptr(gam), ptr(bet), sc, sh, 3 * C, int(silu), ptr(ya), B, HW, C, G,
                                   stream()) == 0
    out = {"y": sha(y), "mean": sha(mean), "rstd": sha(rstd), "apply_y": sha(ya)}
    for grad_beta in (0.0, 1.0):
        dx = torch.full((B * HW, C), 7.0, device=DEV, dtype=td)
        dg, db = old_g.clone(), old_b.clone()
        demb = torch.full((B, 3 * C), 7.0, device=DEV)
        ws.fill_(float("nan"))
        assert lib.vaw_groupnorm_bwd(dt, ptr(dout), ptr(x), ptr(mean), ptr(rstd), ptr(gam), ptr(bet), sc, sh, 3 * C, int(silu),
                                     ptr(dadd) if add else None, ptr(dx), ptr(dg), ptr(db), grad_beta, (ptr(demb) + 4 * C) if film else None,
                                     (ptr(demb) + 8 * C) if film else None, 3 * C, B, HW, C, G, ptr(ws), stream()) == 0
        out.update({f"dgamma_beta{int(grad_beta)}": sha(dg), f"dbeta_beta{int(grad_beta)}": sha(db)})
        if grad_beta == 0.0:
            out["dx"] = sha(dx)
            if film:
                out["dscale_dshift"] = sha(demb)
        else:
            assert out["dx"] == sha(dx), "dx depends on grad_beta"
    return out


def compute(pkg, group):
    """{case name: {output name: sha256}} of one of GROUPS with the package `pkg` (vaw_amd of the tree under test)."""
    L = pkg._lib
    dt, switch, shapes = GROUPS[group]
    res = {}
    try:
        for i, (shape, flags) in enumerate(shapes):
            for film, silu, add in flags:
                L.lib().vaw_debug_gn_flat(-1)
                name = "{}/B{}_HW{}_C{}_G{}/film{:d}_silu{:d}_add{:d}".format(group, *shape, film, silu, add)
                res[name] = run_case(L, dt, switch, shape, film, silu, add, seed=1000 + i)
    finally:
        L.lib().vaw_debug_gn_flat(-1)
    torch.cuda.synchronize()
    return res


def main():
    tree = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--tree" or a.startswith("--tree=")]
    out = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--out" or a.startswith("--out=")]
    sys.path.insert(0, os.path.abspath(tree[0]) if tree else os.path.dirname(os.path.dirname(HERE)))
    import vaw_amd
    print("package:", os.path.dirname(os.path.abspath(vaw_amd.__file__)), flush=True)
    bits = {}
    for group in GROUPS:
        first, second = compute(vaw_amd, group), compute(vaw_amd, group)
        if first != second:
            sys.exit(f"{group}: two runs of the same tree differ in {[c for c in first if first[c] != second[c]]}: nothing written")
        bits.update(first)
        print(f"  {group}: {len(first)} cases, twice the same", flush=True)
    path = out[0] if out else os.path.join(HERE, "gn_bits.json")
    with open(path, "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(bits)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
