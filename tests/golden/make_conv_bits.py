#!/usr/bin/env python3
"""Generate tests/golden/conv_bits.json: sha256 of the bytes vaw_conv3x3 writes, recorded on the MI355X from the commit BEFORE its
checks and launch choices moved into vaw_conv3x3_plan.  tests/test_gpu_conv_bits.py recomputes the same cases at head and compares
the hashes.

    python tests/golden/make_conv_bits.py --tree <checkout of the commit to record, built in place> [--out FILE]

(or, ops.conv3x3 being the same Python on both sides, this tree with VAW_HIP_LIB naming that commit's libvaw_hip.so: how the
committed file was made)

The cases are the parity table of tests/conv_parity.py (this tree's, whatever --tree says): every kernel, mode, tile width,
epilogue, reduce and bias-gradient path, on that table's seeded inputs.  Only what exists on both sides of the change is called:
ops.conv3x3 and the vaw_debug_gemm_tile switch.  No tensor is stored: a case is a name and one hash per output (C = y, dx or dW;
colsum; rowsum = the bias gradient), or "declined" where vaw_conv3x3 leaves the shape to the explicit path.  The scratch workspace is
NaN-filled before every call.  Every group is computed twice and nothing is written if the two runs differ (the kernels sum in a
fixed order, so they should not)."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conv_parity as cp      # noqa: E402

DEV = "cuda"
GROUPS = ("geo", "ragged", "ch", "epi", "bg", "split", "byshape")       # the first word of a case's name
TDT = {"bf16": torch.bfloat16, "f32": torch.float32}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(pkg, c):
    """{output name: sha256} of one launch of the case, or "declined\""""
    L, ops = pkg._lib, pkg.ops
    t = cp.make_inputs(c)
    gc = cp.gemm_case(c)
    dev = lambda name, dt: t[name].to(TDT[dt]).to(DEV).contiguous()
    mode = c["mode"]
    ten = {"act": dev("x" if mode == 0 else "dy", "bf16")}
    if mode == 2:
        ten["act2"] = dev("x", "bf16")
    else:
        ten["w"] = dev("w", "bf16")
    if c["bias"]:
        ten["bias"] = dev("bias", "f32")
    if c["resid"]:
        ten["resid"] = dev("resid", "bf16" if c["resid"] == "act" else "f32")
    ten["out"] = dev("C_old", "f32") if c["beta"] != 0.0 else torch.full((gc["M"], gc["N"]), 7.0, device=DEV, dtype=TDT[cp.out_dt(c)])
    if c["colsum"]:
        ten["colsum_out"] = dev("colsum_old", "f32")
    if c["rowsum"]:
        ten["rowsum_a_out"] = dev("rowsum_old", "f32")
    args, kw = cp.plan_call(c, {k: v.data_ptr() for k, v in ten.items()})
    ops.scratch_f32(torch.device(DEV, torch.cuda.current_device()), 0).fill_(float("nan"))
    L.lib().vaw_debug_gemm_tile(c["tile"])
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ran = ops.conv3x3(*args, **kw)
    finally:
        L.lib().vaw_debug_gemm_tile(-1)
    torch.cuda.synchronize()
    if not ran:
        return "declined"
    out = {"C": sha(ten["out"])}
    if c["colsum"]:
        out["colsum"] = sha(ten["colsum_out"])
    if c["rowsum"]:
        out["rowsum"] = sha(ten["rowsum_a_out"])
    return out


def compute(pkg, group):
    """{case name: {output name: sha256} | "declined"} of the cases of one of GROUPS with the package `pkg` (vaw_amd of the tree under test)"""
    return {n: run_case(pkg, c) for n, c in cp.CASES.items() if n.split("_")[0] == group}


def main():
    tree = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--tree" or a.startswith("--tree=")]
    out = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--out" or a.startswith("--out=")]
    sys.path.insert(0, os.path.abspath(tree[0]) if tree else os.path.dirname(os.path.dirname(HERE)))
    import vaw_amd
    print("package:", os.path.dirname(os.path.abspath(vaw_amd.__file__)), "library:", vaw_amd._lib.LIB_PATH, flush=True)
    bits = {}
    for group in GROUPS:
        first, second = compute(vaw_amd, group), compute(vaw_amd, group)
        if first != second:
            sys.exit(f"{group}: two runs of the same tree differ in {[c for c in first if first[c] != second[c]]}: nothing written")
        bits.update(first)
        print(f"  {group}: {len(first)} cases, twice the same", flush=True)
    assert set(bits) == set(cp.CASES)
    path = out[0] if out else os.path.join(HERE, "conv_bits.json")
    with open(path, "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(bits)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
