#!/usr/bin/env python3
"""Step time and peak memory of a DiT or UNet training step with activation recomputation off and on.

    python tools/ckpt_bench.py --model DiT-XL --patch 2 --latent 64 --batch 256 [--steps 10 --warmup 3]
    python tools/ckpt_bench.py --model ADM_64 --batch 256          (UNet_32 ADM_32 UNet_64 ADM_64 ADM_128 ADM_256 ADM_512 LDM)

Each mode runs in a child process of its own (a clean allocator, and one mode's workspace never sits beside the other's).  A
mode whose workspace plan (ops.dit_ws_plan) plus an estimate of the parameter / optimizer state exceeds the free memory of the card is reported as
"does not fit" WITHOUT being tried (--force tries anyway).  One JSON line per mode (step_ms: median over --steps optimizer steps,
HIP events; fwd_ms: the model's forward alone, the part recomputation runs twice), then one summary line.  The UNets have no
workspace plan: nothing is predicted for them, a mode that does not fit ends as "out of memory" (the child catches it)."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


UNETS = ("UNet_32", "ADM_32", "UNet_64", "ADM_64", "ADM_128", "ADM_256", "ADM_512", "LDM")


def child_unet(a, ckpt):
    import copy

    import torch

    import bench
    import vaw_amd
    dev = torch.device("cuda", 0)
    torch.manual_seed(42)
    cond = a.model.startswith(("ADM", "LDM"))
    model = getattr(vaw_amd, a.model)(num_classes=1000, class_cond=cond, dropout=a.dropout, use_checkpoint=ckpt,
                                      compute_dtype="fp32" if a.fp32 else "bf16")
    S, C = model.image_size, model.in_channels
    free, total = torch.cuda.mem_get_info(dev)
    rec = dict(mode="on" if ckpt else "off", model=a.model, latent=S, batch=a.batch, dtype="f32" if a.fp32 else "bf16",
               dropout=a.dropout, params=sum(p.numel() for p in model.parameters()), card_free=free, card_total=total, plan_total=0)
    try:
        model = model.to(dev)
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():          # the zero-initialised convs would make every block an identity
            for p in model.parameters():
                if p.requires_grad:
                    p.add_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
        ema_model = copy.deepcopy(model)
        args = bench.make_args(in_chans=C, dataset="Latent" if C == 4 else "CelebA", image_size=S, class_cond=cond, amp=not a.fp32,
                               activation_checkpointing=ckpt, hip_graph=False)
        opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
        diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                         model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                         loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
        gb = torch.Generator().manual_seed(3)

        def batch():
            if C == 4:          # latent models read cat[mean, std] of the VAE posterior
                x = torch.cat([torch.randn(a.batch, 4, S, S, generator=gb) * 4, torch.rand(a.batch, 4, S, S, generator=gb) * 1.45 + 0.05], 1)
            else:
                x = torch.rand(a.batch, C, S, S, generator=gb) * 2 - 1
            return x.to(dev), torch.randint(0, 1000, (a.batch,), generator=gb).to(dev)
        batches = [batch() for _ in range(2)]
        tr = vaw_amd.Trainer(args, dev, model, ema_model, opt, sched, diff, bench._Loader(batches))
        assert model.activation_checkpointing is bool(ckpt)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for s in range(a.warmup):
            tr.train_step(s + 1)
        torch.cuda.synchronize()
        times = []
        for s in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = tr.train_step(a.warmup + s + 1)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        peak = torch.cuda.max_memory_allocated()
        xf, tf = torch.randn(a.batch, C, S, S, device=dev), torch.rand(a.batch, device=dev) * 999
        fwd = []
        with torch.no_grad():          # the forward alone: what the recomputation repeats (less the GroupNorm statistics passes)
            for _ in range(max(3, a.steps // 2)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model(xf, tf, y=batches[0][1]) if cond else model(xf, tf)
                e1.record()
                e1.synchronize()
                fwd.append(e0.elapsed_time(e1))
        fwd.sort()
        rec.update(status="ok", step_ms=round(times[len(times) // 2], 3), step_ms_min=round(times[0], 3), step_ms_max=round(times[-1], 3),
                   fwd_ms=round(fwd[len(fwd) // 2], 3), loss=float(loss), max_memory_allocated=peak, allocated_before_steps=base,
                   img_per_s=round(1e3 * a.batch / times[len(times) // 2], 1))
    except torch.OutOfMemoryError as e:
        rec.update(status="out of memory", why=str(e).splitlines()[0][:200], max_memory_allocated=torch.cuda.max_memory_allocated())
    print(json.dumps(rec), flush=True)


def child(a, ckpt):
    if a.model in UNETS:
        return child_unet(a, ckpt)
    import torch

    import bench
    import vaw_amd
    from vaw_amd import _lib as L
    from vaw_amd import ops
    dev = torch.device("cuda", 0)
    torch.manual_seed(42)
    model = vaw_amd.DiT_models[a.model](image_size=a.latent, patch_size=a.patch, in_channels=4, class_dropout_prob=0.0, num_classes=1000,
                                        learn_sigma=False, compute_dtype="fp32" if a.fp32 else "bf16", activation_checkpointing=ckpt)
    plan = ops.dit_ws_plan(L.F32 if a.fp32 else L.BF16, a.batch, model.T, model.D, model.Dm, model.depth, model.num_heads, model.Kp,
                           model.No, True, ckpt)
    n_par = sum(p.numel() for p in model.parameters())
    # A HEURISTIC for the "does not fit" pre-check only (masters, gradients, AdamW moments, EMA, bf16 shadow); what a step really
    # takes is the max_memory_allocated of a mode that ran
    state = n_par * (4 + 4 + 8 + 4 + (0 if a.fp32 else 2))
    free, total = torch.cuda.mem_get_info(dev)
    rec = dict(mode="on" if ckpt else "off", model=f"{a.model}/{a.patch}", latent=a.latent, batch=a.batch, tokens=a.batch * model.T,
               dtype="f32" if a.fp32 else "bf16", plan_total=plan.total, plan_blocks=model.depth * (plan.block_bytes + plan.block_stat_bytes),
               plan_shared=plan.shared_bytes, state_bytes_estimate=state, card_free=free, card_total=total)
    if plan.total + state > free and not a.force:
        rec.update(status="does not fit", why=f"plan {plan.total / 1e9:.1f} GB + estimated state {state / 1e9:.1f} GB > free {free / 1e9:.1f} GB (not tried)")
        print(json.dumps(rec), flush=True)
        return
    model = model.to(dev)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():          # adaLN-Zero would make every block an identity
        for p in model.parameters():
            if p.requires_grad:
                p.add_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
    import copy
    ema_model = copy.deepcopy(model)
    args = bench.make_args(image_size=a.latent, amp=not a.fp32, activation_checkpointing=ckpt, hip_graph=False)
    opt = vaw_amd.FusedAdamW(model, lr=args.lr, betas=(0.9, 0.95), weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    diff = vaw_amd.GaussianDiffusion(args=args, betas=vaw_amd.get_named_beta_schedule("cosine", 1000),
                                     model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    gb = torch.Generator().manual_seed(3)
    S = a.latent
    batches = [(torch.cat([torch.randn(a.batch, 4, S, S, generator=gb) * 4, torch.rand(a.batch, 4, S, S, generator=gb) * 1.45 + 0.05], 1).to(dev),
                torch.randint(0, 1000, (a.batch,), generator=gb).to(dev)) for _ in range(2)]
    tr = vaw_amd.Trainer(args, dev, model, ema_model, opt, sched, diff, bench._Loader(batches))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        for s in range(a.warmup):
            tr.train_step(s + 1)
        torch.cuda.synchronize()
        times = []
        for s in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = tr.train_step(a.warmup + s + 1)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        # the forward alone (no_grad, same workspace): the share of the step that recomputation runs a second time
        xf, tf = torch.randn(a.batch, 4, S, S, device=dev), torch.rand(a.batch, device=dev) * 999
        fwd = []
        with torch.no_grad():
            for _ in range(max(3, a.steps // 2)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model(xf, tf, batches[0][1])
                e1.record()
                e1.synchronize()
                fwd.append(e0.elapsed_time(e1))
        fwd.sort()
        rec.update(fwd_ms=round(fwd[len(fwd) // 2], 3))
        rec.update(status="ok", step_ms=round(times[len(times) // 2], 3), step_ms_min=round(times[0], 3), step_ms_max=round(times[-1], 3),
                   loss=float(loss), max_memory_allocated=torch.cuda.max_memory_allocated(), allocated_before_steps=base,
                   workspace_bytes=model._ws_cur.nbytes(), img_per_s=round(1e3 * a.batch / times[len(times) // 2], 1))
    except torch.OutOfMemoryError as e:
        rec.update(status="out of memory", why=str(e).splitlines()[0][:200], max_memory_allocated=torch.cuda.max_memory_allocated())
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="DiT-B", choices=["DiT-S", "DiT-B", "DiT-L", "DiT-XL"] + list(UNETS))
    ap.add_argument("--patch", type=int, default=4)
    ap.add_argument("--latent", type=int, default=32, help="latent side: 32 = 256 px images, 64 = 512 px")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--dropout", type=float, default=0.0, help="UNets: nn.Dropout inside the ResBlocks (device RNG)")
    ap.add_argument("--force", action="store_true", help="try a mode even when its plan says it does not fit")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--child", default=None, choices=["off", "on"], help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per mode")
    a = ap.parse_args()
    if a.child:
        child(a, a.child == "on")
        return 0
    recs = {}
    for mode in a.modes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + [x for x in sys.argv[1:]]
        t0 = time.time()
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:          # (run() has killed and reaped the child)
            print(f"[ckpt_bench] mode {mode}: child still running after {a.timeout} s, killed; stopping", file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            print(f"[ckpt_bench] mode {mode}: child exited with {r.returncode} after {time.time() - t0:.0f} s; stopping", file=sys.stderr)
            print(r.stdout[-2000:], file=sys.stderr)
            return 1                       # nothing more is started on the card after a failed child
        recs[mode] = json.loads(line[-1])
        print(line[-1], flush=True)
    if all(recs.get(m, {}).get("status") == "ok" for m in ("off", "on")):
        off, on = recs["off"], recs["on"]
        print(json.dumps(dict(summary=f"{off['model']} latent {off['latent']} batch {off['batch']} {off['dtype']}",
                              step_ms_off=off["step_ms"], step_ms_on=on["step_ms"], step_ratio=round(on["step_ms"] / off["step_ms"], 4),
                              fwd_ms=off["fwd_ms"], fwd_share_of_step=round(off["fwd_ms"] / off["step_ms"], 4),
                              peak_gb_off=round(off["max_memory_allocated"] / 1e9, 3), peak_gb_on=round(on["max_memory_allocated"] / 1e9, 3),
                              plan_gb_off=round(off["plan_total"] / 1e9, 3), plan_gb_on=round(on["plan_total"] / 1e9, 3))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
