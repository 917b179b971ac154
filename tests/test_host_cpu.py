"""CPU-only checks of the product package: the C ABI loads and exports what include/vaw_hip.h declares, the
host-side mirror of the reference interface (schedules, weight tables, samplers, LR schedule, flat parameter
storage, checkpoints) matches the golden fixtures, and the HIP path refuses to run without a GPU instead of
falling back.  No kernel is launched here."""
import copy
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN, REPO, base_args, load_json, load_pt

import vaw_amd
from vaw_amd import gaussian_diffusion as gd
from oracle import diffusion as od
from oracle import dit as odit


def test_c_abi_exports_every_declared_symbol():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    declared = set(re.findall(r"\b(vaw_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"vaw_epilogue", "vaw_attn_desc"}
    assert len(declared) >= 30
    lib = vaw_amd.lib()
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, f"libvaw_hip.so does not export {missing}"
    assert set(vaw_amd.exported_symbols()) <= declared | {"vaw_version", "vaw_last_error_string"}
    assert lib.vaw_version() >= 100 and isinstance(lib.vaw_last_error_string(), bytes)


_CONSTANT_ALIASES = {"VAW_ATTN_DIR_FWD": "ATTN_FWD", "VAW_ATTN_DIR_BWD": "ATTN_BWD", "VAW_ATTN_DIR_BWD_COLSUM": "ATTN_BWD_COLSUM"}


def test_binding_agrees_with_an_independent_reading_of_every_declaration():
    """Every function, struct, enumerator and #define of include/vaw_hip.h, read by the regular expressions of tests/abi_cases.py
    (vaw_amd._abi is not asked): each function is exported by the built library and bound with the restype and argtypes its
    prototype spells, each struct has a Structure class with the fields in order and kind, each constant has its Python name."""
    import ctypes as C
    import abi_cases as ac
    from vaw_amd import _lib, ops
    code, structs, kind = ac.CODE, ac.STRUCTS, ac.kind
    assert len(ac.ENUMS) == 14 and set(structs) == set(ac.STRUCT_CLASSES)
    names = [n for _, n, _ in ac.PROTOS]
    assert len(names) == len(set(names)) >= 141 and sorted(names) == vaw_amd.exported_symbols()
    assert {"vaw_debug_force_rowwise_attention", "vaw_debug_force_generic_gemm", "vaw_debug_gemm_tile", "vaw_debug_gn_flat",
            "vaw_debug_cu_hog"} <= set(names)
    lib, raw = vaw_amd.lib(), C.CDLL(vaw_amd.LIB_PATH)
    typed = 0
    for name in names:
        assert hasattr(raw, name), f"libvaw_hip.so does not export {name}"
        assert name in vars(lib), f"{name} is not bound"
        want = ac.assert_bound_as_declared(lib, name)
        typed += sum(t is not C.c_void_p and issubclass(t, C._Pointer) for t in want)
    assert typed >= 24          # the struct pointers and the five _host arrays: the rule above is not vacuous
    for cname, body in structs.items():
        cls = getattr(_lib, ac.STRUCT_CLASSES[cname])
        assert issubclass(cls, C.Structure) and getattr(ops, ac.STRUCT_CLASSES[cname], cls) is cls
        fields = []
        for decl in body.split(";")[:-1]:
            ctype, first = " ".join(decl.split(",")[0].split()).rsplit(" ", 1)
            for f in [first] + [f.strip() for f in decl.split(",")[1:]]:
                # vaw_epilogue.colsum_rows_out is the one HOST address among the fields (read and written by vaw_gemm's host side)
                fields.append((f, kind(ctype, f, host=(cname, f) == ("vaw_epilogue", "colsum_rows_out"))))
        assert cls._fields_ == fields, (cname, cls._fields_, fields)
    # sizeof, as a C compiler prints it for the header on x86-64
    sizes = {"vaw_epilogue": 128, "vaw_wgrad_problem": 88, "vaw_fp8_quant_job": 72, "vaw_gemm_knobs": 64, "vaw_gemm_launch": 104,
             "vaw_gemm_fp8_launch": 88, "vaw_reduce_job": 32, "vaw_row_launch": 40, "vaw_attn_desc": 88, "vaw_attn_launch": 56,
             "vaw_gn_launch": 96, "vaw_conv3x3_launch": 112, "vaw_cast_colsum_launch": 32, "vaw_dit_ws_plan_t": 72}
    assert {c: C.sizeof(getattr(_lib, p)) for c, p in ac.STRUCT_CLASSES.items()} == sizes
    constants = re.findall(r"\b(VAW_[A-Z0-9_]+) = (-?\d+)", code) + re.findall(r"#define (VAW_\w+) (-?\d+)\n", code)
    assert len(constants) >= 75 and len(set(n for n, _ in constants)) == len(constants)
    for cname, value in constants:
        assert getattr(_lib, _CONSTANT_ALIASES.get(cname, cname[4:])) == int(value), cname
    assert (_lib.F32, _lib.BF16, _lib.ERR_INVALID, _lib.GV_WARP_SPEC, _lib.ROW_GATE_LN_FWD, _lib.RESAMPLER_MAX_T) == (0, 1, -1, 7, 8, 4096)
    assert _lib.AV_NAMES[_lib.AV_BWD_BIG_NT4] == "bwd_big_nt4" and _lib.GV_NAMES[_lib.GV_RING256] == "ring256"
    assert _lib.CVR_NAMES == ("CVR_NONE", "CVR_F32", "CVR_F32_ROWSUM", "CVR_SLAB_T") and _lib.CVB_NAMES[3] == "CVB_SEPARATE"


def test_header_parser_reads_the_subset_and_refuses_the_rest():
    from vaw_amd._abi import AbiError, Type, parse
    h = parse("""
        typedef enum { VAW_A = 0, VAW_B = -3 } vaw_kind;
        typedef struct { int a, b; const float* p; int64_t n; } vaw_job;
        /* int vaw_not_declared(int x); */
        // int vaw_not_declared_either(int x);
        #define VAW_COLS 12
        int vaw_nothing(void);
        int64_t vaw_count(vaw_kind kind, const vaw_job* jobs, vaw_stream stream);
        const char* vaw_text(void);
        void vaw_split(
            int a,
            const double* b_host
            , float c);
    """)
    assert h.structs == {"vaw_job": [("a", Type("int", False)), ("b", Type("int", False)), ("p", Type("float", True)), ("n", Type("int64_t", False))]}
    assert h.enums == {"vaw_kind": {"VAW_A": 0, "VAW_B": -3}} and h.defines == {"VAW_COLS": 12}
    assert sorted(h.functions) == ["vaw_count", "vaw_nothing", "vaw_split", "vaw_text"]
    assert h.functions["vaw_nothing"] == (Type("int", False), [])
    assert h.functions["vaw_count"] == (Type("int64_t", False), [(Type("vaw_kind", False), "kind"), (Type("vaw_job", True), "jobs"),
                                                                 (Type("vaw_stream", False), "stream")])
    assert h.functions["vaw_text"] == (Type("char", True), [])
    assert h.functions["vaw_split"] == (Type("void", False), [(Type("int", False), "a"), (Type("double", True), "b_host"), (Type("float", False), "c")])
    for bad, line, what in (("int vaw_f(size_t n);", 1, "unknown type 'size_t'"),
                            ("int vaw_f(int a);\n\nunsigned vaw_g(void);", 3, "unknown type 'unsigned'"),
                            ("int vaw_f(int a);\nstruct s { int a; };", 2, "unrecognised construct"),
                            ("int vaw_f(int a)\nint vaw_g(void);", 1, "unrecognised construct"),
                            ("int vaw_f(void (*cb)(int));", 1, "unrecognised construct"),
                            ("int vaw_f(int a, b);", 1, "unrecognised declarator"),
                            ("typedef struct { float *a, *b; } vaw_s;", 1, "unrecognised declarator"),
                            ("typedef enum { VAW_A = 0, VAW_B } vaw_e;", 1, "enumerator 'VAW_B'"),
                            ("int vaw_f(void);\nint vaw_f(void);", 2, "vaw_f is declared twice"),
                            ("\n#pragma once", 2, "unrecognised preprocessor line"),
                            ("#define VAW_X (1 << 4)", 1, "unrecognised preprocessor line"),
                            ("int vaw_f(int a);\nstatic const int k = 3;", 2, "unrecognised")):
        with pytest.raises(AbiError, match=re.escape(f"include/vaw_hip.h:{line}: {what}")):
            parse(bad)


def test_no_cpu_fallback():
    m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=1, num_heads=2, num_classes=10)
    with pytest.raises(vaw_amd.VawError):
        m(torch.zeros(2, 4, 8, 8), torch.zeros(2), torch.zeros(2, dtype=torch.long))
    d = _prod()
    with pytest.raises(vaw_amd.VawError):
        d.q_sample(torch.zeros(2, 3, 4, 4), torch.zeros(2, dtype=torch.long))
    with pytest.raises(vaw_amd.VawError):
        vaw_amd.ops.timestep_embedding(torch.zeros(3), 8)


def _prod(sched="cosine", mt="EPSILON", wt="lambda", **kw):
    return vaw_amd.GaussianDiffusion(args=base_args(weight_type=wt, **kw), betas=vaw_amd.get_named_beta_schedule(sched, 1000),
                                     model_mean_type=vaw_amd.ModelMeanType[mt], model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                     loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)


def test_schedule_tables_bit_exact():
    g = np.load(os.path.join(GOLDEN, "diffusion_tables.npz"))
    for sched in ("linear", "cosine", "linear_logsnr"):
        d = _prod(sched)
        for k in g.files:
            if k.startswith(sched + "."):
                np.testing.assert_array_equal(getattr(d, k.split(".", 1)[1]), g[k], err_msg=k)
    np.testing.assert_array_equal(vaw_amd.get_named_beta_schedule("linear", 250), g["linear250.betas"])
    with pytest.raises(NotImplementedError):
        vaw_amd.get_named_beta_schedule("nope", 10)
    assert _prod()._scale_timesteps(torch.tensor([3])).dtype == torch.float32


def test_loss_weight_function_and_device_table():
    rec = load_json("loss_weight.json")
    t = torch.tensor(rec["t"])
    d0 = _prod()
    for key, exp in rec["diffusion"].items():
        mt, wt = key.split("/")
        a = gd._extract_into_tensor(d0.sqrt_alphas_cumprod, t, t.shape).clone()
        s = gd._extract_into_tensor(d0.sqrt_one_minus_alphas_cumprod, t, t.shape).clone()
        if "error" in exp:
            with pytest.raises(ValueError):
                vaw_amd.compute_mse_loss_weight(vaw_amd.ModelMeanType[mt], wt, t, a, s, 1, 1)
            continue
        w = vaw_amd.compute_mse_loss_weight(vaw_amd.ModelMeanType[mt], wt, t, a, s, 1, 1)
        assert str(w.dtype) == exp["dtype"]
        np.testing.assert_array_equal(w.double().numpy(), np.array(exp["w"]), err_msg=key)
        if mt != "VECTOR":
            # the resident f32 weight table the kernels gather from == the reference's per-batch arithmetic
            tb = _prod(mt=mt, wt=wt)._tables("cpu")
            np.testing.assert_array_equal(tb["w"][t].double().numpy(), np.array(exp["w"], dtype=np.float64), err_msg=key)
    tf = torch.tensor(rec["flow_t"], dtype=torch.float32)
    for key, exp in rec["flow"].items():
        parts = key.split("/")
        fm = vaw_amd.FlowMatching(args=base_args(path_type=parts[0]), model_mean_type=vaw_amd.ModelMeanType.VECTOR)
        if parts[1] == "interpolant":
            for n, v in zip(("a", "s", "da", "ds"), fm.interpolant(tf)):
                np.testing.assert_array_equal(v.double().numpy(), np.array(exp[n]), err_msg=key + n)
    # oracle and product agree on every table entry for the recipe used by run.sh
    o = od.GaussianDiffusion(args=base_args(), betas=od.get_named_beta_schedule("cosine", 1000),
                             model_mean_type=od.ModelMeanType.EPSILON, model_var_type=od.ModelVarType.FIXED_LARGE,
                             loss_type=od.LossType.MSE, rescale_timesteps=True)
    tall = torch.arange(1000)
    w_ref = od.compute_mse_loss_weight(od.ModelMeanType.EPSILON, "lambda", tall, od.extract(o.sqrt_alphas_cumprod, tall, tall.shape).clone(),
                                       od.extract(o.sqrt_one_minus_alphas_cumprod, tall, tall.shape).clone())
    assert torch.equal(_prod()._tables("cpu")["w"], w_ref)


def test_unsupported_objectives_raise():
    x = torch.zeros(2, 3, 4, 4)
    # learned variance / KL losses are built on the HIP path: on CPU tensors they fail loudly, never fall back
    d = vaw_amd.GaussianDiffusion(args=base_args(), betas=vaw_amd.get_named_beta_schedule("cosine", 10),
                                  model_mean_type=vaw_amd.ModelMeanType.EPSILON,
                                  model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.KL)
    with pytest.raises(vaw_amd.VawError):
        d.training_losses(lambda *a, **k: x, x, t=torch.zeros(2, dtype=torch.long), noise=x)
    # the per-timestep table the variational-bound kernel reads (columns 2, 3, 4, 5, 0, 1, 11 of the one reverse-process table) =
    # the reference's float64 tables cast like _extract_into_tensor
    for vt, mt in (("LEARNED_RANGE", "EPSILON"), ("FIXED_LARGE", "START_X"), ("FIXED_SMALL", "EPSILON")):
        kw = dict(args=base_args(), betas=vaw_amd.get_named_beta_schedule("linear", 50), loss_type=vaw_amd.LossType.MSE)
        d = vaw_amd.GaussianDiffusion(model_mean_type=vaw_amd.ModelMeanType[mt], model_var_type=vaw_amd.ModelVarType[vt], **kw)
        o = od.GaussianDiffusion(args=base_args(), betas=od.get_named_beta_schedule("linear", 50), loss_type=od.LossType.MSE,
                                 model_mean_type=od.ModelMeanType[mt], model_var_type=od.ModelVarType[vt])
        tab, tall = d._sample_table(), torch.arange(50)
        ex = lambda arr: od.extract(arr, tall, tall.shape)
        assert torch.equal(tab[:, 2], ex(o.posterior_mean_coef1)) and torch.equal(tab[:, 3], ex(o.posterior_mean_coef2))
        assert torch.equal(tab[:, 4], ex(o.posterior_log_variance_clipped))
        aux = {"LEARNED_RANGE": np.log(o.betas), "FIXED_SMALL": o.posterior_log_variance_clipped,
               "FIXED_LARGE": np.log(np.append(o.posterior_variance[1], o.betas[1:]))}[vt]
        assert torch.equal(tab[:, 5], ex(aux))
        if mt == "EPSILON":
            assert torch.equal(tab[:, 0], ex(o.sqrt_recip_alphas_cumprod)) and torch.equal(tab[:, 1], -ex(o.sqrt_recipm1_alphas_cumprod))
        assert tab[:, 11].tolist() == [1.0] + [0.0] * 49
    d = vaw_amd.GaussianDiffusion(args=base_args(), betas=vaw_amd.get_named_beta_schedule("cosine", 10),
                                  model_mean_type=vaw_amd.ModelMeanType.VELOCITY,
                                  model_var_type=vaw_amd.ModelVarType.FIXED_LARGE, loss_type=vaw_amd.LossType.KL)
    with pytest.raises(RuntimeError):       # as the reference (:394-399)
        d._vb_terms_bpd(x, None, x, x, torch.zeros(2, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        _prod(time_dist=["lognorm", 0, 1]).sample_t(x)
    with pytest.raises(NotImplementedError):
        vaw_amd.DiT(image_size=8, patch_size=2, hidden_size=64, depth=1, num_heads=2, learn_align=True)


def test_lr_schedule_samplers_latent_sampling():
    rec = load_json("misc.json")
    for s, a, b, c in rec["lr"]:
        assert vaw_amd.warmup_cosine_lr(s, 5, 50, 1e-4, 1e-6, True) == a
        assert vaw_amd.warmup_cosine_lr(s, 5, 50, 1e-4, 1e-6, False) == b
        assert vaw_amd.warmup_cosine_lr(s, 0, 50, 1e-4, 0.0, True) == c
    from types import SimpleNamespace
    diff = SimpleNamespace(num_timesteps=20)
    s = vaw_amd.create_named_schedule_sampler("loss-second-moment", diff)
    assert s.weights().tolist() == rec["lsm_weights_before"]
    rng = np.random.RandomState(0)
    for _ in range(15):
        s.update_with_all_losses(list(range(20)), (rng.rand(20) * (1 + np.arange(20))).tolist())
    np.testing.assert_allclose(s.weights(), rec["lsm_weights_after"], rtol=1e-14)
    np.random.seed(3)
    idx, w = s.sample(16, "cpu")
    assert idx.tolist() == rec["lsm_sample_idx"]
    np.testing.assert_allclose(w.double().numpy(), rec["lsm_sample_w"], rtol=1e-6)
    s.update_with_local_losses(torch.tensor([1, 2]), torch.tensor([0.5, 0.25]))     # single-process branch
    u = vaw_amd.create_named_schedule_sampler("uniform", diff)
    np.random.seed(3)
    idx, w = u.sample(8, "cpu")
    assert idx.tolist() == rec["uni_sample_idx"] and w.double().tolist() == rec["uni_sample_w"]
    with pytest.raises(NotImplementedError):
        vaw_amd.create_named_schedule_sampler("nope", diff)
    lat = torch.tensor(rec["sfl_in"], dtype=torch.float32)
    torch.manual_seed(1)
    assert vaw_amd.sample_from_latent(lat, 0.18215, cpu_rng=True).double().tolist() == rec["sfl_out"]


def test_dit_same_seed_same_weights_and_keys_as_reference():
    g = load_pt("dit_tiny.pt")
    for tag in ("p2", "p4"):
        torch.manual_seed(11)
        p = vaw_amd.DiT(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, **g[f"{tag}/kw"])
        torch.manual_seed(11)
        o = odit.DiT(in_channels=4, class_dropout_prob=0.0, num_classes=10, learn_sigma=False, **g[f"{tag}/kw"])
        sp, so = p.state_dict(), o.state_dict()
        assert list(sp.keys()) == list(so.keys())
        for k in sp:
            assert torch.equal(sp[k], so[k]), k
    b = vaw_amd.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.1, num_classes=1000, learn_sigma=False)
    ob = odit.DiT_B(image_size=32, patch_size=4, in_channels=4, class_dropout_prob=0.1, num_classes=1000, learn_sigma=False)
    assert sum(p.numel() for p in b.parameters()) == sum(p.numel() for p in ob.parameters()) == 130_426_432
    assert b.y_embedder.embedding_table.num_embeddings == 1001


def test_flat_storage_views_groups_deepcopy_state_dict():
    m = vaw_amd.DiT(image_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=2, num_classes=10)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.ensure_flat()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])
    off = m._flat_offsets
    # all adaLN weights are one contiguous [(6L+2)D, D] matrix, biases likewise
    D = 64
    assert off["blocks.1.adaLN_modulation.1.weight"][0] == off["blocks.0.adaLN_modulation.1.weight"][0] + 6 * D * D
    assert off["final_layer.adaLN_modulation.1.weight"][0] == off["blocks.0.adaLN_modulation.1.weight"][0] + 12 * D * D
    assert off["final_layer.adaLN_modulation.1.bias"][0] == off["blocks.0.adaLN_modulation.1.bias"][0] + 12 * D
    p = m.blocks[0].attn.qkv.weight
    assert p.data_ptr() == m._flat.data_ptr() + 4 * off["blocks.0.attn.qkv.weight"][0]
    with torch.no_grad():
        p.add_(1.0)
    o0 = off["blocks.0.attn.qkv.weight"][0]
    assert torch.equal(m._flat[o0:o0 + p.numel()].view_as(p), p)           # in-place updates land in the buffer
    assert off["pos_embed"][0] >= m._flat_n_train                          # frozen entries sit after the trainable range
    bounds = m.grad_stage_bounds()
    covered = sorted(bounds.values())
    assert covered[0][0] == 0 and covered[-1][1] == m._flat_n_train
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))          # buckets tile the gradient buffer exactly
    e = copy.deepcopy(m)
    e.ensure_flat()
    assert e._flat.data_ptr() != m._flat.data_ptr() and e._flat_offsets == m._flat_offsets
    assert all(torch.equal(a, b) for a, b in zip(e.state_dict().values(), m.state_dict().values()))
    e.load_state_dict(before)
    assert torch.equal(e.blocks[0].attn.qkv.weight, before["blocks.0.attn.qkv.weight"])
    m.attach_grads()
    assert m.grads_live() and p.grad.data_ptr() == m.flat_grads().data_ptr() + 4 * o0
    m.zero_grad_flat()
    assert not m.grads_live()


def test_checkpoint_roundtrip_and_module_prefix(tmp_path):
    args = base_args(logdir=str(tmp_path), model="DiT-B", mean_type="EPSILON")
    net = nn.Linear(4, 3)
    ema_net = copy.deepcopy(net)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=vaw_amd.get_lr_lambda(args))
    net(torch.ones(2, 4)).sum().backward()
    opt.step(); sched.step()
    path = vaw_amd.save_checkpoint(args, 7, net, opt, ema_model=ema_net, scheduler=sched)
    assert path.endswith("DiT-B_EPSILON_cosine_7.pth")
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"model", "optimizer", "step", "ema_model", "scheduler"} and ck["step"] == 7

    class Wrapped(nn.Module):          # what a data-parallel wrapper looks like: keys get a 'module.' prefix
        def __init__(self, m):
            super().__init__()
            self.module = m
    net2, ema2 = Wrapped(nn.Linear(4, 3)), nn.Linear(4, 3)
    opt2 = torch.optim.AdamW(net2.parameters(), lr=1e-3)
    got = vaw_amd.load_checkpoint(path, model=net2, optimizer=opt2, ema_model=ema2)
    assert got["step"] == 7 and torch.equal(net2.module.weight, net.weight) and torch.equal(ema2.weight, ema_net.weight)
    path2 = vaw_amd.save_checkpoint(args, 8, net2, opt2)
    assert all(k.startswith("module.") for k in torch.load(path2, weights_only=True)["model"])
    net3 = nn.Linear(4, 3)
    vaw_amd.load_checkpoint(path2, model=net3)                      # prefixed checkpoint into a bare model
    assert torch.equal(net3.weight, net.weight)
    args.parallel = False
    vaw_amd.set_random_seed(args, 5)
    a = torch.rand(3)
    vaw_amd.set_random_seed(args, 5)
    assert torch.equal(a, torch.rand(3))


def test_device_prefetcher_cpu_passthrough():
    """On CPU the prefetcher is a transparent, re-iterable wrapper that keeps batch order and the sampler handle."""
    class _L(list):
        sampler = "S"
    batches = _L((torch.full((2, 3), float(i)), torch.tensor([i, i])) for i in range(5))
    pf = vaw_amd.DevicePrefetcher(batches, "cpu", depth=2)
    for _ in range(2):                                   # re-iterable
        got = list(pf)
        assert len(got) == 5 and all(torch.equal(g[0], b[0]) and torch.equal(g[1], b[1]) for g, b in zip(got, batches))
    assert pf.sampler == "S" and len(pf) == 5


def _standin(x, t, **kw):
    """tests/golden/make_goldens.py::sampling_model (the deterministic stand-in denoiser of the sampler fixtures)."""
    tt = t.float().view(-1, 1, 1, 1)
    m = 0.6 * torch.tanh(x) + 0.1 * torch.sin(tt * 0.01)
    if kw.get("y") is not None:
        m = m + 0.02 * kw["y"].view(-1, 1, 1, 1).float()
    return m


def test_edm_sampler_vs_reference_golden():
    """vaw_amd.EDMDenoiser / edm_sample against tools/cfg_edm.py (Net + ablation_sampler) run on the same stand-in denoiser and CPU
    RNG stream: five (discretization, schedule, scaling, solver, prediction type, chain) combinations incl. the stochastic churn."""
    g = load_pt("samplers.pt")
    for name, rec in g["edm"].items():
        net = vaw_amd.EDMDenoiser(_standin, img_resolution=8, img_channels=3, label_dim=10, **rec["net"])
        assert net.sigma_min == pytest.approx(rec["sigma_min"], rel=1e-6) and net.sigma_max == pytest.approx(rec["sigma_max"], rel=1e-6)
        torch.testing.assert_close(net.u[::100], rec["u_sample"], rtol=1e-6, atol=0)
        torch.manual_seed(321)
        x = vaw_amd.edm_sample(net, g["edm_latents"], class_labels=g["y"], **rec["sampler"])
        assert x.dtype == torch.float64
        torch.testing.assert_close(x, rec["x"], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}: {m}")


def test_flow_sde_sampler_vs_reference_golden_and_ode_grid_solvers():
    g = load_pt("samplers.pt")
    for key, ref in g["flow_sde"].items():
        path, mt, solver = key.split("/")
        fm = vaw_amd.FlowMatching(args=base_args(path_type=path, sampler_type="sde"), model_mean_type=vaw_amd.ModelMeanType[mt], device="cpu")
        torch.manual_seed(77)
        x = vaw_amd.flow_sde_sample(fm, _standin, g["flow_noise"], num_steps=9, solver=solver, y=g["y"])
        # the reference's SDE sampler starts AT t = 1, where alpha_t = 0 (linear, eps-prediction: inf) and the float32 cosine
        # path has g^2 = 2 sigma sigma' < 0 (sqrt -> NaN for every parametrisation): the fixture records those non-finite
        # results and the restatement reproduces them element for element
        torch.testing.assert_close(x, ref, rtol=1e-5, atol=1e-6, equal_nan=True, msg=lambda m: f"{key}: {m}")
        assert torch.equal(torch.isfinite(x), torch.isfinite(ref))
    assert sum(bool(torch.isfinite(v).all()) for v in g["flow_sde"].values()) == 6
    # ODE: fixed-grid solvers converge to one another as the grid refines (torchdiffeq's adaptive dopri5 is refused, not restated)
    fm = vaw_amd.FlowMatching(args=base_args(path_type="linear"), model_mean_type=vaw_amd.ModelMeanType.VECTOR, device="cpu")
    fine = vaw_amd.flow_ode_sample(fm, _standin, g["flow_noise"], num_steps=400, solver="rk4", y=g["y"])
    err = {s: float((vaw_amd.flow_ode_sample(fm, _standin, g["flow_noise"], num_steps=40, solver=s, y=g["y"]) - fine).abs().max())
           for s in ("euler", "midpoint", "heun", "rk4")}
    assert err["rk4"] < 1e-5 and err["heun"] < 2e-3 and err["midpoint"] < 2e-3 and err["euler"] < 5e-2 and err["rk4"] < err["heun"] < err["euler"]
    with pytest.raises(NotImplementedError):
        vaw_amd.flow_ode_sample(fm, _standin, g["flow_noise"], solver="dopri5")
    with pytest.raises(NotImplementedError):
        sc = vaw_amd.FlowMatching(args=base_args(path_type="linear"), model_mean_type=vaw_amd.ModelMeanType.SCORE, device="cpu")
        vaw_amd.flow_ode_sample(sc, _standin, g["flow_noise"], num_steps=3, solver="euler")


@pytest.mark.parametrize("n,world,shuffle,drop_last", [(103, 4, True, False), (103, 4, True, True), (64, 8, False, False), (5, 8, True, False),
                                                       (17, 3, False, True)])
def test_sharded_sampler_equals_torch_distributed_sampler(n, world, shuffle, drop_last):
    """The reference shards its dataset with torch's DistributedSampler (main.py:166-180) and calls set_epoch(step) every step
    (tools/trainer.py:70-71): same index stream per rank and epoch, and the ranks tile the (padded / trimmed) epoch."""
    from torch.utils.data import DistributedSampler
    data = list(range(n))
    for epoch in (0, 3):
        seen = []
        for rank in range(world):
            ref = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=shuffle, seed=7, drop_last=drop_last)
            ref.set_epoch(epoch)
            mine = vaw_amd.ShardedSampler(n, world, rank, shuffle=shuffle, seed=7, drop_last=drop_last)
            mine.set_epoch(epoch)
            assert list(mine) == list(ref) and len(mine) == len(ref)
            seen += list(mine)
        if not drop_last:
            assert set(seen) == set(data)


def test_sharded_sampler_in_a_loader_the_way_trainer_drives_it():
    """The loader contract of Trainer (tools/trainer.py:38,52,70-71): re-iterable, `.sampler.set_epoch(step)` called every step when
    args.parallel.  A minimal batch loader over ShardedSampler, wrapped in DevicePrefetcher (which forwards `.sampler`): the ranks'
    batches of one epoch tile the dataset, and set_epoch through the wrapper reshuffles them."""
    n, world, bs = 40, 2, 5
    data, labels = torch.arange(n).float().view(n, 1), torch.arange(n) % 10

    class Loader:
        def __init__(self, rank):
            self.sampler = vaw_amd.ShardedSampler(n, world, rank, shuffle=True, seed=3)

        def __len__(self):
            return len(self.sampler) // bs

        def __iter__(self):
            idx = list(self.sampler)
            for i in range(0, len(idx) - bs + 1, bs):
                j = torch.tensor(idx[i:i + bs])
                yield data[j], labels[j]

    loaders = [vaw_amd.DevicePrefetcher(Loader(r), "cpu", depth=2) for r in range(world)]
    seen = {}
    for step in (0, 1):
        for ld in loaders:
            ld.sampler.set_epoch(step)            # what Trainer.train_step does first (trainer.py:70-71)
        got = [torch.cat([x.view(-1) for x, _ in ld]).long().tolist() for ld in loaders]
        assert sorted(got[0] + got[1]) == list(range(n)), "the two ranks must tile the epoch"
        seen[step] = got
    assert seen[0] != seen[1], "set_epoch through the prefetcher must reshuffle"
    assert len(loaders[0]) == n // world // bs


@pytest.mark.parametrize("name", ["UNet-32", "ADM-32", "UNet-64", "LDM"])
def test_unet_factories_have_the_reference_structure(name):
    """Every UNet factory of models/unet.py:921-1032 builds (no GPU needed to construct) with the state_dict keys, shapes and
    parameter count of the oracle's factory (itself pinned to the reference by unet_tiny.pt / bigcfg.pt and the nparams goldens).
    Conv weights are kept channels-last inside the flat buffer, but the state_dict speaks the reference's [Co][Ci][3][3]."""
    import vaw_amd
    from oracle import unet as ounet
    kw = dict(num_classes=10, class_cond=True)
    torch.manual_seed(3)
    ref = getattr(ounet, name.replace("-", "_"))(**kw)
    torch.manual_seed(3)
    got = getattr(vaw_amd.unet, name.replace("-", "_"))(compute_dtype="fp32", **kw)
    sd_r, sd_g = ref.state_dict(), got.state_dict()
    assert list(sd_r) == list(sd_g)
    assert all(sd_r[k].shape == sd_g[k].shape for k in sd_r)
    assert sum(p.numel() for p in ref.parameters()) == sum(p.numel() for p in got.parameters())
    for k in list(sd_r)[:8] + list(sd_r)[-8:]:       # same seed, same construction order => same initial weights
        torch.testing.assert_close(sd_g[k], sd_r[k], rtol=0, atol=0)


class _StrictH5Array:
    """Stand-in for an h5py dataset: integer, slice or STRICTLY INCREASING index-array reads only (h5py's fancy-index rule)."""

    def __init__(self, a):
        self.a, self.reads = a, 0

    def __len__(self):
        return len(self.a)

    def __getitem__(self, i):
        self.reads += 1
        if isinstance(i, np.ndarray):
            assert i.ndim == 1 and (np.diff(i) > 0).all(), "h5py wants increasing indices without repeats"
        return self.a[i]


def test_latent_h5_dataset_contract_and_loader():
    """vaw_amd.LatentH5Dataset mirrors the reference's `Latent` dataset (datasets/data_loader.py:62-81; layout written by
    preprocessing/encode_latent.py:95-126: '<split>_latents' f32 [N, 8, 32, 32] = cat[mean, std], '<split>_labels' uint16) on a
    duck-typed handle (h5py is not in this image: real-file parity is unpinned, the contract is what is tested): item dtypes and
    values, one sorted read per array and batch with the rows back in request order (repeats included), the sharded sampler +
    batch loader + prefetcher chain the Trainer consumes, and sample_from_latent on what comes out."""
    import vaw_amd
    rng = np.random.default_rng(0)
    N = 37
    lat = rng.standard_normal((N, 8, 4, 4)).astype(np.float32)
    lab = rng.integers(0, 1000, N).astype(np.uint16)
    h = {"train_latents": _StrictH5Array(lat), "train_labels": _StrictH5Array(lab),
         "val_latents": _StrictH5Array(lat[:5]), "val_labels": _StrictH5Array(lab[:5])}
    ds = vaw_amd.LatentH5Dataset(h, "train")
    assert len(ds) == N and len(vaw_amd.LatentH5Dataset(h, "val")) == 5
    x, y = ds[7]
    assert x.dtype == torch.float32 and y.dtype == torch.long and x.shape == (8, 4, 4)
    assert torch.equal(x, torch.from_numpy(lat[7])) and int(y) == int(lab[7])
    idx = [30, 2, 2, 19, 0, 36, 19]
    r0 = h["train_latents"].reads
    xb, yb = ds.batch(idx)
    assert h["train_latents"].reads == r0 + 1                                  # one read for the whole batch
    assert torch.equal(xb, torch.from_numpy(lat[idx])) and torch.equal(yb, torch.from_numpy(lab[idx].astype(np.int64)))
    # data-parallel input side: rank r of 2 sees its half of every epoch's permutation, batches of 4, last partial batch dropped
    seen = []
    for rank in range(2):
        smp = vaw_amd.ShardedSampler(len(ds), 2, rank, shuffle=True, seed=3)
        loader = vaw_amd.DevicePrefetcher(vaw_amd.LatentBatchLoader(ds, 4, smp), "cpu")
        loader.sampler.set_epoch(5)
        batches = list(loader)
        assert len(batches) == len(loader) == len(smp) // 4
        order = list(smp)
        for k, (xb, yb) in enumerate(batches):
            want = order[4 * k:4 * k + 4]
            assert torch.equal(xb, torch.from_numpy(lat[want])) and torch.equal(yb, torch.from_numpy(lab[want].astype(np.int64)))
            seen += want
    assert len(set(seen)) >= N - 5                                              # the two ranks cover the set (minus the dropped tail)
    z = vaw_amd.sample_from_latent(batches[0][0], 0.18215, cpu_rng=True)
    assert z.shape == (4, 4, 4, 4)
    # the object travels to DataLoader workers before any file is open
    import pickle
    ds2 = pickle.loads(pickle.dumps(vaw_amd.LatentH5Dataset({"train_latents": lat, "train_labels": lab})))
    assert torch.equal(ds2[3][0], torch.from_numpy(lat[3]))
    with pytest.raises(ValueError):
        vaw_amd.LatentH5Dataset({"train_latents": lat, "train_labels": lab[:-1]})


# ------------------------------------------------------------------------------------------------
# Launch plan of the row kernels (vaw_row_plan: host arithmetic only, the launchers take every choice from it)
# ------------------------------------------------------------------------------------------------
ROW_LDS_MAX = 160 * 1024          # gfx950: LDS per CU


def _row_bound(p):
    """__launch_bounds__ of the variant (layernorm.hip); the register-fused kernel drops to 512 threads from NV = 4 on"""
    from vaw_amd import _lib as L
    if p.variant == L.RV_ROW_FUSE:
        return 512 if p.nv > 3 else 1024
    return {L.RV_LN_FWD: 256, L.RV_ROW_BWD: 1024, L.RV_ROW_GATE: 1024, L.RV_ROW_FUSE8: 512}.get(p.variant, 256)


def test_row_plan_sweep_respects_lds_launch_bounds_chunking_and_workspace():
    """Every entry point, D = 4 ... 2048: the LDS a launch asks for fits a CU, the block fits the variant's launch bounds, the chunks
    cover the T rows with none empty, vaw_row_bwd_workspace_floats is enough for the chunking the plan wants, and the fused pass
    cuts rows exactly as the pair it replaces (nc and waves) wherever it promises bitwise equality with it (D <= 1280)."""
    from vaw_amd import _lib as L
    from vaw_amd.ops import row_plan
    lib = vaw_amd.lib()
    bwd = [(L.ROW_LN_BWD, L.F32), (L.ROW_LN_BWD, L.BF16), (L.ROW_GATE_BWD, L.F32), (L.ROW_GATE_BWD, L.BF16),
           (L.ROW_GATE_BWD_FP8, L.BF16), (L.ROW_LN_BWD_GATE, L.F32), (L.ROW_LN_BWD_GATE, L.BF16), (L.ROW_LN_BWD_GATE_FP8, L.BF16)]
    bad = []
    for D in range(4, 2049, 4):
        nv = -(-D // 256)
        for T in (1, 7, 8, 9, 64, 100, 256, 1024):
            for B in (1, 2, 32, 128, 256, 300):
                wsf = lib.vaw_row_bwd_workspace_floats(B, T, D)
                for kind in (L.ROW_LN_FWD, L.ROW_LN_FWD_FP8):
                    p = row_plan(kind, L.BF16, B, T, D)
                    assert (p.variant, p.nv, p.block, p.lds_bytes, p.workspace_floats) == (L.RV_LN_FWD, nv if nv <= 6 else 8, 256, 0, 0)
                    assert p.grid_x >= 1 and (kind == L.ROW_LN_FWD or p.grid_x <= 2048)
                plans = {}
                for kind, dt in bwd:
                    for ws in (0, wsf, 1 << 60):
                        p = row_plan(kind, dt, B, T, D, workspace_floats=ws)
                        plans[kind, dt, ws] = p
                        where = f"kind={kind} dt={dt} B={B} T={T} D={D} ws={ws}: variant {p.variant} nc {p.nc} rpc {p.rows_per_chunk} " \
                                f"block {p.block} lds {p.lds_bytes}"
                        if p.lds_bytes > ROW_LDS_MAX:
                            bad.append("LDS " + where)
                        if not (64 <= p.block <= _row_bound(p) and p.block % 64 == 0):
                            bad.append("block " + where)
                        assert p.nv == (nv if nv <= 6 else 8) and p.nv * 256 >= D, where
                        assert p.grid_x == B and p.nc >= 1 and p.rows_per_chunk >= 1, where
                        assert p.nc * p.rows_per_chunk >= T and (p.nc - 1) * p.rows_per_chunk < T, where
                        assert p.block // 64 == min(p.rows_per_chunk, 8 if (nv <= 5 or kind in (L.ROW_LN_BWD_GATE, L.ROW_LN_BWD_GATE_FP8)) else 16), where
                        assert p.workspace_floats <= ws and (p.nc == 1) == (p.workspace_floats == 0), where
                        if ws == 0:
                            assert p.nc == 1, where
                    # the workspace the library sizes is what the plan wants: same chunking as with an unlimited one
                    assert (plans[kind, dt, wsf].nc, plans[kind, dt, wsf].block) == (plans[kind, dt, 1 << 60].nc, plans[kind, dt, 1 << 60].block)
                if D <= 1280:         # bitwise fused == pair: the same row partition (chunks x waves) on both sides
                    for ws in (0, wsf):
                        for fused, pair in (((L.ROW_LN_BWD_GATE, L.F32), [(L.ROW_LN_BWD, L.F32), (L.ROW_GATE_BWD, L.F32)]),
                                            ((L.ROW_LN_BWD_GATE, L.BF16), [(L.ROW_LN_BWD, L.BF16), (L.ROW_GATE_BWD, L.BF16)]),
                                            ((L.ROW_LN_BWD_GATE_FP8, L.BF16), [(L.ROW_LN_BWD, L.BF16), (L.ROW_GATE_BWD_FP8, L.BF16)])):
                            f = plans[fused + (ws,)]
                            for k in pair:
                                u = plans[k + (ws,)]
                                if (u.nc, u.rows_per_chunk, u.block) != (f.nc, f.rows_per_chunk, f.block):
                                    bad.append(f"split fused {fused} vs {k}: B={B} T={T} D={D} ws={ws}: nc {f.nc} / {u.nc}, "
                                               f"block {f.block} / {u.block}")
                    f = plans[L.ROW_LN_BWD_GATE, L.BF16, wsf]
                    assert f.variant in (L.RV_ROW_FUSE8, L.RV_ROW_FUSE)
                    # the LDS-slab kernel wherever its slabs fit, the register form only where they do not
                    if (f.variant == L.RV_ROW_FUSE8) != ((2 + 4 * f.block // 64) * D * 4 <= ROW_LDS_MAX):
                        bad.append(f"variant B={B} T={T} D={D}: {f.variant}")
    widths = {}
    for b in bad:
        widths.setdefault(b.split()[0], set()).add(int(re.search(r"D=(\d+)", b).group(1)))
    summary = {k: f"D in [{min(v)}, {max(v)}] ({len(v)} widths)" for k, v in widths.items()}
    assert not bad, f"{len(bad)} bad plans: {summary}, e.g.\n" + "\n".join(bad[:6] + bad[-6:])


def test_row_plan_colsum_paths():
    """vaw_colsum's path: bf16 x 8 (bf16, N and ldx multiples of 8, 16-byte aligned base, M >= 1024), vec4 (ldx % 4 == 0 and aligned
    base), scalar otherwise; the workspace is vaw_colsum_workspace_floats for the 128-row kernel, less for the 512-row ones."""
    from vaw_amd import _lib as L
    from vaw_amd.ops import row_plan
    lib = vaw_amd.lib()
    for dt in (L.F32, L.BF16):
        for M in (1, 3, 511, 512, 1023, 1024, 1100, 4097):
            for N, ldx in ((8, 8), (264, 264), (264, 1584), (260, 1560), (3, 3), (7, 9), (768, 7 * 768)):
                for base in (0x10000, 0x10004, 0x10008, 0x10010 + 2):
                    p = row_plan(L.ROW_COLSUM, dt, M, 1, N, ldx=ldx, base_addr=base)
                    aligned = base % 16 == 0
                    if dt == L.BF16 and N % 8 == 0 and ldx % 8 == 0 and aligned and M >= 1024:
                        want, rows = L.RV_COLSUM_BF16X8, 128
                    elif ldx % 4 == 0 and aligned:
                        want, rows = L.RV_COLSUM_VEC4, 512
                    else:
                        want, rows = L.RV_COLSUM_SCALAR, 512
                    assert (p.variant, p.rows_per_chunk, p.nc, p.block, p.lds_bytes) == (want, rows, -(-M // rows), 256, 0)
                    assert p.grid_x == -(-N // 256) and p.workspace_floats == p.nc * N <= lib.vaw_colsum_workspace_floats(M, N)
    with pytest.raises(vaw_amd.VawError):
        row_plan(L.ROW_COLSUM, L.F32, 10, 1, 8, ldx=4)
    with pytest.raises(vaw_amd.VawError):
        row_plan(L.ROW_LN_BWD, L.F32, 2, 8, 2052)


# ------------------------------------------------------------------------------------------------
# Launch plan of the attention kernels (vaw_attn_plan: host arithmetic only, vaw_attn_fwd / _bwd / _bwd_colsum take every choice
# from it)
# ------------------------------------------------------------------------------------------------
ATTN_LDS_DEFAULT = 64 * 1024      # what a launch may ask for without raising its cap
_ATTN_SWITCHES = ("VAW_ATTN_FWD_BIG", "VAW_ATTN_BWD_BIG", "VAW_ATTN_QG2", "VAW_ATTN_BWD_G2")


class _attn_env:
    """set the attention switches of vaw_attn_plan (read on every call) for a block; None = unset (the default)"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in _ATTN_SWITCHES}
        for k in _ATTN_SWITCHES:
            v = self.kw.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _attn_layouts(B, H, T, hd):
    """(name, desc, k offset, v offset) in elements for the four layouts the library serves"""
    from vaw_amd import ops
    D = H * hd
    out = [("token", ops.attn_desc_token_major(B, H, T, hd), D, 2 * D)]
    for new in (True, False):
        desc, ko, vo = ops.attn_desc_nhwc(B, H, T, hd, new)
        out.append(("nhwc_new" if new else "nhwc_legacy", desc, ko, vo))
    out.append(("channel", ops.attn_desc_channel_major(B, H, T, hd), D * T, 2 * D * T))
    return out


def _check_attn_plan(p, direction, dt, desc, addrs, sw):
    """the preconditions of the variant the plan picked, its grid, LDS and column-sum rows; returns a failure string or None"""
    from vaw_amd import _lib as L
    B, H, T, hd = desc.B, desc.H, desc.T, desc.hd
    q, k, v, o, dq, dk, dv = addrs
    fwd = direction == L.ATTN_FWD
    strides_ok = desc.q_sd == 1 and desc.o_sd == 1 and all(s % 8 == 0 for s in (desc.q_sb, desc.q_sh, desc.q_st, desc.o_sb,
                                                                                      desc.o_sh, desc.o_st))
    mfma_ok = (dt == L.BF16 and 8 <= hd <= 128 and hd % 8 == 0 and T % 64 == 0 and strides_ok and all(a % 16 == 0 for a in (q, k, v, o))
               and (fwd or all(a % 8 == 0 for a in (dq, dk, dv))))
    name = L.AV_NAMES[p.variant]
    where = f"dir={direction} dt={dt} B={B} H={H} T={T} hd={hd} sw={sw} -> {name}/{p.hd_image} grid {p.grid_x}x{p.grid_y} lds {p.lds_bytes}"
    if p.status != 0 or p.block != 256 or p.grid_y != B * H:
        return "grid " + where
    if p.lds_bytes > ROW_LDS_MAX or (not p.lds_cap_raised and p.lds_bytes > ATTN_LDS_DEFAULT) or p.lds_bytes <= 0:
        return "LDS " + where
    if mfma_ok != (p.variant != L.AV_ROWWISE):
        return "mfma eligibility " + where
    cap = B * max(T // 64, 1)
    if p.variant == L.AV_ROWWISE:
        want_lds = 16 * (hd + T) if fwd else 16 * (2 * hd + 2 * T)
        ok = (p.hd_image == 0 and p.launches == (1 if fwd else 2) and p.grid_x == -(-T // 4) and p.lds_bytes == want_lds
              and not p.lds_cap_raised and p.colsum_rows == 0)
        return None if ok else "rowwise " + where
    fwd_variants = (L.AV_FWD_T64, L.AV_FWD_G1, L.AV_FWD_G2, L.AV_FWD_BIG)
    if (p.variant in fwd_variants) != fwd or not p.lds_cap_raised:
        return "direction " + where
    wgr = {L.AV_FWD_T64: 64, L.AV_FWD_G1: 64, L.AV_FWD_G2: 128, L.AV_FWD_BIG: 128, L.AV_BWD_T64: 64, L.AV_BWD_G1: 64, L.AV_BWD_G2: 128,
           L.AV_BWD_BIG_NT2: 128, L.AV_BWD_BIG_NT4: 256}[p.variant]
    big = p.variant in (L.AV_FWD_BIG, L.AV_BWD_BIG_NT2, L.AV_BWD_BIG_NT4)
    pre = {L.AV_FWD_T64: T == 64, L.AV_BWD_T64: T == 64,
           L.AV_FWD_G1: True, L.AV_BWD_G1: True,
           L.AV_FWD_G2: hd <= 96 and sw["VAW_ATTN_QG2"] != "0",
           L.AV_BWD_G2: 64 < hd <= 96 and p.hd_image == 96 and sw["VAW_ATTN_BWD_G2"] != "0",
           L.AV_FWD_BIG: 32 < hd <= 96 and (hd > 64 or sw["VAW_ATTN_FWD_BIG"] == "1") and sw["VAW_ATTN_FWD_BIG"] != "0",
           L.AV_BWD_BIG_NT2: 32 < hd <= 96 and sw["VAW_ATTN_BWD_BIG"] in (None, "2"),
           L.AV_BWD_BIG_NT4: 32 < hd <= 96 and sw["VAW_ATTN_BWD_BIG"] == "1"}[p.variant]
    if not pre or T % wgr != 0 or T > 1024 or p.grid_x * wgr != T and p.variant not in (L.AV_FWD_T64, L.AV_BWD_T64):
        return "preconditions " + where
    if p.variant in (L.AV_FWD_T64, L.AV_BWD_T64) and p.grid_x != 1:
        return "t64 grid " + where
    img_ok = p.hd_image in ((64, 96) if big else (32, 64, 96, 128)) and hd <= p.hd_image and (big or p.hd_image - hd < 32)
    if not img_ok:
        return "image " + where
    want_launches = 1 if fwd or p.variant == L.AV_BWD_T64 else 2
    if p.launches != want_launches:
        return "launches " + where
    if direction == L.ATTN_BWD_COLSUM:
        want = B if p.variant == L.AV_BWD_T64 else B * T // wgr
        if p.colsum_rows != want or p.colsum_rows > cap:
            return "colsum rows " + where
    elif p.colsum_rows != 0:
        return "colsum rows " + where
    return None


def test_attn_plan_sweep_preconditions_lds_grid_and_colsum_rows():
    """Every (T, hd, B*H, dtype, layout, alignment, switch) case: each variant is picked only where its kernel's preconditions hold
    (sequence multiple, head width, strides, 16-byte operands, 8-byte gradients), the MFMA kernels wherever those hold, the LDS a
    launch asks for fits a CU (and 64 KiB where the cap is not raised), grid.y = B*H, and the column-sum rows are the variant's
    and within the capacity vaw_attn_bwd_colsum checks."""
    from vaw_amd import _lib as L
    from vaw_amd.ops import attn_plan
    Ts = (1, 2, 17, 63, 64, 65, 100, 128, 192, 256, 320, 512, 768, 1024, 1025)
    hds = (1, 8, 16, 24, 32, 33, 40, 64, 72, 96, 100, 104, 120, 128, 136, 256)
    aligns = {"aligned": (0, 0), "base+2": (2, 2), "base+8": (8, 8), "grad+2": (0, 2), "grad+8": (0, 8)}
    fwd_sw = [dict(VAW_ATTN_FWD_BIG=f, VAW_ATTN_QG2=g) for f in (None, "0", "1", "2") for g in (None, "0", "1")]
    bwd_sw = [dict(VAW_ATTN_BWD_BIG=b, VAW_ATTN_BWD_G2=g) for b in (None, "0", "1", "2") for g in (None, "0", "1")]
    bad, seen = [], set()
    for direction, switches in ((L.ATTN_FWD, fwd_sw), (L.ATTN_BWD, bwd_sw), (L.ATTN_BWD_COLSUM, bwd_sw)):
        for sw in switches:
            full = {k: sw.get(k) for k in _ATTN_SWITCHES}
            with _attn_env(**sw):
                for T in Ts:
                    for hd in hds:
                        for B, H in ((1, 1), (3, 2)) + (((65535, 1), (1, 65536), (256, 256)) if T in (64, 256) and hd in (64, 72) else ()):
                            for lay, desc, ko, vo in _attn_layouts(B, H, T, hd):
                                for dt in (L.F32, L.BF16):
                                    es = 4 if dt == L.F32 else 2
                                    for al, (off, goff) in aligns.items():
                                        base, obase, gbase = 1 << 20, 1 << 32, 1 << 36
                                        addrs = (base + off, base + off + es * ko, base + off + es * vo, obase + off, gbase + goff,
                                                 gbase + goff + es * ko, gbase + goff + es * vo)
                                        if B * H >= 65536 or T > 1024:
                                            with pytest.raises(vaw_amd.VawError):
                                                attn_plan(direction, dt, desc, *addrs)
                                            continue
                                        p = attn_plan(direction, dt, desc, *addrs)
                                        seen.add((direction, p.variant, p.hd_image))
                                        err = _check_attn_plan(p, direction, dt, desc, addrs, full)
                                        if err:
                                            bad.append(f"{err} layout={lay} align={al}")
    assert not bad, f"{len(bad)} bad plans, e.g.\n" + "\n".join(bad[:10])
    # every kernel instantiation is reachable by some case of the sweep
    want = ({(L.ATTN_FWD, L.AV_ROWWISE, 0), (L.ATTN_BWD, L.AV_ROWWISE, 0), (L.ATTN_FWD, L.AV_FWD_BIG, 64), (L.ATTN_FWD, L.AV_FWD_BIG, 96)}
            | {(L.ATTN_FWD, v, i) for v in (L.AV_FWD_T64, L.AV_FWD_G1) for i in (32, 64, 96, 128)}
            | {(L.ATTN_FWD, L.AV_FWD_G2, i) for i in (32, 64, 96)}
            | {(L.ATTN_BWD, v, i) for v in (L.AV_BWD_T64, L.AV_BWD_G1) for i in (32, 64, 96, 128)}
            | {(L.ATTN_BWD, L.AV_BWD_G2, 96)} | {(L.ATTN_BWD, v, i) for v in (L.AV_BWD_BIG_NT2, L.AV_BWD_BIG_NT4) for i in (64, 96)})
    assert {s for s in seen if s[0] != L.ATTN_BWD_COLSUM} == want


def test_attn_plan_refusals():
    """check_desc's refusals and a rowwise LDS request that could not launch come back as errors (before any launch)"""
    from vaw_amd import _lib as L
    from vaw_amd.ops import AttnDesc, attn_desc_token_major, attn_plan
    for direction in (L.ATTN_FWD, L.ATTN_BWD, L.ATTN_BWD_COLSUM):
        for desc in (attn_desc_token_major(1, 2, 1025, 64), attn_desc_token_major(1, 65536, 64, 64), attn_desc_token_major(256, 256, 64, 64),
                     AttnDesc(1, 2, 64, 0, 64, 0, 64, 1, 64, 0, 64, 1, 1.0), AttnDesc(1, 2, 64, -8, 64, 8, 64, 1, 64, 8, 64, 1, 1.0),
                     attn_desc_token_major(0, 2, 64, 64),
                     AttnDesc(1, 1, 0, 64, 64, 64, 64, 1, 64, 64, 64, 1, 0.125)):
            for dt in (L.F32, L.BF16):
                with pytest.raises(vaw_amd.VawError):
                    attn_plan(direction, dt, desc, 0, 0, 0, 0)
        with pytest.raises(vaw_amd.VawError, match="dt"):
            attn_plan(direction, L.FP8, attn_desc_token_major(1, 2, 64, 64), 0, 0, 0, 0)
    # rowwise: 16 (hd + T) bytes forward, 16 (2 hd + 2 T) backward, with the default cap of 64 KiB
    for T, hd, fwd_ok, bwd_ok in ((1024, 3072, True, False), (1024, 3073, False, False), (1024, 1024, True, True),
                                  (1024, 1025, True, False), (1, 2047, True, True), (1, 2048, True, False)):
        desc = attn_desc_token_major(1, 1, T, hd)
        for direction, ok in ((L.ATTN_FWD, fwd_ok), (L.ATTN_BWD, bwd_ok)):
            if ok:
                assert attn_plan(direction, L.F32, desc, 0, 0, 0, 0).variant == L.AV_ROWWISE
            else:
                with pytest.raises(vaw_amd.VawError, match="LDS"):
                    attn_plan(direction, L.F32, desc, 0, 0, 0, 0)


def _production_attention_shapes():
    """(model, H, T, hd, new_order) of every attention block of the DiT and UNet presets, walked on the meta device"""
    from vaw_amd import dit, unet
    shapes = set()
    with torch.device("meta"):
        for name, patch in (("DiT-B", 4), ("DiT-XL", 2)):
            m = dit.DiT_models[name](image_size=32, patch_size=patch, in_channels=4, class_dropout_prob=0.1, num_classes=1000,
                                     learn_sigma=True)
            T = m.x_embedder.num_patches
            for blk in m.blocks:
                H = blk.attn.num_heads
                shapes.add((f"{name}/{patch}", H, T, blk.attn.qkv.weight.shape[1] // H, True))
        for name, build in unet.UNet_models.items():
            m = build(compute_dtype="fp32")
            res = m.image_size
            for seq in list(m.input_blocks) + [m.middle_block] + list(m.output_blocks):
                for layer in seq:
                    if isinstance(layer, unet.AttentionBlock):
                        shapes.add((name, layer.num_heads, res * res, layer.channels // layer.num_heads, layer.attention.new_order))
                    elif isinstance(layer, unet.Downsample) or (isinstance(layer, unet.ResBlock) and layer.down):
                        res //= 2
                    elif isinstance(layer, unet.Upsample) or (isinstance(layer, unet.ResBlock) and layer.up):
                        res *= 2
    return sorted(shapes)


# today's launch for every production attention shape, default switches, bf16, aligned: (variant, hd_image, grid_x, lds_bytes)
# forward and backward, keyed by (T, hd)
_PINNED_ATTN = {
    (64, 64): (("fwd_t64", 64, 1, 24576), ("bwd_t64", 64, 1, 32768)),
    (256, 72): (("fwd_big", 96, 2, 53248), ("bwd_big_nt2", 96, 2, 56832)),
    (256, 96): (("fwd_big", 96, 2, 53248), ("bwd_big_nt2", 96, 2, 56832)),
    (64, 96): (("fwd_t64", 96, 1, 39936), ("bwd_t64", 96, 1, 53248)),
    (1024, 64): (("fwd_g2", 64, 8, 49152), ("bwd_big_nt2", 64, 8, 41984)),
    (256, 64): (("fwd_g2", 64, 2, 49152), ("bwd_big_nt2", 64, 2, 35840)),
    (1024, 32): (("fwd_g2", 32, 8, 24576), ("bwd_g1", 32, 16, 16896)),
    (256, 32): (("fwd_g2", 32, 2, 24576), ("bwd_g1", 32, 4, 16896)),
    (64, 32): (("fwd_t64", 32, 1, 12288), ("bwd_t64", 32, 1, 16384)),
    (16, 64): (("rowwise", 0, 4, 1280), ("rowwise", 0, 4, 2560)),         # the 4 x 4 middle blocks of UNet-32 / ADM-32
    (16, 32): (("rowwise", 0, 4, 768), ("rowwise", 0, 4, 1536)),
}


def test_attn_plan_pins_production_shapes():
    """The launch each model's attention takes today (the refactor onto vaw_attn_plan changed none): every (H, T, hd) of the
    DiT-B/4, DiT-XL/2 and UNet presets, in the layout the model uses, with the default switches."""
    from vaw_amd import _lib as L
    from vaw_amd import ops
    shapes = _production_attention_shapes()
    got = {(m, H, T, hd) for m, H, T, hd, _ in shapes}
    # the table of the model zoo, as the presets build it
    assert {(m, T, hd) for m, _, T, hd in got} == ({
        ("DiT-B/4", 64, 64), ("DiT-XL/2", 256, 72), ("UNet-64", 256, 96), ("UNet-64", 64, 96), ("UNet-32", 256, 64), ("UNet-32", 64, 64),
        ("UNet-32", 16, 64), ("ADM-32", 256, 32), ("ADM-32", 64, 32), ("ADM-32", 16, 32), ("LDM", 1024, 32), ("LDM", 256, 32), ("LDM", 64, 32)}
        | {(m, T, 64) for m in ("ADM-64", "ADM-128", "ADM-256", "ADM-512") for T in (1024, 256, 64)})
    with _attn_env():
        for m, H, T, hd, new_order in shapes:
            for B in (1, 32):
                if m.startswith("DiT"):
                    desc, ko, vo = ops.attn_desc_token_major(B, H, T, hd), H * hd, 2 * H * hd
                else:
                    desc, ko, vo = ops.attn_desc_nhwc(B, H, T, hd, new_order)
                q = 1 << 20
                addrs = (q, q + 2 * ko, q + 2 * vo, 1 << 30)
                fwd = ops.attn_plan(L.ATTN_FWD, L.BF16, desc, *addrs)
                bwd = ops.attn_plan(L.ATTN_BWD_COLSUM, L.BF16, desc, *addrs, q + (1 << 28), q + (1 << 28) + 2 * ko, q + (1 << 28) + 2 * vo)
                got_f = (L.AV_NAMES[fwd.variant], fwd.hd_image, fwd.grid_x, fwd.lds_bytes)
                got_b = (L.AV_NAMES[bwd.variant], bwd.hd_image, bwd.grid_x, bwd.lds_bytes)
                assert (got_f, got_b) == _PINNED_ATTN[T, hd], (m, H, T, hd)
                assert fwd.grid_y == bwd.grid_y == B * H
                assert bwd.colsum_rows == (0 if T % 64 else B if T == 64 else B * T // (64 * (1 if got_b[0] == "bwd_g1" else 2)))


# ------------------------------------------------------------------------------------------------------------------------------
# Launch plan of vaw_gemm (vaw_gemm_plan: host arithmetic only, vaw_gemm takes every launch choice from it)
# ------------------------------------------------------------------------------------------------------------------------------
_GEMM_WS = 1 << 26          # floats of the grow-only scratch ops.gemm hands to vaw_gemm
_GEMM_ADDR = 1 << 20
# tile rows per partial row of column sums, dynamic LDS and workgroup size of each variant (csrc/gemm_plan.h and the kernels)
_GEMM_CS_ROWS = {"t128_bk32": 128, "t128_bk64": 128, "ring256": 256, "persistent": 128, "parked_drain": 64, "warp_spec": 64}


def _gemm_lds(name, p):
    return {"generic": 2 * 16 * 144 * 4, "t128_bk32": 64 * 132 * 4 + 2048, "t128_bk64": 4 * 128 * 64 * 2 + 2048,
            "ring256": 4 * 32768 + 8192, "persistent": 2 * (4 + p.ntw) * 8192 + 32768, "small_m": p.stages * (p.mb + p.nb) * 8192,
            "parked_drain": 3 * (2 + p.ntw) * 8192 + 16384, "warp_spec": 3 * (2 + p.ntw) * 8192}[name]


def _gemm_epilogues(M, N):
    """name -> (epilogue keywords, wants a colsum_partial capacity, the smallest workspace the call can need)"""
    a = _GEMM_ADDR
    slabs, cs = 2 * M * N, -(-M // 128) * N
    return {"plain_f32": (dict(out_f32=True), False, slabs), "plain_bf16": ({}, False, slabs),
            "bias_gelu_aux": (dict(bias=a, act=1, aux_out=a), False, 0),
            "gate_resid": (dict(bias=a, aux_out=a, gate=a, gate_ld=N, resid=a, rows_per_batch=8, out_f32=True), False, 0),
            "colsum_out": (dict(colsum_out=a), False, cs), "colsum_partial": ({}, True, cs),
            "rowsum_a_out": (dict(rowsum_a_out=a, out_f32=True), False, 64 * M),
            # both at once: the column-sum rows are folded before the separate row-sum pass takes the workspace over (vaw_gemm)
            "rowsum_colsum": (dict(rowsum_a_out=a, colsum_out=a, out_f32=True), False, max(64 * M, cs))}


def _check_gemm_plan(p, L, dt, ak, bk, M, N, K, off, epi, cap, ws, knobs, seen):
    """the invariants of one planned launch; -> its variant name"""
    name = L.GV_NAMES[p.variant]
    ctx = (name, dt, ak, bk, M, N, K, off, sorted(epi), cap, ws, knobs.tile)
    lda, ldb = (K if ak else M), (K if bk else N)
    es = 2 if dt == L.BF16 else 4
    colsum, rowsum = bool(epi.get("colsum_out")) or cap is not None, bool(epi.get("rowsum_a_out"))
    if name != "generic":       # the preconditions of the MFMA kernels
        assert dt == L.BF16 and not knobs.force_generic and N % 8 == 0 and K % 64 == 0 and lda % 8 == 0 and ldb % 8 == 0, ctx
        assert off == 0 and M >= 16 and N >= 16 and (ak or M % 8 == 0) and N % 8 == 0 and epi.get("gate_ld", 0) % 4 == 0, ctx
        assert (ak and not rowsum) if name in ("small_m", "parked_drain", "warp_spec") else True, ctx
        if name in ("parked_drain", "warp_spec"):
            assert K // 64 >= 12 and M >= 128 and p.split == 1 and p.epi_kind in (L.P8_STORE, L.P8_GELU, L.P8_DGELU, L.P8_GATE), ctx
            assert (p.epi_kind == L.P8_DGELU) <= (not bk) and (p.epi_kind in (L.P8_GELU, L.P8_GATE)) <= bool(bk), ctx
        if name == "persistent":
            assert (p.epi_kind == L.P8_SLAB) == (p.split > 1) and 0 <= p.epi_kind <= L.P8_RESID and p.epi_kind != L.P8_WGRAD, ctx
            seen.add(("persistent", p.epi_kind))
        elif p.epi_kind >= 0:
            seen.add((name, p.epi_kind))
        assert (p.epi_kind >= 0) == (name in ("persistent", "parked_drain", "warp_spec")), ctx
    assert p.lds_bytes == _gemm_lds(name, p) <= 160 * 1024, ctx
    # tile parameters, grid and block
    tiles = lambda bm, bn: -(-M // bm) * -(-N // bn)
    if name == "generic":
        assert (p.grid_x, p.grid_y, p.grid_z, p.block, p.bkt) == (-(-N // 128), -(-M // 128), p.split, 256, 16), ctx
        nk = -(-K // 16)
    elif name.startswith("t128"):
        assert p.bkt == (32 if name == "t128_bk32" else 64) and p.block == 256, ctx
        want = (8 * -(-tiles(128, 128) // p.xcd_parts), 1) if p.xcd_parts else (tiles(128, 128), p.split)
        assert (p.grid_x, p.grid_y, p.grid_z) == want + (1,), ctx
        nk = K // p.bkt
    elif name == "ring256":
        assert (p.grid_x, p.grid_y, p.grid_z, p.block, p.bkt) == (tiles(256, 256), p.split, 1, 512, 32), ctx
        nk = K // 32
    elif name == "small_m":
        assert (p.mb, p.nb) in ((1, 1), (1, 2), (2, 2)) and p.stages in (3, 4) and p.split == 1 and p.block == 256, ctx
        assert (p.grid_x, p.grid_y, p.grid_z) == (tiles(64 * p.mb, 64 * p.nb), 1, 1), ctx
        nk = K // 64
    else:
        bm = 256 if name == "persistent" else 128
        assert p.ntw in (3, 4) and (p.grid_y, p.grid_z) == (1, 1), ctx
        assert p.grid_x == min(tiles(bm, 64 * p.ntw) * p.split, knobs.cus), ctx
        loaders = 8 if (p.ntw == 3 and knobs.ws_loaders == 8) else 4
        assert p.block == (512 + 64 * loaders if name == "warp_spec" else 512), ctx
        nk = K // 64
    assert 0 < p.grid_x < 2 ** 31 and 0 < p.grid_y < 2 ** 31 and 0 < p.grid_z < 2 ** 31, ctx
    assert (p.ntw != 0) == (name in ("persistent", "parked_drain", "warp_spec")) and (p.mb != 0) == (name == "small_m"), ctx
    # split-K: no empty split, only where slabs can be reduced; the XCD mapping exactly where it applies
    assert p.split >= 1 and -(-nk // -(-nk // p.split)) == p.split, ctx
    xcd_on = name.startswith("t128") and knobs.xcdsplit and p.split in (2, 4, 8)
    assert p.xcd_parts == (8 // p.split if xcd_on else 0), ctx
    out_f32 = bool(epi.get("out_f32")) or dt == L.F32
    if p.split > 1:
        assert not colsum and not (set(epi) & {"bias", "act", "aux_out", "gate", "resid"}), ctx
    assert p.reduce == (L.GR_NONE if p.split == 1 else L.GR_BF16 if not out_f32 else
                        L.GR_F32_ROWSUM if p.rowsum_mode == L.GS_FUSED else L.GR_F32), ctx
    # row sums of A, column sums of C
    assert (p.rowsum_mode != L.GS_NONE) == rowsum and (p.rowsum_mode == L.GS_FUSED) <= (name.startswith("t128") and not ak), ctx
    want_cs = L.GC_NONE if not colsum else L.GC_SEPARATE if name == "generic" else L.GC_DEFERRED if cap is not None else L.GC_FOLD
    assert p.colsum_mode == want_cs, ctx
    rows_per = 64 * p.mb if name == "small_m" else _GEMM_CS_ROWS.get(name)
    assert p.colsum_rows == (0 if not colsum else 1 if name == "generic" else -(-M // rows_per)), ctx
    # workspace: slabs, then row-sum partials; column-sum rows from 0, never with slabs; a pass reuses it afterwards
    slab = p.split * M * N if p.split > 1 else 0
    rowp = p.split * M if p.rowsum_mode == L.GS_FUSED else 0
    fold = p.colsum_rows * N if p.colsum_mode == L.GC_FOLD else 0
    assert not (fold and (slab or rowp)), ctx
    passes = (p.rowsum_mode == L.GS_SEPARATE and not ak) + (p.colsum_mode == L.GC_SEPARATE)
    assert p.workspace_floats_used >= slab + rowp + fold and (passes or p.workspace_floats_used == slab + rowp + fold), ctx
    assert p.launches == 1 + (p.split > 1) + (p.rowsum_mode == L.GS_FUSED and p.split == 1) + (fold > 0) + 2 * passes, ctx
    # the status: exactly the refusals the call earns
    refused = (cap is not None and p.colsum_rows > cap) or (p.rowsum_mode == L.GS_SEPARATE and ak) or p.workspace_floats_used > ws
    assert (p.status != 0) == bool(refused), ctx
    seen.add(name)
    return name


def _sweep_gemm_plans(L, ops, knobs, dts, offs, wss, seen, Ms=(1, 15, 16, 64, 100, 128, 256, 2048, 4096, 8192, 16384, 32768)):
    import ctypes as C
    plan_fn, p = L.lib().vaw_gemm_plan, L.GemmLaunch()
    n = 0
    for M in Ms:
        for N in (8, 16, 64, 192, 768, 1152, 2304, 3072):
            for ename, (epi, partial, tight) in _gemm_epilogues(M, N).items():
                caps = (None,) if not partial else (-(-M // 64), "below")
                for dt in dts:
                    for K in (4, 64, 768, 2048, 3072, 16384, 65536):
                        for ak, bk in ((1, 1), (1, 0), (0, 0), (0, 1)):
                            lda, ldb = (K if ak else M), (K if bk else N)
                            for off in offs:
                                for ws in wss:
                                    if off not in (0, "A") and (dt != L.BF16 or ws != "ample"):
                                        continue       # B, C and the epilogue operands off by 2 bytes: where an MFMA kernel was possible
                                    ws = {"none": 0, "tight": tight, "ample": _GEMM_WS}[ws]
                                    if "rowsum_a_out" in epi and ws < 64 * M:
                                        continue       # refused before planning (test_gemm_plan_refusals)
                                    if "colsum_out" in epi and ws < tight:
                                        continue
                                    addr = {o: _GEMM_ADDR + (2 if off == o else 0) for o in "ABC"}
                                    epi_off = dict(epi)
                                    if off == "epi":
                                        first = next((f for f in ("bias", "aux_out", "gate", "resid") if f in epi), None)
                                        if first is None:
                                            continue
                                        epi_off[first] = epi[first] + 2
                                    for cap in caps:
                                        if cap == "below":      # one row less than the launch just planned writes
                                            if p.colsum_rows < 2 or p.status != 0:
                                                continue
                                            cap = p.colsum_rows - 1
                                        p = ops.gemm_plan(dt, ak, bk, M, N, K, addr["A"], lda, addr["B"], ldb, addr["C"], N,
                                                          workspace_floats=ws, knobs=knobs, colsum_partial_rows=cap, check_status=False,
                                                          **epi_off)
                                        _check_gemm_plan(p, L, dt, ak, bk, M, N, K, off, epi, cap, ws, knobs, seen)
                                        n += 1
    return n


def test_gemm_plan_sweep_default_knobs():
    """Every launch vaw_gemm_plan makes with the default knobs on 256 CUs, over the cross of sizes (multiples of no tile, of every
    tile, beyond every threshold), the four layouts, both dtypes, aligned operands and A, B, C or an epilogue operand 2 bytes off, eight epilogues (colsum_partial with
    capacity above and one row below need) and no / tight / ample workspace: each variant only where its kernel's preconditions
    hold, LDS by the variant's formula and within 160 KiB, no empty split, the XCD mapping exactly where it applies, grids below
    2^31, workspace regions within the workspace and disjoint, column-sum rows by the variant's tile rows, launches counted, and a
    refusal exactly where capacity, layout or workspace earn one."""
    from vaw_amd import _lib as L
    from vaw_amd import ops
    seen = set()
    n = _sweep_gemm_plans(L, ops, ops.default_gemm_knobs(), (L.BF16, L.F32), (0, "A", "B", "C", "epi"), ("none", "tight", "ample"), seen)
    assert n > 100000
    # (the 256 x 256 ring is behind the persistent kernel in the order of preference: by shape it gets what that one declines, which
    #  with these epilogues is nothing; the parked-drain and warp-specialised kernels are off by default: the knob sweep reaches them)
    assert {"generic", "t128_bk32", "t128_bk64", "persistent", "small_m"} <= seen, seen
    assert {("persistent", k) for k in (L.P8_STORE, L.P8_GELU, L.P8_GATE, L.P8_SLAB)} <= seen, seen


_GEMM_KNOB_CASES = ([dict(tile=t) for t in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 14)] +
                    [dict(force_generic=1), dict(bk=32), dict(bk=64), dict(pd=1), dict(ws=1), dict(ws=1, ws_loaders=8), dict(ws=1, ws_loaders=5), dict(xcdsplit=0),
                     dict(sm_max_m=2048), dict(sm_wide_m=4096), dict(sm_nb=2), dict(sm_stages=3), dict(cus=248), dict(tile=9), dict(tile=12)])

def _gemm_plan_linear_layers(L, ops, knobs, seen):
    """the launches of a DiT block's Linear layers (and a UNet skip add, a pos-embed row add, a weight gradient) at three sizes"""
    a = _GEMM_ADDR
    layers = ((1, 1, dict(bias=a)), (1, 1, dict(bias=a, act=1, aux_out=a)), (1, 0, dict(act=2, aux_in=a)), (1, 0, dict(act=2, aux_in=a, colsum_out=a)),
              (1, 1, dict(bias=a, aux_out=a, gate=a, gate_ld=768, resid=a, rows_per_batch=64, out_f32=True)), (1, 0, {}),
              (1, 1, dict(bias=a, resid=a, resid_is_act=True)), (1, 1, dict(bias=a, rowadd=a, rows_per_batch=8)), (0, 0, dict(out_f32=True)))
    for M, N, K in ((256, 768, 768), (16384, 768, 3072), (32768, 3072, 768)):
        for ak, bk, epi in layers:
            p = ops.gemm_plan(L.BF16, ak, bk, M, N, K, a, K if ak else M, a, K if bk else N, a, N, workspace_floats=_GEMM_WS, knobs=knobs, **epi)
            _check_gemm_plan(p, L, L.BF16, ak, bk, M, N, K, 0, epi, None, _GEMM_WS, knobs, seen)


@pytest.mark.parametrize("case", _GEMM_KNOB_CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_gemm_plan_sweep_knobs(case):
    """The same invariants with every vaw_debug_gemm_tile value the tests use and each knob at a non-default value (bf16, aligned:
    the knobs act on the MFMA kernels only), on the sweep's shapes and on the launches of the Linear layers."""
    from vaw_amd import _lib as L
    from vaw_amd import ops
    knobs, seen = ops.default_gemm_knobs(**case), set()
    n = _sweep_gemm_plans(L, ops, knobs, (L.BF16,), (0,), ("none", "ample"), seen, Ms=(16, 100, 256, 2048, 4096, 16384, 32768))
    assert n > 5000
    _gemm_plan_linear_layers(L, ops, knobs, seen)


def test_gemm_plan_reaches_every_variant_and_epilogue_kind():
    """Over the knob cases, the Linear-layer launches reach every variant and every epilogue kind of the three kernels that
    specialise on it."""
    from vaw_amd import _lib as L
    from vaw_amd import ops
    seen = set()
    for case in [{}] + _GEMM_KNOB_CASES:
        _gemm_plan_linear_layers(L, ops, ops.default_gemm_knobs(**case), seen)
    assert set(L.GV_NAMES) <= seen, seen
    for name, kinds in (("persistent", (L.P8_STORE, L.P8_GELU, L.P8_DGELU, L.P8_GATE, L.P8_SLAB, L.P8_ANY, L.P8_RESID)),
                        ("parked_drain", (L.P8_STORE, L.P8_GELU, L.P8_DGELU, L.P8_GATE)),
                        ("warp_spec", (L.P8_STORE, L.P8_GELU, L.P8_DGELU, L.P8_GATE))):
        assert {(name, k) for k in kinds} <= seen, (name, seen)


def _gemm_kernel_name(L, name, p, dt, ak, bk):
    """the kernel a variant launches, template arguments included, as a kernel trace spells it (prefix)"""
    b = lambda v: "true" if v else "false"
    return {"generic": "gemm_generic_kernel<float, %s, %s>" % (b(ak), b(bk)) if dt == L.F32 else "gemm_generic_kernel",
            "t128_bk32": "gemm_bf16_kernel<%s, %s, 32, 0>" % (b(ak), b(bk)), "t128_bk64": "gemm_bf16_kernel<%s, %s, 64, 0>" % (b(ak), b(bk)),
            "ring256": "gemm_bf16_big_kernel<%s, %s>" % (b(ak), b(bk)),
            "persistent": "gemm_p8_kernel<%s, %s, %d, %d, " % (b(ak), b(bk), p.ntw, p.epi_kind),
            "small_m": "gemm_sm_kernel<%s, %d, %d, %d>" % (b(bk), p.nb, p.stages, p.mb),
            "parked_drain": "gemm_pd_kernel<%s, %d, %d>" % (b(bk), p.ntw, p.epi_kind),
            "warp_spec": "gemm_ws_kernel<%s, %d, %d, %d>" % (b(bk), p.ntw, p.epi_kind, (p.block - 512) // 64)}[name]


def test_gemm_plan_matches_recorded_launches():
    """tests/golden/gemm_launches.json (GEMM_LAUNCHES.md) is a kernel trace of the commit BEFORE the plan existed: every distinct
    vaw_gemm call of a training step of DiT-B/4 (batch 256, 32, 64), DiT-XL/2 and the 32 x 32 UNet, plus the calls by which the GPU
    tests force each kernel.  For every entry the plan, with default knobs (the entry's forced tile) and 256 CUs, gives the recorded
    kernel -- template arguments included: layout, stage depth, tile shape, ring depth, epilogue kind, loader waves --, grid and
    workgroup size, and its passes account for every further kernel the call enqueued.  (The trace reports a kernel's static LDS
    only: it is held where there is any, i.e. on the generic kernel.)"""
    from vaw_amd import _lib as L
    from vaw_amd import ops
    rec = load_json("gemm_launches.json")["entries"]
    assert len(rec) >= 150
    seen = set()
    for ent in rec:
        c, ks = ent["call"], ent["kernels"]
        epi = {f: _GEMM_ADDR for f in ("bias", "aux_in", "aux_out", "gate", "resid", "rowadd", "colsum_out", "rowsum_a_out") if c[f]}
        epi.update({f: c[f] for f in ("act", "gate_ld", "rows_per_batch", "alpha", "beta", "out_f32", "colsum_beta", "resid_is_act",
                                      "rowsum_a_beta")})
        p = ops.gemm_plan(c["dt"], c["a_kmajor"], c["b_kmajor"], c["M"], c["N"], c["K"], _GEMM_ADDR + c["off"][0], c["lda"],
                          _GEMM_ADDR + c["off"][1], c["ldb"], _GEMM_ADDR + c["off"][2], c["ldc"], workspace_floats=c["ws"],
                          knobs=ops.default_gemm_knobs(tile=c["tile"]), colsum_partial_rows=c["colsum_partial_cap"], **epi)
        name = L.GV_NAMES[p.variant]
        ctx = (c, name, ks)
        want = _gemm_kernel_name(L, name, p, c["dt"], c["a_kmajor"], c["b_kmajor"])
        assert ks[0]["name"].startswith(want) if "<" in want else want in ks[0]["name"], ctx + (want,)
        assert ks[0]["grid"] == [p.grid_x, p.grid_y, p.grid_z] and ks[0]["block"] == [p.block, 1, 1], ctx + (p.grid_x, p.grid_y, p.grid_z, p.block)
        assert ks[0]["lds"] in (0, p.lds_bytes) and (name != "generic" or ks[0]["lds"] == p.lds_bytes), ctx + (p.lds_bytes,)
        # the kernels behind it: the split-K reduce (by output type), the fold of the column-sum rows, the vaw_colsum passes
        rest = [k["name"] for k in ks[1:]]
        assert len(ks) == p.launches, ctx + (p.launches,)
        reduces = [n for n in rest if "splitk_reduce_kernel" in n]
        assert len(reduces) == (p.reduce != L.GR_NONE), ctx + (p.reduce,)
        if reduces:
            assert ("splitk_reduce_kernel<float>" in reduces[0]) == (p.reduce != L.GR_BF16), ctx + (p.reduce,)
            assert ks[1]["name"] == reduces[0], ctx
        assert sum("colsum_final_kernel" in n for n in rest) == (p.colsum_mode == L.GC_FOLD) + (p.rowsum_mode == L.GS_FUSED and p.split == 1) + \
            (p.colsum_mode == L.GC_SEPARATE) + (p.rowsum_mode == L.GS_SEPARATE), ctx
        seen.add(name if c["tile"] < 0 else name + "/forced")
    # by shape, the training steps reach these; the other three kernels are reached through the tests' forced tiles
    assert {"generic", "t128_bk32", "t128_bk64", "persistent", "small_m", "ring256/forced", "parked_drain/forced", "warp_spec/forced"} <= seen, seen


def test_gemm_plan_refusals():
    """Every argument check of vaw_gemm is the plan's: status VAW_ERR_INVALID with the reason, before anything could be launched."""
    from vaw_amd import _lib as L
    from vaw_amd import ops
    a, k = _GEMM_ADDR, ops.default_gemm_knobs()

    def refused(match, dt=L.BF16, ak=1, bk=1, M=256, N=256, K=256, A=a, lda=None, B=a, ldb=None, Cp=a, ldc=None, **kw):
        p = ops.gemm_plan(dt, ak, bk, M, N, K, A, K if lda is None else lda, B, K if ldb is None else ldb, Cp, N if ldc is None else ldc,
                          knobs=k, check_status=False, **kw)
        assert p.status == -1 and match in L.lib().vaw_last_error_string().decode(), (match, p.status, L.lib().vaw_last_error_string())
        with pytest.raises(vaw_amd.VawError, match=match):
            ops.gemm_plan(dt, ak, bk, M, N, K, A, K if lda is None else lda, B, K if ldb is None else ldb, Cp, N if ldc is None else ldc,
                          knobs=k, **kw)
    for bad in (dict(M=0), dict(N=0), dict(K=0), dict(A=0), dict(B=0), dict(Cp=0)):
        refused("bad sizes", **bad)
    refused("must fit 31 bits", M=1 << 31, ak=1)
    refused("must fit 31 bits", N=1 << 31, ldb=256, ldc=1 << 31)
    refused("leading dimension too small", lda=255)
    refused("leading dimension too small", ldb=255)
    refused("leading dimension too small", ldc=255)
    refused("leading dimension too small", ak=0, M=512, lda=256)
    refused("excludes colsum_out", colsum_partial_rows=8, colsum_out=a, workspace_floats=_GEMM_WS)
    refused("rowsum_a_out needs a workspace", ak=0, rowsum_a_out=a, out_f32=True)
    refused("rowsum_a_out needs a workspace", ak=0, rowsum_a_out=a, out_f32=True, workspace_floats=64 * 256 - 1)
    refused("unknown act", act=3)
    refused("act=2 needs aux_in", act=2)
    refused("need rows_per_batch", gate=a, gate_ld=256)
    refused("need rows_per_batch", rowadd=a)
    refused("beta needs f32 output", beta=1.0)
    refused("colsum_out needs a workspace", colsum_out=a)
    refused("colsum_out needs a workspace", colsum_out=a, workspace_floats=2 * 256 - 1)
    refused("colsum_partial_out holds 3 rows, this launch writes 4", colsum_partial_rows=3)
    refused("rowsum_a_out is defined for a_kmajor = 0", rowsum_a_out=a, out_f32=True, workspace_floats=_GEMM_WS)
    refused("needs a workspace", dt=L.F32, colsum_partial_rows=8)          # generic kernel: the column sums are a pass of their own
    refused("grid too large", M=(1 << 31) - 8, N=(1 << 31) - 8, K=64, lda=64, ldb=64, bias=a)
    # and a call that passes them all
    assert ops.gemm_plan(L.BF16, 1, 1, 256, 256, 256, a, 256, a, 256, a, 256, knobs=k).status == 0


# ------------------------------------------------------------------------------------------------
# Launch plan of GroupNorm (vaw_gn_plan: host arithmetic only, vaw_groupnorm_fwd / _apply / _bwd take every choice from it)
# ------------------------------------------------------------------------------------------------
_GN_FIELDS = "@9i6qi"          # vaw_gn_launch: variant rows nch nt rpi grid_x grid_y grid_z block | lds ws off_part off_sums off_s1 off_s2 | status


def _gn_want(switch, dt, B, HW, C, G):
    """The rule and the launch restated: the fields of vaw_gn_launch for each pass (_lib.GN_* = 0 .. 3), or None where the plan refuses."""
    if dt not in (0, 1) or min(B, HW, C, G) <= 0 or C % 4 or C % G or G > 64 or B >= 65536:
        return None
    rows = 0
    if switch != 0 and dt == 1 and C % 8 == 0 and C // 8 <= 256 and C <= 2048 and B * HW < 2 ** 30 and HW * C < 2 ** 31:
        rows = next((r for r in (512, 256, 128) if B * -(-HW // r) >= 512), 128 if switch == 1 else 0)
    flat, rows = rows > 0, rows or 512
    nch = -(-HW // rows)
    if not flat and nch > 65535:
        return None
    nt = 256 // (C // 8) * (C // 8) if flat else 0
    geom = (int(flat), rows, nch, nt, nt // (C // 8) if flat else 0) + ((B * nch, 1, 1) if flat else (-(-C // 64), B, nch)) + (256,)
    BC, BG, part = B * C, B * G, 4 * nch * B * C          # part: the backward's chunk partials, in front of its other regions
    sums_lds = lambda planes: 4 * (2 * 256 * 8 + 2 * 2048 if flat else planes * 16 * 64)
    bwd_ws = part + 4 * BC + 2 * BG
    return [geom + (sums_lds(2), 2 * nch * BC, 0, -1, -1, -1, 0), geom + (0, 0, -1, -1, -1, -1, 0),
            geom + (sums_lds(4), bwd_ws, 0, part, part + 4 * BC, part + 4 * BC + BG, 0),
            geom + (0, bwd_ws, -1, -1, part + 4 * BC, part + 4 * BC + BG, 0)]


def test_gn_plan_sweep_variant_geometry_and_workspace():
    """Every field is the restated rule's (so a shape's four passes share one geometry: the apply pass is the forward's); chunks cover
    HW, none empty; flat fits its workgroup and the LDS arrays of its sums kernels (red: 2 rpi C <= 4096 floats, chs: 2 C <= 4096);
    quad fits grid.y / grid.z; every workspace fits vaw_groupnorm_workspace_floats under any switch, its regions do not overlap."""
    import struct
    from vaw_amd.ops import gn_plan
    lib = vaw_amd.lib()
    try:
        for C in list(range(4, 2049, 4)) + [2052, 4096]:
            groups = sorted({G for G in (1, 32, 64, C // 4) if C % G == 0})
            for B in (1, 2, 3, 127, 128, 256, 511, 512, 4096):
                for HW in (1, 16, 127, 128, 129, 512, 513, 1024, 4096, 16384):
                    cap = lib.vaw_groupnorm_workspace_floats(B, HW, C)
                    for switch, dt, G in ((s, d, g) for s in (-1, 0, 1) for d in (0, 1) for g in groups):
                        lib.vaw_debug_gn_flat(switch)
                        want, where = _gn_want(switch, dt, B, HW, C, G), f"switch={switch} dt={dt} B={B} HW={HW} C={C} G={G}"
                        if want is None:
                            assert G > 64, where
                            for gn_pass in range(4):
                                with pytest.raises(vaw_amd.VawError):
                                    gn_plan(gn_pass, dt, B, HW, C, G)
                            continue
                        for gn_pass in range(4):
                            got = struct.unpack_from(_GN_FIELDS, gn_plan(gn_pass, dt, B, HW, C, G))
                            assert got == want[gn_pass], f"{where} pass={gn_pass}: {got} != {want[gn_pass]}"
                        flat, rows, nch, nt, rpi, gx, gy, gz, block = want[0][:9]          # the properties, on the fields just compared
                        assert nch * rows >= HW > (nch - 1) * rows and block == 256, where
                        if flat:
                            assert nt == 256 // (C // 8) * (C // 8) and 1 <= rpi == nt // (C // 8) and nt <= block and 2 * rpi * C <= 4096 \
                                and 2 * C <= 4096 and (gx, gy, gz) == (B * nch, 1, 1), where
                        else:
                            assert (gx, gy, gz) == (-(-C // 64), B, nch) and gy <= 65535 and gz <= 65535, where
                        assert want[0][10:12] == (2 * nch * B * C, 0) and want[0][10] <= cap and want[1][10:15] == (0, -1, -1, -1, -1), where
                        ws, part, sums, s1, s2 = want[2][10:15]
                        assert 0 == part and part + 4 * nch * B * C <= sums and sums + 4 * B * C <= s1 and s1 + B * G <= s2 and s2 + B * G <= ws <= cap, where
                        assert want[3][10:15] == (ws, -1, -1, s1, s2), where
    finally:
        lib.vaw_debug_gn_flat(-1)


def test_gn_plan_refusals_and_production_pins():
    """Refused: a dtype that is neither f32 nor bf16 (the fp8 tags used to run as bf16), C % 4, C % G, G > 64, B >= 65536, a size <= 0,
    a quad launch of more than 65535 chunks (grid.z).  Pinned: the five shapes of tools/gn_bench.py (UNet_64) at bf16 under the
    default switch, worked out by hand from the rule before the plan existed."""
    from vaw_amd import _lib as L
    from vaw_amd.ops import gn_plan
    ok = dict(dt=L.BF16, B=2, HW=64, C=64, G=32)
    bad = [dict(dt=L.FP8), dict(dt=L.BF8), dict(dt=7), dict(C=66, G=1), dict(C=36, G=8), dict(C=520, G=130), dict(C=260, G=65),
           dict(B=65536), dict(B=0), dict(HW=0), dict(C=0), dict(G=0), dict(B=-1), dict(HW=-5),
           dict(dt=L.F32, B=1, HW=65536 * 512, C=4, G=1), dict(dt=L.BF16, B=1, HW=65535 * 512 + 1, C=4, G=1)]
    pins = {(256, 4096, 192): (L.GNV_FLAT, 512), (256, 1024, 384): (L.GNV_FLAT, 512), (128, 4096, 192): (L.GNV_FLAT, 512),
            (256, 256, 576): (L.GNV_FLAT, 128), (256, 64, 768): (L.GNV_QUAD, 512)}
    for gn_pass in (L.GN_FWD_SUMS, L.GN_APPLY, L.GN_BWD_SUMS, L.GN_BWD_APPLY):
        assert gn_plan(gn_pass, **ok).status == 0
        assert gn_plan(gn_pass, L.F32, 1, 65535 * 512, 4, 1).grid_z == 65535          # the last HW the quad grid holds
        for change in bad:
            with pytest.raises(vaw_amd.VawError):
                gn_plan(gn_pass, **{**ok, **change})
        for (B, HW, C), want in pins.items():
            p = gn_plan(gn_pass, L.BF16, B, HW, C)
            assert (p.variant, p.rows) == want, (B, HW, C, gn_pass, p.variant, p.rows)
    with pytest.raises(vaw_amd.VawError):
        gn_plan(4, **ok)
