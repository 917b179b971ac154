"""Host side of vaw_amd.Sampler without a GPU: label draws, the CPU finish, the host-side guidance predicate, the two
distributed helpers over gloo, and the argument checks of the three sampler entry points of the C ABI."""
import ctypes as C
import os
import socket
import sys
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import vaw_amd
from conftest import REPO, load_pt, sampling_model
from sampler_cases import Standin, sampler_args


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sampler(**kw):
    st = dict(guidance_scale=2.5)
    return vaw_amd.Sampler(sampler_args("ddim", st, **kw), "cpu", Standin(sampling_model), None)


def test_get_y_cond_follows_the_reference_stream_and_its_assertions():
    g = load_pt("sampler.pt")
    rec = g["cases"]["p20_x0_large/always"]
    s = _sampler()
    torch.manual_seed(rec["seed"])
    y = s._get_y_cond(g["sample_size"], g["num_classes"])
    assert y.dtype == torch.int64 and torch.equal(y, rec["labels"][0])          # the first draw of the seeded stream
    assert _sampler(class_cond=False)._get_y_cond(3, 10) is None
    s = _sampler(class_labels=[4, 7])
    torch.manual_seed(0)
    idx = torch.randint(2, (3,))
    torch.manual_seed(0)
    assert torch.equal(s._get_y_cond(3, 10), torch.tensor([4, 7])[idx])
    with pytest.raises(AssertionError, match="class_labels must be integers"):
        _sampler(class_labels=[4, 10])._get_y_cond(3, 10)
    with pytest.raises(AssertionError, match="class_labels must be integers"):
        _sampler(class_labels=[1.0])._get_y_cond(3, 10)
    with pytest.raises(AssertionError, match="must be <= sample_size"):
        _sampler(class_labels=[1, 2, 3, 4])._get_y_cond(3, 10)


def test_inverse_normalize_on_cpu_reproduces_the_fixture_bytes():
    g = load_pt("sampler.pt")
    s = _sampler()
    for name, rec in g["cases"].items():
        for f, img in zip(rec["floats"], rec["images"]):
            got = s._inverse_normalize(f)
            assert got.dtype == torch.uint8 and got.shape == (f.shape[0], f.shape[2], f.shape[3], f.shape[1]) and got.is_contiguous()
            assert torch.equal(got, img), name


def test_guidance_predicate_from_a_host_t_mean_agrees_with_guidance_active():
    g = load_pt("sampling.pt")
    x, y = g["cfg_x"], g["cfg_y"]
    calls = []

    def model(xx, t, **kw):
        calls.append(xx.shape[0])
        return sampling_model(xx, t, **kw)

    for nm, scale, interval, tval in [("plain", 1.0, (-1.0, -1.0), 500.0), ("always", 2.5, (-1.0, -1.0), 500.0),
                                      ("inside", 1.8, (100.0, 600.0), 300.0), ("outside", 1.8, (100.0, 600.0), 800.0)]:
        m = vaw_amd.IntervalCFG(model, 10, scale, interval, True)
        t = torch.full((4,), tval)
        for t_mean in (None, tval):                      # read back from t / handed over by the caller
            del calls[:]
            halves = m.guided_halves(x, t, t_mean=t_mean, y=y)
            assert (halves is not None) == m.guidance_active(tval), (nm, t_mean)
            if halves is None:
                assert calls == []
                torch.testing.assert_close(m.unguided(x, t, y=y), g["cfg"][nm], rtol=1e-6, atol=1e-6)
            else:
                assert calls == [8] and halves.shape == (8, 3, 8, 8)
                torch.testing.assert_close(m.combine(halves), g["cfg"][nm], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(m(x, t, y=y), g["cfg"][nm], rtol=1e-6, atol=1e-6)
        # the host value wins over the tensor: that is what lets the loops skip the read-back
        assert (m.guided_halves(x, torch.full((4,), 800.0), t_mean=300.0, y=y) is not None) == m.guidance_active(300.0)
    # the value the loops hand over: the timestep as the model sees it, mapped and rescaled
    from sampler_cases import spaced
    d, _ = spaced("ddim10_eps_range_eta", sampler_args("ddim", dict(guidance_scale=2.5)))
    seen = []
    d._respaced(lambda xx, t, **kw: seen.append(t))(x, torch.tensor([0, 3, 9, 9]))
    assert [d._host_model_time(i) for i in (0, 3, 9)] == [float(v) for v in seen[0][:3]]
    plain = vaw_amd.GaussianDiffusion(args=sampler_args("ddim", dict(guidance_scale=2.5)), betas=vaw_amd.get_named_beta_schedule("linear", 300),
                                      model_mean_type=vaw_amd.ModelMeanType.EPSILON, model_var_type=vaw_amd.ModelVarType.FIXED_LARGE,
                                      loss_type=vaw_amd.LossType.MSE, rescale_timesteps=True)
    assert [plain._host_model_time(i) for i in (0, 7, 299)] == [float(v) for v in plain._scale_timesteps(torch.tensor([0, 7, 299]))]


def _dist_worker(rank, world, port, q):
    try:
        sys.path.insert(0, REPO)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import vaw_amd
        from sampler_cases import Standin, sampler_args
        vaw_amd.dist_util.setup_dist()
        torch.manual_seed(100 + rank)
        model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))          # ranks start different
        vaw_amd.sync_ema_model(model)
        flat = torch.cat([p.detach().flatten() for p in model.parameters()])
        gathered = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(gathered, flat)
        torch.manual_seed(100)
        ref = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
        assert all(torch.equal(t, torch.cat([p.detach().flatten() for p in ref.parameters()])) for t in gathered), "not rank 0's weights"
        for class_cond in (True, False):
            s = vaw_amd.Sampler(sampler_args("ddim", dict(guidance_scale=2.5), parallel=True, class_cond=class_cond), "cpu", Standin(None), None)
            samples, labels = [], []
            for batch in range(2):
                img = torch.full((3, 8, 8, 3), 10 * batch + rank, dtype=torch.uint8)
                s._gather_samples(samples, labels, img, torch.full((3,), 10 * batch + rank) if class_cond else None, world)
            assert len(samples) == 2 * world and len(labels) == (2 * world if class_cond else 0)
            for batch in range(2):
                for r in range(world):                         # per batch, every rank's block in rank order
                    a = samples[batch * world + r]
                    assert a.dtype.name == "uint8" and a.shape == (3, 8, 8, 3) and (a == 10 * batch + r).all()
                    if class_cond:
                        assert labels[batch * world + r].dtype.name == "int64" and (labels[batch * world + r] == 10 * batch + r).all()
        vaw_amd.dist_util.dist_barrier()
        vaw_amd.dist_util.cleanup_dist()
        q.put((rank, "ok"))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_gather_samples_and_sync_ema_model_over_two_gloo_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in results:
        assert msg == "ok", f"rank {rank}:\n{msg}"


def test_sampler_entry_points_reject_bad_arguments_before_any_launch():
    """Null required pointers, B <= 0, model_ld < per_sample: VAW_ERR_INVALID (-1) from the host-side checks.  No GPU is
    present here, so a launch would have failed with another code."""
    lib = vaw_amd.lib()
    for name in ("vaw_guided_sample_step", "vaw_cfg_combine", "vaw_finish_images"):
        assert name in vaw_amd.exported_symbols() and hasattr(lib, name)
    p = 4096          # never dereferenced: every call below fails its argument check

    def step(kind=2, mc=p, mu=p, vc=p, vu=p, ld=192, x=p, nz=p, coef=p, mm=0, vm=2, sample=p, B=3, n=192):
        return lib.vaw_guided_sample_step(kind, mc, mu, vc, vu, ld, 2.5, x, nz, coef, mm, vm, 1, 0.0, sample, p, None, None, B, n, None)

    for bad in (dict(mc=None), dict(x=None), dict(coef=None), dict(B=0), dict(B=-1), dict(n=0), dict(ld=191), dict(kind=3), dict(kind=-1),
                dict(vm=3), dict(mm=2), dict(vc=None), dict(vu=None), dict(nz=None), dict(sample=None)):
        assert step(**bad) == -1, bad
        assert b"guided_sample_step" in lib.vaw_last_error_string()
    comb = lambda c=p, u=p, ld=192, out=p, B=3, n=192: lib.vaw_cfg_combine(c, u, ld, 2.5, out, B, n, None)
    for bad in (dict(c=None), dict(u=None), dict(out=None), dict(B=0), dict(n=0), dict(ld=100)):
        assert comb(**bad) == -1, bad
        assert b"cfg_combine" in lib.vaw_last_error_string()
    fin = lambda src=p, f64=0, dst=p, B=2, Cn=3, H=8, W=8: lib.vaw_finish_images(src, f64, dst, B, Cn, H, W, None)
    for bad in (dict(src=None), dict(dst=None), dict(B=0), dict(Cn=0), dict(H=0), dict(W=-2), dict(f64=2), dict(src=4098), dict(src=4100, f64=1)):
        assert fin(**bad) == -1, bad
        assert b"finish_images" in lib.vaw_last_error_string()
    x = torch.zeros(2, 3, 8, 8)
    for call in (lambda: vaw_amd.ops.finish_images(x), lambda: vaw_amd.ops.cfg_combine(x, x, 2.0)):
        with pytest.raises(vaw_amd.VawError, match="GPU only"):
            call()


def test_sampler_refusals_and_exports():
    assert vaw_amd.Sampler is vaw_amd.sampler.Sampler and vaw_amd.sync_ema_model is vaw_amd.sampler.sync_ema_model
    st = dict(guidance_scale=2.5)
    with pytest.raises(NotImplementedError, match="decode_fn"):
        vaw_amd.Sampler(sampler_args("ddim", st, in_chans=4), "cpu", Standin(sampling_model), None)
    with pytest.raises(NotImplementedError, match="classifier"):
        vaw_amd.Sampler(sampler_args("ddim", st), "cpu", Standin(sampling_model), None, classifier=object())
    with pytest.raises(ValueError, match="Unsupported model_mode: energy"):
        vaw_amd.Sampler(sampler_args("ddim", st, model_mode="energy"), "cpu", Standin(sampling_model), None).sample(3, 3, 8, 10)
    s = vaw_amd.Sampler(sampler_args("ddim", st, in_chans=4), "cpu", Standin(sampling_model), None, decode_fn=lambda z: z[:, :3])
    assert s.decode_fn is not None
