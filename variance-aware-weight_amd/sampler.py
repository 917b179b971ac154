"""The sampling front end (behaviour of the reference's tools/sampler.py): interval classifier-free guidance
(`IntervalCFG` :10-48, pinned by tests/golden/sampling.pt), `sync_ema_model` :92-94 and the `Sampler` class :97-269 that
turns a trained model into lists of uint8 NHWC image batches and labels for the FID evaluators (pinned by
tests/golden/sampler.pt).  The reverse-process loops live in gaussian_diffusion.py / samplers.py; VAE decode beyond the
`decode_fn` hook and classifier guidance are out of scope."""
import torch
import torch.distributed as dist

from . import dist_util, ops
from .noise import SeededNoise
from .samplers import DPM_SOLVERS, EDMDenoiser, dpm_sample, edm_sample, flow_ode_sample, flow_sde_sample


class IntervalCFG(torch.nn.Module):
    """Guided denoiser:  eps = eps(null) + s * (eps(y) - eps(null)).

    Guidance is active when s != 1, labels are given, and -- if `interval` = (lo, hi) is a proper range with lo >= 0 --
    the batch's mean timestep lies in [lo, hi).  Active calls evaluate the wrapped model ONCE on the batch stacked on
    itself, second half labelled with the null class `num_classes`; inactive calls pass straight through."""

    def __init__(self, model, num_classes, guidance_scale=1.0, interval=(-1.0, -1.0), class_cond=True):
        super().__init__()
        self.model = model
        self.null_label = int(num_classes)
        self.guidance_scale = float(guidance_scale)
        self.interval = interval
        self.class_cond = class_cond

    def guidance_active(self, t_mean):
        """Pure host-side predicate on the mean timestep of a call."""
        if abs(self.guidance_scale - 1.0) < 1e-8:
            return False
        lo, hi = self.interval
        bounded = lo >= 0 and hi > lo
        return (lo <= t_mean < hi) if bounded else True

    @staticmethod
    def _rows(x, t):
        n = x.shape[0]
        t = t.reshape(-1)
        if t.numel() == 1:
            t = t.expand(n)
        elif t.numel() != n:
            raise ValueError(f"IntervalCFG: {t.numel()} timesteps for a batch of {n}")
        return t

    def guided_halves(self, x, t, t_mean=None, **model_kwargs):
        """The model output of the stacked guided call, NOT combined: [2N, ...] with rows [:N] evaluated under the labels and
        rows [N:] under the null label -- or None when guidance is inactive for this call (then `unguided` is the call to
        make).  `t_mean` is the mean timestep as the model sees it, when the caller knows it on the host (the sampling
        loops do); without it the predicate reads t back from the device, as forward always did."""
        n = x.shape[0]
        t = self._rows(x, t)
        y = model_kwargs.get("y")
        if not (self.class_cond and y is not None):
            return None
        if not self.guidance_active(float(t.float().mean()) if t_mean is None else float(t_mean)):
            return None
        if y.shape[0] != n:
            raise AssertionError(f"CFG expects label batch size {n}, but got {y.shape[0]}.")
        stacked = {**model_kwargs, "y": torch.cat((y, y.new_full(y.shape, self.null_label)))}
        out = self.model(x.repeat(2, *([1] * (x.dim() - 1))), t.repeat(2), **stacked)
        return out[0] if isinstance(out, tuple) else out          # DiT returns (eps, aux)

    def unguided(self, x, t, **model_kwargs):
        """The pass-through call of an inactive step."""
        return self.model(x, self._rows(x, t), **model_kwargs)

    def combine(self, out):
        """without + s * (with_label - without) over the stacked output: one kernel for f32 on the GPU (bitwise the three
        tensor operations), the tensor operations anywhere else."""
        n = out.shape[0] // 2
        with_label, without = out[:n], out[n:]
        if out.is_cuda and out.dtype == torch.float32 and not (torch.is_grad_enabled() and out.requires_grad):
            return ops.cfg_combine(with_label, without, self.guidance_scale)
        return without + self.guidance_scale * (with_label - without)

    def forward(self, x, t, **model_kwargs):
        out = self.guided_halves(x, t, **model_kwargs)
        if out is None:
            return self.unguided(x, t, **model_kwargs)
        return self.combine(out)


def sync_ema_model(eval_model):
    """Every rank takes rank 0's parameters (reference :92-94)."""
    for param in eval_model.parameters():
        dist.broadcast(param.data, src=0)


class Sampler:
    """`Sampler(args, device, ema_model, diffusion).sample(num_samples, sample_size, image_size, num_classes)` ->
    (list of uint8 [sample_size, H, W, C] numpy batches, list of int64 label batches), as the reference's class.

    Extensions: `decode_fn(latents) -> images in [-1, 1]` stands where the reference loads a diffusers VAE
    (args.in_chans == 4; the latents are handed over already divided by args.latent_scale); with args.cpu_rng the labels
    and every noise draw come from the CPU generator in the reference's order, which reproduces its CPU stream.
    args.hip_graph=True (EDM, multistep and flow generators, whose loops do not synchronise with the host; not the adaptive
    solver="rk45", whose every step the host decides): the first batch runs eagerly,
    the second is captured into one graph on static label and output buffers, later batches replay it; the labels are drawn
    outside the graph in the same order, so images and labels are those of the eager run.  "auto" or absent: eager.

    Per-sample seeds (optional attributes of args; absent: the global generator, as above).  args.sample_seed = S, an int in
    [0, 2^63): the sample with global index k draws its label and all its noise from a stream of its own, seeded S + k
    (SeededNoise: one counter-based kernel, draw 0 the initial latent, then one draw per hook call of the solver), so image k does
    not depend on sample_size, on the number of ranks, on args.hip_graph or on what was drawn before it.  Row i of batch n of rank
    r of w ranks (w = 1 without args.parallel) is k = sample_start + (n * w + r) * sample_size + i, the order _gather_samples
    lays the batches out in; args.sample_start (default 0) continues an interrupted run; args.sample_shard = (r, w) overrides
    rank and world in that formula (one process standing in for rank r; refused with args.parallel).  Refused with
    args.cpu_rng.  What is promised is the noise and the solver arithmetic around the network, both row-independent; a
    network whose kernels depend on the batch size is its own business.  The adaptive solver="rk45" gets its per-sample
    initial noise too, but controls its steps by an error norm over the whole batch: its images depend on what else is in
    the batch, and nothing is promised there."""

    def __init__(self, args, device, eval_model, diffusion, classifier=None, decode_fn=None):
        if classifier is not None:
            raise NotImplementedError("classifier guidance (cond_fn) is out of scope: pass classifier=None")
        if args.in_chans == 4 and decode_fn is None:
            raise NotImplementedError("in_chans == 4 samples latents: pass decode_fn(latents) -> images in [-1, 1] "
                                      "(the reference's diffusers VAE is not built here)")
        self.args = args
        self.device = device
        self.model = eval_model
        self.diffusion = diffusion
        self.classifier = None
        self.decode_fn = decode_fn if args.in_chans == 4 else None
        self._noise = None          # the SeededNoise of a run under args.sample_seed (_run)

    # ---- pieces -------------------------------------------------------------------------------------------------
    def _cpu_rng(self):
        return bool(getattr(self.args, "cpu_rng", False))

    def _seed_plan(self):
        """(S, o, r, w) of a run under args.sample_seed -- the base seed, the first global index, the rank and the world of
        the index formula -- or None without it."""
        a = self.args
        S, o, shard = getattr(a, "sample_seed", None), getattr(a, "sample_start", None), getattr(a, "sample_shard", None)
        if S is None:
            if o or shard is not None:
                raise ValueError("args.sample_start / args.sample_shard: only with args.sample_seed")
            return None
        is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
        if not (is_int(S) and 0 <= S < 2 ** 63):
            raise ValueError(f"args.sample_seed: {S!r} is not an int in [0, 2^63)")
        o = 0 if o is None else o
        if not (is_int(o) and o >= 0):
            raise ValueError(f"args.sample_start: {o!r} is not a non-negative int")
        if self._cpu_rng():
            raise ValueError("args.sample_seed: not with args.cpu_rng (the noise comes from the per-sample streams or from the CPU "
                             "stream, not both)")
        if shard is not None:
            if a.parallel:
                raise ValueError("args.sample_shard: not with args.parallel (the process group names rank and world)")
            if not (isinstance(shard, (tuple, list)) and len(shard) == 2 and all(is_int(v) for v in shard) and 0 <= shard[0] < shard[1]):
                raise ValueError(f"args.sample_shard: {shard!r} is not (rank, world) with 0 <= rank < world")
            return S, o, shard[0], shard[1]
        if a.parallel:
            return S, o, dist.get_rank(), dist.get_world_size()
        return S, o, 0, 1

    def _sample_indices(self, n, sample_size):
        """The global indices of the rows of this rank's batch number n."""
        _, o, r, w = self._seed_plan()
        first = o + (n * w + r) * sample_size
        return range(first, first + sample_size)

    def _sample_seeds(self, n, sample_size):
        """Their seeds S + k, wrapped to the int64 that holds the same 64-bit pattern."""
        S = self._seed_plan()[0]
        return [(S + k + 2 ** 63) % 2 ** 64 - 2 ** 63 for k in self._sample_indices(n, sample_size)]

    def _build_cfg_model(self, num_classes):
        return IntervalCFG(self.model, num_classes, self.args.guidance_scale, self.args.interval, self.args.class_cond).eval()

    def _build_denoiser(self, image_size, num_classes):
        a = self.args
        return EDMDenoiser(self._build_cfg_model(num_classes), img_resolution=image_size, img_channels=a.in_chans,
                           label_dim=num_classes, noise_schedule=a.path_type, amp=a.amp, pred_type=a.mean_type).to(self.device)

    def _randint(self, high, sample_size):
        if self._noise is not None:
            return self._noise.randint(high)
        if self._cpu_rng():
            return torch.randint(0, high, (sample_size,)).to(self.device)
        return torch.randint(0, high, (sample_size,), device=self.device)

    def _randn(self, shape):
        if self._noise is not None:
            return self._noise.randn(shape)
        if self._cpu_rng():
            return torch.randn(shape).to(self.device)
        return torch.randn(shape, device=self.device)

    def _randn_like(self, x):
        if self._noise is not None:
            return self._noise.randn_like(x)
        if self._cpu_rng():
            return torch.randn(x.shape, dtype=x.dtype).to(x.device)
        return torch.randn_like(x)

    def _get_y_cond(self, sample_size, num_classes):
        if not self.args.class_cond:
            return None
        labels = self.args.class_labels
        if labels is None:
            return self._randint(num_classes, sample_size)
        assert all(isinstance(label, int) and 0 <= label < num_classes for label in labels), f"class_labels must be integers in [0, {num_classes})"
        assert len(labels) <= sample_size, f"len(class_labels) must be <= sample_size ({sample_size})"
        labels = torch.tensor(labels, device=self.device, dtype=torch.long)
        return labels[self._randint(len(labels), sample_size)]

    def _gather_samples(self, all_samples, all_labels, samples, class_labels, world_size):
        if self.args.parallel:
            gathered = [torch.zeros_like(samples) for _ in range(world_size)]
            dist.all_gather(gathered, samples)
            all_samples.extend(batch.cpu().numpy() for batch in gathered)
            if self.args.class_cond:
                gathered = [torch.zeros_like(class_labels) for _ in range(world_size)]
                dist.all_gather(gathered, class_labels)
                all_labels.extend(batch.cpu().numpy() for batch in gathered)
            return
        all_samples.append(samples.cpu().numpy())
        if self.args.class_cond:
            all_labels.append(class_labels.cpu().numpy())

    def _inverse_normalize(self, samples):
        if samples.is_cuda:
            return ops.finish_images(samples)
        return ((samples + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def _process_sample_label(self, samples, class_labels=None):
        if self.decode_fn is not None:
            with torch.no_grad():
                samples = self.decode_fn(samples / self.args.latent_scale)
        return self._inverse_normalize(samples), class_labels

    # ---- the three generators -----------------------------------------------------------------------------------
    def _use_graph(self):
        if getattr(self.args, "hip_graph", None) is not True:
            return False
        why = ("not with solver rk45 (the host decides every step from the error norm: nothing to capture)"
               if self.args.model_mode == "flow" and self.args.solver == "rk45" else
               "not with args.cpu_rng (the noise would come from the host every step)" if self._cpu_rng() else
               "not with args.parallel" if self.args.parallel else
               "the model's forward is not capturable" if getattr(self.model, "graph_capturable", True) is False else
               "needs a CUDA device" if torch.device(self.device).type != "cuda" else None)
        if why:
            raise ValueError(f"args.hip_graph: {why}")
        return True

    def _run(self, draw_batch, num_samples, sample_size, num_classes, progress_bar, desc, graph=False):
        """The loop the reference's three samplers share: sync the EMA weights, then batches of draw_batch(labels) until
        num_samples are there (counted per rank, as the reference does).  graph: from the second batch on draw_batch runs
        as one captured graph.  Under args.sample_seed every batch begins with its rows' seeds copied into the SeededNoise's
        buffer (which a captured graph reads on replay), and labels and noise come from there."""
        self._noise = SeededNoise(self.device) if self._seed_plan() is not None else None
        n_batch = 0
        self.model.eval()
        captured = None          # (graph, static labels, static samples)
        all_samples, all_labels = [], []
        world_size = dist.get_world_size() if self.args.parallel else 1
        if self.args.parallel:
            sync_ema_model(self.model)
            dist.barrier()
        pbar = None
        if progress_bar and dist_util.is_main_process():
            from tqdm import tqdm
            pbar = tqdm(total=num_samples, desc=desc)
        while len(all_samples) * sample_size < num_samples:
            if self._noise is not None:
                self._noise.begin(self._sample_seeds(n_batch, sample_size))
                n_batch += 1
            class_labels = self._get_y_cond(sample_size, num_classes)
            with torch.no_grad():
                if not graph or not all_samples:
                    samples = draw_batch(class_labels)          # eager; with graph: the batch that builds the tables and workspaces
                else:
                    if captured is None:
                        static_labels = None if class_labels is None else class_labels.clone()
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        try:
                            with torch.cuda.graph(g):
                                static_samples = draw_batch(static_labels)
                        except RuntimeError as e:
                            raise ValueError(f"args.hip_graph: the model's forward is not capturable ({e})") from e
                        captured = (g, static_labels, static_samples)
                    elif class_labels is not None:
                        captured[1].copy_(class_labels)
                    captured[0].replay()
                    samples = captured[2]
            samples, class_labels = self._process_sample_label(samples, class_labels)
            self._gather_samples(all_samples, all_labels, samples, class_labels, world_size)
            if pbar is not None:
                pbar.update(samples.shape[0] * world_size)
        return all_samples, all_labels

    def ddim_sampler(self, num_samples, sample_size, image_size, num_classes, progress_bar=False):
        cfg_model = self._build_cfg_model(num_classes)
        shape = (sample_size, self.args.in_chans, image_size, image_size)

        def draw(class_labels):
            return self.diffusion.ddim_sample_loop(cfg_model, shape, device=self.device,
                                                   model_kwargs={"y": class_labels} if self.args.class_cond else {}, cond_fn=None,
                                                   randn_like=self._randn_like if self._noise is not None else None)

        return self._run(draw, num_samples, sample_size, num_classes, progress_bar, "Generating Samples (DDIM)")

    def edm_sampler(self, num_samples, sample_size, image_size, num_classes, progress_bar=False):
        a = self.args
        net = self._build_denoiser(image_size, num_classes)

        def draw(class_labels):
            latents = self._randn([sample_size, net.img_channels, net.img_resolution, net.img_resolution])
            return edm_sample(net, latents, class_labels=class_labels, randn_like=self._randn_like, num_steps=a.sample_steps,
                              solver=a.solver, discretization=a.discretization, schedule=a.schedule, scaling=a.scaling)

        return self._run(draw, num_samples, sample_size, num_classes, progress_bar, f"Generating Samples ({a.solver.capitalize()})",
                         graph=self._use_graph())

    def dpm_sampler(self, num_samples, sample_size, image_size, num_classes, progress_bar=False):
        """The multistep solvers of samplers.dpm_sample (args.solver dpmpp2m | dpmpp2m_sde | expab): one evaluation per step.
        Optional args: eta, s_noise (dpmpp2m_sde; 1.0), order (expab; 3), clip_denoised (False)."""
        a = self.args
        net = self._build_denoiser(image_size, num_classes)

        def draw(class_labels):
            latents = self._randn([sample_size, net.img_channels, net.img_resolution, net.img_resolution])
            return dpm_sample(net, latents, class_labels=class_labels, randn_like=self._randn_like, num_steps=a.sample_steps,
                              solver=a.solver, order=getattr(a, "order", None), discretization=a.discretization,
                              eta=getattr(a, "eta", 1.0), s_noise=getattr(a, "s_noise", 1.0),
                              clip_denoised=getattr(a, "clip_denoised", False))

        return self._run(draw, num_samples, sample_size, num_classes, progress_bar, f"Generating Samples ({a.solver})",
                         graph=self._use_graph())

    def flow_matching_sampler(self, num_samples, sample_size, image_size, num_classes, progress_bar=False):
        a = self.args
        cfg_model = self._build_cfg_model(num_classes)
        sampler_type = getattr(a, "sampler_type", None) or getattr(self.diffusion, "sampler_type", "ode")
        if sampler_type not in ("ode", "sde"):
            raise NotImplementedError(f"Unsupported sampler_type: {sampler_type}")

        def draw(class_labels):
            noise = self._randn([sample_size, a.in_chans, image_size, image_size])
            if sampler_type == "sde":
                return flow_sde_sample(self.diffusion, cfg_model, noise, self.device, num_steps=a.sample_steps, solver=a.solver,
                                       randn_like=self._randn_like, y=class_labels)
            return flow_ode_sample(self.diffusion, cfg_model, noise, self.device, num_steps=a.sample_steps, solver=a.solver,
                                   rtol=getattr(a, "rtol", None), atol=getattr(a, "atol", None), y=class_labels)

        return self._run(draw, num_samples, sample_size, num_classes, progress_bar, f"Generating Samples ({a.solver.capitalize()})",
                         graph=self._use_graph())

    def sample(self, num_samples, sample_size, image_size, num_classes, progress_bar=False):
        if self.args.model_mode == "flow":
            return self.flow_matching_sampler(num_samples, sample_size, image_size, num_classes, progress_bar)
        if self.args.model_mode == "diffusion":
            if self.args.solver == "ddim":
                return self.ddim_sampler(num_samples, sample_size, image_size, num_classes, progress_bar)
            if self.args.solver in DPM_SOLVERS:
                return self.dpm_sampler(num_samples, sample_size, image_size, num_classes, progress_bar)
            return self.edm_sampler(num_samples, sample_size, image_size, num_classes, progress_bar)
        raise ValueError(f"Unsupported model_mode: {self.args.model_mode}")
