"""Public names of vaw_amd."""
from . import dist_util, evaluator, gaussian_diffusion, noise, ops, resample, respace, sampler, utils  # noqa: F401
from ._lib import LIB_PATH, VawError, exported_symbols, lib  # noqa: F401
from .dit import DiT, DiT_B, DiT_L, DiT_S, DiT_XL, DiT_models  # noqa: F401
from .flat import FlatModule  # noqa: F401
from .unet import (ADM_32, ADM_64, ADM_128, ADM_256, ADM_512, LDM, UNet_32, UNet_64, UNet_models, UNetModel,  # noqa: F401
                   create_unet_model)
from .gaussian_diffusion import (FlowMatching, GaussianDiffusion, LossType, ModelMeanType, ModelVarType,  # noqa: F401
                                 compute_mse_loss_weight, get_named_beta_schedule, mean_flat)
from .optim import FusedAdamW  # noqa: F401
from .guard import StepGuard  # noqa: F401
# (`vaw_amd.ema` stays trainer.ema, the function, imported below: reach the module as `from vaw_amd.ema import ...`)
from .ema import (PowerEMA, gamma_to_sigma_rel, lincomb_fold, posthoc_coefficients, posthoc_ema, power_ema_coefficient,  # noqa: F401
                  profile_dot, sigma_rel_to_gamma)
from .parallel import DistributedDataParallel  # noqa: F401
from .data import DevicePrefetcher, LatentBatchLoader, LatentH5Dataset, ShardedSampler  # noqa: F401
from .samplers import EDMDenoiser, dpm_sample, edm_sample, flow_log_likelihood, flow_ode_sample, flow_sde_sample  # noqa: F401
from .noise import SeededNoise  # noqa: F401
from .respace import SpacedDiffusion, space_timesteps  # noqa: F401
from .sampler import IntervalCFG, Sampler, sync_ema_model  # noqa: F401
from .resample import (DeviceLossSecondMomentResampler, LossSecondMomentResampler, UniformSampler, create_named_schedule_sampler)  # noqa: F401
from .trainer import Trainer, ema, sample_from_latent  # noqa: F401
from .utils import get_lr_lambda, load_checkpoint, save_checkpoint, set_random_seed, warmup_cosine_lr  # noqa: F401
from .evaluator import (Evaluator, FIDStatistics, ManifoldEstimator, compute_density_coverage, compute_inception_score,  # noqa: F401
                        compute_kid, compute_prec_recall, compute_statistics, inception_score_from_probs, inception_split_scores,
                        inception_split_scores_from_probs, kid_subset_indices, kid_subset_scores, metrics_from_activations,
                        polynomial_mmd2)
