/* vaw_hip.h -- C ABI of libvaw_hip.so: the MI355X (gfx950) kernels underneath the
 * variance-aware-weighted diffusion training step.
 *
 * The reference (LilYau350/Variance-Aware-Weight) has no FFI for this path: it is
 * Python calling ATen/cuDNN/cuBLAS.  The drop-in boundary is therefore its Python
 * call surface (Trainer.train_step -> GaussianDiffusion.training_losses -> model),
 * mirrored by the `vaw_amd` package, and THIS header is what that package binds
 * through ctypes.  Each entry point names the reference arithmetic it replaces
 * (paths are relative to the reference repository root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *  - no allocation, no synchronisation, no hidden state: safe for stream capture;
 *  - return value: VAW_OK or a negative vaw_status; vaw_last_error_string() gives
 *    the message of the calling thread's last failure;
 *  - "act dtype" is the storage type of activations: VAW_F32 (parity mode) or
 *    VAW_BF16 (throughput mode).  Accumulation, statistics, the residual stream,
 *    gradients of parameters and the optimizer state are always f32.
 */
#ifndef VAW_HIP_H
#define VAW_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { VAW_OK = 0, VAW_ERR_INVALID = -1, VAW_ERR_LAUNCH = -2, VAW_ERR_UNSUPPORTED = -3 } vaw_status;
typedef enum { VAW_F32 = 0, VAW_BF16 = 1,
               VAW_FP8 = 2, VAW_BF8 = 3 /* OCP e4m3fn / e5m2: GEMM operand formats of vaw_gemm_fp8 and vaw_wgrad_grouped only */,
               VAW_F64 = 4 /* output type of vaw_randn_seeded only */ } vaw_dtype;
typedef void* vaw_stream;

int vaw_version(void);
const char* vaw_last_error_string(void);

/* ---------------------------------------------------------------------------
 * Diffusion objective  (tools/gaussian_diffusion.py)
 * ------------------------------------------------------------------------- */

/* q_sample :234-252 with the table gather of _extract_into_tensor :1059-1072 fused in:
 *   x_t[b,:] = tab_a[t[b]] * x0[b,:] + tab_s[t[b]] * noise[b,:]
 * tab_a/tab_s: f32[T] = float(float64 table).  t out of [0,T) poisons the row with NaN.
 * This entry, vaw_mix_rows, vaw_wmse_fwd(_t) and vaw_wmse_bwd(_t): 16-byte loads and stores when per_sample % 4 == 0 and every
 * [B, per_sample] tensor is 16-byte aligned, scalar ones otherwise (any alignment, any length). */
int vaw_qsample_fwd(const float* x0, const float* noise, const int64_t* t, const float* tab_a, const float* tab_s,
                    int num_timesteps, float* x_t, int B, int64_t per_sample, vaw_stream stream);

/* out[b,:] = ca[b]*x[b,:] + cb[b]*y[b,:]  -- FlowMatching.q_sample :1277-1281 and the
 * VELOCITY / VECTOR targets of compute_target :818-832, :1284-1300. */
int vaw_mix_rows(const float* x, const float* y, const float* ca, const float* cb, float* out, int B,
                 int64_t per_sample, vaw_stream stream);

/* training_losses :908-913 fused: target = ca[b]*x0 + cb[b]*noise (compute_target),
 * mse[b] = w[b] * mean_flat((target - model_out)^2)  (tools/nn.py:86-90). */
int vaw_wmse_fwd(const float* model_out, const float* x0, const float* noise, const float* ca, const float* cb,
                 const float* w, float* mse, int B, int64_t per_sample, vaw_stream stream);
/* d(model_out)[b,:] = gmse[b] * w[b] * 2 * (model_out - target) / per_sample */
int vaw_wmse_bwd(const float* model_out, const float* x0, const float* noise, const float* ca, const float* cb,
                 const float* w, const float* gmse, float* dout, int B, int64_t per_sample, vaw_stream stream);

/* The step's passes around the model, each one launch for a chain of tensor operations and bitwise the chain's values
 * (Trainer with VAW_STEP_FUSED unset or 1).
 * latent [B][2][per_sample]: mean and std planes of the VAE posterior of every sample.
 *   x0  = (mean + std * eps) * latent_scale                (tools/trainer.py:21-25)
 *   x_t = tab_a[t] * x0 + tab_s[t] * noise                 (q_sample, as vaw_qsample_fwd)
 *   t_float[b] = float(t[b]) * t_scale                     (_scale_timesteps :1055-1058; t_float may be NULL) */
int vaw_latent_qsample(const float* latent, const float* eps, const float* noise, const int64_t* t, const float* tab_a,
                       const float* tab_s, int num_timesteps, float latent_scale, float t_scale, float* x0, float* x_t,
                       float* t_float, int B, int64_t per_sample, vaw_stream stream);
/* vaw_wmse_fwd / vaw_wmse_bwd with the coefficient gather inside: row b takes ca, cb, w at t[b] (f32[num_timesteps] tables; t out
 * of range poisons the row with NaN), or at b when t is NULL (per-row vectors: the flow-matching objective).
 * mean_out (may be NULL) = sum_b mse[b] / B / accum from a second, single-workgroup launch with a fixed summation order.
 * bwd: d(model_out) of g[0] * inv_count * sum_b mse[b]; g is a device scalar (the gradient of the batch mean), inv_count =
 * 1 / (B * accum) -- what the backward of mean() / accum expands into a vector. */
int vaw_wmse_fwd_t(const float* model_out, const float* x0, const float* noise, const int64_t* t, const float* ca, const float* cb,
                   const float* w, int num_timesteps, float* mse, float* mean_out, float accum, int B, int64_t per_sample,
                   vaw_stream stream);
int vaw_wmse_bwd_t(const float* model_out, const float* x0, const float* noise, const int64_t* t, const float* ca, const float* cb,
                   const float* w, int num_timesteps, const float* g, float inv_count, float* dout, int B, int64_t per_sample,
                   vaw_stream stream);

/* Variational-bound term of the learned-variance objective and the KL losses: _vb_terms_bpd
 * (gaussian_diffusion.py:775-808) = q_posterior_mean_variance :254-276 + the training side of p_mean_variance
 * :278-384 + normal_kl / discretized_gaussian_log_likelihood (tools/losses.py:12-76) + mean_flat / ln 2, fused.
 *   vb[b] = scale * mean_flat(t[b]==0 ? decoder NLL : KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t))) / ln 2
 * coef: f32 [B][16], the per-sample rows of the one per-timestep table (vaw_guided_sample_step below; column layout in
 * csrc/elementwise.hip above SS_NCOEF).  mean_mode 0: model mean = posterior mean of pred_xstart, 1: mean_out itself (PREVIOUS_X).
 * var_mode 0: fixed, 1: LEARNED (var_out = log variance), 2: LEARNED_RANGE (var_out in [-1,1]).  All tensors f32,
 * [B, per_sample] contiguous.  bwd: d_var / d_mean (either may be NULL: the MSE+vb objective detaches the mean). */
int vaw_vb_fwd(const float* mean_out, const float* var_out, const float* x0, const float* x_t, const float* coef,
               int mean_mode, int var_mode, float scale, float* vb, int B, int64_t per_sample, vaw_stream stream);
int vaw_vb_bwd(const float* mean_out, const float* var_out, const float* x0, const float* x_t, const float* coef,
               int mean_mode, int var_mode, float scale, const float* gvb, float* d_mean, float* d_var, int B,
               int64_t per_sample, vaw_stream stream);

/* Likelihood evaluation, one timestep of calc_bpd_loop (gaussian_diffusion.py:950-1005) after the model call, fused:
 * _vb_terms_bpd :775-808 WITH clip_denoised (p_mean_variance :343-368; the training-side kernel above has no clip) and
 * the two report metrics of :989-991.  Per row b, with pred_xstart / model mean / log variance formed per element as
 * in the reverse step below (one shared device function) and never stored:
 *   vb         = mean_flat(t[b]==0 ? decoder NLL : KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t))) / ln 2
 *   xstart_mse = mean_flat((pred_xstart - x0)^2)
 *   mse        = mean_flat((eps - noise)^2),  eps = (sqrt_recip_abar*x_t - pred_xstart) / sqrt_recipm1_abar  (:411-415,
 *                evaluated in f32 in exactly this order: the difference cancels heavily at small t)
 * coef: f32 [B][16], the rows of the reverse step.  mean_out / var_out: row b starts model_ld floats after row b-1
 * (model_ld = per_sample when contiguous, 2*per_sample for the halves of a [B, 2C, H, W] output read in place);
 * x0, x_t, noise are [B, per_sample] contiguous.  mean_mode / var_mode as above.  The three scalars of row b go to
 * out[(b % group)*out_ld + b / group] of each output: with B = K*group rows (K timesteps of `group` samples stacked)
 * one launch fills K adjacent columns of [group, T] row-major outputs whose column 0 the pointers name; group = B,
 * out_ld = 1 gives plain [B] vectors.  Sums run in a fixed order (no atomics): bitwise reproducible, and a row's
 * result does not depend on B.  16-byte loads when per_sample % 4 == 0, model_ld % 4 == 0 and every tensor is 16-byte
 * aligned, scalar loads otherwise. */
int vaw_bpd_terms(const float* mean_out, const float* var_out, int64_t model_ld, const float* x0, const float* x_t,
                  const float* noise, const float* coef, int mean_mode, int var_mode, int clip_denoised, float* vb,
                  float* xstart_mse, float* mse, int64_t out_ld, int group, int B, int64_t per_sample, vaw_stream stream);

/* _prior_bpd :932-948 = q_mean_variance :217-232 at t = T-1 + normal_kl (tools/losses.py:12-39) against N(0, I) +
 * mean_flat / ln 2:  prior_bpd[b] = mean_flat(0.5*(-1 - lv + exp(lv) + (a*x0)^2)) / ln 2  with the two table scalars
 * a = float(sqrt_alphas_cumprod[T-1]), lv = float(log_one_minus_alphas_cumprod[T-1]). */
int vaw_prior_bpd(const float* x0, float sqrt_abar_last, float log_one_minus_abar_last, float* prior_bpd, int B,
                  int64_t per_sample, vaw_stream stream);

/* The one reverse-process step of the sampling side, fused: classifier-free guidance (tools/sampler.py), p_mean_variance
 * (gaussian_diffusion.py:278-384, no denoised_fn / cond_fn) and the update of the sampler:
 *   kind 0  none: only pred_xstart / mean / log_variance are filled
 *   kind 1  p_sample :461-505        kind 2  ddim_sample :603-651 (eta)
 *   kind 3  ddim_reverse_sample :653-689 (eta = 0, the DDIM ODE run from data towards noise):
 *           eps = (sqrt_recip_abar*x - pred_xstart) / sqrt_recipm1_abar,  sample = pred_xstart*sqrt(abar_next) + sqrt(1 - abar_next)*eps;
 *           takes no noise and no variance (noise and var_* NULL, var_mode 0) and writes sample and pred_xstart (mean and
 *           log_variance NULL)
 * coef: f32 [B][16] per-sample rows of the per-timestep table (column layout in csrc/elementwise.hip above SS_NCOEF; built by
 * vaw_amd.GaussianDiffusion._sample_table with the reference's f64 -> f32 casts; columns 0-1 encode the mean type).
 * noise: the randn_like(x) draw of the step (caller's RNG; kinds 1 and 2).  Outputs may be NULL.  The guided model call
 * evaluates the batch stacked on itself (IntervalCFG.forward :41-48), so its [2N, 2C, H, W] output holds four quarters:
 * conditional / unconditional half of the batch, mean / variance channels.  They are read in place: row b of each of
 * mean_cond, mean_uncond, var_cond, var_uncond starts model_ld floats after row b-1 (model_ld >= per_sample).  Per element
 *   m = mean_uncond + guidance_scale * (mean_cond - mean_uncond),   v likewise from the variance quarters
 * in f32 with the difference, the product and the sum each rounded on its own (no fused multiply-add), i.e. bitwise the
 * three tensor operations of :48, which guide every output channel.  Then the per-element step above.
 * mean_uncond == NULL: no guidance, the plain step reading the split halves of a [N, 2C, H, W] output in place
 * (guidance_scale and var_uncond are ignored).  var_cond may be NULL with var_mode 0; var_uncond is needed only when both
 * guided and var_mode != 0.  x, noise and the outputs are [B, per_sample] contiguous.  16-byte loads and stores when
 * per_sample % 4 == 0, model_ld % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise: one loop body at either
 * width, the same bits. */
int vaw_guided_sample_step(int kind, const float* mean_cond, const float* mean_uncond, const float* var_cond,
                           const float* var_uncond, int64_t model_ld, float guidance_scale, const float* x, const float* noise,
                           const float* coef, int mean_mode, int var_mode, int clip_denoised, float eta, float* sample,
                           float* pred_xstart, float* mean, float* log_variance, int B, int64_t per_sample, vaw_stream stream);

/* The combination alone (guided EDM / flow samplers, whose update stays outside):
 *   out[b,:] = uncond[b,:] + guidance_scale * (cond[b,:] - uncond[b,:])     with the rounding rule above.
 * cond / uncond rows are model_ld floats apart, out is [B, per_sample] contiguous. */
int vaw_cfg_combine(const float* cond, const float* uncond, int64_t model_ld, float guidance_scale, float* out, int B,
                    int64_t per_sample, vaw_stream stream);

/* _inverse_normalize :257-258:  ((x + 1) * 127.5).clamp(0, 255).to(uint8).permute(0, 2, 3, 1) in one pass.
 * src: [B, C, H, W] contiguous, f32 (src_f64 = 0) or f64 (src_f64 = 1: EDM samples are finished in float64 as the
 * reference does); dst: [B, H, W, C] contiguous bytes, any alignment.  v = (x + 1) * 127.5 is formed in the source precision,
 * sum and product rounded separately, clamped to [0, 255] and truncated toward zero: for finite x bitwise the expression
 * above.  NaN writes 0.  Any C >= 1.  Destination words that lie wholly inside dst are written as 32-bit words, the ragged
 * first / last bytes singly; nothing outside [dst, dst + B*H*W*C) is touched. */
int vaw_finish_images(const void* src, int src_f64, uint8_t* dst, int B, int C, int H, int W, vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Solver steps of the EDM and flow-matching samplers  (tools/cfg_edm.py: ablation_sampler; tools/gaussian_diffusion.py:
 * sde_sample / ode_sample).  Everything of a step that does not depend on x comes from a device table built once per grid
 * (samplers.py) and is read by row index: nothing is uploaded per step.  Every operation is rounded on its own in the order
 * of the tensor composition (no fused multiply-add, IEEE division and square root).  The model output is read in place:
 * cond / uncond are the rows [:N] / [N:] of the stacked guided output (uncond == NULL: no guidance), row b starting
 * model_ld floats after row b-1, so the [:, :C] slice of a learn_sigma output needs no copy; the guidance combination is
 * that of vaw_cfg_combine.  All other tensors are [B, per_sample] contiguous.  16-byte loads and stores when
 * per_sample % 4 == 0, model_ld % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise.
 * ------------------------------------------------------------------------- */

/* Doubles per row of the EDM table, one row per solver step:
 *   0 s(t_hat)/s(t_cur)   1 noise coefficient   2..9 evaluation at t_hat   10 h = t_next - t_hat   11 alpha*h
 *   12 1 - 1/(2 alpha)   13 1/(2 alpha)   14..21 evaluation at t_mid = t_hat + alpha*h   22, 23 unused
 * evaluation block: +0 s(t)  +1 sigma(t) as float32  +2 c_in  +3 c_in^2  +4 sigma*c_in  (the float32 scalars of the
 * denoiser's preconditioning, stored widened)  +5 dsg/sg + ds/s  +6 dsg*s/sg  +7 chain index handed to the network. */
#define VAW_EDM_COLS 24
/* Floats per row of the flow table, one row per network evaluation at time t:
 *   0 a  1 s  2 a'  3 s'  4 g2 = 2 s s'  5 g2/2  6 s^2  7 a^2 + s^2  8 s a' - a s'  9 sqrt(g2)
 *   of the step that starts at t:  10 dt  11 sqrt(|dt|)  12 dt/2  13 t   14, 15 unused */
#define VAW_FLOW_COLS 16

/* Start of an EDM step:  x_hat = coef[0]*x (+ coef[1]*noise when noise != NULL), float64, and the float32 network input
 * c_in * float(x_hat / s(t_hat)) written to model_in and, when model_in_dup != NULL, to the second half of the stacked
 * guided input as well.  coef: [rows][VAW_EDM_COLS] float64, row < rows. */
int vaw_edm_input(const double* x, const double* noise, const double* coef, int row, int rows, double* x_hat, float* model_in,
                  float* model_in_dup, int B, int64_t per_sample, vaw_stream stream);

/* After a network evaluation of an EDM step.  denoised (float32, as the denoiser forms it) from the network output o and
 * x32 = float(x / s):  pred_type 0 EPSILON x32 - sigma*o,  1 START_X o,  2 VELOCITY c_in^2*x32 - (sigma*c_in)*o;  then in
 * float64 d = k1*x - k2*denoised.
 *   kind 0 Euler:         x_out = x_hat + h*d
 *   kind 1 Heun predict:  d_cur = d (written), x_mid = x_hat + (alpha h)*d, network input of x_mid at t_mid -> model_in(_dup)
 *   kind 2 Heun correct:  d_cur read, x_mid recomputed, d' at (x_mid, t_mid) from the second output,
 *                         x_out = x_hat + h*(w1*d_cur + w2*d') */
int vaw_edm_step(int kind, int pred_type, const float* cond, const float* uncond, int64_t model_ld, float guidance_scale,
                 const double* x_hat, double* d_cur, const double* coef, int row, int rows, double* x_out, float* model_in,
                 float* model_in_dup, int B, int64_t per_sample, vaw_stream stream);

/* One step of the flow samplers after a network evaluation, float32.  Velocity and score of the output under mean_type
 * 0 START_X, 1 EPSILON, 2 VELOCITY, 3 VECTOR (convert_model_output_to_vector / _to_score), drift f = v - (g2/2)*score for the
 * SDE (sde = 1) and f = v for the ODE; row0 is the evaluation the step starts at, row1 the one at its end.
 *   kind 0 Euler:         x_out = (x + f0*dt) + kick,  kick = (sqrt(g2)*noise)*sqrt|dt|  (noise == NULL: no kick -- the ODE and
 *                         the SDE's last step)
 *   kind 1 Heun predict:  the same, with f0 and kick written for the correction
 *   kind 2 Heun correct:  f1 from the second output at x_pred;  SDE x_out = (x + (0.5*(f0 + f1))*dt) + kick,
 *                         ODE x_out = x + (dt/2)*(f0 + f1)
 * x_out_dup != NULL: x_out is written there too (second half of the stacked guided input). */
int vaw_flow_step(int kind, int sde, int mean_type, const float* cond, const float* uncond, int64_t model_ld,
                  float guidance_scale, const float* x, const float* noise, const float* x_pred, float* f0, float* kick,
                  const float* coef, int row0, int row1, int rows, float* x_out, float* x_out_dup, int B, int64_t per_sample,
                  vaw_stream stream);

/* Linear multistep samplers in the data-prediction form (dpm_sample: DPM-Solver++ 2M, its SDE variant, exponential
 * Adams-Bashforth up to order 3; sigma(t) = t, s = 1).  One network evaluation per step; the update is
 *   x' = a*x + b0*D0 + b1*D1 + b2*D2 + c*noise
 * with D0 the denoised image of this evaluation and D1, D2 those of the two steps before (kept as float32: they are float32
 * values).  Doubles per row of the table, one row per step:
 *   0 a   1 b0   2 b1   3 b2   4 c   (float64 coefficients of the update)
 *   5 sigma as float32   6 c_in   7 c_in^2   8 sigma*c_in   (the float32 scalars of the denoiser's preconditioning at this
 *   evaluation, stored widened)   9 c_in of the next evaluation   10, 11 unused */
#define VAW_DPM_COLS 12

/* The network input of the first evaluation:  model_in (and model_in_dup, the second half of the stacked guided input)
 * = c_in * float(x), c_in = coef[row][6] as float32.  coef: [rows][VAW_DPM_COLS] float64, row < rows. */
int vaw_dpm_input(const double* x, const double* coef, int row, int rows, float* model_in, float* model_in_dup, int B,
                  int64_t per_sample, vaw_stream stream);

/* After the network evaluation of step `row`.  o = the (guided) network output, x32 = float(x);  denoised (float32, as the
 * denoiser forms it): pred_type 0 EPSILON x32 - sigma*o,  1 START_X o,  2 VELOCITY c_in^2*x32 - (sigma*c_in)*o;  clamped to
 * [-1, 1] when clip != 0 (NaN stays NaN);  written to d0_out.  Then in float64, every operation rounded on its own,
 *   acc = a*x + b0*double(D0);  d1 != NULL: acc = acc + b1*double(d1);  d2 != NULL (needs d1): acc = acc + b2*double(d2);
 *   noise != NULL: acc = acc + c*noise;   x_out = acc   (x_out may be x: a lane reads its elements before it writes them)
 * and, when model_in != NULL, the next network input coef[row][9] (as float32) * float(x_out) into model_in and, when
 * model_in_dup != NULL, there as well.  The last step (a = 0, b0 = 1) passes no model_in. */
int vaw_dpm_step(int pred_type, int clip, const float* cond, const float* uncond, int64_t model_ld, float guidance_scale,
                 const double* x, const float* d1, const float* d2, const double* noise, const double* coef, int row, int rows,
                 double* x_out, float* d0_out, float* model_in, float* model_in_dup, int B, int64_t per_sample,
                 vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Per-sample seeded noise for the samplers  (the role of StackedRandomGenerator in EDM's generate.py: one stream per sample
 * seed).  Counter-based, so row b of a draw is a pure function of (seeds[b], draw, tag, element) and of nothing else: not of
 * B, of the other rows, of the grid, of the stream, or of what was drawn before.
 * ------------------------------------------------------------------------- */
#define VAW_NOISE_BITS 0     /* the raw 32-bit words */
#define VAW_NOISE_UNIFORM 1  /* float32 u = fmaf((float)r, 2^-32, 2^-33): in (0, 1], the float32 of r then one rounding */
#define VAW_NOISE_NORMAL 2   /* Box-Muller in float32 (logf, sincospif, IEEE sqrt and products; no fast forms):
                              * (r0, r1) -> sqrt(-2 log u0) * (cos, sin)(2 pi u1), (r2, r3) -> the other two */
#define VAW_NOISE_TAG_NOISE 0
#define VAW_NOISE_TAG_LABELS 1

/* out: [B, per_sample] contiguous; seeds: device int64 [B].  Elements 4c .. 4c+3 of row b are the four words of
 * Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) under the key
 * (low 32 bits, high 32 bits) of seeds[b] read as an unsigned 64-bit pattern, at the counter (c, draw, tag, 0).  So a row of 5
 * elements is the first 5 of a row of 8.  dtype: VAW_F32 for modes 0 and 1 (any 4-byte element); VAW_F32, VAW_BF16 (the
 * round-to-nearest-even of the float32 value) or VAW_F64 (its exact widening) for mode 2.  One lane makes one block and stores
 * it whole (16 bytes; 8 for bf16; two 16-byte halves for float64) where the row starts on such a boundary and the block lies
 * inside the row, element by element otherwise; nothing outside out[0 .. B*per_sample) is written.  No atomics and no device
 * state: `draw` is a kernel argument, so a captured launch replays the same draw number on whatever seeds are in memory then.
 * Refused before any launch (VAW_ERR_INVALID): a null pointer, B < 1, per_sample < 1, per_sample >= 2^34 (the block counter is
 * 32 bits), draw outside [0, 2^32), tag < 0, an unknown mode or dtype, mode 0 / 1 with a dtype that is not 4 bytes wide, a
 * pointer not aligned to its element. */
int vaw_randn_seeded(void* out, int dtype, const int64_t* seeds, int B, int64_t per_sample, int64_t draw, int tag, int mode,
                     vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Adaptive explicit Runge-Kutta steps of the flow ODE  (flow_ode_sample(solver="rk45"): Dormand-Prince 5(4), the step
 * controller on the host).  Same conventions as the solver steps above: float32, every operation rounded on its own, the
 * model output read in place, 16-byte accesses when per_sample % 4 == 0, model_ld % 4 == 0 and every pointer is aligned.
 * Sums leave the device as float64: one partial per workgroup (vaw_rk_partial_count of them, a function of the sizes alone)
 * summed in a fixed order, then vaw_rk_sumsq_finish; bitwise reproducible from run to run, no atomics.
 * ------------------------------------------------------------------------- */
#define VAW_RK_STAGES 7       /* network evaluations of a step (the last one is the first of the next: FSAL), slots of k */
#define VAW_RK_MAX_GRID_X 64  /* workgroups along a sample */
int64_t vaw_rk_partial_count(int B, int64_t per_sample);

/* The pass after the network evaluation of stage `stage` (0..6) of a step from x with signed step h:
 *   cond != NULL:  k[slots_host[stage]] = v(output, x_stage) under mean_type (the ODE branch of vaw_flow_step, interpolant from
 *                  coef[row], a [rows][VAW_FLOW_COLS] table at the stage times); x_stage == NULL: the stage state is x.
 *   cond == NULL:  k[slots_host[stage]] is there already (a rejected step tried again with another h, or k1 <- k7 after an
 *                  accepted one: the host swaps slots_host[0] and slots_host[6], nothing is copied).
 *   dy = sum_{s < ncoef} a_host[s] * k[slots_host[s]]   ascending, zero coefficients skipped, left to right
 *   x_out != NULL:     x_out (and x_out_dup) = x + h*dy, the next stage's state, written straight into the network input
 *                      (x_out may be x_stage: every element is read before it is written)
 *   partials != NULL:  partial sums of ((h*dy) / (atol + rtol*max(|x|, |x_new|)))^2, a_host = the error weights
 *   ncoef == 0:        k only.
 * k: [VAW_RK_STAGES][B*per_sample] float32; slots_host: VAW_RK_STAGES host ints in 0..6.  One coefficient vector per call, so
 * the Euler trial of the first-step selection (a_host = {1}) and any other explicit tableau are the same kernel. */
int vaw_rk_stage(int stage, int mean_type, const float* cond, const float* uncond, int64_t model_ld, float guidance_scale,
                 const float* x, const float* x_stage, const float* coef, int row, int rows, float* k, const int* slots_host,
                 const float* a_host, int ncoef, float h, float* x_out, float* x_out_dup, const float* x_new, float atol,
                 float rtol, double* partials, int64_t partials_cap, int B, int64_t per_sample, vaw_stream stream);

/* partials[workgroup] of  sum ((u - v) / (atol + rtol*max(|a|, |b|)))^2  over [B, per_sample] float32 tensors; v == NULL:
 * u alone, b == NULL: |a| alone.  The quotient is float32 (IEEE division), its square and the sums float64. */
int vaw_rk_scaled_sumsq(const float* u, const float* v, const float* a, const float* b, float atol, float rtol,
                        double* partials, int64_t partials_cap, int B, int64_t per_sample, vaw_stream stream);

/* out[0] = the `count` partial sums folded by one workgroup in a fixed order. */
int vaw_rk_sumsq_finish(const double* partials, int64_t count, double* out, vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Log-likelihood of a flow model  (samplers.py: flow_log_likelihood).  With t = 0 data, t = 1 noise and dx/dt = v(x, t):
 *   log p0(x0) = log N(x(1); 0, I) + int_0^1 div v(x(t), t) dt,   div v estimated with fixed Hutchinson probes eps:
 *   g = (d out / d x)^T eps is one vector-Jacobian product of the network, tr ~ sum eps * g.
 * Conventions of the adaptive stages above: float32 state with every operation rounded on its own, the model output read in
 * place by row stride (the first C of a learn_sigma model's 2C channels need no copy), 16-byte accesses when
 * per_sample % 4 == 0, model_ld % 4 == 0 and every pointer is 16-byte aligned, scalar ones with a bound check otherwise.
 * The divergence is float64: products and sums in an order fixed by per_sample alone (no atomics), so a row's bits depend
 * neither on the batch, nor on the alignment, nor on the run.  A row longer than one workgroup's stream (1024 elements)
 * leaves one partial per workgroup, vaw_rk_partial_count(B, per_sample) in all, that a second launch folds left to right.
 * ------------------------------------------------------------------------- */

/* Floats per row of the log-likelihood table, one row per network evaluation at time t:  0 A  1 B  2 t  3 unused,
 * with v = A*x + B*out: convert_model_output_to_vector collapsed per mean type (host float64, stored as float32)
 *   START_X   A = s'/s             B = a' - a s'/s          EPSILON  A = a'/a   B = s' - s a'/a
 *   VELOCITY  A = (a a' + s s')/(a^2 + s^2)   B = (a s' - s a')/(a^2 + s^2)      VECTOR   A = 0   B = 1 */
#define VAW_FLOW_LOGP_COLS 4

/* The pass after the network evaluation and the vector-Jacobian product of stage `stage` (0..VAW_RK_STAGES-1) of an explicit
 * Runge-Kutta step from x with signed step h:
 *   k[stage]    = A*x_stage + B*out            (coef[row]; x_stage == NULL: the stage state is x), float32
 *   d[stage][b] = A*n + B * sum_i eps[b,i]*g[b,i]     float64, n = per_sample
 *   ncoef > 0:  x_out = x + float(h) * sum_{s < ncoef} float(a_host[s]) * k[s]   ascending, zero coefficients skipped, left to
 *               right: the next stage's state, written straight into the next network input -- or, on the last stage, x_new
 *   delta != NULL (last stage, a_host = the step's weights):  delta[b] += h * sum_{s < ncoef} a_host[s] * d[s][b]   float64, same order
 * k: [VAW_RK_STAGES][B*per_sample] float32; d: [VAW_RK_STAGES][B] float64; a_host: ncoef host doubles; x_out must not overlap an input.
 * partials: vaw_rk_partial_count(B, per_sample) doubles, needed (and touched) only when per_sample > 1024. */
int vaw_flow_logp_stage(int stage, const float* out, int64_t model_ld, const float* g, const float* eps, const float* x,
                        const float* x_stage, const float* coef, int row, int rows, float* k, double* d, const double* a_host, int ncoef,
                        double h, float* x_out, double* delta, double* partials, int64_t partials_cap, int B, int64_t per_sample,
                        vaw_stream stream);

/* logp[b] = -1/2 sum_i z[b,i]^2 - (per_sample/2) ln 2 pi, float64, summed as above. */
int vaw_flow_logp_prior(const float* z, double* logp, double* partials, int64_t partials_cap, int B, int64_t per_sample,
                        vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Loss-aware timestep sampling on the device  (tools/resample.py: LossSecondMomentResampler)
 * ------------------------------------------------------------------------- */

/* Most timesteps vaw_resampler_draw takes: its one workgroup keeps p and the CDF in LDS, 16 bytes per timestep. */
#define VAW_RESAMPLER_MAX_T 4096

/* update_with_all_losses :127-141 as the ring the package keeps: for i = 0 .. n-1 IN ORDER
 *   ring[ts[i]][seen[ts[i]] % H] = (double)losses[i];  seen[ts[i]] += 1
 * ring: f64 [T][H], seen: i64 [T].  One thread owns one timestep and walks the batch in order (no atomics), so entries of one
 * call with the same t land in consecutive slots in batch order (wrapping inside a call included) and the result is bitwise
 * reproducible whatever the launch shape.  An entry with t outside [0, T) is skipped and counted: bad[0] += 1. */
int vaw_resampler_update(const int64_t* ts, const float* losses, int n, int T, int H, double* ring, int64_t* seen, int* bad,
                         vaw_stream stream);
/* vaw_resampler_update for a run behind the step guard: a pair whose loss is inf or NaN is not recorded either; it is counted in
 * bad[0] like a pair with t outside [0, T). */
int vaw_resampler_update_finite(const int64_t* ts, const float* losses, int n, int T, int H, double* ring, int64_t* seen, int* bad,
                                vaw_stream stream);

/* weights() :116-125 + ScheduleSampler.sample :38-50 with the uniforms supplied (np.random.choice(p=...) is a right-sided
 * search of the normalised running sum of p):
 *   warm = all(seen >= H);   not warm: p[t] = 1 / T;
 *   warm: w[t] = sqrt(mean_j ring[t][j]^2),  p[t] = w[t] / sum(w) * (1 - uniform_prob) + uniform_prob / T;
 *   c = cumsum(p), c /= c[T-1];   out_t[b] = #{t : c[t] <= u[b]} (clamped to T-1);   out_w[b] = (float)(1 / (T * p[out_t[b]])).
 * All arithmetic is IEEE f64, one rounding per operation (no contraction), in these fixed orders: the mean of squares adds
 * j = 0 .. H-1 ascending into one accumulator, then divides by H; sum(w) forms 64 partial sums, partial l = w[l] + w[l+64] +
 * w[l+128] + ... ascending, then adds the partials l = 0 .. 63 ascending; c is summed strictly left to right.
 * u: f64 [B] uniforms of [0, 1); out_t: i64 [B]; out_w: f32 [B]; p: f64 [T], always written.  One workgroup:
 * T > VAW_RESAMPLER_MAX_T is refused with VAW_ERR_INVALID. */
int vaw_resampler_draw(const double* ring, const int64_t* seen, int T, int H, double uniform_prob, const double* u, int B,
                       int64_t* out_t, float* out_w, double* p, vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Evaluation metrics from activations  (evaluations/evaluator.py: ManifoldEstimator, DistanceBlock, Evaluator.compute_statistics,
 * Evaluator.compute_inception_score)
 * ------------------------------------------------------------------------- */

/* out[i] = sum_k X[i][k]^2 in f32, X: f32 [n][D] row-major, any D >= 1 (rows need no alignment).  Fixed order: 64 partial sums,
 * partial l = x[l]^2 + x[l+64]^2 + ... ascending, folded by the xor butterfly 32, 16, .. 1. */
int vaw_row_sqnorms(const float* X, int64_t n, int D, float* out, vaw_stream stream);

/* _batch_pairwise_distances :415-431 in f32 (the reference casts to fp16 first: a documented difference), never materialised:
 *   d(i, j) = max((norm_u[i] - 2 * dot(U_i, V_j)) + norm_v[j], 0)
 * U: f32 [nu][D], V: f32 [nv][D], norm_*: f32 row square norms (vaw_row_sqnorms).  dot is an f32 MFMA chain over k = 0 .. D-1 in
 * order in one accumulator (K is never split), every operation outside it is rounded on its own, so d(i, j) has the same bits
 * whatever launch computes it: results are independent of how a caller cuts U and V into calls.
 *
 * out[i][0 .. k1) = the k1 smallest d(i, j) over j, ascending (manifold_radii :249-282 takes columns of it).  1 <= k1 <= 16 and
 * k1 <= nv, else VAW_ERR_INVALID.  ws: at least vaw_pairwise_workspace_bytes(nu, nv, k1) bytes (0 for sizes that are refused),
 * which is nu * k1 * 4 bytes times twice the number of column ranges (at most 16) a row tile is cut into; no nu x nv buffer
 * exists.  Partial lists are merged in a fixed order, no float atomics. */
int64_t vaw_pairwise_workspace_bytes(int64_t nu, int64_t nv, int k1);
int vaw_pairwise_ksmallest(const float* U, int64_t nu, const float* V, int64_t nv, int D, const float* norm_u, const float* norm_v,
                           int k1, float* out, void* ws, int64_t ws_bytes, vaw_stream stream);

/* out[i][0 .. k1) = the k1 smallest of the P * k1 values parts[i * row_stride + p * part_stride + q] (p < P, q < k1), ascending;
 * +inf marks an empty slot.  The merge step of vaw_pairwise_ksmallest, exported for callers that cut V into several calls. */
int vaw_ksmallest_merge(const float* parts, int64_t n, int P, int k1, int64_t part_stride, int64_t row_stride, float* out,
                        vaw_stream stream);

/* DistanceBlock.less_thans :403-412 for whole arrays, ORed into the flags (evaluate_pr :346-356 ORs its blocks the same way):
 *   u_in[i][c] |= any_j d(i, j) <= radii_v[j][c]     u_in: uint8 [nu][Kv]
 *   v_in[j][c] |= any_i d(i, j) <= radii_u[i][c]     v_in: uint8 [nv][Ku]
 * radii_u: f32 [nu][Ku], radii_v: f32 [nv][Kv], 1 <= Ku, Kv <= 4.  The caller zeroes the flags before the first call; a flag
 * byte only goes from 0 to 1 (a plain store of 1 by every block that finds a pair), so the result does not depend on any order. */
int vaw_pairwise_within(const float* U, int64_t nu, const float* V, int64_t nv, int D, const float* norm_u, const float* norm_v,
                        const float* radii_u, int Ku, const float* radii_v, int Kv, uint8_t* u_in, uint8_t* v_in, vaw_stream stream);

/* Polynomial-kernel row sums on the same tile (kernel inception distance: the unbiased MMD^2 of Binkowski et al. 2018), float64:
 *   rowsum[b][i] = sum_j (gamma * dot(U[u_idx[b][i]], V[v_idx[b][j]]) + coef0)^degree      b < batches, i < nu, j < nv
 * u_idx: int32 [batches][nu], v_idx: int32 [batches][nv], rows of U and V; null = the rows 0 .. nu-1 / 0 .. nv-1 themselves in every
 * batch.  No gathered copy is made.  The caller guarantees that every index is a row of its matrix (vaw_amd.ops checks on the host).
 * skip_diagonal != 0 leaves out the pairs with u_idx[b][i] == v_idx[b][j] (i == j without tables): the i != j sums of the unbiased
 * estimator without a subtraction.  dot is the f32 MFMA chain of the distances, widened to double; t = gamma * dot + coef0, the power
 * t * t * .. * t multiplied left to right, degree in 1 .. 8, gamma and coef0 finite.
 * Summation order, fixed by (nu, nv) alone, no atomics: the columns are cut into S <= 16 ranges of 128-column tiles; within a range
 * a row's columns with (j mod 64) < 32 go to one float64 partial and the others to a second, each in ascending j; the 2 S partials
 * of a row are added in ascending order.  A second launch gives the same bits, and so does a batch launched alone.
 * ws: at least vaw_pairwise_polysum_workspace_bytes(nu, nv, batches) = batches * nu * 2 S * 8 bytes (0 for sizes that are refused). */
int64_t vaw_pairwise_polysum_workspace_bytes(int64_t nu, int64_t nv, int batches);
int vaw_pairwise_polysum(const float* U, int64_t nu, const float* V, int64_t nv, int D, const int32_t* u_idx, const int32_t* v_idx, int batches,
                         double gamma, double coef0, int degree, int skip_diagonal, double* rowsum, void* ws, int64_t ws_bytes,
                         vaw_stream stream);

/* Density and coverage (Naeem et al. 2020) in one pass over d(i, j) of vaw_pairwise_within, compared strictly (d < r, the published
 * definition; vaw_pairwise_within keeps the reference's d <= r):
 *   u_count[i][q] += #{ j : d(i, j) < radii_v[j][q] }        u_count: int32 [nu][Kv]
 *   v_in[j][q]     = 1 if any i has d(i, j) < radii_v[j][q]   v_in: uint8 [nv][Kv]
 * radii_v: f32 [nv][Kv], 1 <= Kv <= 4.  The caller zeroes both outputs before the first call and may cut U and V into calls in any
 * way: counts are integers and a flag byte only goes from 0 to 1.  ws: at least vaw_pairwise_count_workspace_bytes(nu, nv, Kv)
 * = nu * 2 S * Kv * 4 bytes of per-range counts, which a second kernel adds into u_count. */
int64_t vaw_pairwise_count_workspace_bytes(int64_t nu, int64_t nv, int Kv);
int vaw_pairwise_count_within(const float* U, int64_t nu, const float* V, int64_t nv, int D, const float* norm_u, const float* norm_v,
                              const float* radii_v, int Kv, int32_t* u_count, uint8_t* v_in, void* ws, int64_t ws_bytes, vaw_stream stream);

/* np.mean(X, axis=0) and np.cov(X, rowvar=False) of Evaluator.compute_statistics :175-178 in f64 from f32 X [n][D] (widened
 * exactly).  mu[c] = (sum_i X[i][c]) / n: 16 partial sums per column, partial p = rows p, p+16, ... ascending, added p ascending.
 * sigma[a][b] = (sum_i (X[i][a] - mu[a]) * (X[i][b] - mu[b])) / (n - 1): two-pass and centred, one f64 fma chain over
 * i = 0 .. n-1 ascending per element (f64 vector FMA), computed for a <= b and stored at both places: sigma [D][D] is written
 * fully and is symmetric bit for bit.  n = 1 gives 0 / 0 = NaN as numpy does. */
int vaw_col_mean_f64(const float* X, int64_t n, int D, double* mu, vaw_stream stream);
int vaw_cov_f64(const float* X, int64_t n, int D, const double* mu, double* sigma, vaw_stream stream);

/* Inception score from pool activations (Evaluator.compute_inception_score :180-193 behind _create_softmax_graph: a matrix product
 * without bias, a row softmax, exp(mean_i sum_c p (ln p - ln mean_i p)) per split of rows).
 *
 * vaw_head_logits: logits[i][c] = sum_k X[i][k] * Wt[c][k].  X: f32 [n][D], Wt: f32 [C][D] (the class-major copy of the [D][C]
 * weight), logits: f32, rows ld >= C floats apart.  Any D, C >= 1, rows need no alignment.  One block per 128 x 128 output tile on
 * the pairwise tile: every element is one k-ordered f32 MFMA chain in one accumulator, K is never split, so a logit has the same
 * bits whatever tile or launch made it.  Rows >= n and columns >= C are not stored.
 *
 * vaw_is_rows: per row of `in` (f32 [n][C], rows ld apart), one wave, float64, every sum 64 lane-strided partials in ascending c
 * folded by the xor butterfly.  probs = 0, a row of logits l:  lse = m + log sum_c exp(l_c - m) with m = max_c l_c, and
 * h = sum_c p_c (l_c - lse) with p_c = exp(l_c - lse).  probs = 1, a row of probabilities p:  h = sum_c p_c log p_c, lse = 0.
 *
 * vaw_is_colsums: colsum[s][c] = sum over the rows i of split s of p_ic (p as above; lse from vaw_is_rows, unused when probs) in
 * float64, one chain in ascending i per (s, c), no atomics.  The n rows of the call are the global rows row0 .. row0 + n; split s
 * holds the global rows s * split_size .. (s + 1) * split_size.  colsum: f64 [number of splits][C], the whole array.  A split whose
 * first row lies in this call starts from 0, any other continues from the value in memory: calls must come in ascending row0 and
 * cover every row once, and the result does not depend on where they cut.
 *
 * vaw_is_finish: scores[s] = exp(H - sum_c m_c log m_c), H = (sum_i h_i) / n_s over the n_s rows of split s (the last one ragged),
 * m_c = colsum[s][c] / n_s; h: f64 [N].  This is mean_i sum_c p (ln p - ln m) with the inner sum split.
 *
 * Wherever p = 0 or m_c = 0 the term is its limit 0 (numpy gives 0 * -inf = NaN there). */
int vaw_head_logits(const float* X, int64_t n, int D, const float* Wt, int C, float* logits, int64_t ld, vaw_stream stream);
int vaw_is_rows(const float* in, int64_t n, int C, int64_t ld, int probs, double* lse, double* h, vaw_stream stream);
int vaw_is_colsums(const float* in, const double* lse, int64_t n, int C, int64_t ld, int probs, int64_t row0, int64_t split_size, double* colsum,
                   vaw_stream stream);
int vaw_is_finish(const double* h, const double* colsum, int64_t N, int C, int64_t split_size, double* scores, vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Dense layers  (nn.Linear / Conv2d(k=p,s=p) / Conv1d(k=1) in models/dit.py, models/unet.py;
 * cuBLAS in the reference).  One GEMM entry point, MFMA inside.
 * ------------------------------------------------------------------------- */

typedef struct {
    const float* bias;     /* f32[N] added to every row, or NULL */
    int act;               /* 0 none | 1 GELU(tanh) forward | 2 multiply by GELU'(aux_in) (backward) */
    const void* aux_in;    /* act dtype [M,N] (ld = ldc): pre-activation for act==2 */
    void* aux_out;         /* act dtype [M,N] (ld = ldc): value BEFORE act/gate/residual is stored here, or NULL */
    const float* gate;     /* f32: gate[(m / rows_per_batch) * gate_ld + n], or NULL */
    int64_t gate_ld;
    const void* resid;     /* [M,N] (ld = ldc) residual added AFTER the gate, or NULL; f32 unless resid_is_act */
    const float* rowadd;   /* f32 [rows_per_batch, N] added by (m % rows_per_batch): frozen pos_embed, or NULL */
    int rows_per_batch;    /* tokens per sample (T); required when gate/rowadd is set */
    float alpha;           /* scales the accumulator first */
    float beta;            /* C = beta*C_old + value (f32 output only; 0 = overwrite, C_old not read) */
    int out_f32;           /* 1: C is f32 regardless of act dtype; 0: C has act dtype */
    float* colsum_out;     /* f32[N] or NULL: colsum_out = colsum_beta*colsum_out + sum_m C[m,:] (values as stored),
                            * i.e. the bias gradient of the layer whose output gradient this GEMM produces; taken in
                            * the epilogue (no second pass over C); needs the workspace */
    float colsum_beta;
    int resid_is_act;      /* 1: resid has the act dtype (UNet skip connections), 0: f32 (DiT residual stream) */
    float* rowsum_a_out;   /* f32[M] or NULL: rowsum_a_out = rowsum_a_beta*rowsum_a_out + sum_k op(A)[m,k].  For the weight
                            * gradient dW = dy^T x (a_kmajor = 0) this is the layer's BIAS gradient sum_rows dy, taken from
                            * the dy tiles the MFMA kernel stages anyway (one extra MFMA against a ones operand, fixed
                            * order); other layouts / the generic kernel honour it with a separate pass.  Needs the workspace */
    float rowsum_a_beta;
    float* colsum_partial_out;  /* deferred form of colsum_out (which must then be NULL): the kernel leaves its per-row-tile partial
                                 * column sums of C, [*colsum_rows_out][N] f32 (at most ceil(M/64) rows: size the buffer for that),
                                 * here and does NOT fold them; the caller folds many such buffers in one launch
                                 * (vaw_reduce_rows_batched).  No workspace needed for it */
    int64_t* colsum_rows_out;   /* HOST address, in / out (required with the above): on entry the capacity of colsum_partial_out in
                                 * rows (a launch that needs more fails with VAW_ERR_INVALID before anything runs), on return
                                 * the number of partial rows written */
} vaw_epilogue;

/* C[M,N] = epilogue( alpha * op(A)[M,K] . op(B)[K,N] )
 *   a_kmajor=1: A stored [M][K] (lda = row stride);  0: stored [K][M]
 *   b_kmajor=1: B stored [N][K] (ldb = row stride);  0: stored [K][N]
 * forward  y = x W^T + b : (1,1)   dgrad dx = dy W : (1,0)   wgrad dW = dy^T x : (0,0)
 * A and B are act dtype.  value = acc*alpha + bias -> [aux_out] -> act -> *gate -> +resid -> +rowadd.
 * workspace (f32, may be NULL): lets launches with a plain f32 epilogue (weight gradients: K = B*T, few output
 * tiles) run split-K -- partial slabs [split][M][N] summed in a fixed order by a second kernel, so results do
 * not depend on scheduling.  A workspace of 8*M*N floats is always enough; smaller ones lower the split. */
int vaw_gemm(vaw_dtype dt, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
             const void* B, int64_t ldb, void* C, int64_t ldc, const vaw_epilogue* epi_host, float* workspace,
             int64_t workspace_floats, vaw_stream stream);

/* Weight gradients of many Linear layers in ONE launch: dW_p[M_p,N_p] = beta*dW_p + dy_p[K,M_p]^T . x_p[K,N_p] for
 * p = 0..n_problems-1, all sharing K (= tokens of the batch).  Replaces the per-layer `dy^T x` GEMMs that autograd
 * issues in the reference (models/dit.py:118-155 backward of qkv / proj / fc1 / fc2), deferred to the end of backward:
 * with K = B*T long and M_p*N_p small, a per-layer launch must split K over the chip and move every tile through an
 * f32 slab; all layers together give enough whole tiles for every CU, and only the tiles of the last, partial round are
 * K-split (folded in a fixed order: results do not depend on scheduling).
 * problems: HOST array; desc_dev: device scratch of vaw_wgrad_grouped_desc_bytes(n) bytes that holds the device copy
 * of the table -- upload != 0 (re)writes it on `stream` (pass 1 the first time and whenever a pointer changed).  An upload
 * goes through a pinned staging buffer taken from a pool and returned to it once the copy has completed, so uploading often
 * costs no pinned memory beyond what is in flight at once; the first upload of a table needs memory the pool may have to
 * allocate, which a global-mode stream capture refuses (make a group's first launch outside the capture; later launches with
 * upload == 0 capture).  The same holds for vaw_reduce_rows_batched and vaw_fp8_quantize_delayed_batched.
 * workspace: f32 slabs for the K-split tiles (256 * 256 * n_CUs floats are always enough; smaller ones lower the split). */
typedef struct {
    const void* dy;        /* act dtype (bf16) [K][M], row stride ld_dy */
    const void* x;         /* act dtype (bf16) [K][N], row stride ld_x */
    float* dw;             /* f32 [M][N], row stride ld_dw */
    int64_t M, N, ld_dy, ld_x, ld_dw;
    float alpha;           /* scales dy^T x before it is added (0 = 1) */
    int pad_;
    const float* scale_dy; /* dt = VAW_FP8 / VAW_BF8 only: dy and x are the TRANSPOSED e4m3 copies dy^T [M][K] and x^T [N][K] (k-major), ld_*  */
    const float* scale_x;  /* their row strides, and these DEVICE scalars their per-tensor dequantisation scales (vaw_fp8_quantize) */
} vaw_wgrad_problem;
int64_t vaw_wgrad_grouped_desc_bytes(int n_problems);
int vaw_wgrad_grouped(vaw_dtype dt, int n_problems, const vaw_wgrad_problem* problems, int64_t K, float beta, void* desc_dev,
                      int upload, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* Engine of the bf16 launches of vaw_wgrad_grouped whose tiles are 256 columns wide (every group but the all-N-%-192 ones), process-wide:
 * -1 by shape (the default; VAW_WGRAD_ENGINE, read once on first use, sets another), 0 the 8-wave persistent kernel, 1 the 4-wave
 * kernel (one wave per SIMD, 128 x 128 wave tiles).  The two give bitwise equal results; fp8 and 192-column groups always run the
 * 8-wave kernel.  For measurement and tests. */
void vaw_debug_wgrad_engine(int mode);

/* fp8 operands (OCP e4m3fn, per-tensor scaling) for the Linear GEMMs: BASELINE.json config 5 "DiT-XL/2, fp8 MFMA GEMMs + bf16
 * accum" (model: models/dit.py:373, recipe run.sh:20-26; the reference itself trains that model in bf16 autocast).
 *
 * vaw_fp8_quantize: q[r,c] = fp8(src[r,c] * FMAX / amax|src|) (round to nearest even), qt[c,r] = q[r,c] (optional transposed
 * copy: every fp8 GEMM takes both operands k-major, so dgrad reads W^T and wgrad reads dy^T and x^T), and *scale_out =
 * amax / FMAX (1 for an all-zero tensor), a DEVICE scalar: nothing syncs with the host.  dst_format: VAW_FP8 (e4m3fn, FMAX 448:
 * weights and activations) or VAW_BF8 (e5m2, FMAX 57344: gradients).  src: f32 or bf16 [R][C], row stride ld; q: [R][C] bytes,
 * stride ldq; qt: [C][R] bytes, stride ldt.  C, ld, ldq, ldt multiples of 4.
 * workspace: vaw_fp8_quantize_workspace_floats() floats (amax partials, folded in a fixed order). */
int64_t vaw_fp8_quantize_workspace_floats(void);
int vaw_fp8_quantize(vaw_dtype src_dt, vaw_dtype dst_format, const void* src, int64_t R, int64_t C, int64_t ld, void* q, int64_t ldq,
                     void* qt, int64_t ldt, float* scale_out, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* Delayed scaling (the step after the first): one pass instead of two.  state = 4 floats {scale in use, running max |src|,
 * FMAX / margin, unused}: vaw_fp8_quantize_delayed quantises with state[0] as it stands (values beyond its range saturate) and
 * folds this tensor's max |src| into state[1] (integer atomic max on the bits: order-independent); vaw_fp8_scale_update, once
 * per step over all n states ([n][4] floats), turns every non-zero state[1] into the next scale state[0] = state[1] / state[2]
 * and clears it.  GEMMs take &state[0] as their scale pointer. */
int vaw_fp8_quantize_delayed(vaw_dtype src_dt, vaw_dtype dst_format, const void* src, int64_t R, int64_t C, int64_t ld, void* q,
                             int64_t ldq, void* qt, int64_t ldt, float* state, vaw_stream stream);
int vaw_fp8_scale_update(float* states, int64_t n, vaw_stream stream);
/* vaw_fp8_scale_update for a run behind the step guard: a running max that is not finite (an overflowed tensor of a step the guard
 * refuses) keeps the scale in use, like an all-zero one, instead of making the scale infinite; it is cleared all the same. */
int vaw_fp8_scale_update_finite(float* states, int64_t n, vaw_stream stream);
/* vaw_fp8_quantize_delayed for MANY f32 tensors in one launch (e4m3): the once-per-step re-quantisation of all Linear weights from
 * their f32 masters (the reference's autocast casts the same weights to bf16 on every use, tools/trainer.py:104-108).  jobs: host
 * array; desc_dev: device buffer of vaw_fp8_quantize_batched_desc_bytes(n_jobs) bytes, written when upload != 0 (as for
 * vaw_wgrad_grouped; the addresses are static between steps).  Bytes, transposed copies and running maxima equal the per-tensor calls'. */
typedef struct {
    const float* src;      /* f32 [R][C], row stride ld */
    void* q;               /* e4m3 bytes [R][C], row stride ldq */
    void* qt;              /* e4m3 bytes [C][R], row stride ldt, or NULL */
    float* state;          /* the tensor's delayed-scaling state (4 floats) */
    int64_t R, C, ld, ldq, ldt;
} vaw_fp8_quant_job;
int64_t vaw_fp8_quantize_batched_desc_bytes(int n_jobs);
int vaw_fp8_quantize_delayed_batched(int n_jobs, const vaw_fp8_quant_job* jobs, void* desc_dev, int upload, vaw_stream stream);
/* C[M,N] = epilogue(alpha * *scale_a * *scale_b * A[M,K] . B[N,K]^T): A bytes of a_format (VAW_FP8 | VAW_BF8), B e4m3 bytes,
 * both k-major (K % 128 == 0, row strides multiples of 16), f32 accumulation on v_mfma_scale_f32_16x16x128_f8f6f4 with unit
 * block scales; C and the epilogue operands as for vaw_gemm with dt = VAW_BF16 (bf16 C / aux, or f32 C with out_f32).
 * Epilogues offered: bias (+ colsum_out), either A format; GELU' (+ colsum_out), either; bias + aux_out + GELU and bias +
 * aux_out + gate + f32 residual, e4m3 A.  Others return VAW_ERR_UNSUPPORTED.
 * Weight gradients: vaw_wgrad_grouped with dt = VAW_FP8 (dy^T, x^T e4m3) or VAW_BF8 (dy^T e5m2, x^T e4m3).
 * c_fp8_state != NULL (GELU and GELU' epilogues only): C is written as fp8 BYTES of c_fp8_format (row stride ldc bytes) -- the bf16
 * rounding of each value, divided by the scale in c_fp8_state[0] and saturated, exactly what vaw_fp8_quantize_delayed would make
 * of the bf16 tensor -- and the tensor's max |x| is folded into c_fp8_state[1]; vaw_fp8_transpose then provides the transposed
 * copy.  For fp8 mode's fc1 output and fc2 input gradient, whose bf16 forms have no other reader. */
int vaw_gemm_fp8(vaw_dtype a_format, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const float* scale_a,
                 const void* B, int64_t ldb, const float* scale_b, void* C, int64_t ldc, const vaw_epilogue* epi_host,
                 float* c_fp8_state, vaw_dtype c_fp8_format, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* qt[c][r] = q[r][c] for fp8 bytes; R % 64 == 0, C % 128 == 0, ldq % 8 == 0, ldt % 4 == 0. */
int vaw_fp8_transpose(const void* q, int64_t R, int64_t C, int64_t ldq, void* qt, int64_t ldt, vaw_stream stream);

/* Keep n CUs out of every persistent-GEMM grid from now on (0 = none): for the time a kernel of another stream (a collective)
 * holds CUs of its own -- a persistent workgroup cannot share its CU, and a grid that does not fit runs a second pass. */
void vaw_p8_set_reserved_cus(int n);
/* 1 when these operands can go to a bf16 MFMA kernel: dt = bf16, M >= 16, N >= 16 (any M and N: edge tiles are predicated),
 * N % 8 == 0, K % 64 == 0, lda % 8 == 0, ldb % 8 == 0, A and B 16-byte aligned, and vaw_debug_force_generic_gemm off.  0: the
 * exact-f32 generic kernel.  The OPERAND half of the rule only: vaw_gemm also sends a launch to the generic kernel when C or an
 * epilogue operand is not 16-byte aligned, ldc % 8 != 0, gate_ld % 4 != 0, or A is stored [K][M] with M % 8 != 0 -- ask
 * vaw_gemm_plan for the kernel a whole call gets.  For measurement and tests. */
int vaw_gemm_uses_bf16_mfma(vaw_dtype dt, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                            int64_t ldb);

/* Launch plan of vaw_gemm: the one host function it takes every launch choice from (pure arithmetic, so it can be asked without
 * a GPU).  A / B / C are the addresses vaw_gemm would be given and the pointers of `epi_host` are used for null-ness and alignment
 * only (colsum_rows_out is read: the stated capacity); workspace_floats = 0 stands for a NULL workspace.
 * knobs: NULL = the process's own -- the environment, read once on first use (VAW_GEMM_BIG, _BK, _PD, _WS, _XCDSPLIT, _EPI, _DEBUG,
 * VAW_SM_MAX_M, _WIDE_M, _NB, _STAGES, VAW_WS_LOADERS, VAW_P8_NT, _NT_AUX: DESIGN.md lists them), vaw_debug_gemm_tile /
 * vaw_debug_force_generic_gemm, and the CUs the persistent kernels may use now; or an explicit set (cus <= 0: the process's). */
typedef struct {
    int tile;           /* vaw_debug_gemm_tile / VAW_GEMM_BIG: -1 by shape, 0 128 x 128, 1 256 x 256 ring, 2 / 3 persistent with 256 / 192
                         * columns, 4 persistent (width by shape), 5-8 small-M ring (by shape / 64 x 64 / 64 x 128 / 128 x 128),
                         * 9 / 10 / 11 parked-drain and 12 / 13 / 14 warp-specialised (width by shape / 256 / 192) wherever they apply */
    int force_generic;  /* vaw_debug_force_generic_gemm */
    int bk;             /* VAW_GEMM_BK: 32 / 64 pins the 128 x 128 kernel's stage depth (and keeps the other MFMA kernels out); 0 by shape */
    int pd, ws;         /* VAW_GEMM_PD / _WS: parked-drain / warp-specialised kernel by shape (default 0) */
    int xcdsplit;       /* VAW_GEMM_XCDSPLIT: K-range-per-XCD mapping of split-K 128 x 128 launches (default 1) */
    int sm_max_m, sm_wide_m, sm_nb, sm_stages;   /* VAW_SM_*: small-M ring kernel up to this M (8192), 128 x 128 tiles up to this M
                                                  * (0 = off), tile columns / 64 and ring depth (0 = by shape) */
    int ws_loaders;     /* VAW_WS_LOADERS: 8 = eight loader waves for the 192-column warp-specialised kernel (default 4) */
    int epi, debug;     /* VAW_GEMM_EPI (1: register-direct epilogue), VAW_GEMM_DEBUG: kernel flags, no launch choice */
    int p8_nt, nt_aux;  /* VAW_P8_NT (0), VAW_P8_NT_AUX (1): store cache policy of the persistent kernels, no launch choice */
    int cus;            /* CUs the persistent / parked-drain / warp-specialised grids may use */
} vaw_gemm_knobs;
void vaw_gemm_default_knobs(vaw_gemm_knobs* out);   /* every knob at its default (no environment), 256 CUs */
typedef enum {
    VAW_GV_GENERIC = 0,        /* gemm_generic_kernel: any shape, alignment, dtype; exact f32 */
    VAW_GV_T128_BK32 = 1,      /* gemm_bf16_kernel<.., 32, 0>: 128 x 128 tiles */
    VAW_GV_T128_BK64 = 2,      /* gemm_bf16_kernel<.., 64, 0> */
    VAW_GV_RING256 = 3,        /* gemm_bf16_big_kernel: 256 x 256 tiles */
    VAW_GV_PERSISTENT = 4,     /* gemm_p8_kernel<.., ntw, epi_kind>: 256 x 64 ntw tiles */
    VAW_GV_SMALL_M = 5,        /* gemm_sm_kernel<.., nb, stages, mb>: 64 mb x 64 nb tiles */
    VAW_GV_PARKED_DRAIN = 6,   /* gemm_pd_kernel<.., ntw, epi_kind>: 128 x 64 ntw tiles */
    VAW_GV_WARP_SPEC = 7       /* gemm_ws_kernel<.., ntw, epi_kind>: 128 x 64 ntw tiles */
} vaw_gemm_variant;
typedef enum { VAW_GR_NONE = 0, VAW_GR_F32 = 1, VAW_GR_BF16 = 2, VAW_GR_F32_ROWSUM = 3 } vaw_gemm_reduce;    /* splitk_reduce_kernel */
typedef enum { VAW_GS_NONE = 0, VAW_GS_FUSED = 1, VAW_GS_SEPARATE = 2 } vaw_gemm_rowsum_mode;
typedef enum { VAW_GC_NONE = 0, VAW_GC_FOLD = 1, VAW_GC_DEFERRED = 2, VAW_GC_SEPARATE = 3 } vaw_gemm_colsum_mode;
typedef struct {
    int variant;                    /* vaw_gemm_variant */
    int ntw;                        /* persistent / parked-drain / warp-specialised: tile columns / 64 (3 | 4); else 0 */
    int mb, nb, stages;             /* small-M ring: tile rows / 64, tile columns / 64, ring depth; else 0 */
    int bkt;                        /* K depth of one stage: 16 generic, 32 / 64 128 x 128, 32 ring, 64 the others */
    int epi_kind;                   /* persistent / parked-drain / warp-specialised: the P8_* epilogue kind (gemm_epi.h); else -1 */
    int split;                      /* K splits (1 = none) */
    int xcd_parts;                  /* 8 / split for the 128 x 128 kernel's K-range-per-XCD mapping, else 0 */
    int grid_x, grid_y, grid_z, block;
    int64_t lds_bytes;              /* dynamic LDS of the launch (generic: its static LDS) */
    int reduce;                     /* vaw_gemm_reduce: the pass over the split-K slabs (F32_ROWSUM: it also folds the row sums of A) */
    int rowsum_mode;                /* vaw_gemm_rowsum_mode: rowsum_a_out on the MFMA kernel, or a vaw_colsum pass over A */
    int colsum_mode;                /* vaw_gemm_colsum_mode: partial rows folded by vaw_reduce_rows, left to the caller
                                     * (colsum_partial_out), or a vaw_colsum pass over C (generic kernel) */
    int64_t colsum_rows;            /* partial rows of column sums the launch writes (0 without column sums) */
    int64_t workspace_floats_used;  /* slabs [split][M][N], then row-sum partials [split][M]; column-sum rows [colsum_rows][N]
                                     * from 0 (never with slabs); a separate pass reuses the workspace after them (the rows are folded first) */
    int launches;                   /* kernels enqueued, passes included */
    int status;                     /* vaw_status: VAW_OK, or what vaw_gemm returns before launching anything */
} vaw_gemm_launch;
int vaw_gemm_plan(vaw_dtype dt, int a_kmajor, int b_kmajor, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                  int64_t ldc, int64_t A, int64_t B, int64_t C, const vaw_epilogue* epi_host, int64_t workspace_floats,
                  const vaw_gemm_knobs* knobs, vaw_gemm_launch* out);

/* Launch plan of vaw_gemm_fp8, likewise the one host function it takes every check and launch choice from (pure arithmetic: it
 * can be asked without a GPU).  The arguments of vaw_gemm_fp8 with addresses as integers, used for null-ness and alignment only
 * (colsum_rows_out is read: the stated capacity; scale_a / scale_b may be 0), plus cus: the CUs the persistent grid may use,
 * 0 = what the process has now (vaw_p8_set_reserved_cus moves it); a stated value makes the plan a pure function.
 * A refused call returns what vaw_gemm_fp8 returns, with the same error text, and leaves that code in status. */
typedef struct {
    int epi_kind;                   /* P8_* kind of csrc/gemm_epi.h: 0 STORE, 1 GELU, 2 DGELU, 3 GATE, 8 GELU_Q, 9 DGELU_Q (C as fp8
                                     * bytes); -1 while no kind is chosen */
    int a_e5m2;                     /* A holds e5m2 bytes (VAW_BF8), else e4m3 */
    int c_fp8, c_e5m2;              /* C is written as fp8 bytes (c_fp8_state given), and their format */
    int ntw;                        /* tile columns / 64 (3 | 4); tiles are 256 rows */
    int tiles_m, tiles_n;           /* items = tiles_m * tiles_n * split, dealt to the workgroups round-robin */
    int nk;                         /* K tiles of 128 */
    int split;                      /* K splits: always 1 */
    int grid, block;
    int64_t lds_bytes;
    int colsum_mode;                /* vaw_gemm_colsum_mode: NONE, FOLD (partial rows in the workspace, folded by vaw_reduce_rows) or
                                     * DEFERRED (colsum_partial_out) */
    int64_t colsum_rows;            /* partial rows the launch writes: ceil(M / 128), or 0 */
    int64_t workspace_floats_used;  /* colsum_rows * N for FOLD, else 0 */
    int launches;
    int status;
} vaw_gemm_fp8_launch;
int vaw_gemm_fp8_plan(vaw_dtype a_format, int64_t M, int64_t N, int64_t K, int64_t A, int64_t lda, int64_t scale_a, int64_t B,
                      int64_t ldb, int64_t scale_b, int64_t C, int64_t ldc, const vaw_epilogue* epi_host, int64_t c_fp8_state,
                      vaw_dtype c_fp8_format, int64_t workspace, int64_t workspace_floats, int cus, vaw_gemm_fp8_launch* out);

/* out[n] = beta*out[n] + sum_m X[m,n]  (bias gradients). X act dtype, out f32.  Two fixed-order stages through a
 * caller-provided f32 workspace of vaw_colsum_workspace_floats(M,N) elements: no atomics, bitwise reproducible. */
int64_t vaw_colsum_workspace_floats(int64_t M, int64_t N);
int vaw_colsum(vaw_dtype dt, const void* X, int64_t M, int64_t N, int64_t ldx, float* out, float beta,
               float* workspace, int64_t workspace_floats, vaw_stream stream);
/* out[n] = beta*out[n] + sum_{r<R} partial[r,n], r ascending (second stage of the fixed-order column sums) */
int vaw_reduce_rows(const float* partial, int64_t R, int64_t N, float* out, float beta, vaw_stream stream);
/* The same fold for MANY (partial, out) pairs in one launch: out_j[n] = beta*out_j[n] + sum_{r<R_j} partial_j[r,n], each with
 * vaw_reduce_rows' summation tree (bitwise the same results).  Used for the bias gradients of all Linear layers of a group of
 * DiT blocks (autograd of `x W^T + b`, models/dit.py:126-137: db = sum_rows dy), whose partial rows the dy-producing kernels
 * leave behind: one launch per group instead of one per layer.  jobs: host array; desc_dev: device buffer of
 * vaw_reduce_rows_batched_desc_bytes(n_jobs) bytes that receives the table when upload != 0 (as for vaw_wgrad_grouped: once
 * per table; a table whose row counts or addresses moved is a new table). */
typedef struct {
    const float* partial;  /* f32 [R][N] */
    float* out;            /* f32 [N] */
    int64_t R, N;
} vaw_reduce_job;
int64_t vaw_reduce_rows_batched_desc_bytes(int n_jobs);
int vaw_reduce_rows_batched(int n_jobs, const vaw_reduce_job* jobs, float beta, void* desc_dev, int upload, vaw_stream stream);

/* ---------------------------------------------------------------------------
 * DiT pieces  (models/dit.py)
 * ------------------------------------------------------------------------- */

/* modulate(LayerNorm(x), shift, scale) :24-25,125,135: eps=1e-6, no affine.  x: f32 [B*T, D] residual
 * stream; shift/scale: f32 rows of the adaLN output with row stride mod_ld; out: act dtype [B*T, D];
 * mean/rstd: f32 [B*T] saved for backward. */
int vaw_ln_modulate_fwd(vaw_dtype dt, const float* x, const float* shift, const float* scale, int64_t mod_ld,
                        void* out, float* mean, float* rstd, int B, int T, int D, float eps, vaw_stream stream);
/* The GEMM kernels round the gated residual add differently: the persistent kernel's gated epilogue is one fma, the others round the
 * product first.  1 / 0: whether vaw_gemm gives the gated launch [B*T, D] = [B*T, D] x [D, D]^T (bias, aux_out, gate, f32 residual,
 * aligned operands: a DiT block's proj) to the former, with the process's GEMM knobs -- the rounding vaw_gate_resid_ln_modulate_fwd
 * then uses, so that it is bitwise that launch followed by vaw_ln_modulate_fwd.  Host arithmetic, no GPU needed. */
int vaw_gate_resid_fwd_contracts(int B, int T, int D);
/* The gated residual add of a branch and the LayerNorm + modulate that reads its result, in one pass over the rows (bf16 mode;
 * models/dit.py:135-136 -> :125,135 of the next consumer):
 *   x_out[b,t,:] = y[b,t,:] * gate[b,:] + x_in[b,t,:]    (rounded as vaw_gemm's gated-residual epilogue rounds it for these rows today:
 *                                                         vaw_gate_resid_fwd_contracts)
 *   out = modulate(LayerNorm(x_out), shift, scale), mean, rstd    (the bits vaw_ln_modulate_fwd gives on x_out)
 * y, out: bf16 [B*T, D]; x_in, x_out: f32 [B*T, D], not the same buffer; gate (row stride gate_ld), shift / scale (mod_ld): f32 rows
 * per sample.  out == NULL: the residual only -- shift, scale, mean and rstd are not touched.  dt must be VAW_BF16, D % 4 == 0,
 * D <= 2048, the strides multiples of 4 and every base 16-byte aligned: anything else is refused (VAW_ERR_INVALID) before any launch. */
int vaw_gate_resid_ln_modulate_fwd(vaw_dtype dt, const void* y, const float* gate, int64_t gate_ld, const float* x_in, float* x_out,
                                   const float* shift, const float* scale, int64_t mod_ld, void* out, float* mean, float* rstd,
                                   int B, int T, int D, float eps, vaw_stream stream);
/* Backward of the above, fused with the residual-stream gradient:
 *   dx[b,t,:]   = (dres_in ? dres_in : 0) + LN'(dout * (1+scale))
 *   dshift[b,:] = sum_t dout ;  dscale[b,:] = sum_t dout * xhat     (rows with stride dmod_ld)
 * dx may alias dres_in. */
int vaw_ln_modulate_bwd(vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                        const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift,
                        float* dscale, int64_t dmod_ld, int B, int T, int D, float* workspace, int64_t workspace_floats,
                        vaw_stream stream);
/* The same launch with dx_act (may be NULL) = dx rounded to the act dtype, written beside dx: the GEMM operand a cast pass over
 * dx would make (the last LayerNorm backward of a DiT step feeds the patch embedding's weight gradient). */
int vaw_ln_modulate_bwd_cast(vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                             const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift,
                             float* dscale, int64_t dmod_ld, int B, int T, int D, float* workspace, int64_t workspace_floats,
                             void* dx_act, vaw_stream stream);
/* fp8 mode of the DiT blocks (delayed scaling): the same two kernels with their activation output written as fp8 BYTES [B*T][D]
 * -- the bf16 rounding of each value divided by q_state[0], saturated: what vaw_fp8_quantize_delayed makes of the bf16 tensor,
 * which then is never written -- and the tensor's max |x| folded into q_state[1]; vaw_fp8_transpose supplies the transposed copy. */
int vaw_ln_modulate_fwd_fp8(const float* x, const float* shift, const float* scale, int64_t mod_ld, void* q_out, float* q_state,
                            vaw_dtype q_format, float* mean, float* rstd, int B, int T, int D, float eps, vaw_stream stream);
int vaw_gate_bwd_fp8(const float* dres, const void* y, const float* gate, int64_t mod_ld, void* dy_q, float* q_state,
                     vaw_dtype q_format, float* dgate, int64_t dmod_ld, float* dy_colsum_partial, int B, int T, int D,
                     float* workspace, int64_t workspace_floats, vaw_stream stream);
/* Workspace (f32) of vaw_ln_modulate_bwd / vaw_gate_bwd: with it, a sample's T rows are cut into chunks handled by
 * separate workgroups (small per-GPU batches would otherwise leave most CUs idle: one workgroup per sample) and the
 * per-sample column sums are folded over the chunks in a fixed order by a second kernel.  NULL = one workgroup per sample. */
int64_t vaw_row_bwd_workspace_floats(int B, int T, int D);
/* Launch plan of the row kernels: the one host function their entry points take every launch choice from (pure arithmetic: no
 * device call, so it can be asked without a GPU).  kind = the entry point; dt = its act dtype (the fp8 entries: VAW_BF16);
 * rows: B, T, D as the entry point's, workspace_floats = what the caller would pass (0 = none), ldx / base_addr unused;
 * colsum: M = B * T rows (pass T = 1), N = D columns, row stride ldx, base_addr = the address of X (its alignment picks the path).
 *   nc: workgroups per sample (grid.y; > 1: row_bwd_finish_kernel folds them), rows_per_chunk: T rows per chunk;
 *   colsum: nc = partial rows of the workspace (grid.y), rows_per_chunk = rows per partial row.
 * VAW_ROW_GATE_LN_FWD (vaw_gate_resid_ln_modulate_fwd): ldx = the OR of gate_ld and mod_ld, base_addr = the OR of the addresses of
 *   its vector operands; anything but bf16 rows, D % 4 == 0, strides that are multiples of 4 and 16-byte aligned bases is refused. */
typedef enum { VAW_ROW_LN_FWD = 0, VAW_ROW_LN_FWD_FP8 = 1, VAW_ROW_LN_BWD = 2, VAW_ROW_GATE_BWD = 3, VAW_ROW_GATE_BWD_FP8 = 4,
               VAW_ROW_LN_BWD_GATE = 5, VAW_ROW_LN_BWD_GATE_FP8 = 6, VAW_ROW_COLSUM = 7, VAW_ROW_GATE_LN_FWD = 8 } vaw_row_kind;
typedef enum {
    VAW_RV_LN_FWD = 0,          /* ln_modulate_fwd_kernel<T, NV> */
    VAW_RV_ROW_BWD = 1,         /* row_bwd_kernel<T, NV, false>: LayerNorm backward */
    VAW_RV_ROW_GATE = 2,        /* row_bwd_kernel<T, NV, true>: gate backward */
    VAW_RV_ROW_FUSE = 3,        /* row_bwd_kernel<T, NV, false, QOUT, true>: fused, per-sample sums in registers */
    VAW_RV_ROW_FUSE8 = 4,       /* row_bwd_fuse8_kernel<NV, QOUT>: fused, per-wave sums in LDS slabs (bf16) */
    VAW_RV_COLSUM_BF16X8 = 5, VAW_RV_COLSUM_VEC4 = 6, VAW_RV_COLSUM_SCALAR = 7,
    VAW_RV_GATE_LN_FWD = 8      /* gate_resid_ln_fwd_kernel<NV, LN>: gated residual + LayerNorm forward, one wave per row (bf16) */
} vaw_row_variant;
typedef struct {
    int variant;                /* vaw_row_variant */
    int nv;                     /* template slab count: 256-column slabs a lane walks (1..6, 8); colsum: 0 */
    int nc, rows_per_chunk;     /* see above */
    int grid_x, block;          /* grid.x (forward: before the launcher's cap to one resident round), threads per workgroup */
    int64_t lds_bytes;          /* dynamic LDS per workgroup */
    int64_t workspace_floats;   /* f32 workspace the launch uses (0: none) */
} vaw_row_launch;
int vaw_row_plan(vaw_row_kind kind, vaw_dtype dt, int64_t B, int64_t T, int64_t D, int64_t ldx, int64_t base_addr,
                 int64_t workspace_floats, vaw_row_launch* out);
/* Backward of `x + gate.unsqueeze(1) * y` :135-136 w.r.t. the branch:
 *   dy[b,t,:] = dres[b,t,:] * gate[b,:] (act dtype) ; dgate[b,:] = sum_t dres * y ;
 *   dy_colsum_partial (f32 [B, D] or NULL): per-sample sum_t dy -- reduce over B with vaw_reduce_rows to get the
 *   bias gradient of the branch's last Linear without re-reading dy. */
int vaw_gate_bwd(vaw_dtype dt, const float* dres, const void* y, const float* gate, int64_t mod_ld, void* dy,
                 float* dgate, int64_t dmod_ld, float* dy_colsum_partial, int B, int T, int D, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* vaw_ln_modulate_bwd and the vaw_gate_bwd that consumes its dx, as ONE pass over the rows (autograd of models/dit.py:135-136
 * walked backwards: the LayerNorm+modulate of a branch, then the gated residual add in front of it): dx as vaw_ln_modulate_bwd;
 * dy_next = dx * gate_next (act dtype), dgate_next[b,:] = sum_t dx * y_next, dy_colsum_partial [B,D] = per-sample sum_t dy_next.
 * dgate_next shares dmod_ld with dshift / dscale.  Saves the re-read of dx (f32) and a launch; bitwise equal to the pair. */
int vaw_ln_modulate_bwd_gate(vaw_dtype dt, const void* dout, const float* x, const float* mean, const float* rstd,
                             const float* scale, int64_t mod_ld, const float* dres_in, float* dx, float* dshift, float* dscale,
                             int64_t dmod_ld, const void* y_next, const float* gate_next, void* dy_next, float* dgate_next,
                             float* dy_colsum_partial, int B, int T, int D, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* fp8 mode: dy_next as fp8 bytes of its bf16 roundings (see vaw_gate_bwd_fp8) */
int vaw_ln_modulate_bwd_gate_fp8(const void* dout, const float* x, const float* mean, const float* rstd, const float* scale,
                                 int64_t mod_ld, const float* dres_in, float* dx, float* dshift, float* dscale, int64_t dmod_ld,
                                 const void* y_next, const float* gate_next, void* dy_q, float* q_state, vaw_dtype q_format,
                                 float* dgate_next, float* dy_colsum_partial, int B, int T, int D, float* workspace,
                                 int64_t workspace_floats, vaw_stream stream);

/* timm PatchEmbed (dit.py:192) input side: x f32 [B,C,H,W] -> tokens act dtype [B*(H/p)*(W/p), C*p*p],
 * column order (c, i, j) = Conv2d weight flattening. */
int vaw_patchify(vaw_dtype dt, const float* img, void* tok, int B, int C, int H, int W, int p, vaw_stream stream);
/* gradient of patchify w.r.t. the image: dtok f32 [B*h*w, C*p*p] -> dimg f32 [B,C,H,W] */
int vaw_patchify_bwd(const float* dtok, float* dimg, int B, int C, int H, int W, int p, vaw_stream stream);
/* unpatchify :243-256: tokens f32 [B*h*w, p*p*C] (column order (i, j, c)) -> img f32 [B,C,h*p,w*p];
 * vaw_unpatchify_bwd is the transpose map (dimg -> token rows, act dtype). */
int vaw_unpatchify(vaw_dtype dt, const float* tok, float* img, int B, int C, int H, int W, int p,
                   vaw_stream stream);
int vaw_unpatchify_bwd(vaw_dtype dt, const float* dimg, void* dtok, int B, int C, int H, int W, int p,
                       vaw_stream stream);

/* sinusoidal embedding (dit.py:56-74 == tools/nn.py:103-121): out[b] = [cos(t f_i) | sin(t f_i)], act dtype. */
int vaw_timestep_embedding(vaw_dtype dt, const float* t, void* out, int B, int dim, float max_period,
                           vaw_stream stream);
/* SiLU on f32 input; out act dtype.  bwd: dx(f32) += / = dy * silu'(x). */
int vaw_silu_fwd(vaw_dtype dt, const float* x, void* out, int64_t n, vaw_stream stream);
int vaw_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, vaw_stream stream);
/* vaw_silu_bwd that also leaves dx_bf16 (may be NULL) = bf16(dx): the operand of the weight gradient that follows */
int vaw_silu_bwd_cast(const float* x, const float* dy, float* dx, void* dx_bf16, int64_t n, vaw_stream stream);
/* out[b,:] = a[b,:] + table[idx[b],:]  (c = t_emb + y_emb, dit.py:267-269 / unet.py:676) */
int vaw_add_embedding(const float* a, const float* table, const int64_t* idx, float* out, int B, int D,
                      int num_rows, vaw_stream stream);
/* nn.Embedding backward: dtable[r,:] = beta*dtable[r,:] + sum_{b: idx[b]==r} dc[b,:] (b ascending; every row
 * of the table is written, no atomics, no pre-zeroing) */
int vaw_embedding_bwd(const float* dc, const int64_t* idx, float* dtable, int B, int D, int num_rows, float beta,
                      vaw_stream stream);

/* Multi-head attention, softmax(scale * q k^T) v, strided so both layouts of the reference are served:
 *   DiT (timm Attention, dit.py:126): qkv [B*T, 3*H*hd] token-major -> stride_t = 3*H*hd, stride_d = 1
 *   UNet QKVAttention (unet.py:362-390): qkv [B, 3*H*ch, T] channel-major -> stride_t = 1, stride_d = T
 * q/k/v/o point at element (b=0, h=0, t=0, d=0) of each operand; stride_b / stride_h in elements.
 * lse: f32 [B*H*T] (row log-sum-exp, saved for backward). */
typedef struct {
    int B, H, T, hd;
    int64_t q_sb, q_sh, q_st, q_sd; /* shared by q, k, v (same tensor, different base) */
    int64_t o_sb, o_sh, o_st, o_sd;
    float scale;
} vaw_attn_desc;
int vaw_attn_fwd(vaw_dtype dt, const vaw_attn_desc* d_host, const void* q, const void* k, const void* v, void* o,
                 float* lse, vaw_stream stream);
/* dq/dk/dv use the q strides, d_o the o strides.  delta: f32 [B*H*T] workspace. */
int vaw_attn_bwd(vaw_dtype dt, const vaw_attn_desc* d_host, const void* q, const void* k, const void* v,
                 const void* o, const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv,
                 vaw_stream stream);
/* vaw_attn_bwd that also leaves the column sums of dq | dk | dv behind as PARTIAL rows -- the bias gradient of the qkv Linear in
 * front of the attention (timm Attention, models/dit.py:126: db = sum over tokens of dqkv) without a second pass over dqkv:
 * colsum_partial [*rows_out_host][3*H*hd] f32 in packed-qkv column order [3][H][hd]; at most B*T/64 rows: *rows_out_host is in / out --
 * on entry the capacity of the buffer in rows (checked), on return the rows written; fold them with vaw_reduce_rows / vaw_reduce_rows_batched.  Only the bf16 MFMA kernels offer it (token-major or any
 * layout they accept): VAW_ERR_UNSUPPORTED, nothing launched, otherwise -- use vaw_attn_bwd + vaw_colsum then. */
int vaw_attn_bwd_colsum(vaw_dtype dt, const vaw_attn_desc* d_host, const void* q, const void* k, const void* v, const void* o,
                        const void* d_o, const float* lse, float* delta, void* dq, void* dk, void* dv, float* colsum_partial,
                        int64_t* rows_out_host, vaw_stream stream);

/* Launch plan of the attention entry points: the one host function vaw_attn_fwd / vaw_attn_bwd / vaw_attn_bwd_colsum take every
 * launch choice from (pure arithmetic: no device call, so it can be asked without a GPU).  q / k / v / o_or_do / dq / dk / dv are the
 * addresses the entry point would be given (only their alignment matters; o_or_do: o for the forward, d_o for the backward; dq / dk
 * / dv are ignored by the forward).  Reads VAW_ATTN_FWD_BIG, VAW_ATTN_BWD_BIG, VAW_ATTN_QG2 and VAW_ATTN_BWD_G2 on every call.
 * VAW_ERR_INVALID where the descriptor is refused (T > 1024, B*H >= 65536, a size <= 0, a rowwise LDS request over 64 KiB). */
typedef enum { VAW_ATTN_DIR_FWD = 0, VAW_ATTN_DIR_BWD = 1, VAW_ATTN_DIR_BWD_COLSUM = 2 } vaw_attn_dir;
typedef enum {
    VAW_AV_ROWWISE = 0,         /* attention.hip: attn_fwd_rowwise / attn_bwd_q_rowwise + attn_bwd_kv_rowwise <T> */
    VAW_AV_FWD_T64 = 1,         /* attn_fwd_mfma<HD, 1, false>: T == 64 */
    VAW_AV_FWD_G1 = 2,          /* attn_fwd_mfma<HD, 1> */
    VAW_AV_FWD_G2 = 3,          /* attn_fwd_mfma<HD, 2>: T % 128 == 0 */
    VAW_AV_FWD_BIG = 4,         /* attn_fwd_big<HD, 2>: T % 128 == 0 */
    VAW_AV_BWD_T64 = 5,         /* attn_bwd_t64_mfma<HD>: T == 64, one launch */
    VAW_AV_BWD_G1 = 6,          /* attn_bwd_dq_mfma + attn_bwd_dkv_mfma <HD, 1> */
    VAW_AV_BWD_G2 = 7,          /* attn_bwd_dq_mfma + attn_bwd_dkv_mfma <96, 2>: T % 128 == 0 */
    VAW_AV_BWD_BIG_NT2 = 8,     /* attn_bwd_big<HD, 1 | 0, 2>: T % 128 == 0 */
    VAW_AV_BWD_BIG_NT4 = 9      /* attn_bwd_big<HD, 1 | 0, 4>: T % 256 == 0 */
} vaw_attn_variant;
typedef struct {
    int variant;                /* vaw_attn_variant */
    int hd_image;               /* head width of the kernel's LDS image: 32 / 64 / 96 / 128; 0 = rowwise */
    int launches;               /* kernels enqueued */
    int grid_x, grid_y, block;  /* workgroups per (sample, head) along the tokens, B * H, threads per workgroup (VAW_AV_BWD_T64
                                 * enqueues its grid_x * grid_y workgroups as a 1-D grid) */
    int64_t lds_bytes;          /* largest dynamic LDS of its launches */
    int lds_cap_raised;         /* 1: that launch raises its LDS cap with hipFuncSetAttribute (else it must fit the 64 KiB default) */
    int64_t colsum_rows;        /* VAW_ATTN_DIR_BWD_COLSUM: partial rows written; 0 = column sums not offered (and other directions) */
    int status;                 /* vaw_status: VAW_OK, or what the entry point returns before launching anything */
} vaw_attn_launch;
int vaw_attn_plan(int dir, vaw_dtype dt, const vaw_attn_desc* d, int64_t q, int64_t k, int64_t v, int64_t o_or_do, int64_t dq,
                  int64_t dk, int64_t dv, vaw_attn_launch* out);

/* ---------------------------------------------------------------------------
 * UNet pieces  (models/unet.py, tools/nn.py) -- activations are NHWC: [B*H*W pixels, C channels], act dtype
 * ------------------------------------------------------------------------- */

/* conv3x3 (stride 1, pad 1, NHWC) with a narrow side of at most 4 channels: the 3-channel stem and output convs of
 * models/unet.py:492 (conv_nd(dims, in_channels, ch, 3, padding=1)) and :625 (zero_module(conv_nd(dims, input_ch, out_channels, 3, padding=1))).
 * Direct f32-accumulating kernels (K = 27..36 is too short for the MFMA tile).  w has the activation dtype.
 *   mode 0  forward, narrow input:    in [M][Cn]      -> out [M][Cw],  w = [Cw][3][3][Cn], bias [Cw] or NULL
 *   mode 1  input gradient of a conv with a narrow OUTPUT: in = dy [M][Cn] -> out = dx [M][Cw], w = [Cn][3][3][Cw]
 *   mode 2  forward, narrow output:   in [M][Cw]      -> out [M][Cn],  w = [Cn][3][3][Cw], bias [Cn] or NULL
 * Returns VAW_ERR_UNSUPPORTED (nothing launched) when Cn > 4 or Cw % 8 != 0. */
int vaw_conv3x3_narrow(vaw_dtype dt, int mode, const void* in, const void* w, const float* bias, void* out, int B, int H,
                       int W, int Cn, int Cw, vaw_stream stream);

/* GroupNorm32 (tools/nn.py:17-19,93-100; G groups, eps) fused with what follows it in ResBlock._forward
 * (unet.py:236-256):  y = act( GN(x)*gamma + beta [ *(1 + scale[b,c]) + shift[b,c] ] ), act = SiLU if silu else id.
 * scale/shift: f32 rows with stride film_ld (the emb_layers output), or both NULL.  mean/rstd: f32 [B*G] saved.
 * workspace: vaw_groupnorm_workspace_floats(B, HW, C) f32.
 * All three entry points return VAW_ERR_INVALID before any launch for a NULL required pointer, scale without shift (or the
 * reverse) and a pointer off the alignment of the launch vaw_gn_plan picks: 16 bytes for x, y, dout, dx, dx_add on the flat
 * kernels and in f32, 8 bytes for bf16 on the quad kernels; 16 bytes for gamma, beta, scale and shift. */
int64_t vaw_groupnorm_workspace_floats(int B, int HW, int C);
int vaw_groupnorm_fwd(vaw_dtype dt, const void* x, const float* gamma, const float* beta, const float* scale,
                      const float* shift, int64_t film_ld, int silu, void* y, float* mean, float* rstd, int B, int HW,
                      int C, int G, float eps, float* workspace, vaw_stream stream);
/* The apply pass of vaw_groupnorm_fwd alone, on GIVEN statistics (mean/rstd: f32 [B*G], as vaw_groupnorm_fwd saved them):
 * the same kernel under the same plan (vaw_gn_plan, VAW_GN_APPLY), so for the same x, statistics and parameters y is bitwise
 * vaw_groupnorm_fwd's.  One pass over x instead of three: activation recomputation (UNet use_checkpoint). */
int vaw_groupnorm_apply(vaw_dtype dt, const void* x, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, const float* scale, const float* shift, int64_t film_ld, int silu, void* y, int B,
                        int HW, int C, int G, vaw_stream stream);
/* dx = GN'(...) (+ dx_add, act dtype, may be NULL); dgamma/dbeta = grad_beta*old + sum; dscale/dshift rows (stride
 * dfilm_ld) when FiLM.  Fixed-order reductions. */
int vaw_groupnorm_bwd(vaw_dtype dt, const void* dout, const void* x, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, const float* scale, const float* shift, int64_t film_ld,
                      int silu, const void* dx_add, void* dx, float* dgamma, float* dbeta, float grad_beta, float* dscale,
                      float* dshift, int64_t dfilm_ld, int B, int HW, int C, int G, float* workspace, vaw_stream stream);
/* Launch plan of the GroupNorm entry points: the one host function vaw_groupnorm_fwd / _apply / _bwd take every launch choice
 * from (pure arithmetic: no device call, so it can be asked without a GPU).  pass = one streaming launch: the forward is
 * VAW_GN_FWD_SUMS then VAW_GN_APPLY (vaw_groupnorm_apply: that launch alone), the backward VAW_GN_BWD_SUMS then VAW_GN_BWD_APPLY
 * (the small statistics / fold / group kernels between the two go with the sums pass).  Flat -- a thread owns a channel octet
 * (16-byte accesses) of every rpi-th row -- needs: the switch not 0, bf16, C % 8 == 0, C / 8 <= 256, C <= 2048, B * HW < 2^30,
 * HW * C < 2^31 and the largest chunk of 512 / 256 / 128 rows that gives B * ceil(HW / rows) >= 512 workgroups (switch 1: 128 rows
 * where none does); everything else is quad -- a thread owns a channel quad -- on 512-row chunks.  Reads the vaw_debug_gn_flat
 * switch (-1 by shape | 0 never | 1 wherever it can run) on every call.  VAW_ERR_INVALID: dt not f32 / bf16, a size <= 0,
 * C % 4 != 0, C % G != 0, G > 64, B >= 65536, quad with more than 65535 chunks (grid.z). */
typedef enum { VAW_GN_FWD_SUMS = 0, VAW_GN_APPLY = 1, VAW_GN_BWD_SUMS = 2, VAW_GN_BWD_APPLY = 3 } vaw_gn_pass;
typedef enum {
    VAW_GNV_QUAD = 0,           /* gn_fwd_sums / gn_apply / gn_bwd_sums / gn_bwd_apply _kernel<T> */
    VAW_GNV_FLAT = 1            /* gns_fwd_sums / gns_apply / gns_bwd_sums / gns_bwd_apply _kernel */
} vaw_gn_variant;
typedef struct {
    int variant;                /* vaw_gn_variant */
    int rows, nch;              /* rows of a chunk, chunks per sample: nch = ceil(HW / rows) */
    int nt, rpi;                /* flat: live lanes of a workgroup (a multiple of C / 8) and rows per step nt / (C / 8); quad: 0 */
    int grid_x, grid_y, grid_z, block;   /* flat: B * nch workgroups; quad: (ceil(C / 64), B, nch) */
    int64_t lds_bytes;          /* static LDS of the pass's streaming kernel */
    int64_t workspace_floats;   /* f32 workspace the pass reads or writes, from its start (apply: 0);
                                 * never more than vaw_groupnorm_workspace_floats(B, HW, C), whatever the switch */
    int64_t off_part, off_sums, off_s1, off_s2;   /* f32 offsets of its regions, -1 = not used: chunk partials [2 | 4][nch][B][C],
                                 * folded sums [4][B][C], S1 and S2 [B * G] */
    int status;                 /* vaw_status: VAW_OK, or what the entry point returns before launching anything */
} vaw_gn_launch;
int vaw_gn_plan(int pass, vaw_dtype dt, int B, int HW, int C, int G, vaw_gn_launch* out);
/* conv3x3 stride 1 pad 1 as GEMM (round 1: explicit patch matrix).  col[m, tap*C + c] = x[pixel(m)+tap offset, c];
 * vaw_col2im3x3 is the transposed map written as a gather (deterministic): the input gradient from d(col). */
int vaw_im2col3x3(vaw_dtype dt, const void* x, void* col, int B, int H, int W, int C, vaw_stream stream);
int vaw_col2im3x3(vaw_dtype dt, const void* dcol, void* dx, int B, int H, int W, int C, vaw_stream stream);
/* conv3x3 (stride 1, pad 1) as IMPLICIT GEMM on the bf16 MFMA kernel: the patch matrix is never written; padding taps
 * read a zero page.  mode 0: out[M,Co] = conv(act=x[M,Ci]; w) with the vaw_gemm epilogue (bias, residual, column sums);
 * mode 1: out = dx[M,Ci] from act = dy[M,Co]; mode 2: out = dW[Co][9][Ci] f32 = beta*dW + dy^T . patches(x) with
 * act = dy, act2 = x (split-K through the workspace); in mode 2 ep->rowsum_a_out, if set, receives the conv's BIAS
 * gradient rowsum_a_beta*old + sum over pixels of dy[.,co] (taken from the dy tiles already in LDS, fixed order).
 * w: [Co][3][3][Ci] act dtype.  Returns VAW_ERR_UNSUPPORTED
 * (nothing launched) for shapes that need the explicit vaw_im2col3x3 + vaw_gemm path: f32, Ci or Co not a multiple
 * of 64 (mode 0 / 1), ... */
int vaw_conv3x3(vaw_dtype dt, int mode, const void* act, const void* act2, const void* w, void* out, int B, int H, int W,
                int Ci, int Co, const vaw_epilogue* epi_host, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* Launch plan of vaw_conv3x3: the one host function it (and the persistent kernel's conv entry) takes every check and launch choice
 * from (pure arithmetic: it can be asked without a GPU).  The arguments of vaw_conv3x3 with addresses as integers, used for
 * null-ness and alignment only (a NULL workspace counts as workspace_floats = 0); knobs: NULL = the process's own (vaw_gemm_plan
 * describes them; the conv reads tile, force_generic and xcdsplit), cus: the CUs a persistent grid may use, 0 = what the process has
 * (then the knobs' own count, if they state one).
 * Order: invalid arguments (VAW_ERR_INVALID) -> shapes the explicit vaw_im2col3x3 + vaw_gemm path must take (VAW_ERR_UNSUPPORTED)
 * -> workspace checks -> kernel.  The persistent 256-row kernel where the switch and the shape allow (tile 2 / 3 / 4, or by shape
 * from half the CUs' worth of items; modes 0 / 1: bias and act-dtype residual epilogues only, Co resp. Ci >= 64, whole 64-pixel
 * tiles; mode 2: the transposed problem dW^T [9 Ci][Co] with at least two K splits), the 128 x 128 kernel everywhere else.
 * Both "rowsum_a_out (bias gradient) belongs to mode 2" and "mode 2 takes rowsum_a_out, not colsum_out" are refused on EVERY shape;
 * they used to be reached only once the persistent kernel had declined, so that a mode 0 / 1 call with rowsum_a_out was refused at
 * one shape and ran, its argument misread, at another. */
typedef enum { VAW_CVR_NONE = 0, VAW_CVR_F32 = 1, VAW_CVR_F32_ROWSUM = 2, VAW_CVR_SLAB_T = 3 } vaw_conv_reduce;
typedef enum { VAW_CVB_NONE = 0, VAW_CVB_FUSED = 1, VAW_CVB_FOLD = 2, VAW_CVB_SEPARATE = 3 } vaw_conv_bias_grad;
typedef struct {
    int variant;                    /* vaw_gemm_variant: VAW_GV_T128_BK64 (gemm_bf16_kernel<.., 64, CONV>) | VAW_GV_PERSISTENT */
    int ntw;                        /* persistent: tile columns / 64 (3 | 4); else 0 */
    int epi_kind;                   /* persistent: P8_STORE | P8_RESID | P8_SLAB (gemm_epi.h); else -1 */
    int transposed;                 /* 1: the kernel computes dW^T [9 Ci][Co] (persistent, mode 2); the reduce transposes it back */
    int64_t M, N, K;                /* the GEMM problem the kernel runs: mode 0 [pixels][Co] over 9 Ci, mode 1 [pixels][Ci] over 9 Co,
                                     * mode 2 [Co][9 Ci] (transposed: [9 Ci][Co]) over the pixels */
    int split;                      /* K splits (1 = none) */
    int xcd_parts;                  /* 8 / split for the 128 x 128 kernel's K-range-per-XCD mapping, else 0 */
    int grid_x, grid_y, block;
    int64_t lds_bytes;
    int reduce;                     /* vaw_conv_reduce: none | splitk_reduce f32 | the same, folding the bias gradient's partial rows |
                                     * p8_conv_wgrad_reduce_kernel (transposes the slabs; folds the partial rows when there are any) */
    int bias_grad;                  /* vaw_conv_bias_grad: rowsum_a_out of mode 2.  FUSED: partial rows from the kernel, folded by the reduce
                                     * pass; FOLD: the un-split 128 x 128 launch's one row, by vaw_reduce_rows; SEPARATE: a vaw_colsum
                                     * pass over dy (256-column persistent kernel, or no room behind the slabs) */
    int colsum_mode;                /* vaw_gemm_colsum_mode: VAW_GC_NONE | VAW_GC_FOLD (colsum_out, modes 0 / 1: 128 x 128 kernel only) */
    int64_t colsum_rows;            /* partial rows of column sums the launch writes (0 without column sums) */
    int64_t workspace_floats_used;  /* slabs [split][M][N], then bias-gradient partials [split][Co]; column-sum rows from 0 (never with
                                     * slabs); a separate vaw_colsum pass reuses the workspace */
    int launches;                   /* kernels enqueued, passes included */
    int status;                     /* vaw_status: VAW_OK, or what vaw_conv3x3 returns before launching anything */
} vaw_conv3x3_launch;
int vaw_conv3x3_plan(vaw_dtype dt, int mode, int64_t act, int64_t act2, int64_t w, int64_t out, int B, int H, int W, int Ci, int Co,
                     const vaw_epilogue* epi_host, int64_t workspace, int64_t workspace_floats, const vaw_gemm_knobs* knobs, int cus,
                     vaw_conv3x3_launch* plan);
/* conv3x3 weight gradient for the 3-channel stem / output convs (Ci <= 4 or Co <= 4), where a GEMM would be 3 wide:
 * dw[co][tap][ci] (f32, channels-last weight layout) = beta*dw + sum_m dy[m,co] * x[pixel(m)+tap, ci]; chunk
 * partials in the workspace are folded in a fixed order. */
int64_t vaw_conv3x3_wgrad_small_workspace_floats(int B, int H, int W, int Ci, int Co);
int vaw_conv3x3_wgrad_small(vaw_dtype dt, const void* dy, const void* x, float* dw, float beta, int B, int H, int W, int Ci,
                            int Co, float* workspace, int64_t workspace_floats, vaw_stream stream);
/* mode 0: out[Ho,Wo] = s * sum of the 2x2 block of in[2Ho,2Wo] (avg_pool2d with s=1/4; nearest-upsample^T with s=1)
 * mode 1: out[Ho,Wo] = s * in[Ho/2,Wo/2]                        (nearest x2 with s=1; avg_pool2d^T with s=1/4) */
int vaw_resample2(vaw_dtype dt, const void* in, void* out, int B, int Ho, int Wo, int C, int mode, float s,
                  vaw_stream stream);
/* cat[m,:] = [a[m,:Ca] | b[m,:Cb]] (torch.cat(dim=1) of unet.py:684 in NHWC); split=1 copies cat back into a and b */
int vaw_concat_channels(vaw_dtype dt, void* a, void* b, void* cat, int64_t M, int Ca, int Cb, int split,
                        vaw_stream stream);
int vaw_add_inplace(vaw_dtype dt, void* dst, const void* src, int64_t n, vaw_stream stream);
/* ResBlock / resampling variants that no reference factory uses but its constructor accepts (models/unet.py:81-140,206-256):
 *   vaw_mul         out = a * b (act dtype): nn.Dropout(p) as a product with a pre-scaled keep mask (--dropout, main.py:99)
 *   vaw_subsample2  mode 0: out[b,i,j,:] = in[b,2i,2j,:] -- Downsample's stride-2 conv = the stride-1 conv sampled at the even
 *                   pixels; mode 1: its transpose (zeros at the odd pixels).  out is [B,Ho,Wo,C] in both modes
 *   vaw_rowvec_add  h[b,p,:] += e[b,:] (f32 e, row stride ld): `h + emb_out` of use_scale_shift_norm=False
 *   vaw_rowvec_sum  de[b,:] = beta*de[b,:] + sum_p dh[b,p,:]: its backward (fixed-order reduction) */
int vaw_mul(vaw_dtype dt, const void* a, const void* b, void* out, int64_t n, vaw_stream stream);
int vaw_subsample2(vaw_dtype dt, const void* in, void* out, int B, int Ho, int Wo, int C, int mode, vaw_stream stream);
/* nn.Dropout's keep mask at 1 bit per element (what a checkpointed ResBlock keeps: C/8 bytes per pixel instead of 2 C).
 *   vaw_dropout_pack      mask [M][C] act dtype (keep ? 1/(1-p) : 0, as drawn for vaw_mul) -> bits: element i is bit i % 32 of the
 *                         32-bit word i / 32 (1 = kept).  bits holds vaw_dropout_bits_words(M * C) words; the unused high bits of the
 *                         last word are written as 0.  C % 8 != 0: VAW_ERR_INVALID (keep the unpacked mask).
 *   vaw_dropout_bits_fwd  y  = x  * (bit ? keep_scale : 0)   keep_scale = the mask's non-zero value (1/(1-p) rounded to the act
 *   vaw_dropout_bits_bwd  dx = dy * (bit ? keep_scale : 0)   dtype): the f32 product and rounding of vaw_mul, so bitwise its result.
 *                         n % 8 == 0, 16-byte aligned x / y. */
int64_t vaw_dropout_bits_words(int64_t n);
int vaw_dropout_pack(vaw_dtype dt, const void* mask, void* bits, int64_t M, int C, vaw_stream stream);
int vaw_dropout_bits_fwd(vaw_dtype dt, const void* x, const void* bits, float keep_scale, void* y, int64_t n, vaw_stream stream);
int vaw_dropout_bits_bwd(vaw_dtype dt, const void* dy, const void* bits, float keep_scale, void* dx, int64_t n, vaw_stream stream);
int vaw_rowvec_add(vaw_dtype dt, void* h, const float* e, int64_t ld, int B, int HW, int C, vaw_stream stream);
int vaw_rowvec_sum(vaw_dtype dt, const void* dh, float* de, int64_t ld, int B, int HW, int C, float beta, vaw_stream stream);
int vaw_nchw_to_nhwc(vaw_dtype dt, const float* nchw, void* nhwc, int B, int C, int HW, vaw_stream stream);
int vaw_nhwc_to_nchw(vaw_dtype dt, const void* nhwc, float* nchw, int B, int C, int HW, vaw_stream stream);

/* ---------------------------------------------------------------------------
 * Optimizer side  (torch.optim.AdamW at main.py:354, ema() tools/trainer.py:12-18,
 * clip_grad_norm_ tools/trainer.py:60-62)
 * ------------------------------------------------------------------------- */

/* sumsq_out[0] = (accumulate ? sumsq_out[0] : 0) + sum g^2 over n elements; fixed-order two-stage reduction
 * through a workspace of vaw_sumsq_workspace_floats() f32. */
int64_t vaw_sumsq_workspace_floats(void);
int vaw_sumsq(const float* g, int64_t n, float* sumsq_out, int accumulate, float* workspace, vaw_stream stream);
/* One fused pass over flat f32 buffers: decoupled-weight-decay Adam, then EMA, then the bf16 shadow copy.
 *   g' = g * gscale, gscale = clip_max_norm>0 ? min(1, clip_max_norm/(sqrt(*sumsq)+1e-6)) : 1
 *   p *= 1 - lr*wd ; m += (g'-m)(1-b1) ; v = b2 v + (1-b2) g'^2
 *   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
 *   ema = ema*decay + p*(1-decay)   (if ema != NULL)
 *   shadow = bf16(p)                (if shadow != NULL)
 *   g = 0                           (if zero_grad)
 * bc1 = 1-b1^step, bc2 = 1-b2^step are computed on the host. */
int vaw_adamw_ema_step(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2,
                       float ema_decay, const float* sumsq, float clip_max_norm, int zero_grad, vaw_stream stream);
/* Same update with the step-dependent scalars read from DEVICE memory -- hyper = f32[3] {lr, bc1, bc2} -- so the launch
 * carries no per-step host value and a captured hipGraph of the whole training step can be replayed while the LR
 * schedule (LambdaLR, utils.py:75-90) and the bias corrections advance (the host refreshes hyper before each replay). */
int vaw_adamw_ema_step_dev(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                           const float* hyper, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                           const float* sumsq, float clip_max_norm, int zero_grad, vaw_stream stream);

/* ---- step guard (guard.py: StepGuard; FusedAdamW.attach_guard) -----------------------------------------------------------------
 * The device refuses an optimizer step whose gradient is not finite, or whose norm jumps above a running mean, before the update
 * touches the masters, the moments, the EMA or the shadow.  No host value is read or produced: the launches can be captured.
 *
 * vaw_step_guard: one thread reads sumsq[0] (vaw_sumsq of the step's flat gradient) and writes the verdict.  IEEE f64, every
 * operation rounded on its own:
 *   norm = sqrt((double)sumsq[0]);  finite = isfinite(sumsq[0])
 *   spike = finite && spike_factor > 0 && applied >= spike_warmup && norm > spike_factor * mean
 *   ok = finite && !spike
 *   ok:      mean = applied == 0 ? norm : spike_beta * mean + (1 - spike_beta) * norm;  max_norm = max(max_norm, norm);
 *            applied += 1;  in_a_row = 0
 *   not ok:  skipped_nonfinite += 1 (not finite) or skipped_spike += 1;  in_a_row += 1
 *   always:  steps += 1;  last_norm = norm
 * counters: int32 [VAW_GUARD_COUNTERS] = {ok, steps, applied, skipped_nonfinite, skipped_spike, in_a_row};
 * stats: f64 [VAW_GUARD_STATS] = {last_norm, mean, max_norm, 0}.  spike_factor <= 0: no spike test; otherwise it must be > 1;
 * spike_beta in [0, 1); spike_warmup >= 0 (VAW_ERR_INVALID otherwise). */
#define VAW_GUARD_COUNTERS 6
#define VAW_GUARD_STATS 4
int vaw_step_guard(const float* sumsq, int32_t* counters, double* stats, float spike_factor, double spike_beta, int spike_warmup,
                   vaw_stream stream);
/* vaw_adamw_ema_step / _dev behind the verdict ok[0] (device int32, counters[0] of vaw_step_guard).  ok[0] != 0: bitwise the
 * unguarded call on every stream.  ok[0] == 0: nothing is read or written except g = 0 when zero_grad.  The branch is uniform
 * across the grid; the pass is the same device text as the unguarded kernel's. */
int vaw_adamw_ema_step_guarded(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2,
                               float ema_decay, const float* sumsq, float clip_max_norm, int zero_grad, const int32_t* ok,
                               vaw_stream stream);
int vaw_adamw_ema_step_guarded_dev(float* p, float* g, float* m, float* v, float* ema, void* shadow_bf16, int64_t n,
                                   const float* hyper, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                                   const float* sumsq, float clip_max_norm, int zero_grad, const int32_t* ok, vaw_stream stream);
/* ema = ema*decay + src*(1-decay) over n f32 (buffers that are not optimizer-owned, e.g. frozen pos_embed) */
int vaw_ema_update(float* ema, const float* src, int64_t n, float decay, vaw_stream stream);
/* dst(bf16) = src(f32) */
int vaw_cast_bf16(const float* src, void* dst, int64_t n, vaw_stream stream);
/* dst (bf16 [M][N], row stride ld_dst) = src (f32, row stride ld_src) and colsum[n] = beta * colsum[n] + sum_m float(dst[m][n])
 * in ONE pass: bitwise what vaw_cast_bf16 followed by vaw_colsum over dst gives.  Covers M <= 512 (one row block of the column
 * sums' tree), N, ld_src, ld_dst multiples of 4, src and dst 16-byte aligned; anything else is refused with VAW_ERR_INVALID before
 * anything is launched, and the caller keeps the two-step sequence.  vaw_cast_colsum_plan is the host side alone. */
typedef struct {
    int grid_x, block;          /* one workgroup per 256 columns */
    int rows_per_lane;          /* rows a lane walks: ceil(M / 4) */
    int64_t bytes_read, bytes_written;
} vaw_cast_colsum_launch;
int vaw_cast_colsum_plan(int64_t M, int64_t N, int64_t ld_src, int64_t ld_dst, int64_t src_addr, int64_t dst_addr,
                         int64_t colsum_addr, vaw_cast_colsum_launch* out);
int vaw_cast_colsum_bf16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t M, int64_t N, float* colsum,
                         float beta, vaw_stream stream);
/* dst[i] = scale * float(src[i]), src bf16: the way back of a gradient bucket that was all-reduced in bf16 over xGMI
 * (the reference's DDP reduces f32 buckets, main.py:347-348; bf16 halves the bytes on the wire); scale = 1/world when the
 * collective summed.  src and dst 16-byte aligned. */
int vaw_uncast_bf16(const void* src, float* dst, int64_t n, float scale, vaw_stream stream);

/* ---- post-hoc EMA (ema.py: PowerEMA, posthoc_ema; Karras et al. 2024, section 3) ---------------------------------------------
 * Up to VAW_EMA_MAX_PROFILES power-function averages of one flat f32 parameter buffer, tracked every step.  Update number
 * t = 1, 2, ... of the profile with exponent gamma takes e <- e + (p - e) c_t, c_t = 1 - (1 - 1/t)^(gamma + 1). */
#define VAW_EMA_MAX_PROFILES 4
/* step_dev[0] += 1 (that is t), then coef_dev[k] = c_t of gamma_dev[k] for k < K in f64, as -expm1((gamma + 1) log1p(-1/t)):
 * no cancellation at large t, and exactly 1 at t = 1.  One tiny launch that reads nothing from the host, so it and the update
 * below replay from a captured hipGraph while t advances.  K outside 1 .. VAW_EMA_MAX_PROFILES or a NULL pointer is refused. */
int vaw_ema_profiles_coef(int64_t* step_dev, const double* gamma_dev, double* coef_dev, int K, vaw_stream stream);
/* One pass over n f32: p is read once, each of the K average buffers e0 .. e{K-1} is read and written once ((4 + 8 K) B per
 * parameter).  Per element and profile, with c = (float)coef_dev[k]:  e = c == 1 ? p : e + (p - e) * c, every operation rounded
 * on its own -- bitwise the f32 tensor composition e.add((p - e).mul(c)), and an exact copy at t = 1.
 * Refused with VAW_ERR_INVALID before anything is launched: n <= 0, K outside 1 .. VAW_EMA_MAX_PROFILES, a NULL p / coef_dev /
 * e_k with k < K, a buffer that is not 16-byte aligned, any two of the K + 1 ranges of n floats overlapping.  e_k with k >= K
 * is ignored. */
int vaw_ema_profiles_update(const float* p, float* e0, float* e1, float* e2, float* e3, int K, int64_t n, const double* coef_dev,
                            vaw_stream stream);
/* acc[i] += coef * (double)src[i] over n elements, the product and the sum rounded separately: folding snapshots one call at a
 * time in a given order is bitwise numpy's `acc += coef * src.astype(np.float64)` in that order, with 12 B per parameter resident
 * however many are folded.  16-byte accesses when acc and src are 16-byte aligned, element accesses otherwise.  n <= 0, a NULL
 * pointer or overlapping ranges are refused. */
int vaw_lincomb_accum_f64(double* acc, const float* src, double coef, int64_t n, vaw_stream stream);
/* out[i] = (float)acc[i] (round to nearest even) over n elements; same refusals. */
int vaw_f64_to_f32(const double* acc, float* out, int64_t n, vaw_stream stream);

/* ---- activation workspace of the DiT engine (dit.py: _Workspace) -------------------------------------------------------------
 * The one place the engine's buffer sizes are decided (pure host arithmetic: no device call, so it can be asked without a GPU).
 * dtype = the act dtype; B images of T tokens (M = B * T rows), hidden D, MLP width Dm, `depth` blocks, `heads` heads, patch
 * embedding K = Kp, final layer N = No.  defer_wgrad: the caller wants the blocks' weight gradients as grouped launches (granted
 * for bf16 with M % 64 == 0: own_dy says so).  checkpoint = 0: every block keeps a record of its own from forward to backward.
 * checkpoint = 1 (activation recomputation): a block keeps only its input row of the f32 residual stream; ONE record is shared by
 * all blocks, refilled by re-running a block's forward right before its backward.
 *   one record = the act-dtype rows xm, qkv, ao, y1, xm2, hpre, a, y2 ((8 D + 2 Dm) per token), lse and the four LayerNorm
 *   statistics rows (f32), and with own_dy the dy operands dy2, dDm, dy1, dqkv ((5 D + Dm) per token) of the grouped launch.
 * VAW_ERR_INVALID (with a message) for a dtype other than VAW_F32 / VAW_BF16, a size <= 0, D % heads != 0 or a flag not 0 / 1. */
typedef struct {
    int records;                /* block records allocated: depth, or 1 with checkpoint */
    int colsum_sets;            /* sets of bias-gradient partial buffers: depth, or 1 with checkpoint (a block folds its own before the next runs) */
    int own_dy;                 /* 1: a record carries its four dy operands (grouped weight gradients) */
    int Bk;                     /* batch rows of the conditioning path's GEMM operands: B, for bf16 padded to the next multiple of 64 */
    int64_t block_bytes;        /* [M, *] rows ONE block keeps resident from its forward to its backward (x depth): its record's
                                 * rows + both of its residual-stream rows, or with checkpoint the input row alone (4 D per token) */
    int64_t block_stat_bytes;   /* the lse and statistics rows ONE block keeps (0 with checkpoint) */
    int64_t shared_bytes;       /* checkpoint: the shared record, its xres_mid row and the scratch row fc2's residual output goes to
                                 * when a block is recomputed; 0 otherwise */
    int64_t colsum_bytes;       /* all sets of partial column sums */
    int64_t scratch_bytes;      /* backward scratch shared by all blocks (with checkpoint and own_dy: without dDm, dqkv, dyb --
                                 * the shared record's dy operands serve) */
    int64_t cond_bytes;         /* conditioning path, patch embedding, final layer and the last residual-stream row */
    int64_t total;              /* depth * (block_bytes + block_stat_bytes) + shared + colsum + scratch + cond */
} vaw_dit_ws_plan_t;
int vaw_dit_ws_plan(int dtype, int B, int T, int D, int Dm, int depth, int heads, int Kp, int No, int defer_wgrad, int checkpoint,
                    vaw_dit_ws_plan_t* out);

/* ---- gradient-bucket collectives straight on RCCL ------------------------------------------------
 * Replaces the bucket all-reduce torch DDP does for the reference (main.py:347; process group set up in tools/dist_util.py:55).
 * One communicator per process (= per GPU) with a side HIP stream of its own; RCCL is opened with dlopen at the first call
 * (VAW_ERR_UNSUPPORTED when the box has none), so the rest of the library never depends on it.
 *   vaw_comm_unique_id(out)           rank 0: 128 opaque bytes to hand to every rank by any host channel
 *   vaw_comm_init(id, rank, world)    every rank (collective); vaw_comm_world() = 0 before it; vaw_comm_destroy() ends it
 *   vaw_allreduce_bucket_start        buf[0..count) <- MEAN over ranks, in place, ordered behind everything enqueued on `stream`
 *   vaw_reduce_scatter_bucket_start   rank r's chunk (count/world elements at buf + r*chunk) <- mean of that chunk (ZeRO-1 form)
 *   vaw_allgather_bucket_start        every rank's chunk of buf -> all ranks, in place
 *   vaw_allreduce_bucket_wait         `stream` waits for every collective started so far; the host never blocks
 * dt = VAW_F32 or VAW_BF16 (the wire type).  Not capturable into a hipGraph. */
int vaw_comm_unique_id(void* out128);
int vaw_comm_init(const void* id128, int rank, int world);
int vaw_comm_world(void);
int vaw_comm_destroy(void);
int vaw_allreduce_bucket_start(void* buf, int64_t count, vaw_dtype dt, vaw_stream stream);
int vaw_reduce_scatter_bucket_start(void* buf, int64_t count, vaw_dtype dt, vaw_stream stream);
int vaw_allgather_bucket_start(void* buf, int64_t count, vaw_dtype dt, vaw_stream stream);
int vaw_allreduce_bucket_wait(vaw_stream stream);

/* ---- debug and measurement switches ------------------------------------------------------------------------------------------
 * Process-wide state for tests, golden generators and the benchmarks under tools/: no training or sampling path sets them. */
/* on != 0: every attention call takes the row-wise kernels, whatever the shape (vaw_attn_plan answers accordingly) */
void vaw_debug_force_rowwise_attention(int on);
/* on != 0: every vaw_gemm call takes the generic kernel (vaw_gemm_knobs.force_generic) */
void vaw_debug_force_generic_gemm(int on);
/* the GEMM kernel family vaw_gemm_plan prefers wherever it applies (vaw_gemm_knobs.tile); -1: by shape */
void vaw_debug_gemm_tile(int mode);
/* GroupNorm: -1 the flat kernels by shape, 0 never, 1 wherever they can run (vaw_gn_plan) */
void vaw_debug_gn_flat(int mode);
/* n_wgs (1 ... 256) workgroups that each hold a whole CU idle for `microseconds` (<= 2 s) on `stream`: a stand-in for a collective
 * kernel beside the compute kernels (tools/contention_bench.py) */
int vaw_debug_cu_hog(int n_wgs, int microseconds, vaw_stream stream);
/* The pinned staging buffers of the descriptor-table uploads (upload != 0 above), process-wide: how many were ever allocated, their
 * bytes, and how many of them a stream capture holds for good (the others are recycled).  Any pointer may be NULL.  For tests. */
void vaw_debug_upload_table_stats(int64_t* buffers, int64_t* bytes, int64_t* captured);

#ifdef __cplusplus
}
#endif
#endif /* VAW_HIP_H */
