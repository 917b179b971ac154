"""ctypes binding of libvaw_hip.so (include/vaw_hip.h).  No fallback: if the library is missing,
or a call is made without a GPU tensor, this raises."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VAW_HIP_LIB") or os.path.join(_HERE, "libvaw_hip.so")   # (override: measurement builds only)

F32, BF16, FP8, BF8 = 0, 1, 2, 3
F64 = 4          # VAW_F64: output type of vaw_randn_seeded only
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}

_p, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double


class Epilogue(C.Structure):
    _fields_ = [("bias", _p), ("act", _i), ("aux_in", _p), ("aux_out", _p), ("gate", _p), ("gate_ld", _l),
                ("resid", _p), ("rowadd", _p), ("rows_per_batch", _i), ("alpha", _f), ("beta", _f), ("out_f32", _i),
                ("colsum_out", _p), ("colsum_beta", _f), ("resid_is_act", _i), ("rowsum_a_out", _p), ("rowsum_a_beta", _f),
                ("colsum_partial_out", _p), ("colsum_rows_out", C.POINTER(C.c_int64))]


class AttnDesc(C.Structure):
    _fields_ = [("B", _i), ("H", _i), ("T", _i), ("hd", _i), ("q_sb", _l), ("q_sh", _l), ("q_st", _l), ("q_sd", _l),
                ("o_sb", _l), ("o_sh", _l), ("o_st", _l), ("o_sd", _l), ("scale", _f)]


class RowLaunch(C.Structure):
    """vaw_row_launch of include/vaw_hip.h: the launch vaw_row_plan picks for a row-kernel entry point."""
    _fields_ = [("variant", _i), ("nv", _i), ("nc", _i), ("rows_per_chunk", _i), ("grid_x", _i), ("block", _i), ("lds_bytes", _l),
                ("workspace_floats", _l)]


class AttnLaunch(C.Structure):
    """vaw_attn_launch of include/vaw_hip.h: the launch vaw_attn_plan picks for an attention entry point."""
    _fields_ = [("variant", _i), ("hd_image", _i), ("launches", _i), ("grid_x", _i), ("grid_y", _i), ("block", _i), ("lds_bytes", _l),
                ("lds_cap_raised", _i), ("colsum_rows", _l), ("status", _i)]


class GnLaunch(C.Structure):
    """vaw_gn_launch of include/vaw_hip.h: the launch vaw_gn_plan picks for one streaming pass of a GroupNorm entry point."""
    _fields_ = [("variant", _i), ("rows", _i), ("nch", _i), ("nt", _i), ("rpi", _i), ("grid_x", _i), ("grid_y", _i), ("grid_z", _i),
                ("block", _i), ("lds_bytes", _l), ("workspace_floats", _l), ("off_part", _l), ("off_sums", _l), ("off_s1", _l),
                ("off_s2", _l), ("status", _i)]


class GemmKnobs(C.Structure):
    """vaw_gemm_knobs of include/vaw_hip.h: the switches and the CU count vaw_gemm_plan decides by (default_gemm_knobs())."""
    _fields_ = [(n, _i) for n in ("tile", "force_generic", "bk", "pd", "ws", "xcdsplit", "sm_max_m", "sm_wide_m", "sm_nb", "sm_stages",
                                  "ws_loaders", "epi", "debug", "p8_nt", "nt_aux", "cus")]


class GemmLaunch(C.Structure):
    """vaw_gemm_launch of include/vaw_hip.h: the launch vaw_gemm_plan picks for a vaw_gemm call."""
    _fields_ = [("variant", _i), ("ntw", _i), ("mb", _i), ("nb", _i), ("stages", _i), ("bkt", _i), ("epi_kind", _i), ("split", _i),
                ("xcd_parts", _i), ("grid_x", _i), ("grid_y", _i), ("grid_z", _i), ("block", _i), ("lds_bytes", _l), ("reduce", _i),
                ("rowsum_mode", _i), ("colsum_mode", _i), ("colsum_rows", _l), ("workspace_floats_used", _l), ("launches", _i),
                ("status", _i)]


class Conv3x3Launch(C.Structure):
    """vaw_conv3x3_launch of include/vaw_hip.h: the launch vaw_conv3x3_plan picks for a vaw_conv3x3 call."""
    _fields_ = [("variant", _i), ("ntw", _i), ("epi_kind", _i), ("transposed", _i), ("M", _l), ("N", _l), ("K", _l), ("split", _i),
                ("xcd_parts", _i), ("grid_x", _i), ("grid_y", _i), ("block", _i), ("lds_bytes", _l), ("reduce", _i), ("bias_grad", _i),
                ("colsum_mode", _i), ("colsum_rows", _l), ("workspace_floats_used", _l), ("launches", _i), ("status", _i)]


class GemmFp8Launch(C.Structure):
    """vaw_gemm_fp8_launch of include/vaw_hip.h: the launch vaw_gemm_fp8_plan picks for a vaw_gemm_fp8 call."""
    _fields_ = [("epi_kind", _i), ("a_e5m2", _i), ("c_fp8", _i), ("c_e5m2", _i), ("ntw", _i), ("tiles_m", _i), ("tiles_n", _i), ("nk", _i),
                ("split", _i), ("grid", _i), ("block", _i), ("lds_bytes", _l), ("colsum_mode", _i), ("colsum_rows", _l),
                ("workspace_floats_used", _l), ("launches", _i), ("status", _i)]


class DitWsPlan(C.Structure):
    """vaw_dit_ws_plan_t of include/vaw_hip.h: the byte sizes of the DiT engine's activation workspace."""
    _fields_ = [("records", _i), ("colsum_sets", _i), ("own_dy", _i), ("Bk", _i), ("block_bytes", _l), ("block_stat_bytes", _l),
                ("shared_bytes", _l), ("colsum_bytes", _l), ("scratch_bytes", _l), ("cond_bytes", _l), ("total", _l)]


class CastColsumLaunch(C.Structure):
    """vaw_cast_colsum_launch of include/vaw_hip.h: the launch vaw_cast_colsum_bf16 makes."""
    _fields_ = [("grid_x", _i), ("block", _i), ("rows_per_lane", _i), ("bytes_read", _l), ("bytes_written", _l)]


# vaw_attn_dir / vaw_attn_variant
ATTN_FWD, ATTN_BWD, ATTN_BWD_COLSUM = range(3)
(AV_ROWWISE, AV_FWD_T64, AV_FWD_G1, AV_FWD_G2, AV_FWD_BIG, AV_BWD_T64, AV_BWD_G1, AV_BWD_G2, AV_BWD_BIG_NT2,
 AV_BWD_BIG_NT4) = range(10)
AV_NAMES = ("rowwise", "fwd_t64", "fwd_g1", "fwd_g2", "fwd_big", "bwd_t64", "bwd_g1", "bwd_g2", "bwd_big_nt2", "bwd_big_nt4")

# vaw_gemm_variant / vaw_gemm_reduce / vaw_gemm_rowsum_mode / vaw_gemm_colsum_mode; the P8_* epilogue kinds of csrc/gemm_epi.h
GV_GENERIC, GV_T128_BK32, GV_T128_BK64, GV_RING256, GV_PERSISTENT, GV_SMALL_M, GV_PARKED_DRAIN, GV_WARP_SPEC = range(8)
GV_NAMES = ("generic", "t128_bk32", "t128_bk64", "ring256", "persistent", "small_m", "parked_drain", "warp_spec")
GR_NONE, GR_F32, GR_BF16, GR_F32_ROWSUM = range(4)
GS_NONE, GS_FUSED, GS_SEPARATE = range(3)
GC_NONE, GC_FOLD, GC_DEFERRED, GC_SEPARATE = range(4)
# vaw_conv_reduce / vaw_conv_bias_grad
CVR_NONE, CVR_F32, CVR_F32_ROWSUM, CVR_SLAB_T = range(4)
CVR_NAMES = ("CVR_NONE", "CVR_F32", "CVR_F32_ROWSUM", "CVR_SLAB_T")
CVB_NONE, CVB_FUSED, CVB_FOLD, CVB_SEPARATE = range(4)
CVB_NAMES = ("CVB_NONE", "CVB_FUSED", "CVB_FOLD", "CVB_SEPARATE")
P8_STORE, P8_GELU, P8_DGELU, P8_GATE, P8_SLAB, P8_ANY, P8_WGRAD, P8_RESID, P8_GELU_Q, P8_DGELU_Q = range(10)
P8_NAMES = ("P8_STORE", "P8_GELU", "P8_DGELU", "P8_GATE", "P8_SLAB", "P8_ANY", "P8_WGRAD", "P8_RESID", "P8_GELU_Q", "P8_DGELU_Q")

# vaw_row_kind / vaw_row_variant
RESAMPLER_MAX_T = 4096      # VAW_RESAMPLER_MAX_T

(ROW_LN_FWD, ROW_LN_FWD_FP8, ROW_LN_BWD, ROW_GATE_BWD, ROW_GATE_BWD_FP8, ROW_LN_BWD_GATE, ROW_LN_BWD_GATE_FP8, ROW_COLSUM,
 ROW_GATE_LN_FWD) = range(9)
(RV_LN_FWD, RV_ROW_BWD, RV_ROW_GATE, RV_ROW_FUSE, RV_ROW_FUSE8, RV_COLSUM_BF16X8, RV_COLSUM_VEC4, RV_COLSUM_SCALAR,
 RV_GATE_LN_FWD) = range(9)

# vaw_gn_pass / vaw_gn_variant
GN_FWD_SUMS, GN_APPLY, GN_BWD_SUMS, GN_BWD_APPLY = range(4)
GNV_QUAD, GNV_FLAT = range(2)

# name -> argtypes (every function returns int status unless noted)
_PROTOS = {
    "vaw_qsample_fwd": [_p, _p, _p, _p, _p, _i, _p, _i, _l, _p],
    "vaw_mix_rows": [_p, _p, _p, _p, _p, _i, _l, _p],
    "vaw_wmse_fwd": [_p, _p, _p, _p, _p, _p, _p, _i, _l, _p],
    "vaw_wmse_bwd": [_p, _p, _p, _p, _p, _p, _p, _p, _i, _l, _p],
    "vaw_gemm": [_i, _i, _i, _l, _l, _l, _p, _l, _p, _l, _p, _l, C.POINTER(Epilogue), _p, _l, _p],
    "vaw_gemm_uses_bf16_mfma": [_i, _l, _l, _l, _p, _l, _p, _l],
    "vaw_colsum": [_i, _p, _l, _l, _l, _p, _f, _p, _l, _p],
    "vaw_ln_modulate_fwd": [_i, _p, _p, _p, _l, _p, _p, _p, _i, _i, _i, _f, _p],
    "vaw_gate_resid_fwd_contracts": [_i, _i, _i],      # returns 1 / 0, not a status
    "vaw_gate_resid_ln_modulate_fwd": [_i, _p, _p, _l, _p, _p, _p, _p, _l, _p, _p, _p, _i, _i, _i, _f, _p],
    "vaw_ln_modulate_bwd": [_i, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _l, _i, _i, _i, _p, _l, _p],
    "vaw_gate_bwd": [_i, _p, _p, _p, _l, _p, _p, _l, _p, _i, _i, _i, _p, _l, _p],
    "vaw_reduce_rows": [_p, _l, _l, _p, _f, _p],
    "vaw_reduce_rows_batched": [_i, _p, _f, _p, _i, _p],
    "vaw_ln_modulate_bwd_gate": [_i, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _i, _i, _i, _p, _l, _p],
    "vaw_ln_modulate_bwd_gate_fp8": [_p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _l, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _p, _l, _p],
    "vaw_patchify": [_i, _p, _p, _i, _i, _i, _i, _i, _p],
    "vaw_patchify_bwd": [_p, _p, _i, _i, _i, _i, _i, _p],
    "vaw_unpatchify": [_i, _p, _p, _i, _i, _i, _i, _i, _p],
    "vaw_unpatchify_bwd": [_i, _p, _p, _i, _i, _i, _i, _i, _p],
    "vaw_timestep_embedding": [_i, _p, _p, _i, _i, _f, _p],
    "vaw_silu_fwd": [_i, _p, _p, _l, _p],
    "vaw_silu_bwd": [_p, _p, _p, _l, _p],
    "vaw_add_embedding": [_p, _p, _p, _p, _i, _i, _i, _p],
    "vaw_embedding_bwd": [_p, _p, _p, _i, _i, _i, _f, _p],
    "vaw_attn_fwd": [_i, C.POINTER(AttnDesc), _p, _p, _p, _p, _p, _p],
    "vaw_attn_bwd": [_i, C.POINTER(AttnDesc), _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "vaw_attn_bwd_colsum": [_i, C.POINTER(AttnDesc), _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.POINTER(C.c_int64), _p],
    "vaw_comm_unique_id": [_p],
    "vaw_comm_init": [_p, _i, _i],
    "vaw_comm_world": [],
    "vaw_comm_destroy": [],
    "vaw_allreduce_bucket_start": [_p, _l, _i, _p],
    "vaw_reduce_scatter_bucket_start": [_p, _l, _i, _p],
    "vaw_allgather_bucket_start": [_p, _l, _i, _p],
    "vaw_allreduce_bucket_wait": [_p],
    "vaw_groupnorm_fwd": [_i, _p, _p, _p, _p, _p, _l, _i, _p, _p, _p, _i, _i, _i, _i, _f, _p, _p],
    "vaw_groupnorm_apply": [_i, _p, _p, _p, _p, _p, _p, _p, _l, _i, _p, _i, _i, _i, _i, _p],
    "vaw_groupnorm_bwd": [_i, _p, _p, _p, _p, _p, _p, _p, _p, _l, _i, _p, _p, _p, _p, _f, _p, _p, _l, _i, _i, _i, _i, _p, _p],
    "vaw_im2col3x3": [_i, _p, _p, _i, _i, _i, _i, _p],
    "vaw_col2im3x3": [_i, _p, _p, _i, _i, _i, _i, _p],
    "vaw_conv3x3": [_i, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, C.POINTER(Epilogue), _p, _l, _p],
    "vaw_vb_fwd": [_p, _p, _p, _p, _p, _i, _i, _f, _p, _i, _l, _p],
    "vaw_vb_bwd": [_p, _p, _p, _p, _p, _i, _i, _f, _p, _p, _p, _i, _l, _p],
    "vaw_bpd_terms": [_p, _p, _l, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _l, _i, _i, _l, _p],
    "vaw_guided_sample_step": [_i, _p, _p, _p, _p, _l, _f, _p, _p, _p, _i, _i, _i, _f, _p, _p, _p, _p, _i, _l, _p],
    "vaw_cfg_combine": [_p, _p, _l, _f, _p, _i, _l, _p],
    "vaw_finish_images": [_p, _i, _p, _i, _i, _i, _i, _p],
    "vaw_edm_input": [_p, _p, _p, _i, _i, _p, _p, _p, _i, _l, _p],
    "vaw_edm_step": [_i, _i, _p, _p, _l, _f, _p, _p, _p, _i, _i, _p, _p, _p, _i, _l, _p],
    "vaw_dpm_input": [_p, _p, _i, _i, _p, _p, _i, _l, _p],
    "vaw_dpm_step": [_i, _i, _p, _p, _l, _f, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _i, _l, _p],
    "vaw_flow_step": [_i, _i, _i, _p, _p, _l, _f, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _i, _l, _p],
    "vaw_randn_seeded": [_p, _i, _p, _i, _l, _l, _i, _i, _p],
    "vaw_rk_stage": [_i, _i, _p, _p, _l, _f, _p, _p, _p, _i, _i, _p, C.POINTER(_i), C.POINTER(_f), _i, _f, _p, _p, _p, _f, _f, _p, _l, _i, _l, _p],
    "vaw_rk_scaled_sumsq": [_p, _p, _p, _p, _f, _f, _p, _l, _i, _l, _p],
    "vaw_rk_sumsq_finish": [_p, _l, _p, _p],
    "vaw_flow_logp_stage": [_i, _p, _l, _p, _p, _p, _p, _p, _i, _i, _p, _p, C.POINTER(C.c_double), _i, C.c_double, _p, _p, _p, _l, _i, _l, _p],
    "vaw_flow_logp_prior": [_p, _p, _p, _l, _i, _l, _p],
    "vaw_prior_bpd": [_p, _f, _f, _p, _i, _l, _p],
    "vaw_resampler_update": [_p, _p, _i, _i, _i, _p, _p, _p, _p],
    "vaw_resampler_draw": [_p, _p, _i, _i, C.c_double, _p, _i, _p, _p, _p, _p],
    "vaw_conv3x3_narrow": [_i, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "vaw_conv3x3_wgrad_small": [_i, _p, _p, _p, _f, _i, _i, _i, _i, _i, _p, _l, _p],
    "vaw_resample2": [_i, _p, _p, _i, _i, _i, _i, _i, _f, _p],
    "vaw_concat_channels": [_i, _p, _p, _p, _l, _i, _i, _i, _p],
    "vaw_add_inplace": [_i, _p, _p, _l, _p],
    "vaw_mul": [_i, _p, _p, _p, _l, _p],
    "vaw_subsample2": [_i, _p, _p, _i, _i, _i, _i, _i, _p],
    "vaw_dropout_pack": [_i, _p, _p, _l, _i, _p],
    "vaw_dropout_bits_fwd": [_i, _p, _p, _f, _p, _l, _p],
    "vaw_dropout_bits_bwd": [_i, _p, _p, _f, _p, _l, _p],
    "vaw_rowvec_add": [_i, _p, _p, _l, _i, _i, _i, _p],
    "vaw_rowvec_sum": [_i, _p, _p, _l, _i, _i, _i, _f, _p],
    "vaw_nchw_to_nhwc": [_i, _p, _p, _i, _i, _i, _p],
    "vaw_nhwc_to_nchw": [_i, _p, _p, _i, _i, _i, _p],
    "vaw_sumsq": [_p, _l, _p, _i, _p, _p],
    "vaw_adamw_ema_step_dev": [_p, _p, _p, _p, _p, _p, _l, _p, _f, _f, _f, _f, _f, _p, _f, _i, _p],
    "vaw_adamw_ema_step": [_p, _p, _p, _p, _p, _p, _l, _f, _f, _f, _f, _f, _f, _f, _f, _p, _f, _i, _p],
    "vaw_ema_update": [_p, _p, _l, _f, _p],
    "vaw_cast_bf16": [_p, _p, _l, _p],
    "vaw_uncast_bf16": [_p, _p, _l, _f, _p],
    "vaw_wgrad_grouped": [_i, _i, _p, _l, _f, _p, _i, _p, _l, _p],
    "vaw_fp8_quantize": [_i, _i, _p, _l, _l, _l, _p, _l, _p, _l, _p, _p, _l, _p],
    "vaw_fp8_quantize_delayed": [_i, _i, _p, _l, _l, _l, _p, _l, _p, _l, _p, _p],
    "vaw_fp8_scale_update": [_p, _l, _p],
    "vaw_fp8_quantize_delayed_batched": [_i, _p, _p, _i, _p],
    "vaw_gemm_fp8": [_i, _l, _l, _l, _p, _l, _p, _p, _l, _p, _p, _l, C.POINTER(Epilogue), _p, _i, _p, _l, _p],
    "vaw_gemm_fp8_plan": [_i, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, _l, C.POINTER(Epilogue), _l, _i, _l, _l, _i, C.POINTER(GemmFp8Launch)],
    "vaw_fp8_transpose": [_p, _l, _l, _l, _p, _l, _p],
    "vaw_ln_modulate_fwd_fp8": [_p, _p, _p, _l, _p, _p, _i, _p, _p, _i, _i, _i, _f, _p],
    "vaw_gate_bwd_fp8": [_p, _p, _p, _l, _p, _p, _i, _p, _l, _p, _i, _i, _i, _p, _l, _p],
    "vaw_row_plan": [_i, _i, _l, _l, _l, _l, _l, _l, C.POINTER(RowLaunch)],
    "vaw_attn_plan": [_i, _i, C.POINTER(AttnDesc), _l, _l, _l, _l, _l, _l, _l, C.POINTER(AttnLaunch)],
    "vaw_gn_plan": [_i, _i, _i, _i, _i, _i, C.POINTER(GnLaunch)],
    "vaw_gemm_plan": [_i, _i, _i, _l, _l, _l, _l, _l, _l, _l, _l, _l, C.POINTER(Epilogue), _l, C.POINTER(GemmKnobs), C.POINTER(GemmLaunch)],
    "vaw_conv3x3_plan": [_i, _i, _l, _l, _l, _l, _i, _i, _i, _i, _i, C.POINTER(Epilogue), _l, _l, C.POINTER(GemmKnobs), _i, C.POINTER(Conv3x3Launch)],
    "vaw_dit_ws_plan": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(DitWsPlan)],
    "vaw_latent_qsample": [_p, _p, _p, _p, _p, _p, _i, _f, _f, _p, _p, _p, _i, _l, _p],
    "vaw_wmse_fwd_t": [_p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _f, _i, _l, _p],
    "vaw_wmse_bwd_t": [_p, _p, _p, _p, _p, _p, _p, _i, _p, _f, _p, _i, _l, _p],
    "vaw_ln_modulate_bwd_cast": [_i, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _l, _i, _i, _i, _p, _l, _p, _p],
    "vaw_silu_bwd_cast": [_p, _p, _p, _p, _l, _p],
    "vaw_cast_colsum_plan": [_l, _l, _l, _l, _l, _l, _l, C.POINTER(CastColsumLaunch)],
    "vaw_cast_colsum_bf16": [_p, _l, _p, _l, _l, _l, _p, _f, _p],
    "vaw_row_sqnorms": [_p, _l, _i, _p, _p],
    "vaw_pairwise_ksmallest": [_p, _l, _p, _l, _i, _p, _p, _i, _p, _p, _l, _p],
    "vaw_ksmallest_merge": [_p, _l, _i, _i, _l, _l, _p, _p],
    "vaw_pairwise_within": [_p, _l, _p, _l, _i, _p, _p, _p, _i, _p, _i, _p, _p, _p],
    "vaw_pairwise_polysum": [_p, _l, _p, _l, _i, _p, _p, _i, _d, _d, _i, _i, _p, _p, _l, _p],
    "vaw_pairwise_count_within": [_p, _l, _p, _l, _i, _p, _p, _p, _i, _p, _p, _p, _l, _p],
    "vaw_col_mean_f64": [_p, _l, _i, _p, _p],
    "vaw_cov_f64": [_p, _l, _i, _p, _p, _p],
    "vaw_head_logits": [_p, _l, _i, _p, _i, _p, _l, _p],
    "vaw_is_rows": [_p, _l, _i, _l, _i, _p, _p, _p],
    "vaw_is_colsums": [_p, _p, _l, _i, _l, _i, _l, _l, _p, _p],
    "vaw_is_finish": [_p, _p, _l, _i, _l, _p, _p],
}

_lib = None


class VawError(RuntimeError):
    pass


def lib():
    """Load (once) and return the CDLL.  Raises if the HIP library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VawError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        for name, args in _PROTOS.items():
            if not hasattr(L, name) and os.environ.get("VAW_HIP_LIB"):
                continue          # an older measurement build behind VAW_HIP_LIB (A/B runs): entry points added since are simply absent
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _i
        L.vaw_version.restype = _i
        L.vaw_last_error_string.restype = C.c_char_p
        L.vaw_colsum_workspace_floats.argtypes = [_l, _l]
        L.vaw_colsum_workspace_floats.restype = _l
        L.vaw_row_bwd_workspace_floats.argtypes = [_i, _i, _i]
        L.vaw_row_bwd_workspace_floats.restype = _l
        L.vaw_conv3x3_wgrad_small_workspace_floats.argtypes = [_i, _i, _i, _i, _i]
        L.vaw_conv3x3_wgrad_small_workspace_floats.restype = _l
        L.vaw_groupnorm_workspace_floats.argtypes = [_i, _i, _i]
        L.vaw_groupnorm_workspace_floats.restype = _l
        if hasattr(L, "vaw_dropout_bits_words"):
            L.vaw_dropout_bits_words.argtypes = [_l]
            L.vaw_dropout_bits_words.restype = _l
        L.vaw_wgrad_grouped_desc_bytes.argtypes = [_i]
        L.vaw_wgrad_grouped_desc_bytes.restype = _l
        L.vaw_reduce_rows_batched_desc_bytes.argtypes = [_i]
        L.vaw_reduce_rows_batched_desc_bytes.restype = _l
        L.vaw_fp8_quantize_batched_desc_bytes.argtypes = [_i]
        L.vaw_fp8_quantize_batched_desc_bytes.restype = _l
        L.vaw_fp8_quantize_workspace_floats.argtypes = []
        L.vaw_fp8_quantize_workspace_floats.restype = _l
        if hasattr(L, "vaw_pairwise_workspace_bytes"):
            L.vaw_pairwise_workspace_bytes.argtypes = [_l, _l, _i]
            L.vaw_pairwise_workspace_bytes.restype = _l
        if hasattr(L, "vaw_pairwise_polysum_workspace_bytes"):
            L.vaw_pairwise_polysum_workspace_bytes.argtypes = [_l, _l, _i]
            L.vaw_pairwise_polysum_workspace_bytes.restype = _l
            L.vaw_pairwise_count_workspace_bytes.argtypes = [_l, _l, _i]
            L.vaw_pairwise_count_workspace_bytes.restype = _l
        if hasattr(L, "vaw_rk_partial_count"):
            L.vaw_rk_partial_count.argtypes = [_i, _l]
            L.vaw_rk_partial_count.restype = _l
        L.vaw_sumsq_workspace_floats.argtypes = []
        L.vaw_sumsq_workspace_floats.restype = _l
        L.vaw_debug_force_rowwise_attention.argtypes = [_i]
        L.vaw_debug_force_rowwise_attention.restype = None
        L.vaw_debug_force_generic_gemm.argtypes = [_i]
        L.vaw_debug_force_generic_gemm.restype = None
        L.vaw_debug_gemm_tile.argtypes = [_i]
        L.vaw_debug_gemm_tile.restype = None
        if hasattr(L, "vaw_gemm_default_knobs"):
            L.vaw_gemm_default_knobs.argtypes = [C.POINTER(GemmKnobs)]
            L.vaw_gemm_default_knobs.restype = None
        if hasattr(L, "vaw_debug_gn_flat"):      # absent from older measurement builds loaded through VAW_HIP_LIB
            L.vaw_debug_gn_flat.argtypes = [_i]
            L.vaw_debug_gn_flat.restype = None
        L.vaw_p8_set_reserved_cus.argtypes = [_i]
        L.vaw_p8_set_reserved_cus.restype = None
        if hasattr(L, "vaw_debug_wgrad_engine"):      # absent from older measurement builds loaded through VAW_HIP_LIB
            L.vaw_debug_wgrad_engine.argtypes = [_i]
            L.vaw_debug_wgrad_engine.restype = None
        L.vaw_debug_cu_hog.argtypes = [_i, _i, _p]
        L.vaw_debug_cu_hog.restype = _i
        _lib = L
    return _lib


def exported_symbols():
    return sorted(list(_PROTOS) + ["vaw_version", "vaw_last_error_string", "vaw_colsum_workspace_floats",
                                   "vaw_sumsq_workspace_floats", "vaw_groupnorm_workspace_floats", "vaw_wgrad_grouped_desc_bytes",
                                   "vaw_conv3x3_wgrad_small_workspace_floats", "vaw_row_bwd_workspace_floats",
                                   "vaw_fp8_quantize_workspace_floats", "vaw_p8_set_reserved_cus", "vaw_debug_wgrad_engine", "vaw_reduce_rows_batched_desc_bytes", "vaw_fp8_quantize_batched_desc_bytes",
                                   "vaw_gemm_default_knobs", "vaw_dropout_bits_words", "vaw_pairwise_workspace_bytes", "vaw_rk_partial_count",
                                   "vaw_pairwise_polysum_workspace_bytes", "vaw_pairwise_count_workspace_bytes"])


# VAW_STEP_FUSED (read once): 0 restores the step's unfused sequence of launches everywhere -- separate cast / column-sum
# passes in the DiT backward, tensor operations for the latent sample, the coefficient gathers and the batch means of the loss
STEP_FUSED = os.environ.get("VAW_STEP_FUSED", "1") != "0"
# VAW_ROWS_FWD_FUSED (read once): 0 restores the gated-residual epilogue of proj / fc2 followed by a LayerNorm launch of
# its own in the bf16 DiT block forward, in place of the plain store and vaw_gate_resid_ln_modulate_fwd
ROWS_FWD_FUSED = os.environ.get("VAW_ROWS_FWD_FUSED", "1") != "0"


def check(rc, what):
    if rc != 0:
        raise VawError(f"{what} failed ({rc}): {lib().vaw_last_error_string().decode()}")


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise VawError("vaw_amd runs on the GPU only: got a CPU tensor (no CPU fallback exists by design)")
