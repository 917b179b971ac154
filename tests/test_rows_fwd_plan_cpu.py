"""Host plan of vaw_gate_resid_ln_modulate_fwd (vaw_row_plan, kind VAW_ROW_GATE_LN_FWD: host arithmetic, no GPU): swept over the D,
T and B grid of test_host_cpu.py::test_row_plan_sweep_*, the launch stays inside the kernel's launch bounds and the CU's LDS, every
unsupported call is refused by the plan (so before any launch), the existing row kinds and variants kept their values, and the
entry point is declared, exported and bound."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO

import vaw_amd
from vaw_amd import _lib as L
from vaw_amd.ops import row_plan

ROW_LDS_MAX = 160 * 1024          # gfx950: LDS per CU
LAUNCH_BOUND = 256                # __launch_bounds__ of gate_resid_ln_fwd_kernel (layernorm.hip)


def test_plan_sweep_stays_inside_launch_bounds_and_lds():
    for D in range(4, 2049, 4):
        nv = -(-D // 256)
        for T in (1, 7, 8, 9, 64, 100, 256, 1024):
            for B in (1, 2, 32, 128, 256, 300):
                p = row_plan(L.ROW_GATE_LN_FWD, L.BF16, B, T, D, ldx=6 * D)
                where = f"B={B} T={T} D={D}"
                assert p.variant == L.RV_GATE_LN_FWD and p.nv == (nv if nv <= 6 else 8) and p.nv * 256 >= D, where
                assert 64 <= p.block <= LAUNCH_BOUND and p.block % 64 == 0, where
                assert 0 <= p.lds_bytes <= ROW_LDS_MAX and p.workspace_floats == 0, where
                assert p.grid_x >= 1 and p.grid_x * (p.block // 64) >= B * T, where      # one wave per row before the launcher's cap
                assert p.nc == 1 and p.rows_per_chunk == T, where


def test_plan_refuses_what_the_kernel_does_not_cover():
    ok = dict(dt=L.BF16, B=2, T=8, D=64, ldx=6 * 64, base_addr=0x10000)
    row_plan(L.ROW_GATE_LN_FWD, ok["dt"], ok["B"], ok["T"], ok["D"], ldx=ok["ldx"], base_addr=ok["base_addr"])
    for change, word in ((dict(D=62), "D%4"), (dict(D=2052), "D<=2048"), (dict(D=0), "D%4"), (dict(B=0), "D%4"), (dict(dt=L.F32), "bf16"),
                         (dict(dt=L.FP8), "bf16"), (dict(base_addr=0x10008), "16-byte"), (dict(base_addr=0x10002), "16-byte"),
                         (dict(ldx=6 * 64 + 2), "multiples of 4"), (dict(ldx=-4), "multiples of 4")):
        a = dict(ok, **change)
        with pytest.raises(vaw_amd.VawError, match=re.escape(word)):
            row_plan(L.ROW_GATE_LN_FWD, a["dt"], a["B"], a["T"], a["D"], ldx=a["ldx"], base_addr=a["base_addr"])
    with pytest.raises(vaw_amd.VawError, match="bad kind"):
        row_plan(L.ROW_GATE_LN_FWD + 1, L.BF16, 2, 8, 64)


def test_new_kind_and_variant_sit_at_the_end_of_their_lists():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    kinds = dict((k, int(v)) for k, v in re.findall(r"\b(VAW_ROW_[A-Z0-9_]+) = (\d+)", hdr))
    variants = dict((k, int(v)) for k, v in re.findall(r"\b(VAW_RV_[A-Z0-9_]+) = (\d+)", hdr))
    assert kinds["VAW_ROW_GATE_LN_FWD"] == max(kinds.values()) == L.ROW_GATE_LN_FWD == 8
    assert variants["VAW_RV_GATE_LN_FWD"] == max(variants.values()) == L.RV_GATE_LN_FWD == 8
    # the values recorded plans and earlier callers use did not move
    assert [kinds[k] for k in ("VAW_ROW_LN_FWD", "VAW_ROW_LN_FWD_FP8", "VAW_ROW_LN_BWD", "VAW_ROW_GATE_BWD", "VAW_ROW_GATE_BWD_FP8",
                               "VAW_ROW_LN_BWD_GATE", "VAW_ROW_LN_BWD_GATE_FP8", "VAW_ROW_COLSUM")] == list(range(8))
    assert (L.ROW_LN_FWD, L.ROW_COLSUM, L.RV_LN_FWD, L.RV_ROW_FUSE8, L.RV_COLSUM_SCALAR) == (0, 7, 0, 4, 7)
    assert sorted(kinds.values()) == list(range(9)) and sorted(variants.values()) == list(range(9))


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vaw_hip.h")).read()
    m = re.search(r"int vaw_gate_resid_ln_modulate_fwd\(([^;]*)\);", hdr)
    assert m, "include/vaw_hip.h does not declare vaw_gate_resid_ln_modulate_fwd"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 17 and params[0] == "vaw_dtype dt" and params[-1] == "vaw_stream stream"
    lib = vaw_amd.lib()
    assert hasattr(lib, "vaw_gate_resid_ln_modulate_fwd") and "vaw_gate_resid_ln_modulate_fwd" in vaw_amd.exported_symbols()
    fn = lib.vaw_gate_resid_ln_modulate_fwd
    _p, _i, _l, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert list(fn.argtypes) == [_i, _p, _p, _l, _p, _p, _p, _p, _l, _p, _p, _p, _i, _i, _i, _f, _p] and fn.restype is _i
    assert L.ROWS_FWD_FUSED is (os.environ.get("VAW_ROWS_FWD_FUSED", "1") != "0")


def test_entry_point_refuses_before_touching_the_gpu():
    """No GPU here: a refused call returns VAW_ERR_INVALID from the plan; it never reaches the occupancy query or a launch."""
    f = vaw_amd.lib().vaw_gate_resid_ln_modulate_fwd
    a = 0x7f0000000000
    for dt, D, y in ((L.BF16, 62, a), (L.F32, 64, a), (L.BF16, 64, a + 8)):
        assert f(dt, y, a, 384, a, a + 0x100000, a, a, 384, a, a, a, 2, 8, D, 1e-6, None) == -1
        assert vaw_amd.lib().vaw_last_error_string()
    assert f(L.BF16, a, a, 384, a, a, a, a, 384, a, a, a, 2, 8, 64, 1e-6, None) == -1          # x_out must not be x_in
    assert f(L.BF16, None, a, 384, a, a + 0x100000, a, a, 384, a, a, a, 2, 8, 64, 1e-6, None) == -1


def test_rounding_query_follows_the_gemm_plan_of_the_gated_launch():
    """vaw_gate_resid_fwd_contracts: 1 exactly where vaw_gemm_plan gives proj's gated launch of these rows to the persistent kernel."""
    from vaw_amd import ops
    lib = vaw_amd.lib()
    for B, T, D in ((8, 64, 768), (2, 64, 256), (32, 64, 768), (129, 64, 768), (256, 64, 768), (128, 256, 1152), (8, 16, 64), (3, 7, 260)):
        M = B * T
        p = ops.gemm_plan(L.BF16, 1, 1, M, D, D, 0x1000, D, 0x1000, D, 0x1000, D, bias=0x1000, aux_out=0x1000, gate=0x1000, gate_ld=6 * D,
                          resid=0x1000, rows_per_batch=T, out_f32=True, check_status=False)
        want = p.status == 0 and p.variant == L.GV_PERSISTENT and p.epi_kind == L.P8_GATE and p.split == 1
        assert lib.vaw_gate_resid_fwd_contracts(B, T, D) == int(want), (B, T, D)
    assert lib.vaw_gate_resid_fwd_contracts(8, 64, 768) == 0 and lib.vaw_gate_resid_fwd_contracts(256, 64, 768) == 1
    assert lib.vaw_gate_resid_fwd_contracts(0, 64, 768) == 0
