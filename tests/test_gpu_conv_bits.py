"""vaw_conv3x3 writes the bytes it wrote before its checks and launch choices moved into vaw_conv3x3_plan: tests/golden/conv_bits.json
holds sha256 hashes recorded on the MI355X from the commit before that change by tests/golden/make_conv_bits.py, over the cases of
tests/conv_parity.py (every kernel, mode, tile width, epilogue, reduce and bias-gradient path; "declined" where the explicit path
must take the shape)."""
import importlib.util
import os

import pytest

from conftest import GOLDEN, load_json

pytestmark = pytest.mark.gpu

import vaw_amd

_spec = importlib.util.spec_from_file_location("make_conv_bits", os.path.join(GOLDEN, "make_conv_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.mark.parametrize("group", list(bits.GROUPS))
def test_conv3x3_writes_the_recorded_bits(group):
    want = {c: h for c, h in load_json("conv_bits.json").items() if c.split("_")[0] == group}
    got = bits.compute(vaw_amd, group)
    assert want and set(got) == set(want), f"{group}: cases {sorted(set(got) ^ set(want))} are on one side only"
    wrong = [c for c in sorted(want) if want[c] != got[c]]
    assert not wrong, f"{group}: other bytes than recorded in {wrong}"
