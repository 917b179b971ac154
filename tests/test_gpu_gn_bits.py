"""vaw_groupnorm_fwd / _apply / _bwd write the bytes they wrote before GroupNorm moved into csrc/groupnorm.hip behind vaw_gn_plan:
tests/golden/gn_bits.json holds sha256 hashes recorded on the MI355X from the commit before that change by
tests/golden/make_gn_bits.py, which also defines the cases (every variant, chunk size, switch value and flag combination)."""
import importlib.util
import os

import pytest

from conftest import GOLDEN, load_json

pytestmark = pytest.mark.gpu

import vaw_amd

_spec = importlib.util.spec_from_file_location("make_gn_bits", os.path.join(GOLDEN, "make_gn_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.mark.parametrize("group", list(bits.GROUPS))
def test_groupnorm_writes_the_recorded_bits(group):
    want = {c: h for c, h in load_json("gn_bits.json").items() if c.startswith(group + "/")}
    got = bits.compute(vaw_amd, group)
    assert want and set(got) == set(want), f"{group}: cases {sorted(set(got) ^ set(want))} are on one side only"
    wrong = [f"{c}:{k}" for c in sorted(want) for k in sorted(set(want[c]) | set(got[c])) if want[c].get(k) != got[c].get(k)]
    assert not wrong, f"{group}: other bytes than recorded in {wrong}"
