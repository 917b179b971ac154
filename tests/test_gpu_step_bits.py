"""The reverse-step, likelihood, guidance and solver-step kernels write the bytes they wrote before they were folded onto one
per-timestep table, one per-element p_mean_variance and one loop body each: tests/golden/step_bits.json holds sha256 hashes
recorded on the MI355X from the commit before that change (tests/golden/make_step_bits.py, which also defines the cases: vector
and scalar paths, a second grid-stride trip of each, misaligned and odd-stride layouts, every mode / kind / clip / guidance
combination of the step, the variational-bound forward and backward, the EDM and flow solver steps)."""
import importlib.util
import os

import pytest

from conftest import GOLDEN, load_json

pytestmark = pytest.mark.gpu

import vaw_amd

_spec = importlib.util.spec_from_file_location("make_step_bits", os.path.join(GOLDEN, "make_step_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.mark.parametrize("group", bits.GROUPS)
def test_kernels_write_the_recorded_bits(group):
    want = {c: h for c, h in load_json("step_bits.json").items() if c.startswith(group + "/")}
    got = bits.compute(vaw_amd, group)
    assert want and set(got) == set(want), f"{group}: cases {sorted(set(got) ^ set(want))} are on one side only"
    wrong = [f"{c}:{k}" for c in sorted(want) for k in sorted(set(want[c]) | set(got[c])) if want[c].get(k) != got[c].get(k)]
    print(f"{group}: {sum(len(h) for h in want.values())} outputs of {len(want)} cases, {len(wrong)} differ")
    assert not wrong, f"{group}: other bytes than recorded in {wrong}"
