"""Writes tests/golden/rk45.npz and tests/golden/RK45.md: the float64 oracle of flow_ode_sample(solver="rk45").

    python tests/golden/make_rk45_goldens.py

Per case of tests/rk45_cases.py (path x mean type x shape): the inputs, the final state of
scipy.integrate.solve_ivp(method="RK45", rtol=1e-4, atol=1e-5) over the stand-in written in float64 numpy, its nfev, its
attempt count (nfev - 2) / 6 and its accepted steps -- and `dist`, the largest |difference| of the package's float32 tensor
composition (fused=False, CPU) from that state, which the tests take their bounds from.  numpy + scipy compute the oracle;
torch draws the inputs and runs the composition."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import scipy

import rk45_cases as rc
import vaw_amd


def main():
    data, lines = {}, []
    for case in rc.CASES:
        path, mean, shape = case
        x0, y = rc.inputs(shape)
        final, nfev, attempts, accepted = rc.scipy_run(path, mean, x0, y)
        fm = rc.flow(path, mean)
        got = vaw_amd.flow_ode_sample(fm, rc.standin, x0, solver="rk45", rtol=rc.RTOL, atol=rc.ATOL, fused=False, y=y)
        st = fm.last_ode_stats
        assert (st["accepted"], st["accepted"] + st["rejected"]) == (accepted, attempts), (case, st, accepted, attempts)
        dist = float(np.abs(got.double().numpy() - final).max())
        norms = [n for _, _, n in st["trace"]]
        cid = rc.case_id(case)
        data.update({f"{cid}/x0": x0.numpy(), f"{cid}/y": y.numpy(), f"{cid}/final": final, f"{cid}/nfev": np.int64(nfev),
                     f"{cid}/attempts": np.int64(attempts), f"{cid}/accepted": np.int64(accepted), f"{cid}/dist": np.float64(dist)})
        lines.append(f"| {cid} | {accepted} + {attempts - accepted} | {nfev} | {dist:.1e} | "
                     f"{max(n for n in norms if n < 1):.2f} / {min([n for n in norms if n >= 1], default=float('nan')):.2f} |")
    np.savez(os.path.join(HERE, "rk45.npz"), **data)
    with open(os.path.join(HERE, "RK45.md"), "w") as f:
        f.write("# rk45.npz\n\n"
                f"Written by `make_rk45_goldens.py` (numpy {np.__version__}, scipy {scipy.__version__}): float64\n"
                f"`solve_ivp(method=\"RK45\", rtol={rc.RTOL}, atol={rc.ATOL})` from t = 1 to 0 over the stand-in network of\n"
                "`tests/rk45_cases.py`, against which `flow_ode_sample(solver=\"rk45\")` is pinned.  `dist` is the largest\n"
                "|difference| of the float32 tensor composition (`fused=False`, CPU) from scipy's final state: measured, and the\n"
                "base of the tests' bounds (2 x on the CPU for other libm builds, 4 x for the device's tanh / sin).  The last\n"
                "column is the largest accepted and the smallest rejected error ratio of the composition: none is near 1, so a last\n"
                "bit of drift cannot flip a decision.\n\n"
                "| case | accepted + rejected | scipy nfev | dist | error ratios next to 1 |\n|---|---|---|---|---|\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
