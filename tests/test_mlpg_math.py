"""csrc/mlpg_math.h on the host: the precision matrix, the right-hand side, the Cholesky step, the settle test and the
tail factors every MLPG form is built from, compiled by the host compiler without contraction (and once more under
AddressSanitizer and UBSan), solved as the kernels solve -- shared factor,
re-derived last two frames, two sweeps -- and compared with a dense solve of MLPG.generation's system (mlpg.py:94-127)
that tests/native/mlpg_math_check.cpp writes out without the header.

Tolerance.  Two fp64 eliminations of a system whose pivots span 1e-11 .. 1e2 do not agree to the last bit; how far apart
two correct ones are is measured, not guessed: on these cases the dense solve and the committed oracle (oracle/c, a
banded Cholesky in bandmat's order) differ by 1.036e-15 of the trajectory's largest value at the most
(DENSE_VS_ORACLE).  The header's solve gets ten times that against the dense solve; it measured 1.423e-15.  The two
references are held to the same ten times against each other, so that a drift of either shows here and not as a
failure of the header.
"""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mlpg_math_check.cpp")
LENGTHS = (1, 2, 3, 4, 5, 24, 25)
DENSE_VS_ORACLE = 1.036e-15


def _cases():
    rng = np.random.default_rng(20260)
    return [(T, rng.uniform(0.01, 1.0, size=3), rng.normal(size=(T, 3))) for T in LENGTHS for _ in range(4)]


def _run(exe, cases):
    lines = [str(len(cases))]
    for T, var, mean in cases:
        lines.append("{} {!r} {!r} {!r}".format(T, *map(float, var)))
        lines.extend(" ".join(repr(float(x)) for x in row) for row in mean)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, stdout=subprocess.PIPE, text=True).stdout
    return [json.loads(line) for line in out.splitlines()]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_header_solve_matches_dense_solve(tmp_path):
    from oracle import capi
    cases = _cases()
    exe = str(tmp_path / "mlpg_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC], check=True)
    got = _run(exe, cases)
    assert [g["T"] for g in got] == [c[0] for c in cases]
    worst_ref = worst = 0.0
    for (T, var, mean), g in zip(cases, got):
        ref = capi.mlpg(mean, var, 1)[:, 0]
        worst_ref = max(worst_ref, _rel(g["dense"], ref))
        worst = max(worst, _rel(g["header"], g["dense"]))
    print("dense vs oracle {:.3e}, header vs dense {:.3e}".format(worst_ref, worst))
    assert worst_ref <= 10 * DENSE_VS_ORACLE, worst_ref
    assert worst <= 10 * DENSE_VS_ORACLE, worst

    # the same program under the sanitizers: no report (a report ends the run with an error), same numbers
    san = str(tmp_path / "mlpg_math_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", san, SRC], check=True)
    assert _run(san, cases) == got
