"""The wave-per-transform FFT (csrc/wave_fft.h) against the workgroup-per-transform one it replaces in
the 1024-point frame kernels (wd::fft_lds / rfft_lds / irfft_lds): same butterflies, same twiddle
entries, same order of operations -- the outputs must be IDENTICAL bit for bit on random inputs
(complex forward / inverse, real forward / inverse, at 512 and at 1 024 complex points; 8 192 / 4 096 transforms each).
Likewise the two-array form of wd::rfft_lds (two transforms in lockstep: D4C's static centroid) against the
one-array form on 256 pairs of different random arrays: 128, 256 and 2 048 real samples (the smallest swizzled
size, an odd log2 with its radix-2 tail, FFT_PAIR_MAX complex points), the last also with D4C's compile-time
sizes.  Replaces the FFTs inside
pyworld / pysptk that WorldFeatLabelGen.py:792-793, 940-943 and AudioProcessing.py:146-152, 252-255
reach.  The lab (scripts/wave_fft_lab/lab.hip) is built with hipcc on the spot; its schedule is also
checked as a computation graph, and for LDS bank conflicts, on the CPU (tests/test_wave_fft_schedule.py)."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_fft_is_bit_identical_to_the_workgroup_fft(gpu, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "wave_fft_lab")
    src = os.path.join(ROOT, "scripts", "wave_fft_lab", "lab.hip")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "-munsafe-fp-atomics",
                    "-Wno-unused-function", "-o", exe, src], check=True, stdout=subprocess.PIPE,
                   stderr=subprocess.STDOUT, timeout=600)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    rows = re.findall(r"^(\S.*?)\s*: (\d+) of (\d+) values differ", res.stdout, flags=re.M)
    assert len(rows) == 12, res.stdout          # four transforms at 512 and at 1024 complex points, four pair rows
    for name, bad, total in rows[:8]:
        assert int(bad) == 0 and int(total) >= 4096 * 1024 * 2, (name, bad, total)
    # 256 pairs x 2 arrays x (n / 2 + 1) bins x (re, im)
    pair_totals = [256 * 2 * (n // 2 + 1) * 2 for n in (128, 256, 2048, 2048)]
    for (name, bad, total), want in zip(rows[8:], pair_totals):
        assert name.startswith("rfft x 2") and int(bad) == 0 and int(total) == want, (name, bad, total, want)
