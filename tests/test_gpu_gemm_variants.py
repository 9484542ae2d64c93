"""Every row of tests/gemm_cases.py on the GPU (tests/gemm_harness.py): the call must record exactly the variant the
row names (ops.gemm_last_plan), meet the bounds of tests/test_gpu_nn.py against torch float64, leave the NaN / sentinel
frames around its operands as the contract says, give the same bits twice and exactly twice the result under
accumulate.  float32 torch on the CPU is held to the same bounds first: a row whose inputs cannot meet a bound fails
as such, not as a kernel error.  Each row prints its worst error as a fraction of its bound."""
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_gemm_variant(gpu, name):
    from idiaptts_amd import ops
    from gemm_harness import run_case
    c = gc.BY_NAME[name]
    res = run_case(c, gpu, ops)
    print("{}: plan {}".format(name, res.plan))
    print("{}: error / bound {}".format(name, ", ".join(
        "{} {:.3f} (float32 torch {:.3f})".format(k, kernel, cpu) for k, (kernel, cpu) in res.figures.items())))
    assert res.plan == c.expect, (name, "recorded", res.plan, "the row names", c.expect)
    for k, (kernel, cpu) in res.figures.items():
        assert cpu < 1.0, (name, k, "float32 torch misses the bound on these inputs", cpu)
        assert kernel < 1.0, (name, k, "error / bound", kernel)
