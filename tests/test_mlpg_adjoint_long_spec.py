"""The banded restatement of the MLPG adjoint (tests/mlpg_adjoint_long_spec.py) pinned to the dense one
(tests/mlpg_adjoint_spec.py) without a GPU: the band it builds is the upper band of the dense precision matrix, and its
adjoint is the dense adjoint to 1e-12 relative, at lengths on both sides of the last-two-frames rule, one prefetch
block, the forward's change of form and the longest utterance the dense sweep uses."""
import numpy as np
import pytest

import mlpg_adjoint_long_spec as long_spec
import mlpg_adjoint_spec as spec

PINNED_LENGTHS = (1, 2, 3, 17, 194, 300)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("kind", spec.VARIANCE_SETS)
@pytest.mark.parametrize("dim", [1, 5])
@pytest.mark.parametrize("T", PINNED_LENGTHS)
def test_banded_adjoint_equals_the_dense_restatement(T, dim, kind):
    var = spec.variances(kind, dim)
    g = np.random.RandomState(100 * T + dim).standard_normal((T, dim))
    got, ref = long_spec.adjoint(g, var, dim), spec.adjoint(g, var, dim)
    assert got.shape == ref.shape == (T, 3 * dim)
    assert _rel(got, ref) <= 1e-12
    for w in range(3):                               # and window by window, each at its own scale
        assert _rel(got[:, w * dim:(w + 1) * dim], ref[:, w * dim:(w + 1) * dim]) <= 1e-12


@pytest.mark.parametrize("kind", spec.VARIANCE_SETS)
@pytest.mark.parametrize("T", (1, 2, 3, 4, 17, 40))
def test_band_is_the_upper_band_of_the_dense_precision_matrix(T, kind):
    dim = 3
    var = spec.variances(kind, dim)
    ab, P = long_spec.band(T, var, dim), spec.precision(T, var, dim)
    for d in range(dim):
        dense = spec.upper_band(P[d])
        assert np.abs(ab[d] - dense).max() <= 4e-16 * np.abs(dense).max()
        x = np.random.RandomState(T).standard_normal(T)
        assert _rel(long_spec.band_matvec(ab[d], x), P[d] @ x) <= 1e-14


def test_empty_utterance_and_the_stream_batch_table():
    assert long_spec.adjoint(np.zeros((0, 4)), spec.variances("typical", 4), 4).shape == (0, 12)
    assert sum(long_spec.LENGTHS) == 6660 and max(long_spec.LENGTHS) == 2050
    offsets, var, gout, ref = long_spec.stream_case(2, "typical", long_spec.PLACED_LENGTHS)
    assert np.array_equal(gout.astype(np.float32).astype(np.float64), gout)          # both input types: the same gradient
    assert ref.dtype == np.float64 and ref.shape == (offsets[-1], 6) and not ref.flags.writeable
