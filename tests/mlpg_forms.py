"""The MLPG forms the GPU tests force (ops.mlpg_forced), and the form each must record (ops.mlpg_last_form) -- worked
out here from the batch on its own, not with itts_mlpg_choose_form, so that a forced form the dispatcher does not
take fails the tests.  The library's own choice ("auto") is pinned by tests/test_mlpg_dispatch.py."""
from idiaptts_amd import ops
from idiaptts_amd.ops import (MLPG_F32_ROWS, MLPG_NT_IN, MLPG_RING, MLPG_STREAM, MLPG_SWEEPS, MLPG_WIDE,
                              MLPG_WIDENED_COPY)

# name -> ops.mlpg_forced arguments
FORCED = {
    "auto": {},
    "stream": {"solve": "stream"},
    "ring": {"solve": "ring", "width": "narrow"},
    "ring-wide": {"solve": "ring", "width": "wide"},
    "ring-plain": {"solve": "ring", "width": "narrow", "nt": False},
    "ring-nt": {"solve": "ring", "width": "narrow", "nt": True},
}


def expected_form(name, lengths, dim, f32):
    """The form a call over utterances of `lengths` must take under FORCED[name]."""
    lengths = [int(n) for n in lengths]
    t_max, t_total = max(lengths, default=0), sum(lengths)
    if t_total == 0:
        return 0
    f32_copy = MLPG_F32_ROWS | MLPG_WIDENED_COPY if f32 else 0
    if t_max < 194:
        return MLPG_SWEEPS | f32_copy
    if name == "auto":
        return ops.mlpg_choose_form(len(lengths), dim, t_max, t_total, f32)
    assert len(lengths) <= 65535
    if name == "stream":
        return MLPG_STREAM | f32_copy
    wide = MLPG_WIDE if name == "ring-wide" and dim % 2 == 0 else 0
    if f32:
        return MLPG_RING | MLPG_F32_ROWS | wide
    if wide:
        return MLPG_RING | MLPG_WIDE
    if name == "ring-plain":
        return MLPG_RING
    assert name == "ring-nt" or t_total * dim * 8 <= 192 << 20
    return MLPG_RING | MLPG_NT_IN


def check_form(name, lengths, dim, f32, what=""):
    got, want = ops.mlpg_last_form(), expected_form(name, lengths, dim, f32)
    assert got == want, "{}: {} ran, {} expected under {} {}".format(
        what, ops.mlpg_form_name(got), ops.mlpg_form_name(want), name, FORCED[name])
    return got
