"""Times the per-step kernels of the recurrence of one BiLSTM / BiGRU layer (no GEMMs): T steps, B rows, H
units, equal lengths (every tile active).  The persistent recurrences are switched off here
(ITTS_RNN_PERSISTENT=0): at H = 512 they would otherwise take the call.  Every figure is the median of CALLS calls
timed with stream events after one warm-up call; one JSON line per (cell, mode, T, B, H).  Only the C ABI is used,
so the same file runs against any build of the library.
usage: python3 scripts/bench_lstm_steps.py [T B H]..."""
import json
import os
import statistics
import sys

os.environ["ITTS_RNN_PERSISTENT"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from idiaptts_amd import lib as _lib, ops  # noqa: E402
from idiaptts_amd.nn.functional import PackedBatch, _iptr  # noqa: E402

CALLS = 11


def time_calls(fn):
    """median time of one call in seconds"""
    fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for start, end in events:
        start.record()
        fn()
        end.record()
    torch.cuda.synchronize()
    return statistics.median(start.elapsed_time(end) for start, end in events) * 1e-3


def bench(T, B, H):
    dev = torch.device("cuda:0")
    L = _lib.load()
    ndir = 2
    pb = PackedBatch([T] * B, T, False, dev)
    N = pb.N
    for cell, G in (("lstm", 4), ("gru", 3)):
        gin = torch.randn(N, ndir * G * H, device=dev) * 0.1
        whh = torch.randn(ndir, G * H, H, device=dev) * 0.05
        bhh = torch.zeros(ndir, G * H, device=dev)
        y = torch.empty(N, ndir * H, device=dev)
        gates = torch.empty(N, ndir * 4 * H, device=dev)
        aux1 = torch.empty(N, ndir * H, device=dev)
        aux2 = torch.zeros(N, ndir * H, device=dev)
        dy = torch.randn(N, ndir * H, device=dev)
        dg = torch.empty(N, ndir * G * H, device=dev)
        dg2 = torch.empty(N, ndir * G * H, device=dev)
        nbytes = max(L.itts_lstm_state_bytes(B, H, ndir), L.itts_gru_state_bytes(B, H, ndir))
        state = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def fwd(train):
            g, a1 = (gates, aux1) if train else (None, None)
            if cell == "lstm":
                _lib.check(L.itts_lstm_layer_fwd(_iptr(gin), _iptr(whh), None, None,
                                                 _iptr(pb.d_lengths), pb._hptr(), _iptr(pb.d_row_off),
                                                 _iptr(pb.d_rev_row), T, B, H, ndir, _iptr(y), _iptr(g),
                                                 _iptr(a1), None, None, _iptr(state),
                                                 ops._stream()), "f")
            else:
                _lib.check(L.itts_gru_layer_fwd(_iptr(gin), _iptr(whh), _iptr(bhh), None,
                                                _iptr(pb.d_lengths), pb._hptr(), _iptr(pb.d_row_off),
                                                _iptr(pb.d_rev_row), T, B, H, ndir, _iptr(y), _iptr(g),
                                                None, _iptr(state), ops._stream()), "f")

        def bwd():
            if cell == "lstm":
                _lib.check(L.itts_lstm_layer_bwd(_iptr(dy), _iptr(whh), None, _iptr(gates),
                                                 _iptr(aux1), pb._hptr(), _iptr(pb.d_row_off),
                                                 _iptr(pb.d_rev_row), T, B, H, ndir, _iptr(dg),
                                                 None, _iptr(state), ops._stream()), "b")
            else:
                _lib.check(L.itts_gru_layer_bwd(_iptr(dy), _iptr(whh), _iptr(gates),
                                                _iptr(aux2), pb._hptr(), _iptr(pb.d_row_off),
                                                _iptr(pb.d_rev_row), T, B, H, ndir, _iptr(dg),
                                                _iptr(dg2), None, _iptr(state), ops._stream()), "b")

        # fwd_train first: it fills the gates (and the LSTM's cell states) that bwd reads
        for mode, fn in (("fwd_train", lambda: fwd(True)), ("fwd_infer", lambda: fwd(False)), ("bwd", bwd)):
            dt = time_calls(fn)
            print(json.dumps({"cell": cell, "mode": mode, "T": T, "B": B, "H": H, "calls": CALLS,
                              "us_per_step": round(dt / T * 1e6, 3)}), flush=True)


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [400, 64, 512]
    if len(sizes) % 3:
        sys.exit(__doc__)
    for i in range(0, len(sizes), 3):
        bench(*sizes[i:i + 3])


if __name__ == "__main__":
    main()
