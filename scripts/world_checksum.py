"""Prints SHA-1 digests of the WORLD kernels' raw fp64 outputs on fixed synthetic audio -- used to
check that a kernel restructuring (e.g. the LDS FFT's stage fusion) is bit-identical.
usage: python3 scripts/world_checksum.py [arrays.npz]      (the file keeps the F0 arrays, to compare where a
digest differs)"""
import hashlib
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from idiaptts_amd import ops, world
from idiaptts_amd.bench_support import make_audio_batch

kept = {}


def digest(t, keep=None):
    a = t.detach().cpu().numpy()
    if keep:
        kept[keep] = a
    return hashlib.sha1(a.tobytes()).hexdigest()[:16]


def stonemask_own_contour(xu, fs):
    """StoneMask on a caller's contour with frames in (40, 70] Hz, which DIO never gives (its floor is 71 Hz) and
    which take the launch with the long LDS blocks: the contour of tests/test_gpu_world.py."""
    T = world.num_frames(len(xu), fs, 5.0)
    f0 = np.random.default_rng(11).choice([0.0, 30.0, 41.0, 47.5, 55.0, 69.9, 70.0, 70.1, 95.0, 180.0, fs / 12.0 + 1.0],
                                          size=T)
    return ops.stonemask(torch.from_numpy(np.ascontiguousarray(xu)).to(dev), [0, len(xu)],
                         torch.from_numpy(f0).to(dev), [0, T], fs)


dev = torch.device("cuda")
for fs in (16000, 48000):
    raws = make_audio_batch(3, fs, seed=3, min_s=0.5, max_s=1.5)
    x_off = world.offsets([len(r) for r in raws])
    f_off = world.offsets([world.num_frames(len(r), fs, 5.0) for r in raws])
    x = torch.from_numpy(np.concatenate(raws)).to(dev)
    f0 = ops.stonemask(x, x_off, ops.dio(x, x_off, f_off, fs), f_off, fs)
    sp, mc, it = ops.cheaptrick_mcep(x, x_off, f0, f_off, fs, order=59, alpha=0.41 if fs == 16000 else 0.554,
                                     mc_dtype=torch.float64, want_iters=True)
    ap, bap = ops.d4c(x, x_off, f0, f_off, fs, want_bap=torch.float64)
    y, _ = ops.world_synthesize(f0, sp, ap, f_off, fs, dtype=torch.float64)
    pw = ops.mgc2sp(mc, 0.41 if fs == 16000 else 0.554, (sp.shape[1] - 1) * 2, want_pow=True)
    print(fs, "f0", digest(f0, "f0_%d" % fs), "sp", digest(sp), "mc", digest(mc), "it", digest(it), "ap", digest(ap),
          "y", digest(y), "pw", digest(pw))
    print(fs, "stonemask, own contour", digest(stonemask_own_contour(raws[0], fs), "sm_%d" % fs))
    if fs == 16000:
        xh = torch.from_numpy(raws[0]).to(dev)
        fh, st = ops.harvest(xh, [0, len(raws[0])], [0, ops.harvest_num_frames(len(raws[0]), fs)], fs, stages=True)
        print(fs, "harvest f0", digest(fh, "hv_f0"), " ".join("%s %s" % (k, digest(v, "hv_" + k)) for k, v in st.items()))

# 88.2 kHz: a long LDS block is past 80 KB, one wave per workgroup (the case of tests/test_gpu_world.py)
from test_gpu_world import _synthetic
print(88200, "stonemask, own contour", digest(stonemask_own_contour(_synthetic(88200, 0.6, 5), 88200), "sm_88200"))
if len(sys.argv) > 1:
    np.savez(sys.argv[1], **kept)
