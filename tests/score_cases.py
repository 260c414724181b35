"""What the GPU tests of the Scorer's two STFT kernels share (tests/test_gpu_score_spectral.py, tests/test_gpu_score_spatial.py): the batch
of R recordings and its cache of read-only inputs and references, the copies to the device, the bit-for-bit comparison, the WAV writer."""
import numpy as np
import torch

import score_ref

R = 2
LMAX = 40001
_made = {}


def recordings(key, one):
    """one(r) -> a tuple of arrays, for r < R, stacked per position; made once per key, shared and read-only"""
    if key not in _made:
        _made[key] = tuple(np.stack(a) for a in zip(*[one(r) for r in range(R)]))
        for a in _made[key]:
            a.setflags(write=False)
    return _made[key]


def batch(S, C=2, snr43=False):
    """R recordings of score_ref.inputs at LMAX samples: refs [R, S, C, L], est [R, C, L], mix [R, 2, L]"""
    return recordings(("batch", S, C, snr43), lambda r: score_ref.inputs(S, LMAX, 31 + 50 * r, C, snr43))


def targets(S):
    """a different non-zero target per recording where there is more than one reference"""
    return [1, 2] if S >= 3 else [0] * R


def _gpu(dev, *arrays):
    return [torch.tensor(np.ascontiguousarray(a)).to(dev) for a in arrays]      # (a copy: the shared inputs are read-only)


def _target(dev, tg):
    return tg[0] if len(set(tg)) == 1 else torch.tensor(tg, dtype=torch.int64).to(dev)


def _same(a, b):
    """bit for bit, NaN in the same places"""
    return a.shape == b.shape and bool(torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))) and \
        bool(torch.equal(torch.isnan(a), torch.isnan(b)))


def _write_wav(path, data):
    from scipy.io import wavfile
    wavfile.write(path, 16000, data)
