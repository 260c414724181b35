"""The twiddle table of the packed 32768-point real transform (csrc/fft_lds.h), shared by the Auralizer (m2h/audio/render.py) and the
Scorer's alignment (m2h/audio/score.py)."""
import numpy as np

NFFT = 32768


def packed_twiddles(nfft=NFFT):
    """[2, nfft / 2, 2] fp32: exp(-2 pi i k / nfft), k < nfft / 2, interleaved, built in float64 on the host (the feeder's table at this
    length), and the same fp32 values again in the order the transform's stages read them (include/m2h.h, "Auralizer")."""
    M = nfft // 2
    k = np.arange(M, dtype=np.float64)
    t = np.stack([np.cos(2.0 * np.pi * k / nfft), -np.sin(2.0 * np.pi * k / nfft)], axis=1).astype(np.float32)
    staged = np.zeros_like(t)
    for s in range(M.bit_length() - 1):
        half = M >> (s + 1)
        staged[M - (M >> s):M - (M >> s) + half] = t[(np.arange(half) << s) * 2]
    return np.stack([t, staged])


def device_twiddles(device, nfft=NFFT):
    """packed_twiddles(nfft) on `device` (one copy from the host: callers cache the result)"""
    import torch
    return torch.from_numpy(packed_twiddles(nfft)).to(device).contiguous()
