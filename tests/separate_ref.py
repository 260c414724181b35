"""CPU reference of m2h.separate (the semantics in that module's docstring), composed from the oracle as it stands: np_stft per
zero-padded segment, passive_pair, acoustic_mem, np_istft.  Helper module, no tests."""
import numpy as np
import torch

import m2h_oracle as O

SEG = 16000


def tone_noise(R, L, seed, C=2):
    """Noise (sigma 0.05) plus one tone per channel, as tests/test_gpu_stft.py: the noise floor keeps every bin of every non-empty
    frame away from zero, so the downmix phasor is well conditioned."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / 16000.0
    w = rng.standard_normal((R, C, L)) * 0.05
    for r in range(R):
        for c in range(C):
            w[r, c] += 0.3 * np.sin(2 * np.pi * rng.uniform(100, 4000) * t + rng.uniform(0, 6))
    return w.astype(np.float32)


def segments(wave):
    """[R, 2, L] -> [S, R, 2, 16000]: non-overlapping one-second segments, zeros from L on."""
    R, C, L = wave.shape
    S = -(-L // SEG)
    pad = np.zeros((R, C, S * SEG), np.float32)
    pad[:, :, :L] = wave
    return pad.reshape(R, C, S, SEG).transpose(2, 0, 1, 3)


def segment_stft(wave):
    """Complex spectra X [S, R, 2, 512, 32] of every segment on its own (np_stft: reflect padding inside the zero-padded segment)."""
    seg = segments(wave)
    S, R, C, _ = seg.shape
    X = np.zeros((S, R, C, 512, 32), np.complex64)
    for s in range(S):
        for r in range(R):
            for c in range(C):
                X[s, r, c] = O.np_stft(seg[s, r, c])
    return X


def phasor_of(X):
    """Unit phasor of the downmix D = X_left + X_right, [S, R, 512, 32] complex; 1 where |D| == 0 (np.angle(0) = 0)."""
    D = X[:, :, 0].astype(np.complex128) + X[:, :, 1].astype(np.complex128)
    return np.exp(1j * np.angle(D))


def features_of(X):
    """log1p|X| as BHWC [S, R, 512, 32, 2] float32."""
    return np.log1p(np.abs(X)).astype(np.float32).transpose(0, 1, 3, 4, 2)


def inverse(P, ph, L):
    """P [S, R, 512, 32] log1p magnitudes, ph complex unit phasors -> waveform [R, L]."""
    S, R = P.shape[:2]
    y = np.zeros((R, S * SEG), np.float32)
    for s in range(S):
        for r in range(R):
            Z = (np.expm1(np.maximum(P[s, r].astype(np.float64), 0.0)) * ph[s, r]).astype(np.complex64)
            y[r, s * SEG:(s + 1) * SEG] = O.np_istft(Z, 512, SEG)
    return y[:, :L]


def separate(sd, wave, target_class, use_memory):
    """sd: torch state dict without the "actor_critic." root (separator keys, and acoustic_mem.cnn.{0,2}.weight when use_memory).
    wave [R, 2, L] float32 numpy; target_class an int or [R].  Returns (y [R, L], P [R, S, 512, 32], phasor [R, S, 512, 32] complex)."""
    R, _, L = wave.shape
    X = segment_stft(wave)
    S = X.shape[0]
    ph = phasor_of(X)
    feats = features_of(X)
    tc = torch.as_tensor(np.broadcast_to(np.asarray(target_class, np.int64).reshape(-1), (R,)).copy()).reshape(R, 1)
    P = np.zeros((S, R, 512, 32), np.float32)
    prev = torch.zeros(R, 512, 32, 1)
    with torch.no_grad():
        for s in range(S):
            _, mono = O.passive_pair(sd, torch.from_numpy(feats[s]), tc)
            if use_memory:
                prev = O.acoustic_mem(sd, mono, prev)
                mono = prev
            P[s] = mono[..., 0].numpy()
    y = inverse(P, ph, L)
    return y, P.transpose(1, 0, 2, 3), ph.transpose(1, 0, 2, 3)


def rel_l1(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a.astype(np.complex128) - b.astype(np.complex128)).sum() / max(np.abs(b.astype(np.complex128)).sum(), 1e-30))


def torch_state_dict(shapes_seed_dict):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in shapes_seed_dict.items()}
