"""CPU reference of m2h.separate's binaural target (output="binaural"; the semantics in that module's docstring), composed from
tests/separate_ref.py and the oracle as it stands: np_stft per zero-padded segment, the first return value of passive_pair (the
masks of get_binSepMasks), np_istft of max(m, 0) * X per channel.  Overlapped segments are the cross-fade of
tests/separate_overlap_ref.py on k shifted recordings, each channel on its own.  Helper module, no tests."""
import numpy as np
import torch

import m2h_oracle as O
import separate_overlap_ref as OREF
import separate_ref as REF

SEG = REF.SEG


def scaled_spectrum(m, X):
    """m [512, 32] float32 (one channel's mask), X [512, 32] complex64 (that channel's spectrum) -> max(m, 0) * X as complex64."""
    return (np.maximum(m, 0) * X).astype(np.complex64)


def separate_plain(sd, wave, target_class):
    """Non-overlapping segments.  wave [R, 2, L] float32 numpy; target_class an int or [R].
    Returns (y [R, 2, L], masks [R, S, 512, 32, 2])."""
    R, _, L = wave.shape
    X = REF.segment_stft(wave)                      # [S, R, 2, 512, 32]
    S = X.shape[0]
    feats = REF.features_of(X)
    tc = torch.as_tensor(np.broadcast_to(np.asarray(target_class, np.int64).reshape(-1), (R,)).copy()).reshape(R, 1)
    masks = np.zeros((S, R, 512, 32, 2), np.float32)
    y = np.zeros((R, 2, S * SEG), np.float32)
    with torch.no_grad():
        for s in range(S):
            m, _ = O.passive_pair(sd, torch.from_numpy(feats[s]), tc)
            masks[s] = m.numpy()
            for r in range(R):
                for c in range(2):
                    y[r, c, s * SEG:(s + 1) * SEG] = O.np_istft(scaled_spectrum(masks[s, r, :, :, c], X[s, r, c]), 512, SEG)
    return y[:, :, :L], masks.transpose(1, 0, 2, 3, 4)


def separate(sd, wave, target_class, overlap=1):
    """As separate_plain with `overlap` segments over every sample: chain c is the plain path on wave[:, :, c * H:], and each channel is
    the cross-fade of its k chains.  Returns (y [R, 2, L], masks [R, S', 512, 32, 2] in segment order)."""
    assert overlap in OREF.OVERLAPS
    if overlap == 1:
        return separate_plain(sd, wave, target_class)
    L = wave.shape[2]
    H = SEG // overlap
    ys, ms = [], []
    for c in OREF.chains(L, overlap):
        y, m = separate_plain(sd, np.ascontiguousarray(wave[:, :, c * H:]), target_class)
        ys.append(y)
        ms.append(m)
    y = np.stack([OREF.crossfade([yc[:, ch] for yc in ys], L, overlap) for ch in range(2)], axis=1)
    return y, OREF.interleave(ms, L, overlap)
