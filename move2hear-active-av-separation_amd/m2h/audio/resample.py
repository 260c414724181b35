"""Sample-rate conversion by a rational ratio: a Kaiser-windowed-sinc polyphase FIR, designed here, run by csrc/resample.hip.

Definition.  For integer rates f_in, f_out: g = gcd(f_in, f_out), up = f_out / g, down = f_in / g, half = 10 * max(up, down),
N = 2 * half + 1, and in float64
    c = 1 / max(up, down),  m = arange(N) - half,  h = c * sinc(c * m) * kaiser(N, 5.0),  h /= h.sum(),  h *= up
(np.sinc, np.kaiser).  A row x of L_in samples, zero outside [0, L_in), gives L_out = ceil(L_in * up / down) samples
    y[n] = sum_j x[j] * h[n * down - j * up + half].
This is scipy.signal.resample_poly(x, up, down, padtype="constant") with its default window ("kaiser", 5.0); scipy is not imported
here.  The kernel takes h rounded once to fp32 as the polyphase table G[p][k] = h[p + k * up] (zero past the end), [up, T] with
T = ceil(N / up): with t = n * down + half, y[n] = sum_{k < T} G[t mod up][k] * x[t div up - k].

Ratios with max(up, down) <= 1024 are accepted (a table of at most 20 481 floats).  f_in == f_out is the identity and launches nothing.
"""
import math

import numpy as np

MAX_RATIO = 1024
KAISER_BETA = 5.0


def ratio(f_in, f_out):
    """(up, down) of the reduced ratio f_out / f_in; ValueError for rates that are not positive integers or a ratio over the limit."""
    if int(f_in) != f_in or int(f_out) != f_out or f_in < 1 or f_out < 1:
        raise ValueError("m2h.resample: sample rates must be positive integers, got %r -> %r" % (f_in, f_out))
    f_in, f_out = int(f_in), int(f_out)
    g = math.gcd(f_in, f_out)
    up, down = f_out // g, f_in // g
    if max(up, down) > MAX_RATIO:
        raise ValueError("m2h.resample: %d Hz -> %d Hz is the ratio %d/%d; max(up, down) <= %d is supported" % (f_in, f_out, up, down, MAX_RATIO))
    return up, down


def design(f_in, f_out):
    """(up, down, half, h): the reduced ratio and its 2 * half + 1 taps in float64.  Needs neither a GPU nor the library."""
    up, down = ratio(f_in, f_out)
    big = max(up, down)
    half = 10 * big
    n = 2 * half + 1
    c = 1.0 / big
    m = np.arange(n, dtype=np.float64) - half
    h = c * np.sinc(c * m) * np.kaiser(n, KAISER_BETA)
    h /= h.sum()
    h *= up
    return up, down, half, h


def taps_per_output(up, down):
    return -(-(2 * 10 * max(up, down) + 1) // up)


def output_length(L, up, down):
    return -(-int(L) * up // down)


def polyphase_table(h, up):
    """h [N] -> G [up, T], G[p][k] = h[p + k * up], zero past the end."""
    T = -(-len(h) // up)
    padded = np.zeros(T * up, h.dtype)
    padded[:len(h)] = h
    return np.ascontiguousarray(padded.reshape(T, up).T)


class Resampler:
    """Resampler(f_in, f_out, device)(x): x [..., L] fp32 on the device -> [..., ceil(L * up / down)].  Holds up, down, half, taps (the
    float64 design) and the fp32 [up, T] table on the device."""

    def __init__(self, f_in, f_out, device):
        import torch
        self.f_in, self.f_out = int(f_in), int(f_out)
        self.up, self.down, self.half, self.taps = design(f_in, f_out)
        self.T = taps_per_output(self.up, self.down)
        self.device = torch.device(device)
        self.identity = self.up == self.down
        self.table = None
        if not self.identity:
            if self.device.type != "cuda":
                raise RuntimeError("m2h.Resampler: device must be a GPU (got %s); the m2h ops have no CPU path" % (self.device,))
            self.table = torch.from_numpy(polyphase_table(self.taps.astype(np.float32), self.up)).to(self.device)

    def output_length(self, L):
        return output_length(L, self.up, self.down)

    def __call__(self, x):
        import torch
        from .. import ops
        if not torch.is_tensor(x) or x.dim() < 1 or x.shape[-1] < 1:
            raise RuntimeError("m2h.Resampler: expected a tensor [..., L] with L >= 1")
        if x.dtype != torch.float32:
            raise RuntimeError("m2h.Resampler: x must be float32, got %s" % x.dtype)
        if self.identity:
            return x
        if x.device != self.device:
            raise RuntimeError("m2h.Resampler: x lives on %s, the resampler on %s" % (x.device, self.device))
        lead = x.shape[:-1]
        y = ops.resample_poly(x.contiguous().reshape(-1, x.shape[-1]), self.table, self.up, self.down)
        return y.reshape(*lead, y.shape[-1])
