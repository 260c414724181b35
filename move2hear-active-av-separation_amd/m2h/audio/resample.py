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

    def stream(self, lead=()):
        """A ResamplerStream over rows of the shape `lead` (a block is [*lead, n])."""
        return ResamplerStream(self, lead)

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


# ---- block by block ----
def ready_outputs(P, up, down):
    """How many outputs P received input samples determine: output n is emitted once input sample (n * down + half) div up has
    arrived, so this is the number of n >= 0 with (n * down + half) div up < P.  Never more than ceil(P * up / down).  Pure Python; P may
    be an int or an integer numpy array."""
    half = 10 * max(up, down)
    n = (P * up - half - 1) // down + 1
    return np.maximum(n, 0) if isinstance(n, np.ndarray) else max(0, n)


class SampleWindow:
    """The last samples of rows that arrive block by block: buf [*lead, cap] holds the absolute samples [origin, origin + fill) at
    buf[..., : fill].  Two buffers take turns: moving the window copies the kept tail and the new block from one into the other, never
    between overlapping views of one buffer, and costs O(kept + block).  The pair grows (doubling) only when a window needs more than
    cap samples: with blocks of a bounded size the window is allocated once."""

    def __init__(self, lead, device):
        self.lead, self.device = tuple(lead), device
        self.bufs, self.cur, self.cap = [None, None], 0, 0
        self.origin = self.fill = 0

    @property
    def buf(self):
        return self.bufs[self.cur]

    def clear(self):
        self.origin = self.fill = 0

    def advance(self, origin, block=None, extra=0):
        """Move to [origin, old end + n): drops the samples below origin, appends block [*lead, n] or, with extra = n, n samples that the
        caller writes.  origin lies inside [old origin, old end]."""
        import torch
        off = origin - self.origin
        keep = self.fill - off
        assert 0 <= off and keep >= 0, (origin, self.origin, self.fill)
        n = block.shape[-1] if block is not None else int(extra)
        need = keep + n
        if off == 0 and need <= self.cap:                      # nothing to drop: append in place
            dst = self.buf
        else:
            if need > self.cap:
                self.cap = (max(need, 2 * self.cap) + 3) // 4 * 4
                new = [torch.empty(self.lead + (self.cap,), device=self.device, dtype=torch.float32) for _ in range(2)]
                dst, nxt = new[0], 0
            else:
                new, nxt = self.bufs, 1 - self.cur
                dst = new[nxt]
            if keep:
                dst[..., :keep].copy_(self.buf[..., off:off + keep])
            self.bufs, self.cur = new, nxt
        if block is not None and n:
            dst[..., keep:need].copy_(block)
        self.origin, self.fill = origin, need


class ResamplerStream:
    """Resampler(...).stream(lead) -> push(block [*lead, n]) returns every output the samples so far determine (ready_outputs), flush()
    the rest up to ceil(L * up / down); the pieces, concatenated, are Resampler(x) of the concatenated blocks bit for bit, for any
    blocking (m2h_resample_poly_win).  The window keeps the T - 1 samples of history the next output needs."""

    def __init__(self, resampler, lead):
        self.rs, self.lead = resampler, tuple(int(d) for d in lead)
        self.rows = int(np.prod(self.lead)) if self.lead else 1
        self.win = SampleWindow(self.lead, resampler.device)
        self.reset()

    def reset(self):
        self.received = self.emitted = 0
        self.closed = False
        self.win.clear()

    def _j0(self, n):
        return (n * self.rs.down + self.rs.half) // self.rs.up

    def _run(self, count):
        import torch
        from .. import ops
        if count <= 0:
            return torch.empty(self.lead + (0,), device=self.rs.device, dtype=torch.float32)
        w = self.win
        y = ops.resample_poly(w.buf.view(self.rows, w.cap), self.rs.table, self.rs.up, self.rs.down, origin=w.origin, end=self.received, n_first=self.emitted,
                              count=count)
        self.emitted += count
        return y.view(self.lead + (count,))

    def push(self, block):
        import torch
        if self.closed:
            raise RuntimeError("m2h.ResamplerStream: push after flush")
        if not torch.is_tensor(block) or tuple(block.shape[:-1]) != self.lead or block.dim() != len(self.lead) + 1:
            raise RuntimeError("m2h.ResamplerStream: expected a block [%s, n], got %s" % (", ".join(map(str, self.lead)), tuple(block.shape) if torch.is_tensor(block) else type(block).__name__))
        if block.dtype != torch.float32:
            raise RuntimeError("m2h.ResamplerStream: block must be float32, got %s" % block.dtype)
        if self.rs.identity:
            self.received += block.shape[-1]
            self.emitted = self.received
            return block
        if block.device != self.rs.device:
            raise RuntimeError("m2h.ResamplerStream: block lives on %s, the resampler on %s" % (block.device, self.rs.device))
        w = self.win
        # the lowest sample the next output reads; it never moves back, and lies at or below what has arrived
        lo = min(max(self._j0(self.emitted) - (self.rs.T - 1), w.origin), self.received)
        w.advance(lo, block)
        self.received += block.shape[-1]
        return self._run(ready_outputs(self.received, self.rs.up, self.rs.down) - self.emitted)

    def flush(self):
        import torch
        if self.closed:
            raise RuntimeError("m2h.ResamplerStream: flush after flush")
        self.closed = True
        if self.rs.identity or self.received == 0:
            return torch.empty(self.lead + (0,), device=self.rs.device, dtype=torch.float32)
        return self._run(output_length(self.received, self.rs.up, self.rs.down) - self.emitted)
