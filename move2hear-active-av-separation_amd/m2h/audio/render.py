"""Auralizer: binaural recordings of any length from mono sources and binaural RIRs, on the GPU (csrc/render.hip).

Definition.  B = 16000 samples: one second, the Separator's segment and the simulator's step.  Inputs, fp32 on the GPU:

  sources [R, S, L], L >= 1;
  rirs    [R, S, K, Lr, 2], or [R, S, Lr, 2] which means K = 1; Lr >= 1; the ears interleaved in the last axis, as in the feeder and
          in a SoundSpaces RIR file;
  gains   [R, S], optional; the default 1/S makes the mixture the mean of the sources' binaural images, as in the reference.

J = ceil(L / B) blocks; block j is x[jB : min((j+1)B, L)].  K is 1 (a static scene) or exactly J (one RIR per second: a listener or a
source that moves once per second, every second of sound heard through the RIR of the pose it was emitted in); kappa(j) = 0 for K = 1
and j otherwise.

  image[r, s, e, n] = sum_j ( block_j(x[r, s]) * h[r, s, kappa(j), :, e] )[n - jB]      causal, full linear convolution, tail carried
  mix[r, e, n]      = sum_s gains[r, s] . image[r, s, e, n]                             s = 0 .. S-1 in that order

n runs over [0, L_out): L_out = L by default (the recording has the sources' length), L + Lr - 1 with tail=True.  With K = 1 this is
the linear convolution of the whole signal.  `images` carry unit gain.

Differences from BinauralFeeder.convolve_round (m2h/audio/feeder.py), which follows the reference loader over ONE second: there is no
centring (the feeder takes scipy's "same" window, which starts (Lr - 1) // 2 samples into the convolution and cuts the reverberation
at the second's border; here output sample n is convolution sample n and a block's tail runs on into the following seconds), no int16
rounding (the feeder rounds every source's image to int16 and back; here values stay fp32), and no truncation at second borders.

Method: uniformly partitioned overlap-add with partition length B and transform length 32768 (B + B - 1 = 31999 points: no
aliasing).  Pn = ceil(Lr / B) RIR partitions, at most 16 (Lr <= 256000).

  frame_m = IFFT( sum_{p = 0 .. Pn-1, 0 <= m-p < J}  X_{m-p} (.) H_{kappa(m-p), p} )        m = 0 .. J + Pn - 2, p ascending
  image[mB + i] = frame_m[i] + frame_{m-1}[B + i]                                          i < B

Three kernels: m2h_render_spectra (X_j and H_{k,p,e}), m2h_render_frames (products, sum over p, inverse transform), m2h_render_mix
(the two frames over every sample, the gained sum over the sources).  Frames are computed in chunks of at most `max_blocks` output
blocks per (r, s), so frame and spectrum scratch is bounded by max_blocks and Pn, not by L; a chunk recomputes the one frame before
its first output block rather than carrying state, and with K = J only the RIR spectra of the chunk's seconds are resident.  The
arithmetic and its order do not depend on the chunking, on the batch, on `tail`, or on whether one RIR is given once or repeated.
"""
import ctypes

import numpy as np
import torch

from .. import _lib, ops
from .twiddles import device_twiddles

BLOCK = 16000
NFFT = 32768
FRAME = 2 * BLOCK          # samples of a frame that are kept
MAX_PARTITIONS = 16
DEFAULT_MAX_BLOCKS = 1024


def render_plan(L, Lr, K, max_blocks, tail=False):
    """Pure Python: the blocks, partitions, frames and chunks of one render.

    -> {"J", "Pn", "frames" (J + Pn - 1), "L_out", "out_blocks" (ceil(L_out / B)), "chunks"}; a chunk is
    {"out": (o0, o1) output blocks, "frames": (m0, m1) computed for them, "x": (j0, j1) source blocks whose spectra it needs,
    "h": (k0, k1) RIRs whose spectra it needs}.  A chunk holds at most max_blocks output blocks, hence max_blocks + 1 frames: the frame
    before its first output block is computed again."""
    L, Lr, K, max_blocks = int(L), int(Lr), int(K), int(max_blocks)
    if L < 1 or Lr < 1:
        raise ValueError("m2h.Auralizer: sources and RIRs need at least one sample (L = %d, Lr = %d)" % (L, Lr))
    if max_blocks < 1:
        raise ValueError("m2h.Auralizer: max_blocks must be positive, got %d" % max_blocks)
    J, Pn = -(-L // BLOCK), -(-Lr // BLOCK)
    if Pn > MAX_PARTITIONS:
        raise ValueError("m2h.Auralizer: an RIR of %d taps needs %d partitions of %d; the limit is %d partitions (Lr <= %d)"
                         % (Lr, Pn, BLOCK, MAX_PARTITIONS, MAX_PARTITIONS * BLOCK))
    if K != 1 and K != J:
        raise ValueError("m2h.Auralizer: K = %d RIRs per source; 1 (static scene) or J = ceil(L / %d) = %d (one per second) is required" % (K, BLOCK, J))
    F = J + Pn - 1
    L_out = L + Lr - 1 if tail else L
    O = -(-L_out // BLOCK)
    chunks = []
    for o0 in range(0, O, max_blocks):
        o1 = min(o0 + max_blocks, O)
        m0, m1 = max(0, o0 - 1), min(o1, F)
        j0, j1 = max(0, m0 - Pn + 1), min(J, m1)
        chunks.append({"out": (o0, o1), "frames": (m0, m1), "x": (j0, j1), "h": (0, 1) if K == 1 else (j0, j1)})
    return {"J": J, "Pn": Pn, "frames": F, "L_out": L_out, "out_blocks": O, "chunks": chunks}


def chunk_scratch_bytes(plan, chunk, RS, K):
    """Bytes of frame and spectrum scratch one chunk holds for RS (recording, source) pairs (a static scene's RIR spectra included)."""
    (m0, m1), (j0, j1), (k0, k1) = chunk["frames"], chunk["x"], chunk["h"]
    return 4 * RS * ((m1 - m0) * 2 * FRAME + (j1 - j0) * NFFT + 2 * (k1 - k0) * plan["Pn"] * NFFT)


class Auralizer:
    def __init__(self, device, max_blocks=DEFAULT_MAX_BLOCKS):
        if int(max_blocks) < 1:
            raise ValueError("m2h.Auralizer: max_blocks must be positive, got %r" % (max_blocks,))
        self.device = torch.device(device)
        self.max_blocks = int(max_blocks)
        self._twiddles = None
        self._timing = None          # tools/render_bench.py: a list that receives (stage, event) marks

    def _twiddle_table(self):
        """[2, 16384, 2] fp32: exp(-2 pi i k / 32768), k < 16384, interleaved, built in float64 on the host (the feeder's table at this
        length), and the same fp32 values again in the order the transform's stages read them (include/m2h.h, "Auralizer")."""
        if self._twiddles is None:
            self._twiddles = device_twiddles(self.device, NFFT)
        return self._twiddles

    def _mark(self, stage):
        if self._timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.device))
            self._timing.append((stage, ev))

    def _check(self, sources, rirs, gains):
        for name, t in (("sources", sources), ("rirs", rirs)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("m2h.Auralizer: %s must be a torch tensor, got %s" % (name, type(t).__name__))
            if not t.is_cuda or t.device != self.device:
                raise RuntimeError("m2h.Auralizer: %s must live on %s (got %s); the renderer has no CPU path" % (name, self.device, t.device))
            if t.dtype != torch.float32:
                raise RuntimeError("m2h.Auralizer: %s must be float32, got %s" % (name, t.dtype))
        if sources.dim() != 3:
            raise ValueError("m2h.Auralizer: sources must be [R, S, L], got a tensor of shape %s" % (tuple(sources.shape),))
        if rirs.dim() == 4:
            rirs = rirs.unsqueeze(2)
        if rirs.dim() != 5 or rirs.shape[-1] != 2:
            raise ValueError("m2h.Auralizer: rirs must be [R, S, K, Lr, 2] or [R, S, Lr, 2], got a tensor of shape %s" % (tuple(rirs.shape),))
        R, S, L = sources.shape
        if R < 1 or S < 1 or tuple(rirs.shape[:2]) != (R, S):
            raise ValueError("m2h.Auralizer: sources %s and rirs %s do not describe the same R >= 1 recordings of S >= 1 sources"
                             % (tuple(sources.shape), tuple(rirs.shape)))
        if gains is None:
            gains = torch.full((R, S), 1.0 / S, dtype=torch.float32, device=self.device)
        else:
            if not isinstance(gains, torch.Tensor):
                gains = torch.as_tensor(np.asarray(gains, dtype=np.float32)).to(self.device)
            if not gains.is_cuda or gains.device != self.device or gains.dtype != torch.float32:
                raise RuntimeError("m2h.Auralizer: gains must be a float32 tensor on %s" % (self.device,))
            if tuple(gains.shape) != (R, S):
                raise ValueError("m2h.Auralizer: gains must be [R, S] = [%d, %d], got %s" % (R, S, tuple(gains.shape)))
        return sources, rirs, gains

    def render(self, sources, rirs, gains=None, tail=False, return_images=False):
        """-> mix [R, 2, L_out] (, images [R, S, 2, L_out]); the module docstring holds the definition."""
        sources, rirs, gains = self._check(sources, rirs, gains)
        R, S, L = sources.shape
        K, Lr = rirs.shape[2], rirs.shape[3]
        plan = render_plan(L, Lr, K, self.max_blocks, tail)          # raises on K, Lr
        sources, rirs, gains = sources.contiguous(), rirs.contiguous(), gains.contiguous()
        J, Pn, F, L_out = plan["J"], plan["Pn"], plan["frames"], plan["L_out"]
        RS = R * S
        lib = _lib.load()
        dev = self.device
        with torch.cuda.device(dev):
            st = ops._stream(sources)
            tw = ops._ptr(self._twiddle_table())
            mix = torch.empty((R, 2, L_out), device=dev)
            images = torch.empty((R, S, 2, L_out), device=dev) if return_images else None

            def rir_spectra(k0, k1):
                h = torch.empty((RS, k1 - k0, 2, Pn, NFFT), device=dev)
                src = ctypes.c_void_p(rirs.data_ptr() + 4 * k0 * Lr * 2)
                _lib.check(lib.m2h_render_spectra(src, tw, ops._ptr(h), RS, k1 - k0, 2, K * Lr * 2, Lr * 2, 1, Lr, 2, 0, Pn, st), "m2h_render_spectra")
                return h

            self._mark("start")
            hspec = rir_spectra(0, 1) if K == 1 else None
            for ch in plan["chunks"]:
                (o0, o1), (m0, m1), (j0, j1), (k0, k1) = ch["out"], ch["frames"], ch["x"], ch["h"]
                xspec = torch.empty((RS, j1 - j0, NFFT), device=dev)
                _lib.check(lib.m2h_render_spectra(ops._ptr(sources), tw, ops._ptr(xspec), RS, 1, 1, L, 0, 0, L, 1, j0, j1 - j0, st), "m2h_render_spectra")
                if K != 1:
                    hspec = rir_spectra(k0, k1)
                self._mark("render_spectra")
                frames = torch.empty((RS, m1 - m0, 2, FRAME), device=dev)
                _lib.check(lib.m2h_render_frames(ops._ptr(xspec), ops._ptr(hspec), tw, ops._ptr(frames), RS, J, Pn, K, m0, m1 - m0, j0, j1 - j0, k0, k1 - k0,
                                                 st), "m2h_render_frames")
                self._mark("render_frames")
                _lib.check(lib.m2h_render_mix(ops._ptr(frames), ops._ptr(gains), ops._ptr(mix), ops._ptr(images), R, S, m0, m1 - m0, F, o0, o1, L_out, st),
                           "m2h_render_mix")
                self._mark("render_mix")
        return (mix, images) if return_images else mix
