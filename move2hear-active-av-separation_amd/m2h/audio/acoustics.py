"""RoomAcoustics: reverberation time, clarity, direct-to-reverberant ratio and early IACC of binaural RIRs, on the GPU
(csrc/rir_acoustics.hip) -- what the room was like in which a separation score was obtained.

Definition.  Rate 16 kHz; h[q, n, e] fp32, n < Lr <= 256000, e = 0 left, 1 right: `rirs [..., Lr, 2]`, the ears interleaved as the
Auralizer takes them; Q is the product of the leading shape.

1. Onset and direct sound (broadband, sample-exact).  Per ear pk_e = max |h| and npk_e its first index ("peak"; 0 for a silent ear).
   n0[q] ("onset") is the smaller, over the ears with pk_e > 0, of the first n with |h[n, e]| >= 0.1 pk_e (ISO 3382 puts the start 20 dB
   below the maximum; the comparison is made in float64).  One onset for both ears keeps the interaural delay; an ear that is silent
   has no onset of its own and does not take part.  drr[q, e] = 10 log10(D / (T - D)), D = sum of h^2 over |n - npk_e| <= 40 (+- 2.5 ms),
   clipped to the row, T = the sum over the whole row; both fp64 with exact products.  A silent RIR (pk = 0 in both ears) gives n0 = 0
   and NaN in every parameter; an ear that is silent alone gives NaN for that ear (and for the IACC, which needs both).

2. Bands.  Band 0 is broadband, y_0 = h.  Bands 1 .. 6 are the octaves at BAND_CENTRES = 125 .. 4000 Hz: y_b = g_b * h on the zero-
   extended row, g_b a zero-phase FIR of 4097 taps centred on tap 2048 (no delay): the ideal band-pass between fc / sqrt 2 and
   fc sqrt 2 times a Kaiser window with beta = 8.6, built in float64 on the host.  Its 16384-point DFT is real and symmetric and ships
   as the fp32 table octave_masks() [6, 16384], made once per RoomAcoustics.

3. Energy bins.  E[q, e, b, i] = sum over t < 16 of y_b[n0 + 16 i + t]^2 at the samples < Lr, i < Nb = ceil((Lr - n0) / 16); fp64, the
   product taken after widening.  Storage is [Q, 2, 7, ceil(Lr / 16)] with zeros past Nb, because n0 stays on the device.

4. Early IACC per band.  W = [n0, n0 + 1280), the first 80 ms:
   IACF(tau) = sum_{t in W} y_b[t, L] y_b[t + tau, R] / sqrt(sum_W y_b[t, L]^2 . sum_W y_b[t, R]^2), tau = -16 .. 16 samples (+- 1 ms);
   y_0 is zero outside [0, Lr), y_b for b >= 1 is the filtered zero-extended signal wherever W and the lags reach.
   iacc[q, b] = (max_tau |IACF|, the tau it is taken at, the lowest on ties); NaN, NaN where the denominator is not positive.

5. Decay and clarity, fp64 algebra on E per (q, e, b).  EDC[i] = sum_{j >= i} E[j], summed from the end backwards;
   Lv[i] = 10 log10(EDC[i] / EDC[0]).  For each of the ranges (0, -10), (-5, -25), (-5, -35) dB the least-squares line of Lv[i] against
   t_i = i / 1000 s over the bins with lo >= Lv[i] >= hi; T = -60 / slope: edt, t20, t30; fewer than two bins in a range give NaN.
   c50, c80 = 10 log10(sum_{i < 50 / 80} E / sum_{i >= 50 / 80} E); d50 = sum_{i < 50} E / sum E; ts = sum (i + 0.5) / 1000 . E[i] / sum E.
   ACOUSTIC_ORDER = ("edt", "t20", "t30", "c50", "c80", "d50", "ts").

6. No noise-floor compensation: there is no Lundeby truncation of the decay curve.  The RIRs this project analyses are simulated and
   carry no noise floor, so the backward integral has nothing to be cut off from; a MEASURED RIR that has one reads long, on t30 first.

Method (include/m2h.h): m2h_rir_onset (two passes over a row), m2h_rir_band_energy (both ears of a 16384-sample segment ride one
complex transform in LDS, multiplied by the band's real mask; 766 bins per segment; segment 0 also gives the IACF sums) and
m2h_rir_decay (a reverse scan of a row of bins per wave).  No band signal and no decay curve is stored, no step synchronises with the
host, and the bits of an RIR's results depend on that RIR alone -- not on the batch, not on `return_energy`.
"""
import numpy as np
import torch

from .. import ops
from .twiddles import device_twiddles

RATE = 16000
MAX_TAPS = 256000
BIN = 16
NFFT = 16384
TAPS = 4097
KAISER_BETA = 8.6
BAND_CENTRES = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
BANDS = 1 + len(BAND_CENTRES)
ACOUSTIC_ORDER = ("edt", "t20", "t30", "c50", "c80", "d50", "ts")
DEFAULT_MAX_BIN_BYTES = 1 << 30


def octave_taps():
    """[6, 4097] float64: the band filters g_b, tap 2048 the centre."""
    n = np.arange(TAPS, dtype=np.float64) - (TAPS // 2)
    win = np.kaiser(TAPS, KAISER_BETA)
    out = np.empty((len(BAND_CENTRES), TAPS))
    for b, fc in enumerate(BAND_CENTRES):
        f1, f2 = fc / np.sqrt(2.0), fc * np.sqrt(2.0)
        nz = np.where(n == 0, 1.0, n)
        ideal = (np.sin(2.0 * np.pi * f2 / RATE * n) - np.sin(2.0 * np.pi * f1 / RATE * n)) / (np.pi * nz)
        ideal[TAPS // 2] = 2.0 * (f2 - f1) / RATE
        out[b] = ideal * win
    return out


def octave_masks():
    """[6, 16384] fp32: the 16384-point DFT of every g_b with its centre tap at sample 0 -- real and symmetric -- in natural bin order."""
    g = octave_taps()
    z = np.zeros((g.shape[0], NFFT))
    half = TAPS // 2
    z[:, :half + 1] = g[:, half:]
    z[:, NFFT - half:] = g[:, :half]
    lower = np.fft.rfft(z, axis=1).real                                       # bins 0 .. 8192; bin 16384 - k is bin k
    return np.concatenate([lower, lower[:, -2:0:-1]], axis=1).astype(np.float32)


class RoomAcoustics:
    def __init__(self, device, max_bin_bytes=DEFAULT_MAX_BIN_BYTES):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("m2h.RoomAcoustics: device must be a GPU (got %s); the analysis has no CPU path" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.max_bin_bytes = int(max_bin_bytes)
        self.masks = self._twiddles = None
        if torch.cuda.is_available():
            self._tables()           # made once, here: analyze() itself never waits for the host
        self._timing = None          # tools/rir_bench.py: a list that receives (stage, event) marks

    def _tables(self):
        if self.masks is None:
            self.masks = torch.from_numpy(octave_masks()).to(self.device).contiguous()
            self._twiddles = device_twiddles(self.device, 2 * NFFT)
        return self.masks, self._twiddles

    def _mark(self, stage):
        if self._timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.device))
            self._timing.append((stage, ev))

    def _check(self, rirs):
        if not isinstance(rirs, torch.Tensor):
            raise TypeError("m2h.RoomAcoustics: rirs must be a torch tensor, got %s" % type(rirs).__name__)
        if rirs.dtype != torch.float32:
            raise RuntimeError("m2h.RoomAcoustics: rirs must be float32, got %s" % rirs.dtype)
        if rirs.dim() < 2 or rirs.shape[-1] != 2:
            raise ValueError("m2h.RoomAcoustics: rirs must be [..., Lr, 2] with the ears in the last axis, got a tensor of shape %s" % (tuple(rirs.shape),))
        Lr = int(rirs.shape[-2])
        if not 1 <= Lr <= MAX_TAPS:
            raise ValueError("m2h.RoomAcoustics: an RIR of %d taps; 1 .. %d are supported" % (Lr, MAX_TAPS))
        if rirs.numel() == 0:
            raise ValueError("m2h.RoomAcoustics: rirs of shape %s hold no RIR" % (tuple(rirs.shape),))
        if not rirs.is_cuda or rirs.device != self.device:
            raise RuntimeError("m2h.RoomAcoustics: rirs must live on %s (got %s); the analysis has no CPU path" % (self.device, rirs.device))
        return Lr

    def analyze(self, rirs, return_energy=False):
        """-> {"onset" [...] int32, "peak" [..., 2] int32, "drr" [..., 2], "params" [..., 2, 7, 7] (ear, band, ACOUSTIC_ORDER),
        "iacc" [..., 7, 2] (value, lag), "energy" [..., 2, 7, ceil(Lr / 16)] with return_energy, "band_centres": BAND_CENTRES}; fp64 unless
        stated, on the device; the module docstring holds the definition."""
        Lr = self._check(rirs)
        lead = tuple(rirs.shape[:-2])
        h = rirs.reshape(-1, Lr, 2).contiguous()
        Q = h.shape[0]
        nbs = -(-Lr // BIN)
        step = max(1, min(ops.RIR_MAX_BATCH, self.max_bin_bytes // (2 * BANDS * nbs * 8)))
        masks, twiddles = self._tables()
        parts = {k: [] for k in ("onset", "peak", "drr", "params", "iacc", "energy")}
        self._mark("start")
        for q0 in range(0, Q, step):
            hq = h[q0:q0 + step]
            onset, peak, sums, drr = ops.rir_onset(hq)
            self._mark("rir_onset")
            energy, _, iacc = ops.rir_band_energy(hq, onset, sums, masks, twiddles)
            self._mark("rir_band_energy")
            params = ops.rir_decay(energy)
            self._mark("rir_decay")
            for k, v in (("onset", onset), ("peak", peak), ("drr", drr), ("params", params), ("iacc", iacc)):
                parts[k].append(v)
            if return_energy:
                parts["energy"].append(energy)
        out = {}
        for k, v in parts.items():
            if v:
                t = v[0] if len(v) == 1 else torch.cat(v)
                out[k] = t.reshape(lead + tuple(t.shape[1:]))
        out["band_centres"] = BAND_CENTRES
        return out
