"""Separation of binaural recordings of any length: waveform in, the target class's waveform out.

    sep = Separator("ckpt.pth", torch.device("cuda", 0))
    mono = sep.separate(wave, target_class)          # wave [R, 2, L] (or [2, L]) fp32 at 16 kHz  ->  [R, L]
    mono = sep.separate(wave, target_class, sample_rate=44100)     # any supported rate in, the same rate and length out
    mono = sep.separate(wave, target_class, overlap=2)             # one-second segments every half second, cross-faded
    binaural = sep.separate(wave, target_class, output="binaural") # the target in both ears, [R, 2, L]; "both": (mono, binaural)

Semantics (the CPU statement of the same thing is tests/separate_ref.py):
  * the recording is cut into S = ceil(L / 16000) non-overlapping one-second segments -- the agent's steps; samples at or past L are zero;
  * every segment is transformed on its own with the feeder's STFT (m2h.audio.stft.STFT, mode 1: n_fft 1023, hop 512, periodic
    Hann, centred, the reflect padding of 511 taken inside the zero-padded segment): 32 frames, log1p|X|, [512, 32, 2];
  * the output phase is the phase of the downmix spectrum D = X_left + X_right, kept as the unit phasor D / |D| and as (1, 0) where
    |D| == 0 (np.angle(0) = 0) -- at inference there is no ground-truth phase to borrow, as PPOTrainer.eval() does;
  * get_binSepMasks -> convert_bin2mono give pred_mono; with the acoustic memory P_0 = mem(pred_mono_0, 0) and
    P_s = mem(pred_mono_s, P_{s-1}) (eval()'s recurrence without an episode boundary), without it P_s = pred_mono_s;
  * the networks work on log1p magnitudes: the inverse transform gets expm1(max(P, 0)) times the phasor, then the evaluation
    path's iSTFT (n_fft 1022 inferred from 512 bins, length 16000); the segments are concatenated and cut at L.

Overlapped segments (``overlap=k``, k in {1, 2, 4}, H = 16000 / k; k = 1 is the above, unchanged):
  * segment s covers samples [s * H, s * H + 16000) for every s >= 0 with s * H < L: S' = ceil(L / H) segments, zeros from L on; each
    is transformed, separated and inverted exactly as above, which gives v_s[t], t = 0 .. 15999;
  * the memory runs k interleaved chains: segment s belongs to chain s mod k, its predecessor is segment s - k, the first segment
    of every chain starts from zeros -- each chain is the recurrence above over consecutive, non-overlapping seconds, started
    c * H samples late.  Batch rows are segment-major, so step g of all chains is the contiguous batch of the rows of segments
    [g * k, min(g * k + k, S')): one memory call of up to k * R rows per second of audio, and no more dependent steps than k = 1;
  * the cross-fade window is w[t] = sin^2(pi (t + 1/2) / 16000) (``crossfade_window``: float64 on the host, rounded once to fp32),
    strictly positive, its k shifts summing to k / 2; W[n] = sum_s w[n - s * H] over the segments that cover n, and
    y[n] = sum_s w[n - s * H] * v_s[n - s * H] / W[n] for n < L (m2h_sep_istft_xfade; where one segment covers n, y[n] = v_s);
  * so chain c is the k = 1 path applied to wave[:, :, c * H:], and the CPU statement is the cross-fade of tests/separate_ref.py on
    k shifted recordings (tests/separate_overlap_ref.py); spectrograms come back in segment order, P [R, S', 512, 32].
Lead-in segments before sample 0, other windows and other overlap factors are not part of this.

Other sample rates (``sample_rate=f``): the recording is converted to 16 kHz, separated exactly as above, converted back with the
reversed ratio and cut at L.  The conversion is the polyphase FIR of m2h/audio/resample.py (csrc/resample.hip): for the reduced ratio
up / down = f_out / f_in, half = 10 * max(up, down), h = c * sinc(c * m) * kaiser(2 * half + 1, 5.0) with c = 1 / max(up, down) over
m = -half .. half, normalised to sum up, and y[n] = sum_j x[j] * h[n * down - j * up + half] for n < ceil(L * up / down), x zero
outside the recording -- scipy.signal.resample_poly(x, up, down, padtype="constant") with its default window.  The 16 kHz
recording has L16 = ceil(L * 16000 / f) samples; its back-conversion never has fewer than L.  Spectrograms are those of the
16 kHz recording.  Rates with max(up, down) <= 1024 are supported (tests/resample_ref.py is the CPU statement).

Binaural target (``output="binaural"`` -> [R, 2, L], ``output="both"`` -> (mono, binaural); tests/separate_binaural_ref.py is the CPU
statement).  The first U-Net predicts the target in both ears: its two masks times the mixture magnitude are the separated binaural
magnitude the reference trains and scores.  For every segment s and recording r, X_c [512, 32] (the segment's spectrum of channel c),
M = log1p|X| and m = get_binSepMasks({M, target_class}) [512, 32, 2] are exactly what the mono path uses, and
  * the predicted spectrum of channel c is the mixture's own complex spectrum scaled by the clamped mask, Y_c = max(m[..., c], 0) * X_c:
    magnitude max(m_c |X_c|, 0) -- the clamp the second U-Net's input applies -- with the phase of X_c.  No phase is invented, and
    there is no phasor, no log1p / expm1 round trip and no second U-Net on this path;
  * v_{s,c} = np_istft(Y_c as complex64, hop 512, length 16000), the evaluation path's inverse transform as for the mono output;
  * the segments are placed exactly as for the mono output, each channel on its own: overlap=1 concatenated and cut at L, overlap=k
    cross-faded with the same window and normalisation, sample_rate=f both channels converted back with the same Resampler;
  * the acoustic memory and convert_bin2mono take no part: use_memory=True with output="binaural" is a ValueError.  With "both" the
    transform and the first U-Net run once, the binaural branch of a chunk finishes before the second U-Net starts, and the mono
    output is the "mono" call's bit for bit.
  The path is NOT transparent at m == 1: the reference's forward transform has n_fft 1023 and its inverse 1022 (the mono path inherits
  the same convention), and on the CPU np_istft(np_stft(segment)) reproduces the end-to-end test signal (noise plus one tone per
  channel) only to rel-L1 0.44 (0.27 .. 0.61 per channel, with the tone's frequency).  A mask of ones is not an identity, and
  nothing here promises one.
  The clamp is live: with the synthetic test weights about 54 % of the mask values are negative (mask range -11.5 .. 13.3).
In HIP: m2h_sep_bin_rows scales the forward GEMM's rows in place (masks are bin-major, rows frame-major: a transpose through LDS) into
the inverse GEMM's operand, and the inverse GEMM's rows are those of 2R mono recordings -- row ((sl*R + r)*2 + c)*32 + t is row
((sl*2R + (2r + c))*32 + t -- so m2h_sep_istft_ola / m2h_sep_istft_xfade write the contiguous [R, 2, L] result viewed as [2R, L].

A live feed (``st = sep.stream(target_class, recordings=R, use_memory=None, sample_rate=16000, overlap=1, output="mono")``): the same
separation for a recording that arrives block by block.  st.push(block [R, 2, n]), n >= 0, returns the samples that became final
([R, m], [R, 2, m] or the pair, m >= 0), st.flush() the rest, st.reset() goes back to sample 0 with the same buffers.
  * Defining property: with x the blocks pushed so far, concatenated, the returned pieces, concatenated, equal
    sep.separate(x, target_class, use_memory=..., sample_rate=..., overlap=..., output=...), whatever the blocking; after flush() they
    hold exactly L samples.  Bit for bit where the pushes run the batches separate() runs, to the U-Nets' batch-size tolerance otherwise;
  * segment s is processed as soon as sample s * H + 15999 has arrived; a sample is final once every segment that covers it is done, so
    after P samples exactly stream_emitted(P, overlap) = H * ((P - 16000) div H + 1) have been returned (0 while P < 16000).  No segment
    of the future covers a final sample: W[n] does not depend on the unknown L.  flush() processes every remaining segment with
    s * H < L (samples at or past L zero, as offline) and cuts the output at L;
  * at another rate every stage returns all that its input determines (the converter emits output n once input sample
    (n * down + half) div up has arrived: m2h.audio.resample.ResamplerStream), stream_returned(P, sample_rate, overlap) samples after P,
    and the backlog stays under 1.01 seconds;
  * the memory keeps one state per chain c = s mod overlap, zeros at the start, carried across pushes; the segments that complete in one
    push are one segment-major U-Net batch, split at max_segments rows; several streams of one Separator do not disturb each other;
  * the input and the cross-fade's partial sums live in windows [rows][cap] of absolute samples [origin, origin + cap) read and written
    by the window entry points of the glue kernels (m2h_sep_frames_win, m2h_sep_istft_ola_win, m2h_sep_istft_xfade_win,
    m2h_resample_poly_win: the offline kernels themselves, a recording being the window that holds all of it); a push costs
    O(block + one second).  return_spectrograms is not offered.

The two DFTs are dense 1024 x 1024 GEMMs (ops.linear) and follow the calling thread's arithmetic like the U-Nets; framing, the
magnitude / phasor store, the inverse transform's operand and the overlap-add are the HIP kernels of csrc/separate.hip, which
read the recording and write the output in place: no padded, framed or angle copies.
"""
import numpy as np
import torch

from . import ops

SEGMENT = ops.SEP_SEGMENT
SAMPLE_RATE = 16000
SEPARATOR_ROOTS = ("binSep_enc.", "binSep_dec.", "bin2mono_enc.", "bin2mono_dec.")
MEMORY_ROOT = "acoustic_mem."
# rows of a U-Net batch.  Measured on 16 recordings of 600 s in bf16x3 (tools/separate_bench.py): 64 rows 89 K, 256 rows 203 K, 1024 rows
# 282 K seconds of audio per second -- below a few hundred rows of 512 x 32 the U-Nets' 22 launches are bound by their boundaries.
# 1024 rows hold 0.5 GB of transform buffers and half the activations of the benchmark's batch (256 spectrograms of 512 x 256).
DEFAULT_MAX_SEGMENTS = 1024
OVERLAPS = (1, 2, 4)
OUTPUTS = ("mono", "binaural", "both")


def segment_plan(L, max_segments):
    """The chunks a recording of L samples is processed in: a list of (first_segment, n_segments) covering its ceil(L / 16000)
    one-second segments in order, each of at most max_segments segments.  Pure Python."""
    L, max_segments = int(L), int(max_segments)
    if L < 1:
        raise ValueError("segment_plan: a recording needs at least one sample, got L = %d" % L)
    if max_segments < 1:
        raise ValueError("segment_plan: max_segments must be at least 1, got %d" % max_segments)
    S = -(-L // SEGMENT)
    return [(s0, min(max_segments, S - s0)) for s0 in range(0, S, max_segments)]


def overlap_plan(L, overlap, max_segments):
    """segment_plan for overlapped segments: (first_segment, n_segments) chunks covering the ceil(L / (16000 / overlap)) segments in
    order.  A chunk holds max(overlap, max_segments) segments rounded down to a multiple of overlap, so that a memory step (the
    `overlap` segments of one second) never straddles two chunks; only the last chunk may hold fewer.  overlap = 1 is segment_plan.
    Pure Python."""
    L, overlap, max_segments = int(L), int(overlap), int(max_segments)
    if overlap not in OVERLAPS:
        raise ValueError("overlap_plan: overlap must be one of %s, got %d" % (OVERLAPS, overlap))
    if L < 1:
        raise ValueError("overlap_plan: a recording needs at least one sample, got L = %d" % L)
    if max_segments < 1:
        raise ValueError("overlap_plan: max_segments must be at least 1, got %d" % max_segments)
    hop = SEGMENT // overlap
    S = -(-L // hop)
    per = max(overlap, max_segments) // overlap * overlap
    return [(s0, min(per, S - s0)) for s0 in range(0, S, per)]


def crossfade_window(dtype=np.float32):
    """w[t] = sin^2(pi (t + 1/2) / 16000), t = 0 .. 15999, computed in float64 and rounded once to dtype: strictly positive (its
    minimum is 9.64e-9), symmetric, and its shifts by 16000 / k sum to k / 2 for k = 2 and 4."""
    t = np.arange(SEGMENT, dtype=np.float64)
    return (np.sin(np.pi * (t + 0.5) / SEGMENT) ** 2).astype(dtype)


def split_checkpoint(ckpt):
    """(separator state dict, memory state dict or None, memory variant or None) of any accepted checkpoint form: a passive
    checkpoint (the 124 separator entries) or a PPO checkpoint, as a {"state_dict", "config"} file's dict or a bare state dict,
    with or without the "actor_critic." root.  The memory variant is "ddppo" (cnn.0, cnn.2) or "bn" (cnn.0, cnn.1.*, cnn.3).
    Values stay what they were (tensors or arrays); works without a GPU."""
    if not isinstance(ckpt, dict):
        raise RuntimeError("m2h.separate: a checkpoint must be a dict, got %s" % type(ckpt).__name__)
    sd = ckpt["state_dict"] if "state_dict" in ckpt and isinstance(ckpt["state_dict"], dict) else ckpt
    root = "actor_critic."
    if any(k.startswith(root) for k in sd):
        sd = {k[len(root):]: v for k, v in sd.items() if k.startswith(root)}
    sep = {k: v for k, v in sd.items() if k.startswith(SEPARATOR_ROOTS)}
    if not sep:
        raise RuntimeError("m2h.separate: the checkpoint holds no separator weights (%s*); its first keys are %s"
                           % ("* / ".join(SEPARATOR_ROOTS), list(sd)[:3]))
    mem = {k[len(MEMORY_ROOT):]: v for k, v in sd.items() if k.startswith(MEMORY_ROOT + "cnn.")}
    if not mem:
        return sep, None, None
    return sep, mem, ("bn" if "cnn.3.weight" in mem else "ddppo")


def _as_tensor(v):
    return v.detach().clone() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))


class Separator:
    """checkpoint: a path (torch.load) or a dict in any form ``split_checkpoint`` accepts.  math: the arithmetic of the U-Nets and
    the two DFTs (ops.MATH_FP32 or ops.MATH_BF16X3).  max_segments: the largest U-Net batch in one-second segments; activations and
    transform buffers are allocated per chunk, never for the whole recording."""

    def __init__(self, checkpoint, device, math=ops.MATH_BF16X3, max_segments=DEFAULT_MAX_SEGMENTS):
        from .audio.stft import ISTFT, STFT
        from .common.spaces import move2hear_observation_space
        from .pretrain.passive.policy import Move2HearPassiveWoMemoryPolicy
        from .rl.models.memory_nets import AcousticMem
        if math not in (ops.MATH_FP32, ops.MATH_BF16X3):
            raise ValueError("m2h.Separator: math must be ops.MATH_FP32 or ops.MATH_BF16X3")
        if int(max_segments) < 1:
            raise ValueError("m2h.Separator: max_segments must be at least 1, got %s" % (max_segments,))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("m2h.Separator: device must be a GPU (got %s); the m2h ops have no CPU path" % (self.device,))
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
        sep_sd, mem_sd, variant = split_checkpoint(checkpoint)
        self.math, self.max_segments = math, int(max_segments)
        self.policy = Move2HearPassiveWoMemoryPolicy(move2hear_observation_space())
        self.policy.load_state_dict({k: _as_tensor(v) for k, v in sep_sd.items()}, strict=True)
        self.policy = self.policy.to(self.device).eval()
        self.memory = None
        if mem_sd is not None:
            self.memory = AcousticMem(use_ddppo=(variant == "ddppo"))
            self.memory.load_state_dict({k: _as_tensor(v) for k, v in mem_sd.items()}, strict=True)
            self.memory = self.memory.to(self.device).eval()
        for p in list(self.policy.parameters()) + (list(self.memory.parameters()) if self.memory is not None else []):
            p.requires_grad_(False)
        fwd, inv = STFT(self.device), ISTFT(self.device)
        self._W_fwd, self._W_inv = fwd.W, inv.W
        self._win_fwd = torch.cat((fwd.window, torch.zeros(ops.SEP_LD - fwd.n_fft, device=self.device)))
        self._win_inv = inv.window
        self._win_xfade = None   # the cross-fade window, on the device from the first overlap > 1 call on
        self._timing = None    # tools/separate_bench.py: a list that takes (stage, event) marks
        self._resamplers = {}  # sample rate -> (Resampler to 16 kHz, Resampler back)

    def _mark(self, stage):
        if self._timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.device))
            self._timing.append((stage, ev))

    def _memory_scope(self, R):
        """The arithmetic of the memory's steps over R recordings: up to AcousticMem.SMALL_BATCH rows the DD-PPO variant's whole forward
        is one launch, an fp32 kernel, taken in an fp32 scope; otherwise the tiled path in the separator's own arithmetic."""
        small = self.memory._use_ddppo and R <= self.memory.SMALL_BATCH
        return ops.math_scope(ops.MATH_FP32 if small else self.math)

    def resamplers(self, sample_rate):
        """(to 16 kHz, back) for a recording's sample rate, built once per rate; ValueError for a rate that is not supported."""
        from .audio.resample import Resampler
        key = int(sample_rate) if int(sample_rate) == sample_rate else sample_rate
        if key not in self._resamplers:
            self._resamplers[key] = (Resampler(key, SAMPLE_RATE, self.device), Resampler(SAMPLE_RATE, key, self.device))
        return self._resamplers[key]

    def _arguments(self, use_memory, overlap, output, recordings=1):
        """separate()'s and stream()'s checks of what they share, before anything else is looked at -> (use_memory, want_mono, want_bin)."""
        if isinstance(overlap, bool) or overlap not in OVERLAPS:
            raise ValueError("m2h.Separator: overlap must be one of %s, got %r" % (OVERLAPS, overlap))
        if not isinstance(output, str) or output not in OUTPUTS:
            raise ValueError("m2h.Separator: output must be one of %s, got %r" % (OUTPUTS, output))
        want_mono, want_bin = output != "binaural", output != "mono"
        if not want_mono and use_memory:
            raise ValueError("m2h.Separator: output=\"binaural\" runs no acoustic memory (it refines the mono prediction only); "
                             "leave use_memory at None or False, or ask for output=\"both\"")
        if isinstance(recordings, bool) or int(recordings) != recordings or recordings < 1:
            raise ValueError("m2h.Separator: recordings must be a positive int, got %r" % (recordings,))
        if use_memory is None:
            use_memory = want_mono and self.memory is not None
        if use_memory and self.memory is None:
            raise RuntimeError("m2h.Separator: use_memory=True, but the checkpoint has no acoustic_mem.cnn.* weights")
        return bool(use_memory), want_mono, want_bin

    def _target_classes(self, target_class, R):
        """One class per recording, [R] int64 on the device, from one int or R of them."""
        tc = torch.as_tensor(target_class, dtype=torch.int64).reshape(-1)
        if tc.numel() == 1:
            tc = tc.expand(R)
        if tc.numel() != R:
            raise RuntimeError("m2h.Separator: target_class must be one int or one per recording (%d), got %d values" % (R, tc.numel()))
        return tc.to(self.device).contiguous()

    def _xfade_window(self):
        if self._win_xfade is None:
            self._win_xfade = torch.from_numpy(crossfade_window()).to(self.device)
        return self._win_xfade

    def _memory_steps(self, P, c0, cn, R, k, states):
        """The memory over the rows P of segments [c0, c0 + cn), k interleaved chains: segment s belongs to chain s mod k and its predecessor
        is segment s - k, so one step is up to k consecutive segments, one per chain, and one memory call.  states[c] = (rows, i): chain
        c's state is rows[i * R:(i + 1) * R] of an earlier step's output; None, zeros, at the start.  Updated in place."""
        steps = []
        with self._memory_scope(k * R):
            for sl in range(0, cn, k):
                n = min(k, cn - sl)
                pm = P[sl * R:(sl + n) * R]
                st = [states[(c0 + sl + i) % k] for i in range(n)]
                if all(s is None for s in st):
                    prev = torch.zeros_like(pm)
                elif all(s is not None and s[0] is st[0][0] and s[1] == i for i, s in enumerate(st)):
                    prev = st[0][0][:n * R]      # one earlier step wrote these chains in this order (always so in a file): its rows as they are
                else:
                    prev = torch.cat([torch.zeros_like(pm[:R]) if s is None else s[0][s[1] * R:(s[1] + 1) * R] for s in st])
                out = self.memory(pm, prev)
                for i in range(n):
                    states[(c0 + sl + i) % k] = (out, i)
                steps.append(out)
        return torch.cat(steps) if len(steps) > 1 else steps[0]

    def _chunk(self, c0, cn, hop, tc, source, sinks, states=None, keep=None):
        """Segments [c0, c0 + cn) at `hop` as one U-Net batch: frames, DFT, the U-Nets, the memory, inverse DFT, overlap-add or cross-fade.
        source = (buf [R, 2, cap], origin, end): the absolute samples [origin, origin + cap) of a recording of which `end` have arrived;
        sinks = (mono rows [R, cap'] or None, binaural rows [2R, cap'] or None, origin, end) likewise.  end = None: the whole recording
        (ops.sep_frames).  states: the memory's per-chain states (_memory_steps), None to run without it.  keep: three lists that take
        the chunk's P, phasor and masks."""
        buf, origin, end = source
        y, yb, y_origin, y_end = sinks
        R = buf.shape[0]

        def place(out_frames, rows):
            if hop == SEGMENT:
                ops.sep_istft_ola(out_frames, self._win_inv, rows, c0, cn, origin=y_origin, end=y_end)
            else:
                ops.sep_istft_xfade(out_frames, self._win_inv, self._xfade_window(), rows, hop, c0, cn, origin=y_origin, end=y_end)

        frames = ops.sep_frames(buf, self._win_fwd, c0, cn, hop=hop, origin=origin, end=end)
        spec = ops.linear(frames, self._W_fwd, None, name="separate.dft")
        mag, phasor = ops.sep_stft_post(spec, cn * R)
        del frames
        if yb is None:
            del spec
        self._mark("stft")
        masks = self.policy.get_binSepMasks({"mixed_bin_audio_mag": mag, "target_class": tc.repeat(cn)})
        if yb is not None:
            # finished before the second U-Net: the spectrum buffer is not held alongside that U-Net's activations.
            # The inverse GEMM's rows are those of 2R mono recordings: ((sl*R + r)*2 + c)*32 + t = ((sl*2R + (2r + c))*32 + t.
            self._mark("unets")
            masks = masks.contiguous()
            rows = ops.sep_bin_rows(spec, masks)
            del spec
            out_frames = ops.linear(rows, self._W_inv, None, name="separate.idft")
            del rows
            place(out_frames, yb)
            del out_frames
            self._mark("istft_bin")
            if keep is not None:
                keep[2].append(masks.reshape(cn, R, ops.SEP_BINS, ops.SEP_FRAMES, 2))
            if y is None:
                return
        P = self.policy.convert_bin2mono(masks, mixed_audio=mag)
        self._mark("unets")
        if states is not None:
            P = self._memory_steps(P, c0, cn, R, SEGMENT // hop, states)
            self._mark("memory")
        rows = ops.sep_istft_pre(P, phasor)
        out_frames = ops.linear(rows, self._W_inv, None, name="separate.idft")
        place(out_frames, y)
        self._mark("istft")
        if keep is not None:
            keep[0].append(P.reshape(cn, R, ops.SEP_BINS, ops.SEP_FRAMES))
            keep[1].append(phasor.reshape(cn, R, ops.SEP_BINS, ops.SEP_FRAMES, 2))

    @torch.no_grad()
    def separate(self, wave, target_class, use_memory=None, return_spectrograms=False, sample_rate=SAMPLE_RATE, overlap=1, output="mono"):
        """wave [R, 2, L] or [2, L] fp32 on this separator's device, L >= 1; target_class: an int or one per recording.
        Returns the separated waveform [R, L] ([L] for a [2, L] input); with return_spectrograms also P [R, S, 512, 32] (the
        log1p magnitude the inverse transform was given) and the phasor [R, S, 512, 32, 2].  sample_rate: the recording's rate;
        other than 16000 the recording is converted to 16 kHz and the result back (module docstring), the output has the
        input's rate and length, and S counts the seconds of the 16 kHz recording.  overlap: 1, 2 or 4 one-second segments over
        every sample, cross-faded (module docstring); S is then ceil(L / (16000 / overlap)), in segment order.
        output: "mono" (the above), "binaural" or "both" (module docstring, "Binaural target").  "binaural" returns the target in both
        ears [R, 2, L] ([2, L] for a [2, L] input), with return_spectrograms also the first U-Net's masks [R, S, 512, 32, 2]; it runs
        no memory, and use_memory=True given with it is a ValueError.  "both" returns (mono, binaural), with return_spectrograms
        (mono, binaural, P, phasor, masks); its mono is the "mono" call's bit for bit."""
        use_memory, want_mono, want_bin = self._arguments(use_memory, overlap, output)
        overlap = int(overlap)
        if not torch.is_tensor(wave):
            raise RuntimeError("m2h.Separator: wave must be a torch tensor, got %s" % type(wave).__name__)
        single = wave.dim() == 2
        if single:
            wave = wave.unsqueeze(0)
        if wave.dim() != 3 or wave.shape[1] != 2 or wave.shape[2] < 1 or wave.shape[0] < 1:
            raise RuntimeError("m2h.Separator: expected a binaural recording [R, 2, L] or [2, L] with L >= 1, got %s" % (tuple(wave.shape[1:] if single else wave.shape),))
        if wave.dtype != torch.float32:
            raise RuntimeError("m2h.Separator: wave must be float32, got %s" % wave.dtype)
        if wave.device != self.device:
            raise RuntimeError("m2h.Separator: wave lives on %s, the separator on %s" % (wave.device, self.device))
        tc = self._target_classes(target_class, wave.shape[0])
        wave = wave.contiguous()
        to16 = back = None
        if sample_rate != SAMPLE_RATE:
            to16, back = self.resamplers(sample_rate)
        L_given = wave.shape[2]
        if to16 is not None:
            with torch.cuda.device(self.device):
                self._mark("start")
                wave = to16(wave)
                self._mark("resample_in")
        R, _, L = wave.shape
        y = torch.empty((R, L), device=self.device, dtype=torch.float32) if want_mono else None
        yb = torch.empty((R, 2, L), device=self.device, dtype=torch.float32) if want_bin else None
        keep = ([], [], []) if return_spectrograms else None
        states = [None] * overlap
        with torch.cuda.device(self.device), ops.math_scope(self.math):
            if to16 is None:
                self._mark("start")
            # the recording itself is the source window and the outputs themselves the sinks (end = None: the whole of it)
            for s0, ns in overlap_plan(L, overlap, max(1, self.max_segments // R)):
                self._chunk(s0, ns, SEGMENT // overlap, tc, (wave, 0, None), (y, yb.view(2 * R, L) if want_bin else None, 0, None),
                            states if use_memory else None, keep)
            if back is not None:
                if want_mono:
                    y = back(y)[:, :L_given].contiguous()      # ceil(ceil(L a / b) b / a) >= L: never short
                if want_bin:
                    yb = back(yb)[:, :, :L_given].contiguous()
                self._mark("resample_out")
        res = ((y,) if want_mono else ()) + ((yb,) if want_bin else ())
        if return_spectrograms:
            if want_mono:
                res += (torch.cat(keep[0]).transpose(0, 1).contiguous(), torch.cat(keep[1]).transpose(0, 1).contiguous())
            if want_bin:
                res += (torch.cat(keep[2]).transpose(0, 1).contiguous(),)
        if single:
            res = tuple(a[0] for a in res)
        return res[0] if len(res) == 1 else res

    def stream(self, target_class, recordings, use_memory=None, sample_rate=SAMPLE_RATE, overlap=1, output="mono"):
        """A SeparatorStream: the same separation for `recordings` binaural feeds that arrive block by block (module docstring,
        "A live feed").  The argument checks are separate()'s."""
        return SeparatorStream(self, target_class, recordings, use_memory, sample_rate, overlap, output)


def stream_emitted(P, overlap):
    """Samples a 16 kHz SeparatorStream has returned once P samples have arrived (before flush): segment s is processed as soon as
    sample s * H + 15999 is there, H = 16000 / overlap, and a sample is final once no later segment covers it.  Pure Python; P may be an
    int or an integer numpy array."""
    if isinstance(overlap, bool) or overlap not in OVERLAPS:
        raise ValueError("stream_emitted: overlap must be one of %s, got %r" % (OVERLAPS, overlap))
    hop = SEGMENT // int(overlap)
    n = hop * ((P - SEGMENT) // hop + 1)
    return np.maximum(n, 0) if isinstance(n, np.ndarray) else max(0, n)


def stream_returned(P, sample_rate, overlap):
    """Samples a SeparatorStream at any supported rate has returned once P samples have arrived (before flush): every stage returns all
    that its input determines -- the converter to 16 kHz (m2h.audio.resample.ready_outputs), stream_emitted, the converter back.  The
    backlog P - stream_returned(P) stays under 1.01 seconds.  Pure Python; P may be an int or an integer numpy array."""
    from .audio.resample import ratio, ready_outputs
    if sample_rate == SAMPLE_RATE:
        return stream_emitted(P, overlap)
    up, down = ratio(sample_rate, SAMPLE_RATE)
    return ready_outputs(stream_emitted(ready_outputs(P, up, down), overlap), down, up)


class SeparatorStream:
    """Separator.stream(...): push(block [R, 2, n]) returns what is final, flush() the rest.  The pieces, concatenated, are
    separate() of the concatenated blocks (module docstring, "A live feed").  Holds the windows of the input and of the cross-fade's
    partial sums (m2h.audio.resample.SampleWindow), one memory state per chain and, for other sample rates, three ResamplerStreams."""

    def __init__(self, sep, target_class, recordings, use_memory=None, sample_rate=SAMPLE_RATE, overlap=1, output="mono"):
        from .audio.resample import SampleWindow
        self.use_memory, self.want_mono, self.want_bin = sep._arguments(use_memory, overlap, output, recordings)
        self.sep, self.R, self.overlap, self.hop = sep, int(recordings), int(overlap), SEGMENT // int(overlap)
        R, dev = self.R, sep.device
        self.tc = sep._target_classes(target_class, R)
        self.to16 = self.back_mono = self.back_bin = None
        if sample_rate != SAMPLE_RATE:
            to16, back = sep.resamplers(sample_rate)
            self.to16 = to16.stream((R, 2))
            self.back_mono = back.stream((R,)) if self.want_mono else None
            self.back_bin = back.stream((R, 2)) if self.want_bin else None
        self.win_in = SampleWindow((R, 2), dev)
        self.win_mono = SampleWindow((R,), dev) if self.want_mono and self.overlap > 1 else None
        self.win_bin = SampleWindow((R, 2), dev) if self.want_bin and self.overlap > 1 else None
        self.reset()

    def reset(self):
        """Back to sample 0: the same settings and buffers, the memory's states cleared."""
        self.received = self.emitted = 0          # samples of the caller's rate
        self.P16 = self.next_seg = 0              # 16 kHz samples received, segments processed
        self.closed = False
        self.states = [None] * self.overlap
        for w in (self.win_in, self.win_mono, self.win_bin):
            if w is not None:
                w.clear()
        for rs in (self.to16, self.back_mono, self.back_bin):
            if rs is not None:
                rs.reset()

    def _empty(self):
        dev = self.sep.device
        return ((torch.empty((self.R, 0), device=dev),) if self.want_mono else ()) + ((torch.empty((self.R, 2, 0), device=dev),) if self.want_bin else ())

    def _core(self, block, final):
        """One block [R, 2, n] at 16 kHz -> the samples that became final, as a tuple (mono?, binaural?)."""
        sep, R, k, H = self.sep, self.R, self.overlap, self.hop
        s1 = self.next_seg
        self.win_in.advance(min(s1 * H, self.P16), block)
        self.P16 += block.shape[-1]
        end = self.P16
        ready = -(-end // H) if final else (0 if end < SEGMENT else (end - SEGMENT) // H + 1)
        ns = ready - s1
        if ns <= 0:
            return self._empty()
        origin = s1 * H
        stop = min(end, (s1 + ns - 1) * H + SEGMENT)                 # the samples these segments cover: [origin, stop)
        m = (stop if final else (s1 + ns) * H) - origin              # of which final
        y = yb = None
        if k == 1:                                                   # written straight into the returned tensors, the window [origin, origin + m)
            y = torch.empty((R, m), device=sep.device, dtype=torch.float32) if self.want_mono else None
            yb = torch.empty((R, 2, m), device=sep.device, dtype=torch.float32) if self.want_bin else None
            sinks = (y, yb.view(2 * R, m) if yb is not None else None, origin, end)
        else:                                                        # added onto the partial sums
            for w in (self.win_mono, self.win_bin):
                if w is not None:
                    w.advance(origin, extra=stop - origin - w.fill)
            sinks = (self.win_mono.buf.view(R, -1) if self.want_mono else None, self.win_bin.buf.view(2 * R, -1) if self.want_bin else None, origin, end)
        per = max(1, sep.max_segments // R)
        for c0 in range(s1, s1 + ns, per):
            sep._chunk(c0, min(per, s1 + ns - c0), H, self.tc, (self.win_in.buf, self.win_in.origin, end), sinks, self.states if self.use_memory else None)
        self.next_seg = s1 + ns
        if k > 1:
            res = ()
            for w in (self.win_mono, self.win_bin):
                if w is not None:
                    res += (w.buf[..., :m].clone(),)
                    w.advance(origin + m)                            # the partial sums that later segments still cover stay
            return res
        return ((y,) if self.want_mono else ()) + ((yb,) if self.want_bin else ())

    def _step(self, block, final):
        with torch.cuda.device(self.sep.device), ops.math_scope(self.sep.math):
            if self.to16 is None:
                res = self._core(block, final)
            else:
                b16 = self.to16.push(block)
                if final:
                    b16 = torch.cat((b16, self.to16.flush()), dim=-1)
                pieces = self._core(b16, final)
                res = ()
                for piece, back in zip(pieces, [b for b in (self.back_mono, self.back_bin) if b is not None]):
                    out = back.push(piece)
                    if final:
                        out = torch.cat((out, back.flush()), dim=-1)[..., :self.received - self.emitted].contiguous()   # never short (separate())
                    res += (out,)
        self.emitted += res[0].shape[-1]
        return res[0] if len(res) == 1 else res

    @torch.no_grad()
    def push(self, block):
        """block [R, 2, n] fp32 on the separator's device, n >= 0 -> the samples that became final: [R, m], [R, 2, m] or the pair."""
        if self.closed:
            raise RuntimeError("m2h.SeparatorStream: push after flush")
        if not torch.is_tensor(block):
            raise RuntimeError("m2h.SeparatorStream: a block must be a torch tensor, got %s" % type(block).__name__)
        if block.dim() != 3 or block.shape[0] != self.R or block.shape[1] != 2:
            raise RuntimeError("m2h.SeparatorStream: expected a block [%d, 2, n], got %s" % (self.R, tuple(block.shape)))
        if block.dtype != torch.float32:
            raise RuntimeError("m2h.SeparatorStream: a block must be float32, got %s" % block.dtype)
        if block.device != self.sep.device:
            raise RuntimeError("m2h.SeparatorStream: the block lives on %s, the separator on %s" % (block.device, self.sep.device))
        self.received += block.shape[2]
        return self._step(block, False)

    @torch.no_grad()
    def flush(self):
        """The rest: every remaining segment, samples past the end zero, the output cut at the number of samples pushed.  Closes the stream."""
        if self.closed:
            raise RuntimeError("m2h.SeparatorStream: flush after flush")
        self.closed = True
        return self._step(torch.empty((self.R, 2, 0), device=self.sep.device, dtype=torch.float32), True)
