#!/usr/bin/env python3
"""Cost of m2h.audio.score (the Scorer): the Gram launch's rate against the chip's copy rate, and the float64 post-processing's share.

    python tools/score_bench.py --out profiles/score_bench.json      # every case, each in a child process under a timeout
    python tools/score_bench.py --case 16x3x600c2                    # one case in this process
    python tools/score_bench.py --align 1024 --align 8192 --out profiles/score_align_bench.json     # the aligned scorer, every case at every D
    python tools/score_bench.py --case 1x2x60c2 --align 8192         # one case of it in this process
    python tools/score_bench.py --spectral --out profiles/score_spectral_bench.json                 # the STFT distance, every case
    python tools/score_bench.py --case 16x3x600c1 --spectral         # one case of it in this process
    python tools/score_bench.py --spatial --out profiles/score_spatial_bench.json                   # the interaural cues, the two-channel cases
    python tools/score_bench.py --case 16x3x600c2 --spatial          # one case of it in this process
    python tools/score_bench.py --itd --out profiles/score_itd_bench.json                           # the broadband ITD, the two-channel cases
    python tools/score_bench.py --case 16x3x600c2 --itd              # one case of it in this process
    python tools/score_bench.py --stoi --out profiles/score_stoi_bench.json                         # STOI / ESTOI, every case
    python tools/score_bench.py --case 1x2x60c2 --stoi               # one case of it in this process
    python tools/score_bench.py --bss --out profiles/score_bss_bench.json                           # BSS-eval SDR / SIR / SAR at 512 taps, every case
    python tools/score_bench.py --case 1x2x60c2 --bss                # one case of it in this process

Cases (R recordings x S sources x seconds, C channels): 16x3x600 and 1x2x60, each with C = 1 and C = 2; per-second windows.  Timing: HIP
events on the stream around the Gram launch and around everything after it (Scorer._timing), summed over the repetitions.

  ms_per_call             first to last event of one Scorer.score
  gram_ms, gram_bytes_per_s   the m2h_score_gram launch: R C N L fp32 samples read (N = S + 3 rows per (recording, channel); with C = 2 both
                          channels' workgroups read the mixture) plus the fp64 rows written, over its time
  gram_share_of_copy_rate that rate over 6.29 TB/s, the chip's measured float4 copy rate
  post_share              m2h_score_windows and the float64 algebra (metrics_from_gram), as a share of ms_per_call
  torch_gram_ms           the same tile Grams from torch: the signals stacked, .double(), one batched matmul over the tiles and a sum; timed
                          before and after the new path (two recordings at a time above 4 GiB of float64 operands); its largest
                          relative difference from the kernel's Grams is recorded
With --align D (Scorer.score(..., align=D); the estimate is the unaligned case's, rolled by 137 samples):
  align_corr_ms           the m2h_align_corr launches of one call (one per group of recordings under max_corr_bytes)
  lag_pick_ms             the two m2h_score_windows over the tile correlations and lags_from_corr
  gram_lag_ms, post_ms    the m2h_score_gram_lag launch, and everything after it
  corr_flops_per_s        three 32768-point real transforms per (recording, channel, tile) at 2.5 n log2 n flops, over align_corr_ms
  torch_fft_corr_ms       the whole-recording correlation from torch.fft in the same run, before and after: rfft of the target and of the
                          estimate zero-padded to the next power of two at or above 2 L, conj(S) X, irfft, the lags -D .. D sliced out
                          (two recordings at a time above 2^26 points); whether its lags equal the Scorer's is recorded
With --spectral (the m2h_score_spectral launch of Scorer.score(..., spectral=True), timed alone with HIP events):
  spectral_ms             one launch: the seven fp64 sums of every (recording, channel, second) straight from the waveforms
  flops_unfolded, share_of_fp32_matrix_peak   3 signals x 32 frames x 2 (re, im) x 1023 x 1024 flop per tile -- the count of the unfolded
                          transform, which the kernel halves by folding x[n] +- x[1023 - n] -- over spectral_ms, against 157.3 TFLOP/s
  stored_spectrum_ms      the same sums from the existing pieces in the same run, before and after: m2h_stft_frames and the fp32 GEMM of
                          m2h.audio.stft.STFT on the three signals' seconds (frames and spectra stored), then torch float64 reductions,
                          one recording at a time; its largest relative difference from the kernel's sums is recorded
  extra_ms_in_score       what spectral=True adds to one Scorer.score (launch, two m2h_score_windows, spectral_from_sums)
With --spatial (the m2h_score_spatial launch of Scorer.score(..., spatial=True), timed alone with HIP events, twice; two-channel cases
only: the cues compare the ears, a mono case has none):
  spatial_ms              one launch: the [3, 32, 4] fp64 band sums of every (recording, second) straight from the waveforms
  spectral_c2_ms, spatial_over_spectral   m2h_score_spectral on the same tensors in the same run (the same six transforms per second)
  stored_spectrum_ms      the same sums from m2h_stft_frames, the fp32 GEMM of m2h.audio.stft.STFT on the six signals' seconds (frames and
                          spectra stored) and torch float64 reductions, before and after; its largest difference from the kernel's sums,
                          relative to the band's energies sqrt(PL PR) (a cross term may be near 0), is recorded
  extra_ms_in_score       what spatial=True adds to one Scorer.score (launch, two m2h_score_windows, spatial_from_sums)
With --itd (Scorer.score(..., itd=True); every launch timed alone with HIP events; two-channel cases only):
  itd_ms                  m2h_score_itd, one launch, twice: the [3, 256, 2] fp64 cross-spectra of every (recording, second)
  spatial_ms, itd_over_spatial   m2h_score_spatial on the same tensors in the same run, before and after (the same staging, twice the MFMAs)
  windows_ms, gcc_ms      the two m2h_score_windows over the tile sums, and m2h_itd_gcc on the whole recordings' and the windows' rows
  stored_gcc_ms           the same definition from the existing pieces in the same run, before and after: m2h_stft_frames and the fp32 GEMM
                          of m2h.audio.stft.STFT on the six signals' seconds (frames and spectra stored), torch float64 products and
                          sums, and GCC-PHAT as a torch float64 matmul against the cos / sin matrices, one recording at a time; the
                          largest difference of its functions from the kernels' is recorded
  extra_ms_in_score       what itd=True adds to one Scorer.score (the launches, itd_has_band, itd_from_gcc)
With --stoi (Scorer.score(..., stoi=True): the whole recording and every one-second window are ranges of the same launches):
  resample_ms, ranges_ms  m2h_stoi_resample and the five launches of m2h_stoi_ranges, each timed alone with HIP events, twice
  bytes                   what each stage has to move at least (every sample, frame slot and envelope counted once), from the shapes
  torch_stoi_ms           the yardstick in the same run, before and after: the same definition composed on the GPU from Resampler, unfold,
                          boolean-mask compaction (one host synchronisation per range), torch.fft.rfft and float64 tensor algebra, one
                          recording at a time; the largest difference of its six numbers from the kernels' is recorded
  extra_ms_in_score       what stoi=True adds to one Scorer.score
With --bss (Scorer.score(..., bss=512); per-stage HIP events on the stream, Scorer._timing):
  corr_ms, solve_ms, project_ms, metrics_ms   m2h_bss_corr with the m2h_score_windows that adds its tiles; bss_filters (torch float64: the
                          index gather and one Cholesky factorisation and solve per system); m2h_bss_project; the windows and bss_from_sums
  corr_flops_per_s, project_flops_per_s       2 S (S + 2) T Lr and 4 (S + 1) T (Lr + T - 1) flop per (recording, channel) over the stage's time,
                          and their share of the published fp64 vector peak, 78.6 TFLOP/s
  torch_bss_ms            the yardstick in the same run, before and after: the same definition composed on the GPU from torch.fft
                          correlations in float64, the same factorisations, and float64 conv1d for the two projections, one (recording,
                          channel) at a time; the largest difference of its nine numbers from the Scorer's, whole and track, is recorded
  extra_ms_in_score       what bss=512 adds to one Scorer.score
No threshold is set anywhere: the file reports what came out.  Every GPU step runs under its own timeout and the driver stops at the
first failure.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "move2hear-active-av-separation_amd"))

CASES = {"16x3x600c1": (16, 3, 600, 1, 10), "16x3x600c2": (16, 3, 600, 2, 10), "1x2x60c1": (1, 2, 60, 1, 200), "1x2x60c2": (1, 2, 60, 2, 200)}  # R, S, s, C, reps
ORDER = ("16x3x600c1", "16x3x600c2", "1x2x60c1", "1x2x60c2")
SEG = 16000
COPY_RATE = 6.29e12


def timed(fn, n):
    """milliseconds per call of fn over n calls, between two HIP events on the current stream"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def torch_gram(refs, est, mix, step):
    """[R, C, J, N] sums and [R, C, J, N, N] products from torch, `step` recordings at a time (L a multiple of the tile)"""
    import torch
    R, S, C, L = refs.shape
    sums, prods = [], []
    for r0 in range(0, R, step):
        r1 = min(r0 + step, R)
        a = torch.cat([refs[r0:r1].transpose(1, 2), est[r0:r1].unsqueeze(2), mix[r0:r1].unsqueeze(1).expand(r1 - r0, C, 2, L)], dim=2)   # [r, C, N, L]
        a = a.reshape(r1 - r0, C, S + 3, L // SEG, SEG).transpose(2, 3).double()                                                         # [r, C, J, N, tile]
        sums.append(a.sum(-1))
        prods.append(a @ a.transpose(-1, -2))
    return torch.cat(sums), torch.cat(prods)


def run_case(case):
    import torch
    from m2h import ops
    from m2h.audio.score import Scorer
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    dev = torch.device("cuda", 0)
    L, N = seconds * SEG, S + 3
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = 0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g)
    sc = Scorer(dev)
    step = R if R * C * N * L * 8 <= (4 << 30) else 2

    def staged():
        marks = []
        sc._timing = marks
        torch.cuda.synchronize()
        for _ in range(reps):
            sc.score(est, refs, mix)
        torch.cuda.synchronize()
        sc._timing = None
        ms = dict.fromkeys(("score_gram", "metrics"), 0.0)
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            if name != "start":
                ms[name] += e0.elapsed_time(e1)
        return {k: v / reps for k, v in ms.items()}

    # warm-up of every shape, and the two Grams against each other
    res0 = sc.score(est, refs, mix)
    tiles = ops.score_gram(refs, est, mix, SEG)
    ts, tp = torch_gram(refs, est, mix, step)
    iu = torch.triu_indices(N, N, device=dev)
    want = torch.cat([ts, tp[..., iu[0], iu[1]]], dim=-1)
    diff = float(((tiles - want).abs() / want.abs().clamp_min(1e-300)).max())
    finite = bool(torch.isfinite(res0["whole"]).all())
    del ts, tp, want, tiles
    torch.cuda.synchronize()

    yard = lambda: torch_gram(refs, est, mix, step)                                     # noqa: E731
    before = timed(yard, max(1, reps // 5))
    t = staged()
    after = timed(yard, max(1, reps // 5))
    gram_bytes = R * C * N * L * 4 + R * C * (L // SEG) * (N + N * (N + 1) // 2) * 8
    total = t["score_gram"] + t["metrics"]
    rate = gram_bytes / (t["score_gram"] * 1e-3)
    res = {"case": case, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps, "ms_per_call": total, "gram_ms": t["score_gram"],
           "gram_bytes": gram_bytes, "gram_bytes_per_s": rate, "gram_share_of_copy_rate": rate / COPY_RATE, "post_ms": t["metrics"],
           "post_share": t["metrics"] / total, "audio_s_per_s": R * seconds / (total * 1e-3), "torch_gram_ms": [before, after],
           "torch_gram_recordings_per_step": step, "torch_gram_over_kernel": 0.5 * (before + after) / t["score_gram"],
           "kernel_vs_torch_gram_max_rel": diff, "whole_scores_finite": finite, "whole_si_sdr_db": float(res0["whole"][0, 0, 0])}
    print(json.dumps(res))
    return res


FP32_MATRIX_PEAK = 157.3e12
SPECTRAL_FLOPS_PER_TILE = 3 * 32 * 2 * 1023 * 1024


def stored_spectrum_sums(stft, g, e, b):
    """[R, C, J, 7] float64 from the existing pieces: g, e, b [R, C, L] (L a multiple of a second) -> frames and spectra of every second
    stored by m2h_stft_frames and the fp32 GEMM of `stft`, then torch float64 reductions; one recording at a time"""
    import torch
    from m2h import _lib, ops
    lib = _lib.load()
    R, C, L = g.shape
    J, T, nb = L // SEG, 32, stft.nb
    out = []
    for r in range(R):
        wave = torch.stack([g[r], e[r], b[r]]).reshape(3 * C * J, SEG).contiguous()
        frames = torch.empty((3 * C * J * T, stft.ld), device=g.device)
        _lib.check(lib.m2h_stft_frames(ops._ptr(wave), ops._ptr(stft.window), ops._ptr(frames), 3 * C * J, SEG, T, stft.n_fft, stft.hop, stft.ld,
                                       ops._stream(wave)), "m2h_stft_frames")
        spec = ops.linear(frames, stft.W, None, name="stft.dft").view(3, C, J, T, stft.ld)
        re, im = spec[..., :nb].double(), spec[..., nb:2 * nb].double()
        mag = torch.sqrt(re * re + im * im)
        tot = lambda x: x.sum(dim=(-2, -1))                                              # noqa: E731
        dist = lambda i: (tot((mag[i] - mag[0]) ** 2), tot((re[i] - re[0]) ** 2 + (im[i] - im[0]) ** 2))   # noqa: E731
        out.append(torch.stack([tot(mag[0] ** 2), tot(mag[1] ** 2), tot(mag[2] ** 2), *dist(1), *dist(2)], dim=-1))
    return torch.stack(out)


def run_spectral_case(case):
    import torch
    from m2h import ops
    from m2h.audio.score import Scorer
    from m2h.audio.stft import STFT
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    dev = torch.device("cuda", 0)
    L = seconds * SEG
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = 0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g)
    sc, stft = Scorer(dev), STFT(dev)
    table = sc._spectral_table()
    base = mix if C == 2 else 0.5 * (mix[:, :1] + mix[:, 1:])

    kernel = lambda: ops.score_spectral(refs, est, mix, 0, table)                       # noqa: E731
    stored = lambda: stored_spectrum_sums(stft, refs[:, 0], est, base)                  # noqa: E731
    res0 = sc.score(est, refs, mix, spectral=True)                                      # warm-up of every shape
    got, want = kernel(), stored()
    diff = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
    del want
    torch.cuda.synchronize()
    n_stored = max(1, reps // 10)
    before = timed(stored, n_stored)
    ms = timed(kernel, reps)
    plain = timed(lambda: sc.score(est, refs, mix), reps)
    full = timed(lambda: sc.score(est, refs, mix, spectral=True), reps)
    after = timed(stored, n_stored)
    ms2 = timed(kernel, reps)
    flops = R * C * seconds * SPECTRAL_FLOPS_PER_TILE
    res = {"case": case, "spectral": True, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps, "tiles": R * C * seconds,
           "spectral_ms": [ms, ms2], "flops_unfolded": flops, "flops_per_s_unfolded": flops / (min(ms, ms2) * 1e-3),
           "share_of_fp32_matrix_peak": flops / (min(ms, ms2) * 1e-3) / FP32_MATRIX_PEAK, "stored_spectrum_ms": [before, after],
           "stored_spectrum_reps": n_stored, "stored_over_kernel": 0.5 * (before + after) / (0.5 * (ms + ms2)), "score_ms": plain,
           "score_spectral_ms": full, "extra_ms_in_score": full - plain, "audio_s_per_s": R * seconds / (full * 1e-3),
           "kernel_vs_stored_max_rel": diff, "stft_l2_whole": float(res0["spectral_whole"][0, 0, 0])}
    print(json.dumps(res))
    return res


def stored_spectrum_band_sums(stft, sig):
    """[R, J, 3, 32, 4] float64 from the existing pieces: sig [R, 3, 2, L] (L a multiple of a second) -> frames and spectra of every second
    stored by m2h_stft_frames and the fp32 GEMM of `stft`, then torch float64 reductions; one recording at a time"""
    import torch
    from m2h import _lib, ops
    lib = _lib.load()
    R, _, _, L = sig.shape
    J, T, nb = L // SEG, 32, stft.nb
    out = []
    for r in range(R):
        wave = sig[r].reshape(6 * J, SEG).contiguous()
        frames = torch.empty((6 * J * T, stft.ld), device=sig.device)
        _lib.check(lib.m2h_stft_frames(ops._ptr(wave), ops._ptr(stft.window), ops._ptr(frames), 6 * J, SEG, T, stft.n_fft, stft.hop, stft.ld,
                                       ops._stream(wave)), "m2h_stft_frames")
        spec = ops.linear(frames, stft.W, None, name="stft.dft").view(3, 2, J, T, stft.ld)
        re, im = spec[..., :nb].double(), spec[..., nb:2 * nb].double()
        lr, li, rr, ri = re[:, 0], im[:, 0], re[:, 1], im[:, 1]                              # [3, J, T, 512]
        terms = torch.stack([lr * lr + li * li, rr * rr + ri * ri, lr * rr + li * ri, li * rr - lr * ri], dim=-1)
        out.append(terms.view(3, J, T, 32, 16, 4).sum(dim=(2, 4)).transpose(0, 1))          # [J, 3, 32, 4]
    return torch.stack(out)


def run_spatial_case(case):
    import torch
    from m2h import ops
    from m2h.audio.score import Scorer
    from m2h.audio.stft import STFT
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    if C != 2:
        raise SystemExit("score_bench: --spatial compares the two ears; case %s is mono" % case)
    dev = torch.device("cuda", 0)
    L = seconds * SEG
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = 0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g)
    sc, stft = Scorer(dev), STFT(dev)
    table = sc._spectral_table()

    kernel = lambda: ops.score_spatial(refs, est, mix, 0, table)                        # noqa: E731
    yardstick = lambda: ops.score_spectral(refs, est, mix, 0, table)                    # noqa: E731
    stored = lambda: stored_spectrum_band_sums(stft, torch.stack([refs[:, 0], est, mix], dim=1))   # noqa: E731
    res0 = sc.score(est, refs, mix, spatial=True)                                       # warm-up of every shape
    got, want = kernel(), stored()
    scale = torch.sqrt(want[..., 0:1] * want[..., 1:2])
    diff = float(((got - want).abs() / scale).max())
    del want, scale
    yardstick()
    torch.cuda.synchronize()
    n_stored = max(1, reps // 10)
    before = timed(stored, n_stored)
    ms = timed(kernel, reps)
    spec = timed(yardstick, reps)
    plain = timed(lambda: sc.score(est, refs, mix), reps)
    full = timed(lambda: sc.score(est, refs, mix, spatial=True), reps)
    after = timed(stored, n_stored)
    ms2 = timed(kernel, reps)
    spec2 = timed(yardstick, reps)
    flops = R * C * seconds * SPECTRAL_FLOPS_PER_TILE
    res = {"case": case, "spatial": True, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps, "workgroups": 3 * R * seconds,
           "spatial_ms": [ms, ms2], "spectral_c2_ms": [spec, spec2], "spatial_over_spectral": (ms + ms2) / (spec + spec2), "flops_unfolded": flops,
           "flops_per_s_unfolded": flops / (min(ms, ms2) * 1e-3), "share_of_fp32_matrix_peak": flops / (min(ms, ms2) * 1e-3) / FP32_MATRIX_PEAK,
           "stored_spectrum_ms": [before, after], "stored_spectrum_reps": n_stored, "stored_over_kernel": 0.5 * (before + after) / (0.5 * (ms + ms2)),
           "score_ms": plain, "score_spatial_ms": full, "extra_ms_in_score": full - plain, "audio_s_per_s": R * seconds / (full * 1e-3),
           "kernel_vs_stored_max_rel_to_band_energy": diff, "ild_err_whole_db": float(res0["spatial_whole"][0, 0])}
    print(json.dumps(res))
    return res


def stored_spectrum_gcc(stft, sig, cs):
    """[R, 1 + J, 3, 257] float64, the ITD's GCC-PHAT functions (whole recording, then per-second windows) from the existing pieces:
    sig [R, 3, 2, L] (L a multiple of a second) -> frames and spectra of every second stored by m2h_stft_frames and the fp32 GEMM of `stft`,
    torch float64 products and sums, the PHAT weight, and a float64 matmul against cs = (cos, sin) [250, 257]; one recording at a time"""
    import torch
    from m2h import _lib, ops
    from m2h.audio.score import ITD_BINS
    lib = _lib.load()
    R, _, _, L = sig.shape
    J, T, nb = L // SEG, 32, stft.nb
    out = []
    for r in range(R):
        wave = sig[r].reshape(6 * J, SEG).contiguous()
        frames = torch.empty((6 * J * T, stft.ld), device=sig.device)
        _lib.check(lib.m2h_stft_frames(ops._ptr(wave), ops._ptr(stft.window), ops._ptr(frames), 6 * J, SEG, T, stft.n_fft, stft.hop, stft.ld,
                                       ops._stream(wave)), "m2h_stft_frames")
        spec = ops.linear(frames, stft.W, None, name="stft.dft").view(3, 2, J, T, stft.ld)
        re, im = spec[..., ITD_BINS[0]:ITD_BINS[1]].double(), spec[..., nb + ITD_BINS[0]:nb + ITD_BINS[1]].double()
        lr, li, rr, ri = re[:, 0], im[:, 0], re[:, 1], im[:, 1]                              # [3, J, T, 250]
        cre, cim = (lr * rr + li * ri).sum(dim=2), (li * rr - lr * ri).sum(dim=2)            # [3, J, 250]
        cre, cim = torch.cat([cre.sum(dim=1, keepdim=True), cre], dim=1), torch.cat([cim.sum(dim=1, keepdim=True), cim], dim=1)
        mag = torch.sqrt(cre * cre + cim * cim)
        safe = torch.where(mag > 0, mag, torch.ones_like(mag))
        g = (torch.where(mag > 0, cre / safe, torch.zeros_like(cre)) @ cs[0] + torch.where(mag > 0, cim / safe, torch.zeros_like(cim)) @ cs[1])
        out.append((g / float(ITD_BINS[1] - ITD_BINS[0])).transpose(0, 1))                   # [1 + J, 3, 257]
    return torch.stack(out)


def run_itd_case(case):
    import numpy as np
    import torch
    from m2h import ops
    from m2h.audio.score import ITD_BINS, ITD_LAGS, ITD_UPSAMPLE, Scorer
    from m2h.audio.stft import STFT
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    if C != 2:
        raise SystemExit("score_bench: --itd compares the two ears; case %s is mono" % case)
    dev = torch.device("cuda", 0)
    L, J = seconds * SEG, seconds
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    refs[:, :, 1, 5:] = 0.8 * refs[:, :, 0, :L - 5] + 0.1 * refs[:, :, 1, 5:]            # every source's right ear mostly its left one, 5 samples later
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = 0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g)
    sc, stft = Scorer(dev), STFT(dev)
    table, tab = sc._spectral_table(), sc._itd_table()
    k, i = np.arange(*ITD_BINS), np.arange(ITD_LAGS) - ITD_LAGS // 2
    ang = 2.0 * np.pi * ((k[:, None] * i[None, :]) % (1023 * ITD_UPSAMPLE)) / (1023 * ITD_UPSAMPLE)
    cs = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)])).to(dev)

    kernel = lambda: ops.score_itd(refs, est, mix, 0, table)                            # noqa: E731
    yardstick = lambda: ops.score_spatial(refs, est, mix, 0, table)                     # noqa: E731
    stored = lambda: stored_spectrum_gcc(stft, torch.stack([refs[:, 0], est, mix], dim=1), cs)   # noqa: E731
    res0 = sc.score(est, refs, mix, itd=True)                                           # warm-up of every shape
    tiles = kernel().view(R, 1, J, 1536)
    windows = lambda: torch.cat([ops.score_windows(tiles, 1, J, 1), ops.score_windows(tiles, J, 1, 1)], dim=2)   # noqa: E731
    ws = windows().view(R, 1 + J, 3, 256, 2)
    gcc = lambda: ops.itd_gcc(ws, tab, *ITD_BINS)                                       # noqa: E731
    want = stored()
    diff = float((res0["itd_gcc"] - want).abs().max())
    del want
    yardstick()
    torch.cuda.synchronize()
    n_stored = max(1, reps // 10)
    before = timed(stored, n_stored)
    spat = timed(yardstick, reps)
    ms = timed(kernel, reps)
    win_ms = timed(windows, reps)
    gcc_ms = timed(gcc, reps)
    plain = timed(lambda: sc.score(est, refs, mix), reps)
    full = timed(lambda: sc.score(est, refs, mix, itd=True), reps)
    after = timed(stored, n_stored)
    ms2 = timed(kernel, reps)
    spat2 = timed(yardstick, reps)
    flops = R * C * seconds * SPECTRAL_FLOPS_PER_TILE // 2                              # half the bins
    res = {"case": case, "itd": True, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps, "workgroups": 3 * R * seconds,
           "itd_ms": [ms, ms2], "spatial_ms": [spat, spat2], "itd_over_spatial": (ms + ms2) / (spat + spat2), "flops_unfolded": flops,
           "flops_per_s_unfolded": flops / (min(ms, ms2) * 1e-3), "share_of_fp32_matrix_peak": flops / (min(ms, ms2) * 1e-3) / FP32_MATRIX_PEAK,
           "windows_ms": win_ms, "gcc_ms": gcc_ms, "gcc_rows": R * (1 + J) * 3, "tile_sum_bytes": R * J * 1536 * 8,
           "stored_gcc_ms": [before, after], "stored_gcc_reps": n_stored, "stored_over_kernels": 0.5 * (before + after) / (0.5 * (ms + ms2) + win_ms + gcc_ms),
           "score_ms": plain, "score_itd_ms": full, "extra_ms_in_score": full - plain, "audio_s_per_s": R * seconds / (full * 1e-3),
           "kernels_vs_stored_max_abs_gcc": diff, "itd_whole_us": [float(v) for v in res0["itd_whole"][0, :3]], "peak_whole": [float(v) for v in res0["itd_whole"][0, 6:]]}
    print(json.dumps(res))
    return res


def torch_stoi(rs, win, x, y, b, ranges):
    """[C, len(ranges), 6] float64: STOI / ESTOI (m2h/audio/score.py, "STOI") of one recording composed from torch on the GPU.  x, y, b
    [C, L] at 16 kHz; ranges at 10 kHz.  The boolean mask costs one host synchronisation per range."""
    import torch
    dev, eps, clip = x.device, 2.0 ** -52, 1.0 + 10.0 ** 0.75
    edges = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
    bands = torch.zeros((257, 15), dtype=torch.float64, device=dev)
    for j in range(15):
        bands[edges[j]:edges[j + 1], j] = 1.0
    nan6 = torch.full((6,), float("nan"), dtype=torch.float64, device=dev)

    def normalise(a, dim):
        a = a - a.mean(dim=dim, keepdim=True)
        return a / (a.norm(dim=dim, keepdim=True) + eps)

    def pair(X, Y):                                                                     # [15, nseg, 30] each
        alpha = X.norm(dim=-1, keepdim=True) / (Y.norm(dim=-1, keepdim=True) + eps)
        d = (normalise(X, -1) * normalise(torch.minimum(alpha * Y, clip * X), -1)).sum(dim=(0, 2)) / 15.0
        de = (normalise(normalise(X, -1), 0) * normalise(normalise(Y, -1), 0)).sum(dim=(0, 2)) / 30.0
        return d.mean(), de.mean()

    out = []
    x10 = rs(torch.stack([x, y, b], dim=1).contiguous())                                # [C, 3, L10]
    for c in range(x.shape[0]):
        row = []
        for s, e in ranges:
            nf = max(0, -(-(e - s - 256) // 128))
            if nf < 31:
                row.append(nan6)
                continue
            fw = x10[c, :, s:e].unfold(-1, 256, 128)[:, :nf] * win                       # [3, nf, 256]
            en = 20.0 * torch.log10(fw[0].double().norm(dim=-1) + eps)
            kept = fw[:, en > en.max() - 40.0]                                           # (synchronises)
            K = kept.shape[1]
            if K < 31:
                row.append(nan6)
                continue
            ola = torch.zeros((3, (K + 1) * 128), device=dev)
            ola[:, :K * 128] += kept[..., :128].reshape(3, K * 128)
            ola[:, 128:] += kept[..., 128:].reshape(3, K * 128)
            spec = torch.fft.rfft(ola.unfold(-1, 256, 128)[:, :K - 1] * win, 512)       # [3, K - 1, 257]
            env = torch.sqrt((spec.real.double() ** 2 + spec.imag.double() ** 2) @ bands).transpose(1, 2)      # [3, 15, K - 1]
            seg = env.unfold(-1, 30, 1)                                                 # [3, 15, K - 30, 30]
            (d1, e1), (d2, e2) = pair(seg[0], seg[1]), pair(seg[0], seg[2])
            row.append(torch.stack([d1, e1, d2, e2, d1 - d2, e1 - e2]))
        out.append(torch.stack(row))
    return torch.stack(out)


def run_stoi_case(case):
    import torch
    from m2h import ops
    from m2h.audio import score as SC
    from m2h.audio.resample import Resampler
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    reps = max(1, reps // 5)
    dev = torch.device("cuda", 0)
    L = seconds * SEG
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = 0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g)
    sc, rs = SC.Scorer(dev), Resampler(16000, 10000, dev)
    table, win, tw = sc._stoi_tables()
    plan = SC.score_plan(L)
    sp = SC.stoi_plan(plan)
    base = mix if C == 2 else 0.5 * (mix[:, :1] + mix[:, 1:])

    rtab = sc._stoi_ranges(plan, sp)
    resample = lambda: ops.stoi_resample(refs, est, mix, 0, table)                      # noqa: E731
    x10 = resample()
    ranges = lambda: ops.stoi_ranges(x10, rtab, sp["total"], win, tw)                   # noqa: E731
    yard = lambda: torch.stack([torch_stoi(rs, win, refs[r, 0], est[r], base[r], sp["ranges"]) for r in range(R)])   # noqa: E731
    res0 = sc.score(est, refs, mix, stoi=True)                                          # warm-up of every shape
    got = torch.cat([res0["stoi_whole"][:, :, None], res0["stoi_track"]], dim=2)
    want = yard()
    diff = float(torch.nan_to_num((got - want).abs(), nan=0.0).max())
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(want)))
    del want
    torch.cuda.synchronize()
    before = timed(yard, 1)
    t_res, t_rng = timed(resample, reps), timed(ranges, reps)
    plain = timed(lambda: sc.score(est, refs, mix), reps)
    full = timed(lambda: sc.score(est, refs, mix, stoi=True), reps)
    after = timed(yard, 1)
    t_res2, t_rng2 = timed(resample, reps), timed(ranges, reps)
    RC, L10, slots = R * C, sp["L10"], sp["total"]
    frames = sum(SC.stoi_frames(e - s) for s, e in sp["ranges"])
    samples = sum(e - s for s, e in sp["ranges"])
    nbytes = {"resample": RC * ((3 if C == 2 else 4) * L * 4 + 3 * L10 * 4), "energy": RC * (samples * 4 + frames * 8), "mask": RC * frames * (8 + 4),
              "envelope": RC * (3 * samples * 4 + frames * 4 + 45 * frames * 8), "segments": RC * frames * (45 * 8 + 4 * 8), "mean": RC * frames * 4 * 8}
    kernel = 0.5 * (t_res + t_res2 + t_rng + t_rng2)
    res = {"case": case, "stoi": True, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps, "ranges": len(sp["ranges"]),
           "frame_slots": slots, "frames": frames, "resample_ms": [t_res, t_res2], "ranges_ms": [t_rng, t_rng2], "bytes": nbytes,
           "resample_bytes_per_s": nbytes["resample"] / (min(t_res, t_res2) * 1e-3), "torch_stoi_ms": [before, after], "torch_stoi_reps": 1,
           "torch_stoi_host_synchronisations": RC * len(sp["ranges"]), "torch_over_kernels": 0.5 * (before + after) / kernel, "score_ms": plain,
           "score_stoi_ms": full, "extra_ms_in_score": full - plain, "audio_s_per_s": R * seconds / (full * 1e-3),
           "kernels_vs_torch_max_abs": diff, "nan_in_the_same_places": same_nan, "stoi_whole": float(res0["stoi_whole"][0, 0, 0]),
           "estoi_whole": float(res0["stoi_whole"][0, 0, 1]), "kept_frames_whole": int(res0["stoi_frames"][0, 0, 0])}
    print(json.dumps(res))
    return res


FP64_VECTOR_PEAK = 78.6e12     # flop/s, the published fp64 vector peak of the MI355X
BSS_TAPS = 512


def torch_bss(s, ys, j, T, tile, chunk=1 << 20):
    """The ten sums of every tile of one (recording, channel), composed from torch: s [S, L] and ys [2, L] fp32 (estimate, baseline), L a
    multiple of the tile -> [J, 10] float64.  torch.fft correlations, Cholesky, float64 conv1d in chunks of `chunk` outputs."""
    import torch
    import torch.nn.functional as F
    S, L = s.shape
    N = L + T - 1
    nfft = 1 << (N - 1).bit_length()
    sd, yd = s.double(), ys.double()
    Fs, Fy = torch.fft.rfft(sd, nfft), torch.fft.rfft(yd, nfft)

    def lags(A, B):                                                                     # sum_t a[t] b[t + d], d = -(T - 1) .. T - 1
        c = torch.fft.irfft(torch.conj(A) * B, nfft)
        return torch.cat([c[..., nfft - (T - 1):], c[..., :T]], dim=-1)

    a = torch.arange(T, device=s.device)
    idx = (T - 1) + a[:, None] - a[None, :]
    c = torch.stack([lags(Fs[i:i + 1], Fs) for i in range(S)])                          # [S, S, 2 T - 1]
    p = torch.stack([lags(Fs[i:i + 1], Fy)[:, T - 1:] for i in range(S)])               # [S, 2, T]
    del Fs, Fy
    G = c[:, :, idx].permute(0, 2, 1, 3).reshape(S * T, S * T)
    h = torch.cholesky_solve(p.permute(0, 2, 1).reshape(S * T, 2), torch.linalg.cholesky_ex(G)[0])
    g = torch.cholesky_solve(p[j].t().contiguous(), torch.linalg.cholesky_ex(c[j, j][idx])[0])
    w = torch.zeros((4, S, T), dtype=torch.float64, device=s.device)                    # P and s_t of the estimate, then of the baseline
    w[0], w[2] = h[:, 0].reshape(S, T), h[:, 1].reshape(S, T)
    w[1, j], w[3, j] = g[:, 0], g[:, 1]
    w = w.flip(-1).contiguous()                                                         # conv1d correlates
    inp = F.pad(sd, (T - 1, T - 1))[None]
    comp = torch.cat([F.conv1d(inp[:, :, n0:min(n0 + chunk, N) + T - 1], w)[0] for n0 in range(0, N, chunk)], dim=-1)     # [4, N]
    yz = F.pad(yd, (0, T - 1))
    sq = []
    for q in range(2):
        P, st, y = comp[2 * q], comp[2 * q + 1], yz[q]
        sq += [st * st, (y - st) ** 2, (P - st) ** 2, P * P, (y - P) ** 2]
    sq = torch.stack(sq)                                                                # [10, N]
    sums = sq[:, :L].reshape(10, L // tile, tile).sum(-1)
    sums[:, -1] += sq[:, L:].sum(-1)                                                    # the last tile owns the tail
    return sums.t()


def run_bss_case(case):
    import torch
    from m2h.audio import score as SC
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    reps = max(1, reps // 10)
    dev = torch.device("cuda", 0)
    L, T = seconds * SEG, BSS_TAPS
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = 0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g)
    sc = SC.Scorer(dev)
    plan = SC.score_plan(L)
    base = mix if C == 2 else 0.5 * (mix[:, :1] + mix[:, 1:])
    J = plan["J"]

    def yard():
        rows = []
        for r in range(R):
            for c in range(C):
                tiles = torch_bss(refs[r, :, c], torch.stack([est[r, c], base[r, c]]), 0, T, SEG)
                rows.append(torch.cat([tiles.sum(0, keepdim=True), tiles]))              # whole, then the one-second track
        return SC.bss_from_sums(torch.stack(rows).view(R, C, 1 + J, 10))

    def staged():
        marks = []
        sc._timing = marks
        torch.cuda.synchronize()
        for _ in range(reps):
            sc.score(est, refs, mix, bss=T)
        torch.cuda.synchronize()
        sc._timing = None
        ms = {}
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            if name != "start":
                ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1) / reps
        return ms

    res0 = sc.score(est, refs, mix, bss=T)                                              # warm-up of every shape
    got = torch.cat([res0["bss_whole"][:, :, None], res0["bss_track"]], dim=2)
    want = yard()
    diff = float(torch.nan_to_num((got - want).abs(), nan=0.0, posinf=0.0).max())
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(want)))
    del want
    torch.cuda.synchronize()
    before = timed(yard, 1)
    ms = staged()
    plain = timed(lambda: sc.score(est, refs, mix), reps)
    full = timed(lambda: sc.score(est, refs, mix, bss=T), reps)
    after = timed(yard, 1)
    ms2 = staged()
    RC = R * C
    flops = {"corr": RC * 2.0 * S * (S + 2) * T * L, "project": RC * 4.0 * (S + 1) * T * (L + T - 1)}
    kernels = 0.5 * sum(ms[k] + ms2[k] for k in ("bss_corr", "bss_solve", "bss_project", "bss_metrics"))
    per = C * J * S * (S + 2) * T * 8
    res = {"case": case, "bss": T, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps,
           "corr_ms": [ms["bss_corr"], ms2["bss_corr"]], "solve_ms": [ms["bss_solve"], ms2["bss_solve"]],
           "project_ms": [ms["bss_project"], ms2["bss_project"]], "metrics_ms": [ms["bss_metrics"], ms2["bss_metrics"]],
           "systems": 2 * RC, "system_size": S * T, "corr_bytes_per_recording": per, "corr_groups": -(-R // max(1, sc.max_corr_bytes // per)),
           "flops": flops, "corr_flops_per_s": flops["corr"] / (min(ms["bss_corr"], ms2["bss_corr"]) * 1e-3),
           "project_flops_per_s": flops["project"] / (min(ms["bss_project"], ms2["bss_project"]) * 1e-3),
           "torch_bss_ms": [before, after], "torch_bss_reps": 1, "torch_over_bss_stages": 0.5 * (before + after) / kernels,
           "score_ms": plain, "score_bss_ms": full, "extra_ms_in_score": full - plain, "audio_s_per_s": R * seconds / (full * 1e-3),
           "scorer_vs_torch_max_abs_db": diff, "nan_in_the_same_places": same_nan, "sdr_whole_db": float(res0["bss_whole"][0, 0, 0]),
           "si_sdr_whole_db": float(res0["whole"][0, 0, 0])}
    res["corr_share_of_fp64_vector_peak"] = res["corr_flops_per_s"] / FP64_VECTOR_PEAK
    res["project_share_of_fp64_vector_peak"] = res["project_flops_per_s"] / FP64_VECTOR_PEAK
    print(json.dumps(res))
    return res


def run_align_case(case, D):
    import torch
    from m2h.audio.score import Scorer, lags_from_corr
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, C, reps = CASES[case]
    dev = torch.device("cuda", 0)
    L = seconds * SEG
    g = torch.Generator(device=dev).manual_seed(7)
    refs = torch.randn((R, S, C, L), device=dev, generator=g) * 0.1 + 0.01
    mix = torch.stack([refs[:, :, 0].mean(1), refs[:, :, C - 1].mean(1)], dim=1) + 0.02 * torch.randn((R, 2, L), device=dev, generator=g)
    est = torch.roll(0.8 * refs[:, 0] + 0.03 * torch.randn((R, C, L), device=dev, generator=g), 137, dims=-1)
    sc = Scorer(dev)
    nfft = 1 << (2 * L - 1).bit_length()
    step = R if R * nfft <= (1 << 26) else 2

    def torch_corr():
        """[R, C, 2 D + 1]: sum_t s[t] x[t + d] over the whole recording, d = -D .. D, from torch.fft"""
        rows = []
        for r0 in range(0, R, step):
            s, x = torch.fft.rfft(refs[r0:r0 + step, 0], nfft), torch.fft.rfft(est[r0:r0 + step], nfft)
            c = torch.fft.irfft(torch.conj(s) * x, nfft)
            rows.append(torch.cat([c[..., nfft - D:], c[..., :D + 1]], dim=-1))
        return torch.cat(rows)

    def staged():
        marks = []
        sc._timing = marks
        torch.cuda.synchronize()
        for _ in range(reps):
            sc.score(est, refs, mix, align=D)
        torch.cuda.synchronize()
        sc._timing = None
        ms = dict.fromkeys(("align_corr", "lag_pick", "score_gram", "metrics"), 0.0)
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            if name != "start":
                ms[name] += e0.elapsed_time(e1)
        return {k: v / reps for k, v in ms.items()}

    res0 = sc.score(est, refs, mix, align=D)                                            # warm-up of every shape
    lag = res0["lag"]
    torch_lag = lags_from_corr(torch_corr().double())
    torch.cuda.synchronize()
    before = timed(torch_corr, max(1, reps // 2))
    t = staged()
    after = timed(torch_corr, max(1, reps // 2))
    J = res0["plan"]["J"]
    flops = 3 * R * C * J * 2.5 * 32768 * 15
    total = sum(t.values())
    res = {"case": case, "align": D, "R": R, "S": S, "C": C, "audio_seconds_per_recording": seconds, "reps": reps, "ms_per_call": total,
           "align_corr_ms": t["align_corr"], "lag_pick_ms": t["lag_pick"], "gram_lag_ms": t["score_gram"], "post_ms": t["metrics"],
           "corr_bytes": R * C * J * (2 * D + 1) * 8, "corr_groups": -(-R // max(1, sc.max_corr_bytes // (C * J * (2 * D + 1) * 8))),
           "corr_flops_per_s": flops / (t["align_corr"] * 1e-3), "audio_s_per_s": R * seconds / (total * 1e-3),
           "torch_fft_corr_ms": [before, after], "torch_fft_points": nfft, "torch_fft_recordings_per_step": step,
           "torch_fft_over_align_corr_and_pick": 0.5 * (before + after) / (t["align_corr"] + t["lag_pick"]),
           "lags_all_137": bool((lag == 137).all()), "torch_fft_lags_equal": bool((torch_lag == lag).all()),
           "whole_scores_finite": bool(torch.isfinite(res0["whole"]).all()), "whole_si_sdr_db": float(res0["whole"][0, 0, 0])}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    ap.add_argument("--align", type=int, action="append", default=None, metavar="D", help="measure the aligned scorer at this largest lag (repeat)")
    ap.add_argument("--spectral", action="store_true", help="measure the STFT distance's launch (Scorer.score(..., spectral=True))")
    ap.add_argument("--spatial", action="store_true", help="measure the interaural cues' launch (Scorer.score(..., spatial=True)); two-channel cases")
    ap.add_argument("--itd", action="store_true", help="measure the broadband ITD's launches (Scorer.score(..., itd=True)); two-channel cases")
    ap.add_argument("--stoi", action="store_true", help="measure STOI / ESTOI (Scorer.score(..., stoi=True)) against its composition from torch")
    ap.add_argument("--bss", action="store_true", help="measure BSS-eval SDR / SIR / SAR at 512 taps (Scorer.score(..., bss=512)) against its composition from torch")
    ap.add_argument("--out", default=None, help="driver mode: JSON file for all cases")
    ap.add_argument("--timeout", type=int, default=120, help="driver mode: seconds per case")
    args = ap.parse_args()
    if (args.spectral or args.spatial or args.itd or args.stoi or args.bss) and args.align or args.spectral + args.spatial + args.itd + args.stoi + args.bss > 1:
        raise SystemExit("score_bench: --spectral, --spatial, --itd, --stoi, --bss and --align are measured separately")
    if args.case is not None:
        if args.bss:
            run_bss_case(args.case)
        elif args.stoi:
            run_stoi_case(args.case)
        elif args.itd:
            run_itd_case(args.case)
        elif args.spatial:
            run_spatial_case(args.case)
        elif args.spectral:
            run_spectral_case(args.case)
        elif args.align:
            for D in args.align:
                run_align_case(args.case, D)
        else:
            run_case(args.case)
        return
    results = []
    for case, D in [(case, D) for D in (args.align or [None]) for case in ORDER if CASES[case][3] == 2 or not (args.spatial or args.itd)]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case] + ([] if D is None else ["--align", str(D)]) + \
            (["--spectral"] if args.spectral else []) + (["--spatial"] if args.spatial else []) + (["--itd"] if args.itd else []) + (["--stoi"] if args.stoi else []) + (["--bss"] if args.bss else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-4000:])
            raise SystemExit("score_bench: case %s failed with status %d; stopping" % (case, r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        results.append(json.loads(line))
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/score_bench.py", "device": "MI355X (gfx950)", "copy_rate_bytes_per_s": COPY_RATE,
                       **({"fp32_matrix_peak_flops_per_s": FP32_MATRIX_PEAK} if args.spectral or args.spatial or args.itd else {}),
                       **({"fp64_vector_peak_flops_per_s": FP64_VECTOR_PEAK} if args.bss else {}), "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
