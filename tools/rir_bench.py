#!/usr/bin/env python3
"""Rate of m2h.audio.acoustics (RoomAcoustics): RIRs analysed per second, each launch's share of the time, and the same definition
composed from torch.fft for comparison.

    python tools/rir_bench.py --out profiles/rir_bench.json

Cases (leading shape, taps): 1x2 RIRs of 16000 taps; 16x3x600 RIRs of 16000 taps (a moving listener: one RIR per second of a 600 s batch).
Timing: HIP events on the stream after every launch of every chunk (RoomAcoustics._timing); a launch's time is the sum of its
intervals, the time per batch is first-to-last event, the median over the timed repetitions.

The composed path states the same definition with what torch offers: onset by a masked argmax, the six band signals at full length by
torch.fft.rfft / irfft at 32768 points, the bins by a gather from the onset, the decay curve by flip / cumsum, the regressions by masked
sums, the IACF by 33 shifted products.  It stores six full-length band signals and a decay curve per RIR and ear, so it runs in chunks of
--composed-chunk RIRs.  The driver times composed, new, composed: the two composed runs give that path's run-to-run spread.  No
threshold is set anywhere: the file reports what came out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "move2hear-active-av-separation_amd"))

CASES = {"1x2": ((1, 2), 16000, 50), "16x3x600": ((16, 3, 600), 16000, 3)}      # leading shape, taps, timed repetitions
STAGES = ("rir_onset", "rir_band_energy", "rir_decay")
RANGES = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))


def composed(h, taps_spec, nfft):
    """h [Q, Lr, 2] fp32 -> params [Q, 2, 7, 7], iacc [Q, 7, 2] in fp64: the definition from torch ops, band signals at full length."""
    import torch
    Q, Lr, _ = h.shape
    dev = h.device
    mag = h.abs()
    pk = mag.amax(1, keepdim=True)
    first = torch.where(mag >= 0.1 * pk, torch.arange(Lr, device=dev)[None, :, None], Lr).amin(1)
    n0 = first.amin(1).clamp(max=Lr - 1)                                        # [Q]
    H = torch.fft.rfft(h, n=nfft, dim=1)                                        # [Q, bins, 2]
    bands = [torch.nn.functional.pad(h, (0, 0, 2048, 2048))]                    # sample n at index n + 2048
    for b in range(taps_spec.shape[0]):
        bands.append(torch.roll(torch.fft.irfft(H * taps_spec[b][None, :, None], n=nfft, dim=1), 2048, dims=1)[:, :Lr + 4096])
    y = torch.stack(bands, 1)                                                   # [Q, 7, Lr + 4096, 2]
    nbs = -(-Lr // 16)
    t = torch.arange(nbs * 16, device=dev)[None, :] + n0[:, None]               # [Q, nbs * 16]
    idx = (t.clamp(max=Lr - 1) + 2048)[:, None, :, None].expand(Q, 7, nbs * 16, 2)
    seg = torch.gather(y, 2, idx).double() * (t < Lr)[:, None, :, None]
    E = (seg * seg).reshape(Q, 7, nbs, 16, 2).sum(3).permute(0, 3, 1, 2)        # [Q, 2, 7, nbs]
    edc = E.flip(-1).cumsum(-1).flip(-1)
    lv = 10.0 * torch.log10(edc / edc[..., :1])
    ti = torch.arange(nbs, device=dev, dtype=torch.float64) / 1000.0
    out = []
    for lo, hi in RANGES:
        m = ((lv <= lo) & (lv >= hi)).double()
        n = m.sum(-1)
        lvz = torch.where(m > 0, lv, torch.zeros_like(lv))
        mt, ml = (m * ti).sum(-1) / n, lvz.sum(-1) / n
        x = (ti - mt[..., None]) * m
        slope = (x * (lvz - ml[..., None] * m)).sum(-1) / (x * x).sum(-1)
        out.append(torch.where(n >= 2, -60.0 / slope, torch.full_like(slope, float("nan"))))
    tot = E.sum(-1)
    for k in (50, 80):
        out.append(10.0 * torch.log10(E[..., :k].sum(-1) / E[..., k:].sum(-1)))
    out.append(E[..., :50].sum(-1) / tot)
    out.append((E * (torch.arange(nbs, device=dev, dtype=torch.float64) + 0.5) / 1000.0).sum(-1) / tot)
    params = torch.stack(out, -1)
    w = torch.arange(1280, device=dev)[None, :] + n0[:, None] + 2048
    L = torch.gather(y[..., 0], 2, w[:, None, :].expand(Q, 7, 1280)).double()
    cross = []
    for tau in range(-16, 17):
        Rt = torch.gather(y[..., 1], 2, (w + tau)[:, None, :].expand(Q, 7, 1280)).double()
        cross.append((L * Rt).sum(-1))
        if tau == 0:
            er = (Rt * Rt).sum(-1)
    iacf = torch.stack(cross, -1).abs() / torch.sqrt((L * L).sum(-1) * er)[..., None]
    val, arg = iacf.max(-1)
    return params, torch.stack([val, arg.double() - 16.0], -1)


def run_case(case, composed_chunk):
    import numpy as np
    import torch
    from m2h.audio import acoustics as A
    if not torch.cuda.is_available():
        raise SystemExit("rir_bench: no GPU; this measurement has no CPU path")
    lead, Lr, reps = CASES[case]
    dev = torch.device("cuda", 0)
    Q = int(np.prod(lead))
    g = torch.Generator(device=dev).manual_seed(7)
    env = torch.pow(10.0, -3.0 * torch.arange(Lr, device=dev) / (0.5 * A.RATE))          # T60 = 0.5 s
    rirs = torch.randn(lead + (Lr, 2), device=dev, generator=g) * env[:, None] * 0.2
    rirs[..., 40, 0] += 1.0
    rirs[..., 45, 1] += 0.7
    ra = A.RoomAcoustics(dev)
    nfft = 32768
    spec = np.zeros((6, nfft))
    spec[:, :2049], spec[:, nfft - 2048:] = A.octave_taps()[:, 2048:], A.octave_taps()[:, :2048]
    taps_spec = torch.from_numpy(np.fft.rfft(spec, axis=1).real.astype(np.float32)).to(dev)
    flat = rirs.reshape(Q, Lr, 2)

    def time_new():
        times = []
        for i in range(reps + 1):
            ra._timing = []
            out = ra.analyze(rirs)
            torch.cuda.synchronize()
            marks, ra._timing = ra._timing, None
            per = {s: 0.0 for s in STAGES}
            for (_, e0), (s, e1) in zip(marks[:-1], marks[1:]):
                per[s] += e0.elapsed_time(e1)
            if i:                                                                # (the first run warms up)
                times.append((marks[0][1].elapsed_time(marks[-1][1]), per))
        times.sort(key=lambda t: t[0])
        return times[len(times) // 2], out

    def time_composed():
        times = []
        for i in range(min(reps, 3) + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs = [composed(flat[q:q + composed_chunk], taps_spec, nfft) for q in range(0, Q, composed_chunk)]
            e1.record()
            torch.cuda.synchronize()
            if i:
                times.append(e0.elapsed_time(e1))
        return sorted(times)[len(times) // 2], (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))

    c1, (cp, ci) = time_composed()
    (ms, per), out = time_new()
    c2, _ = time_composed()
    p = out["params"].reshape(Q, 2, 7, 7)
    ok = torch.isfinite(p) & torch.isfinite(cp)
    rel = float(((p - cp).abs()[ok] / cp.abs()[ok].clamp(min=1e-3)).max())
    return {"case": case, "rirs": Q, "taps": Lr, "ms_per_batch": ms, "rirs_per_second": Q / (ms * 1e-3),
            "launch_share": {s: per[s] / ms for s in STAGES}, "launch_ms": per,
            "composed_ms_per_batch": [c1, c2], "composed_chunk": composed_chunk, "ratio_composed_over_new": min(c1, c2) / ms,
            "worst_relative_difference_of_params_between_the_paths": rel,
            "lags_equal": bool((out["iacc"].reshape(Q, 7, 2)[..., 1] == ci[..., 1]).all())}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=None)
    parser.add_argument("--case", action="append", choices=sorted(CASES), default=None)
    parser.add_argument("--composed-chunk", type=int, default=1200)
    args = parser.parse_args()
    rows = []
    for case in args.case or list(CASES):
        rows.append(run_case(case, args.composed_chunk))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/rir_bench.py", "cases": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
