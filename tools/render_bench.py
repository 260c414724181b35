#!/usr/bin/env python3
"""Rate of m2h.audio.render (the Auralizer): seconds of audio rendered per second, and each launch's share of the time.

    python tools/render_bench.py --out profiles/render_bench.json      # every case, each in a child process under a timeout
    python tools/render_bench.py --case 16x3x600 [--path new|composed|both] [--max-blocks N]     # one case in this process

Cases (R recordings x S sources x seconds, RIR taps): 1x2x60 with Lr = 8000; 16x3x600 with Lr = 16000; 1x2x60p3 with Lr = 48000 (three
partitions).  Static scenes, default gains, no tail, no images.  Timing: HIP events on the stream after every launch group of every
chunk (Auralizer._timing); a launch's time is the sum of its intervals, the rate is R x seconds of audio over first-to-last event.

--path composed is the same mixture from what existed before the Auralizer: whole-length torch.fft.rfft of the sources and of both ears
of the RIRs at the next power of two above L + Lr - 1, the product, torch.fft.irfft, the cut at L and the gained sum over the sources.
The driver times composed, new, composed: the two composed runs give that path's run-to-run spread, which is the margin of the
comparison; the rel-L1 between the two results is recorded.  No threshold is set anywhere: the file reports what came out.
Every GPU step runs under its own timeout and the driver stops at the first failure.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "move2hear-active-av-separation_amd"))

CASES = {"1x2x60": (1, 2, 60, 8000, 200), "16x3x600": (16, 3, 600, 16000, 5), "1x2x60p3": (1, 2, 60, 48000, 200)}   # R, S, seconds, Lr, timed repetitions
STAGES = ("render_spectra", "render_frames", "render_mix")
SEG = 16000


def composed_render(sources, rirs, gains, mark):
    import torch
    L, Lr = sources.shape[-1], rirs.shape[2]
    nfft = 1 << (L + Lr - 2).bit_length()
    mark("start")
    X = torch.fft.rfft(sources, n=nfft)                        # [R, S, bins]
    H = torch.fft.rfft(rirs, n=nfft, dim=2)                    # [R, S, bins, 2]
    mark("rfft")
    Y = X.unsqueeze(-1) * H
    mark("product")
    images = torch.fft.irfft(Y, n=nfft, dim=2)[:, :, :L]       # [R, S, L, 2]
    mark("irfft")
    mix = (images * gains[:, :, None, None]).sum(1).transpose(1, 2).contiguous()
    mark("mix")
    return mix


def run_case(case, path, max_blocks=None):
    import torch
    from m2h.audio.render import DEFAULT_MAX_BLOCKS, Auralizer, render_plan, chunk_scratch_bytes
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: no GPU; this measurement has no CPU path")
    R, S, seconds, Lr, reps = CASES[case]
    dev = torch.device("cuda", 0)
    L = seconds * SEG
    g = torch.Generator(device=dev).manual_seed(7)
    sources = torch.randn((R, S, L), device=dev, generator=g) * 0.1
    env = torch.exp(-torch.log(torch.tensor(30.0)) * torch.arange(Lr, device=dev) / (Lr - 1))
    rirs = torch.randn((R, S, Lr, 2), device=dev, generator=g) * env[None, None, :, None]
    gains = torch.full((R, S), 1.0 / S, device=dev)
    aur = Auralizer(dev, max_blocks=max_blocks or DEFAULT_MAX_BLOCKS)
    plan = render_plan(L, Lr, 1, aur.max_blocks)

    marks = []

    def mark(stage):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(dev))
        marks.append((stage, ev))

    def new_path():
        aur._timing = marks
        try:
            return aur.render(sources, rirs)
        finally:
            aur._timing = None

    def composed_path():
        return composed_render(sources, rirs, gains, mark)

    def timed(fn, stages):
        del marks[:]
        torch.cuda.synchronize()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        stage_ms = dict.fromkeys(stages, 0.0)
        total = 0.0
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            if name == "start":
                continue                                  # between two repetitions
            dt = e0.elapsed_time(e1)
            stage_ms[name] += dt
            total += dt
        return {"audio_s_per_s": R * seconds * reps / (total * 1e-3), "ms_per_run": total / reps, "stage_share": {k: v / total for k, v in stage_ms.items()}}

    res = {"case": case, "R": R, "S": S, "audio_seconds_per_recording": seconds, "Lr": Lr, "partitions": plan["Pn"], "reps": reps,
           "max_blocks": aur.max_blocks, "chunks": len(plan["chunks"]),
           "chunk_scratch_bytes": max(chunk_scratch_bytes(plan, ch, R * S, 1) for ch in plan["chunks"])}
    order = {"new": ("new",), "composed": ("composed",), "both": ("composed", "new", "composed")}[path]
    fns = {"new": (new_path, STAGES), "composed": (composed_path, ("rfft", "product", "irfft", "mix"))}
    outs = {}
    for name in set(order):                               # warm-up: every shape of the timed window
        outs[name] = fns[name][0]()
    torch.cuda.synchronize()
    if len(outs) == 2:
        a, b = outs["new"].double(), outs["composed"].double()
        res["new_vs_composed_rel_l1"] = float((a - b).abs().sum() / b.abs().sum())
        res["finite"] = bool(torch.isfinite(outs["new"]).all())
    del outs
    for name in order:
        res.setdefault(name, []).append(timed(*fns[name]))
    if path == "both":
        c = [r["audio_s_per_s"] for r in res["composed"]]
        res["composed_spread"] = abs(c[0] - c[1]) / max(c)
        res["speedup_over_composed"] = res["new"][0]["audio_s_per_s"] / (0.5 * (c[0] + c[1]))
        res["composed_is_faster"] = bool(min(c) > res["new"][0]["audio_s_per_s"])
        share = res["new"][0]["stage_share"]
        res["bounding_launch"] = max(share, key=share.get)
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), default=None)
    ap.add_argument("--path", choices=["new", "composed", "both"], default="both")
    ap.add_argument("--max-blocks", type=int, default=None, help="the Auralizer's max_blocks (default: its own)")
    ap.add_argument("--out", default=None, help="driver mode: JSON file for all cases")
    ap.add_argument("--timeout", type=int, default=240, help="driver mode: seconds per case")
    args = ap.parse_args()
    if args.case is not None:
        run_case(args.case, args.path, args.max_blocks)
        return
    results = []
    for case in ("1x2x60", "16x3x600", "1x2x60p3"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--path", args.path]
        if args.max_blocks:
            cmd += ["--max-blocks", str(args.max_blocks)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-4000:])
            raise SystemExit("render_bench: case %s failed with status %d; stopping" % (case, r.returncode))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        results.append(json.loads(line))
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/render_bench.py", "device": "MI355X (gfx950)", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
