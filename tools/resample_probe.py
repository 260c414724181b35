#!/usr/bin/env python3
"""The rate conversion alone, for a profiler: `reps` launches of m2h_resample_poly over rows x seconds of noise.

    python tools/resample_probe.py --f-in 44100 --f-out 16000 [--rows 32] [--seconds 100] [--reps 5]
    rocprofv3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT ... -d prof_out/rs -o c --output-format csv -- python tools/resample_probe.py ...
    python tools/pmc_summary.py prof_out/rs/*counter_collection.csv

Prints one JSON line: milliseconds per launch and the HBM bytes per second of reading the input once and writing the output once.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "move2hear-active-av-separation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--f-in", type=int, default=44100)
    ap.add_argument("--f-out", type=int, default=16000)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from m2h.audio.resample import Resampler
    dev = torch.device("cuda", 0)
    rs = Resampler(args.f_in, args.f_out, dev)
    x = torch.randn((args.rows, args.seconds * args.f_in), device=dev) * 0.05
    y = rs(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        rs(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    print(json.dumps({"ratio": "%d/%d" % (rs.up, rs.down), "taps_per_output": rs.T, "rows": args.rows, "L_in": x.shape[1], "L_out": y.shape[1],
                      "ms": ms, "hbm_gb_per_s": 4 * (x.numel() + y.numel()) / (ms * 1e-3) / 1e9, "products": y.numel() * rs.T}))


if __name__ == "__main__":
    main()
