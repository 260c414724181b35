#!/usr/bin/env python3
"""Separate one sound class out of a binaural recording of any length:

    python separate.py --ckpt F --in mix.wav --target-class K --out out.wav [--no-memory] [--math fp32|bf16x3] [--resample] [--overlap 1|2|4]

``--ckpt``: a passive-separator checkpoint or a PPO checkpoint (``{"state_dict", "config"}`` file or a bare state dict, with or
without the ``actor_critic.`` root).  ``--in``: a two-channel WAV at 16 kHz, int16 or float32.  The output is a mono WAV of the
same length and sample format.  The acoustic memory is used when the checkpoint has one, unless ``--no-memory``.
``--resample``: accept a file at another rate (44.1 kHz, 48 kHz, ...): it is converted to 16 kHz on the GPU, separated, and converted
back, and the output has the input's rate, length and sample format.  Without the flag any other rate is an error.
``--overlap k``: k one-second segments over every sample (a segment every 1/k second), cross-faded with a sin^2 window, instead of
non-overlapping seconds; the default 1 is the plain path.
Semantics, the conversion's and the cross-fade's definition: m2h/separate.py.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "move2hear-active-av-separation_amd"))

SAMPLE_RATE = 16000


def read_wav(path, resample=False):
    """-> (float32 [2, L] in [-1, 1), the file's numpy dtype, the file's sample rate)"""
    import numpy as np
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if rate != SAMPLE_RATE and not resample:
        raise SystemExit("separate.py: %s is sampled at %d Hz; 16000 Hz is required (pass --resample to convert it on the GPU and back)" % (path, rate))
    if data.ndim != 2 or data.shape[1] != 2 or data.shape[0] < 1:
        raise SystemExit("separate.py: %s must be a two-channel (binaural) recording, got an array of shape %s" % (path, data.shape))
    if data.dtype == np.int16:
        wave = data.astype(np.float32) * np.float32(1.0 / 32768.0)
    elif data.dtype == np.float32:
        wave = data
    else:
        raise SystemExit("separate.py: %s holds %s samples; int16 or float32 is required" % (path, data.dtype))
    return np.ascontiguousarray(wave.T), data.dtype, int(rate)


def to_wav_samples(y, dtype):
    """float32 waveform -> samples of the input file's format (int16: round half to even, saturate)"""
    import numpy as np
    if dtype == np.int16:
        return np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return y.astype(np.float32)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--ckpt", required=True)
    parser.add_argument("--in", dest="inp", required=True, help="binaural WAV, 16 kHz, int16 or float32")
    parser.add_argument("--target-class", type=int, required=True)
    parser.add_argument("--out", required=True)
    parser.add_argument("--no-memory", action="store_true", help="do not run the acoustic memory even if the checkpoint has one")
    parser.add_argument("--math", choices=["fp32", "bf16x3"], default="bf16x3")
    parser.add_argument("--max-segments", type=int, default=None, help="largest U-Net batch in one-second segments")
    parser.add_argument("--resample", action="store_true", help="accept an input at another sample rate: convert to 16 kHz, separate, convert back")
    parser.add_argument("--overlap", type=int, choices=[1, 2, 4], default=1, help="one-second segments over every sample, cross-faded (1: non-overlapping)")
    args = parser.parse_args()
    wave, dtype, rate = read_wav(args.inp, args.resample)
    if rate != SAMPLE_RATE:
        from m2h.audio.resample import ratio
        try:
            ratio(rate, SAMPLE_RATE)
        except ValueError as e:
            raise SystemExit("separate.py: %s: %s" % (args.inp, e))
    import torch
    from scipy.io import wavfile
    from m2h import ops
    from m2h.separate import DEFAULT_MAX_SEGMENTS, Separator
    dev = torch.device("cuda", 0)
    sep = Separator(args.ckpt, dev, math=ops.MATH_FP32 if args.math == "fp32" else ops.MATH_BF16X3,
                    max_segments=args.max_segments or DEFAULT_MAX_SEGMENTS)
    y = sep.separate(torch.from_numpy(wave).to(dev), args.target_class, use_memory=False if args.no_memory else None, sample_rate=rate,
                     overlap=args.overlap)
    wavfile.write(args.out, rate, to_wav_samples(y.cpu().numpy(), dtype))
    print("separate.py: wrote %s (%d samples at %d Hz, %.2f s, class %d, memory %s, %s, overlap %d)" % (
        args.out, y.numel(), rate, y.numel() / rate, args.target_class, "on" if (sep.memory is not None and not args.no_memory) else "off", args.math,
        args.overlap))


if __name__ == "__main__":
    main()
