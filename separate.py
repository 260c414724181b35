#!/usr/bin/env python3
"""Separate one sound class out of a binaural recording of any length:

    python separate.py --ckpt F --in mix.wav --target-class K --out out.wav [--no-memory] [--math fp32|bf16x3] [--resample] [--overlap 1|2|4]
                       [--output mono|binaural|both] [--out-binaural bin.wav] [--stream-block N]

``--ckpt``: a passive-separator checkpoint or a PPO checkpoint (``{"state_dict", "config"}`` file or a bare state dict, with or
without the ``actor_critic.`` root).  ``--in``: a two-channel WAV at 16 kHz, int16 or float32.  The output is a mono WAV of the
same length and sample format.  The acoustic memory is used when the checkpoint has one, unless ``--no-memory``.
``--resample``: accept a file at another rate (44.1 kHz, 48 kHz, ...): it is converted to 16 kHz on the GPU, separated, and converted
back, and the output has the input's rate, length and sample format.  Without the flag any other rate is an error.
``--overlap k``: k one-second segments over every sample (a segment every 1/k second), cross-faded with a sin^2 window, instead of
non-overlapping seconds; the default 1 is the plain path.
``--output binaural``: ``--out`` gets the target in both ears, a two-channel WAV (the mixture's own spectrum of each channel scaled by
the first U-Net's clamped mask; no memory, and ``--no-memory`` changes nothing).  ``--output both``: the mono WAV goes to ``--out`` and
the two-channel WAV to ``--out-binaural``, which is required then and an error otherwise.  Both have the input's rate, length and
sample format.
``--stream-block N``: read the input N frames at a time, push every block through a stream (Separator.stream) and write what comes
back as it comes: the recording is never whole in GPU memory, and the result is that of the one-call path (the same samples up to the
batch size of the U-Nets, which follows the blocks).  Works with every option above.
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


def open_wav(path, resample=False):
    """read_wav without reading: -> (the file's samples [L, 2] memory-mapped, their numpy dtype, the file's sample rate)"""
    import numpy as np
    from scipy.io import wavfile
    rate, data = wavfile.read(path, mmap=True)
    if rate != SAMPLE_RATE and not resample:
        raise SystemExit("separate.py: %s is sampled at %d Hz; 16000 Hz is required (pass --resample to convert it on the GPU and back)" % (path, rate))
    if data.ndim != 2 or data.shape[1] != 2 or data.shape[0] < 1:
        raise SystemExit("separate.py: %s must be a two-channel (binaural) recording, got an array of shape %s" % (path, data.shape))
    if data.dtype not in (np.int16, np.float32):
        raise SystemExit("separate.py: %s holds %s samples; int16 or float32 is required" % (path, data.dtype))
    return data, data.dtype, int(rate)


class WavWriter:
    """A WAV file written piece by piece: int16 PCM or IEEE float32, the sizes of the header filled in on close."""

    def __init__(self, path, rate, channels, dtype):
        import struct
        import numpy as np
        self.f = open(path, "wb")
        self.dtype, self.frames, self.channels = np.dtype(dtype), 0, channels
        width = self.dtype.itemsize
        self.f.write(b"RIFF" + struct.pack("<I", 0) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1 if self.dtype == np.int16 else 3, channels, rate,
                                                                                         rate * channels * width, channels * width, 8 * width))
        self.f.write(b"data" + struct.pack("<I", 0))

    def write(self, y):
        """y: float32 [n] or [channels, n]"""
        import numpy as np
        samples = to_wav_samples(y.T if y.ndim == 2 else y, self.dtype)
        self.f.write(np.ascontiguousarray(samples).astype("<" + self.dtype.str[1:]).tobytes())
        self.frames += samples.shape[0]

    def close(self):
        import struct
        size = self.frames * self.channels * self.dtype.itemsize
        self.f.seek(4)
        self.f.write(struct.pack("<I", 36 + size))
        self.f.seek(40)
        self.f.write(struct.pack("<I", size))
        self.f.close()


def stream_file(sep, args, data, dtype, rate):
    """--stream-block: the file's blocks through a SeparatorStream, every returned piece written at once."""
    import numpy as np
    import torch
    st = sep.stream(args.target_class, recordings=1, use_memory=False if args.no_memory else None, sample_rate=rate, overlap=args.overlap, output=args.output)
    paths = (args.out, args.out_binaural) if args.output == "both" else (args.out,)
    writers = [WavWriter(p, rate, 2 if (args.output == "binaural" or i == 1) else 1, dtype) for i, p in enumerate(paths)]
    scale = np.float32(1.0 / 32768.0)

    def put(res):
        for w, y in zip(writers, res if isinstance(res, tuple) else (res,)):
            if y.shape[-1]:
                w.write(y[0].cpu().numpy())

    for a in range(0, data.shape[0], args.stream_block):
        block = np.asarray(data[a:a + args.stream_block])
        block = block.astype(np.float32) * scale if dtype == np.int16 else block
        put(st.push(torch.from_numpy(np.ascontiguousarray(block.T)).to(sep.device).unsqueeze(0)))
    put(st.flush())
    for w in writers:
        w.close()
    return [(p, w.frames, w.channels) for p, w in zip(paths, writers)]


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
    parser.add_argument("--output", choices=["mono", "binaural", "both"], default="mono",
                        help="mono: the target's mono waveform; binaural: the target in both ears (two channels); both: mono to --out, binaural to --out-binaural")
    parser.add_argument("--out-binaural", default=None, help="with --output both: the two-channel WAV")
    parser.add_argument("--stream-block", type=int, default=None, help="read the input N frames at a time and push them through a stream")
    args = parser.parse_args()
    if args.stream_block is not None and args.stream_block < 1:
        parser.error("--stream-block needs a positive number of frames")
    if (args.output == "both") != (args.out_binaural is not None):
        parser.error("--output both needs --out-binaural PATH, and --out-binaural is given with --output both only")
    if args.stream_block is not None:
        wave, dtype, rate = open_wav(args.inp, args.resample)
    else:
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
    if args.stream_block is not None:
        for path, frames, channels in stream_file(sep, args, wave, dtype, rate):
            memory = "on" if (channels == 1 and sep.memory is not None and not args.no_memory) else "off"
            print("separate.py: wrote %s (%d samples at %d Hz, %.2f s, class %d, memory %s, %s, overlap %d, blocks of %d)%s" % (
                path, frames, rate, frames / rate, args.target_class, memory, args.math, args.overlap, args.stream_block, ", two channels" if channels == 2 else ""))
        return
    res = sep.separate(torch.from_numpy(wave).to(dev), args.target_class, use_memory=False if args.no_memory else None, sample_rate=rate,
                       overlap=args.overlap, output=args.output)
    outs = ((args.out, res[0]), (args.out_binaural, res[1])) if args.output == "both" else ((args.out, res),)
    for path, y in outs:
        y = y.cpu().numpy()
        wavfile.write(path, rate, to_wav_samples(y.T if y.ndim == 2 else y, dtype))      # two channels: [L, 2] in the file
        memory = "on" if (y.ndim == 1 and sep.memory is not None and not args.no_memory) else "off"
        print("separate.py: wrote %s (%d samples at %d Hz, %.2f s, class %d, memory %s, %s, overlap %d)%s" % (
            path, y.shape[-1], rate, y.shape[-1] / rate, args.target_class, memory, args.math, args.overlap, ", two channels" if y.ndim == 2 else ""))


if __name__ == "__main__":
    main()
