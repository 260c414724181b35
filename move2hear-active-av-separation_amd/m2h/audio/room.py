"""RoomSimulator: binaural RIRs of shoebox rooms by the image-source method, on the GPU (csrc/room_sim.hip) -- the first stage of the
audio scenario: it makes the `rirs` that Auralizer.render, Separator, Scorer and RoomAcoustics.analyze consume.

Definition.  RATE = 16000 Hz, C = 343 m/s, HEAD_RADIUS = 0.0875 m, HALF_WIDTH = 41, EAR_PATTERN = 0.3.

1. Images (Allen and Berkley).  An image of the source s in the room (Lx, Ly, Lz) is indexed by p in {0, 1}^3 and m in Z^3.  Along an axis
   with room size L its coordinate is (1 - 2 p) s + 2 m L; it has |m - p| reflections on the wall at 0 and |m| on the wall at L.  Its
   gain is G = the product over the axes of beta_lo^|m - p| beta_hi^|m|, with 0^0 = 1; its order is the sum of the six exponents.  With
   max_order = N only the images of order <= N count; N = 0 is the direct sound.
2. Ears.  u = (-sin yaw, cos yaw, 0).  The left ear (e = 0) sits at listener + HEAD_RADIUS u with axis +u, the right at
   listener - HEAD_RADIUS u with axis -u.  Per image and ear v is the vector from the ear to the image, d = |v|, cos = v . axis / d
   (1 where d = 0), and the amplitude A = G ((1 - EAR_PATTERN) + EAR_PATTERN cos) / (4 pi max(d, HEAD_RADIUS)).
   These are two spaced receivers with a sub-cardioid pattern: the interaural time difference comes from the spacing, the level
   difference is the same at every frequency and at most 8 dB.  There are NO HRTFs -- none ship with the project -- so there is no
   pinna or head-shadow colouring and no elevation cue.
3. Fractional delay.  tau = d RATE / C, k = floor(tau).  The image adds A sinc(x) (1 + cos(pi x / 41)) / 2, x = n - tau, to h[n, e] for
   n = k - 40 .. k + 41 (82 taps) at 0 <= n < taps.  The window is zero at |x| = 41, so the tap set cuts no step.  h is the sum over all
   images.
4. Precision.  d, tau, k and tau - k are formed in float64: in float32 a delay of 250 000 samples has an ulp of 0.016 samples, errors of
   per cent in the taps.  Tap weights and sums are float32.

Cost.  The images that reach `taps` samples fill a sphere of radius C taps / RATE: the work grows with taps^3 / volume of the room.  A
5 x 4 x 3 m room has 23 555 candidate images at taps = 3200 and about 2.8 million at taps = 16000.

Reverberation time.  The decay of an image-source RIR is NOT Eyring's: `beta_from_t60` is a starting point, RoomAcoustics.analyze is
the measurement.  A float64 prototype of this definition in a 5 x 4 x 3 m room with taps = t60 x 16000 reads a T20 of 0.30 s for a
requested 0.2 s and of 0.46 s for 0.3 s.

Method (include/m2h.h, m2h_room_sim): one launch, grid (time tiles of ops.ROOM_TILE samples, RIRs); a workgroup enumerates the images of
its tile's shell, a lane adds the taps of its own sample in enumeration order.  No atomics, no host synchronisation; the bits of an RIR
depend on that RIR's inputs alone -- not on the batch, not on chunking, not on the run.  Values are not checked without
`validate=True`: an RIR with a parameter that is not finite (or beyond 1e5), a room side below 0.5 m, or a source or head centre
outside its room comes back as NaN.
"""
import torch

from .. import ops

RATE = 16000
C = 343.0
HEAD_RADIUS = 0.0875
HALF_WIDTH = 41
EAR_PATTERN = 0.3
MAX_TAPS = ops.ROOM_MAX_TAPS


def beta_from_t60(room, t60):
    """room [R, 3], t60 a number or [R] tensor (s) -> [R, 6]: the same coefficient on every wall from Eyring's formula,
    alpha = 1 - exp(-0.161 V / (S t60)), beta = sqrt(1 - alpha).  Torch algebra where `room` lives, no synchronisation.  A starting point:
    the reverberation time of the image-source RIR is not Eyring's (module docstring)."""
    if not isinstance(room, torch.Tensor) or room.dim() != 2 or room.shape[1] != 3:
        raise ValueError("m2h.beta_from_t60: room must be a [R, 3] tensor, got %s" % (tuple(room.shape) if isinstance(room, torch.Tensor) else type(room).__name__,))
    V = room[:, 0] * room[:, 1] * room[:, 2]
    S = 2.0 * (room[:, 0] * room[:, 1] + room[:, 1] * room[:, 2] + room[:, 0] * room[:, 2])
    t60 = t60.to(room.dtype) if isinstance(t60, torch.Tensor) else float(t60)      # (a number stays on the host: copying it would wait)
    beta = torch.sqrt(torch.exp(-0.161 * V / (S * t60)))
    return beta[:, None].expand(-1, 6).contiguous()


class RoomSimulator:
    def __init__(self, device, chunk=ops.ROOM_MAX_BATCH):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("m2h.RoomSimulator: device must be a GPU (got %s); the simulation has no CPU path" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.chunk = int(chunk)                      # RIRs of one launch
        if not 1 <= self.chunk <= ops.ROOM_MAX_BATCH:
            raise ValueError("m2h.RoomSimulator: chunk = %d RIRs per launch; 1 .. %d are supported" % (self.chunk, ops.ROOM_MAX_BATCH))

    def _arg(self, name, t, shapes):
        if not isinstance(t, torch.Tensor):
            raise TypeError("m2h.RoomSimulator: %s must be a torch tensor, got %s" % (name, type(t).__name__))
        if t.dtype not in (torch.float32, torch.float64):
            raise RuntimeError("m2h.RoomSimulator: %s must be float32 or float64, got %s" % (name, t.dtype))
        if not any(t.dim() == len(s) and all(w is None or w == g for w, g in zip(s, t.shape)) for s in shapes):
            want = " or ".join("[%s]" % ", ".join("*" if w is None else str(w) for w in s) for s in shapes)
            raise ValueError("m2h.RoomSimulator: %s must be %s, got a tensor of shape %s" % (name, want, tuple(t.shape)))

    def simulate(self, room, beta, sources, listener, yaw, taps, max_order=None, validate=False):
        """room [R, 3] (m), beta [R, 6] (walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz), sources [R, S, 3], listener [R, 3] or [R, K, 3] (the head
        centre), yaw [R] or [R, K] (radians about z), fp32 or fp64 on the device -> [R, S, taps, 2] fp32, or [R, S, K, taps, 2] with the K
        axis: the layouts Auralizer.render and RoomAcoustics.analyze take.  max_order: None for every image that reaches the taps.
        validate=True checks the values (one synchronisation) and raises ValueError; without it nothing waits for the host."""
        taps = int(taps)
        if not 1 <= taps <= MAX_TAPS:
            raise ValueError("m2h.RoomSimulator: taps = %d; 1 .. %d are supported" % (taps, MAX_TAPS))
        if max_order is not None and int(max_order) < 0:
            raise ValueError("m2h.RoomSimulator: max_order = %d; an order >= 0 or None is required" % int(max_order))
        self._arg("room", room, [(None, 3)])
        R = int(room.shape[0])
        self._arg("beta", beta, [(R, 6)])
        self._arg("sources", sources, [(R, None, 3)])
        S = int(sources.shape[1])
        self._arg("listener", listener, [(R, 3), (R, None, 3)])
        moving = listener.dim() == 3
        K = int(listener.shape[1]) if moving else 1
        self._arg("yaw", yaw, [(R, K)] if moving else [(R,)])
        if R * S * K == 0:
            raise ValueError("m2h.RoomSimulator: R = %d rooms, S = %d sources, K = %d positions hold no RIR" % (R, S, K))
        for name, t in (("room", room), ("beta", beta), ("sources", sources), ("listener", listener), ("yaw", yaw)):
            if not t.is_cuda or t.device != self.device:
                raise RuntimeError("m2h.RoomSimulator: %s must live on %s (got %s); the simulation has no CPU path" % (name, self.device, t.device))
        f64 = torch.float64
        lis, yw = listener.to(f64).reshape(R, K, 3), yaw.to(f64).reshape(R, K)
        if validate:
            rm, bt, sr = room.to(f64), beta.to(f64), sources.to(f64)
            ok = (rm > 0).all() & (bt >= 0).all() & (bt <= 1).all() & torch.isfinite(yw).all()
            ok = ok & (sr >= 0).all() & (sr <= rm[:, None, :]).all() & (lis >= 0).all() & (lis <= rm[:, None, :]).all()
            if not bool(ok):                         # the one synchronisation
                raise ValueError("m2h.RoomSimulator: room sizes must be positive, sources and listener must lie inside their room and beta in [0, 1]")
        params = torch.cat([room.to(f64)[:, None, None, :].expand(R, S, K, 3), beta.to(f64)[:, None, None, :].expand(R, S, K, 6),
                            sources.to(f64)[:, :, None, :].expand(R, S, K, 3), lis[:, None, :, :].expand(R, S, K, 3),
                            yw[:, None, :, None].expand(R, S, K, 1)], dim=-1).reshape(R * S * K, ops.ROOM_PARAMS)
        Q = R * S * K
        parts = [ops.room_sim(params[q0:q0 + self.chunk], taps, max_order) for q0 in range(0, Q, self.chunk)]
        out = parts[0] if len(parts) == 1 else torch.cat(parts)
        return out.reshape((R, S, K, taps, 2) if moving else (R, S, taps, 2))
