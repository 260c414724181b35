"""Scorer: the quality of a separated recording of any length against its ground truth, on the GPU (csrc/score.hip).

Definition.  Inputs, fp32 on the GPU; the last stride is 1 and every other stride is arbitrary (views are read in place; a non-unit
last stride is an error, not a hidden copy):

  references [R, S, L] or [R, S, C, L], 1 <= S <= 6, C in {1, 2}: the target and the interferers as they are in the mixture, e.g. the
             `images` of Auralizer.render(..., return_images=True) times their gains;
  estimate   [R, L] or [R, C, L]: the separated target (C as in `references`; [R, L] means C = 1);
  mixture    [R, 2, L]: what the separator was given;
  target     an int, or R ints, in [0, S): which reference the estimate is an estimate of;
  L >= 1.

Tiles and windows.  A tile is `tile` samples (default 16000: one second, the Separator's segment); J = ceil(L / tile), the last tile may
be short.  Windows are counted in tiles: `window` = w >= 1 tiles long, a window every `hop` = h >= 1 tiles.  There are M = 1 windows if
J <= w, else M = ceil((J - w) / h) + 1; window m covers the tiles [m h, min(m h + w, J)).  (With h > w the windows leave tiles out, and
the last one may then start at or past J: it is empty, n = 0.)  score_plan() returns all this in pure Python.

Every window, and the whole recording, is scored as the reference scores one clip (common/eval_metrics.py: preprocess :172-199, then
scale_bss_eval :60-122 with all S references).  n is the window's sample count; every signal has ITS OWN MEAN OVER THAT WINDOW removed.
For channel c the signals are the S references' channel c, the estimate's channel c, and the baseline: for C = 1 the mean of the two
mean-removed mixture channels (preprocess(is_mono=True)), for C = 2 the mixture's channel c (scale_bss_eval's docstring: each channel
independently).  The eleven numbers, in eval_metrics.METRIC_ORDER, are scale_bss_eval_helper's (:12-57) with its two EPS terms: with s the
target, x the estimate, P the references' Gram matrix,

  alpha = <s, x> / <s, s>         snr = 10 log10(<s, s> / |x - s|^2)          si_sdr = 10 log10(|alpha s|^2 / |x - alpha s|^2)
  srr = -10 log10((1 - 1 / alpha)^2)                                          sd_sdr = snr + 10 log10(alpha^2)
  b = solve(P, refs^T (x - alpha s)) + EPS       e_interf = refs b            e_artif = x - alpha s - e_interf + EPS
  si_sir = 10 log10(|alpha s|^2 / |e_interf|^2)                               si_sar = 10 log10(|alpha s|^2 / |e_artif|^2)

then si_sdri, sd_sdri, snri, si_siri, si_sari: the estimate's number minus the baseline's.  No time alignment is made unless `align`
is given (below).

Degenerate cases.  A source whose centred energy in the window is 0 (digital silence, or not positive after rounding) is left out of the
projection: its coefficient is 0.  If the target's energy is 0 or n < 2, all eleven numbers are NaN.  If the reduced normal equations
cannot be solved (info != 0 of torch.linalg.solve_ex, a pivot that is exactly 0: duplicate references; solve_pivoted), the SIR / SAR numbers and their improvements are NaN.
Quadratic forms that are non-negative in exact arithmetic are clamped at 0, so a perfect estimate scores +inf, not NaN.  Otherwise
IEEE rules apply, as in numpy with warnings off.

Method.  All of the above follows from the sums and the Gram matrix of the N = S + 3 signals s_0 .. s_{S-1}, est_c, mix_l, mix_r of a
window: <a - mean a, b - mean b> = sum a b - (sum a)(sum b) / n, the baseline is a linear combination of mix_l and mix_r, and norms of
residuals are quadratic forms.  m2h_score_gram reads every signal once and writes those sums per (recording, channel, tile) in fp64 with
exact products (an fp32 Gram loses the noise norm, a difference of Gram entries, exactly where a good separator scores: DESIGN.md §8.6);
m2h_score_windows adds a window's tiles in tile order -- never a difference of prefix sums, so a window's score does not depend on what
precedes it -- and metrics_from_gram does the algebra in torch float64, batched over recordings, channels and windows.

Alignment.  score(..., align=None) is all of the above, unchanged.  align=D, a Python int in 1 .. 8192, is the largest lag searched, in
samples; it requires tile + 2 D <= 32768 and L >= 2 D + 2 (a ValueError that names the values, before any launch).  For recording r and
channel c let s = references[r, target_r, c] and x = estimate[r, c].  The scored region is the reference samples t in [D, L - D): the
same for every recording and every lag, so the plan never depends on device data.  Lr = L - 2 D; tiles and windows are
score_plan(Lr, tile, window, hop) counted from sample D, and align_plan(L, D, tile, window, hop) returns them in pure Python:
score_plan's dict plus "offset": D, with "samples" in coordinates of the input.

  ct[r, c, j, d + D] = sum_t s[t] x[t + d]        t over tile j of the region, d = -D .. D

The signals are raw: no mean is removed, so a DC offset adds a pedestal n . mean(s) . mean(x) to every lag and flattens the peak.  A
window's correlation is the sum of its tiles' ct in tile order, in float64; the whole recording's is the sum over all J tiles.  The lag
of a window is the d that maximises |c[d]|; among equal maxima the smallest |d| wins, then the negative one, so digital silence gives
lag 0 (lags_from_corr).  Every window and the whole recording are then scored exactly as above on references[..., D : L - D],
mixture[..., D : L - D] and estimate[r, c, D + lag_rc : L - D + lag_rc], where lag_rc is the WHOLE-RECORDING lag of that recording and
channel: the two ears are aligned independently.  The windows' own lags are reported ("lag_track") but not used for scoring: they show
drift.  m2h_align_corr (csrc/align.hip) computes ct by one 32768-point circular correlation per tile in fp32 (the Auralizer's transform,
fft_lds.h; no wrap-around reaches the lags kept) and writes it as float64; m2h_score_windows adds the tiles; m2h_score_gram_lag is
m2h_score_gram reading the region with the estimate moved by the lag, which it takes from device memory and clamps to [-D, D].
Recordings are processed in groups whose ct stays under `max_corr_bytes` (a single recording above it goes alone); they are
independent, so grouping changes no bit.  No host synchronisation, and no copy from the host apart from the twiddle table on a
Scorer's first aligned call.  Not done: sub-sample lags, caller-supplied lags, inputs of unequal length.

Spectral.  score(..., spectral=True) adds the paper's other number, the STFT distance (common/eval_metrics.py:306-366,
STFT_L2_distance), per window and over the whole recording, next to the eleven above, which do not change by a bit.  The tile must be
16000 (one second, the Separator's segment): any other tile is a ValueError that names it, before any launch.  For recording r and
channel c the three signals are taken RAW -- no mean is removed, because the reference's spectrograms are of the raw audio:
g = references[r, target_r, c], e = estimate[r, c], and the baseline b = 0.5 (mixture[r, 0] + mixture[r, 1]) for C = 1, mixture[r, c]
for C = 2.  Tiles and windows are score_plan's / align_plan's; with align=D the same region [D, L - D) is used and the estimate is read
lag[r, c] samples later, exactly as m2h_score_gram_lag reads it.  The spectrogram of a tile is the one the Separator's U-Net sees for
that second (m2h/separate.py, m2h.audio.stft.STFT, oracle.np_stft): the tile's samples zero-extended to 16000 where the recording ends,
reflect-padded by 511 on both sides INSIDE THE TILE (np.pad(mode="reflect"); neighbouring seconds are never read), 32 frames of 1023
samples every 512, the periodic Hann window rounded to float32, a 1023-point DFT, bins 0 .. 511: F = 512, T = 32.  With G, E, B the
complex spectrograms of g, e, b, a tile's seven sums over its F T bins are

  0 sum |G|^2   1 sum |E|^2   2 sum |B|^2   3 sum (|E| - |G|)^2   4 sum |E - G|^2   5 sum (|B| - |G|)^2   6 sum |B - G|^2

and a window's sums are its tiles' sums added in tile order (m2h_score_windows).  With Q the window's tile count (J for the whole
recording) the eight numbers, in SPECTRAL_ORDER, float64:

  stft_l2 = sums[3] / (2 F T Q)          stft_l2_complex = sums[4] / (2 F T Q)          sc = sqrt(sums[3] / sums[0])
  stft_l2_base, stft_l2_complex_base, sc_base: the same with sums 5, 6 and 5 / 0
  stft_l2i = stft_l2_base - stft_l2      stft_l2_complexi = stft_l2_complex_base - stft_l2_complex     (positive: better than the mixture)

stft_l2 is the reference's mono number: the mean over (re, im), F and T of the squared distance with the ground truth's phase on both
sides, which reduces to (|E| - |G|)^2; for a one-second recording it is STFT_L2_distance(...)[1] with pred_mono = |STFT(e)| and
gt_mono_comps = (|G|, angle G).  For C = 2 the paper's binaural number is the two ears' stft_l2 ADDED; that addition is left to the
caller.  Q = 0 gives NaN; otherwise IEEE rules apply (a silent target makes sc NaN or inf).  m2h_score_spectral (csrc/score_spectral.hip)
computes the seven sums of every tile straight from the waveforms -- the transform on the exact fp32 matrix instruction, squares added
in fp64, no frame or spectrum ever in memory -- and spectral_from_sums does the rest in torch float64.  No host synchronisation, and no
copy from the host apart from the transform table on a Scorer's first spectral call.

Spatial.  score(..., spatial=True) adds the interaural cues of the estimate against the target's, with the mixture as baseline: what
the numbers above, which score each ear on its own, cannot see (the same mono waveform in both ears scores well on all of them and has
lost the direction the target came from).  It needs C = 2 and tile = 16000: a mono call or any other tile is a ValueError that names
the offending value, before any launch; the eleven numbers and the spectral ones do not change by a bit.  Per recording r there are
three BINAURAL signals, all taken raw: G = references[r, target_r] (the target), E = estimate[r], B = mixture[r] (the baseline).  Tiles,
windows and the spectrogram of a tile are exactly those of "Spectral" (spectral_table() serves both kernels).  The F = 512 bins form
NB = 32 bands of 16 bins, band j = bins 16 j .. 16 j + 15, about 250 Hz wide.  With X_L, X_R the two ears' spectrograms of a signal x, a
tile's four sums over a band's 16 bins x 32 frames, in this order:

  0 PL = sum |X_L|^2   1 PR = sum |X_R|^2   2 CRE = sum Re(X_L conj X_R) = sum (ReL ReR + ImL ImR)
  3 CIM = sum Im(X_L conj X_R) = sum (ImL ReR - ReL ImR)

The tile sums are [R, J, 3, 32, 4] float64 (signal G, E, B; band; sum) and a window's sums are its tiles' sums added in tile order
(m2h_score_windows with RC = R and K = 384).  Alignment: with align=D the region is [D, L - D) as above, but BOTH EARS of the estimate
are read at ONE lag, lag[r, 0] (the left ear's whole-recording lag, clamped to [-D, D]): reading each ear at its own lag would cancel
the very interaural delay that is being measured.  The per-ear lags are in the result ("lag") for whoever wants their difference.

The cues of a signal in a band, from a window's sums (spatial_from_sums, element-wise torch float64 on any device):

  ILD = 10 log10(PL / PR) dB       IPD = atan2(CIM, CRE) rad, positive when the right ear is late       IC = hypot(CRE, CIM) / sqrt(PL PR)

The errors are band means weighted by the target's band energy w_j = PL_G + PR_G.  A band is valid for a signal x (E or B) where
w_j > 0 and PL and PR of both G and x are > 0 (all three errors use this one rule); sums run over the valid bands only, numerator and
denominator alike, and no valid band gives NaN.  The nine numbers, in SPATIAL_ORDER:

  ild_err = sum w |ILD_E - ILD_G| / sum w                    over all 32 bands, dB
  ipd_err = sum w |wrap(IPD_E - IPD_G)| / sum w              wrapped to (-pi, pi], over the bands 0 .. 5 (SPATIAL_IPD_BANDS: bins below 96,
                                                             about 1.5 kHz, where phase is a usable cue), rad
  ic_err  = sum w |IC_E - IC_G| / sum w                      over all 32 bands
  ild_err_base, ipd_err_base, ic_err_base                    the same with B in place of E
  ild_erri, ipd_erri, ic_erri                                baseline minus estimate (positive: closer to the target's image than the mixture)

The whole-recording numbers are the long-term cues of the SUMMED spectra (all J tiles' sums added first), not the mean of the track.
m2h_score_spatial (csrc/score_spatial.hip) computes the tile sums straight from the waveforms -- the same folded transform on the exact
fp32 matrix instruction, the four fp32 values of a bin converted to fp64 before they are multiplied, no frame or spectrum ever in
memory.  No host synchronisation; the only copy from the host is the transform table, once.  The broadband ITD in microseconds is
itd=True, below.

ITD.  score(..., itd=True) adds the number spatial-audio work reports first: the broadband interaural time difference of the target, the
estimate and the mixture, in microseconds, as the peak of the PHAT-weighted generalised cross-correlation (GCC-PHAT) of the two ears,
per window and over the whole recording.  It needs C = 2 and tile = 16000, as spatial=True does (a ValueError that names the offending
value, before any launch; a non-bool itd is a TypeError); every other number is unchanged by a bit.

Signals, tiles and spectra are those of "Spatial", unchanged: G = references[r, target_r], E = estimate[r], B = mixture[r], raw; the
spectrogram of a one-second tile is the Separator's; with align=D the region is [D, L - D) and BOTH EARS of the estimate are read at the
left ear's lag, so that the delay being measured survives the alignment.

Tile sums.  For every (recording, tile, signal) and every bin k = 0 .. 255 the cross-spectrum summed over the tile's 32 frames,

  CRE_k = sum_f Re(X_L conj X_R)      CIM_k = sum_f Im(X_L conj X_R)

-- exactly the cross term of "Spatial", per bin instead of per band of 16: float64 [R, J, 3, 256, 2].  A window's sums are its tiles'
added in tile order and the whole recording's are all J tiles added (m2h_score_windows with RC = R and K = 1536); as in "Spatial" the
whole-recording number is the cue of the SUMMED spectra, not the mean of the track.

GCC-PHAT of a window.  The band is ITD_BINS = (6, 256): the bins k_lo = 6 .. k_hi - 1 = 255, about 94 Hz to 4 kHz.  ITD_MAX_LAG = 16
samples (+-1 ms) and ITD_UPSAMPLE = 8: the lags are tau_i = i / 8 samples for i = -128 .. 128, NL = 257 of them.  With
Phi_k = CRE_k + j CIM_k and the PHAT weight Phat_k = Phi_k / |Phi_k|, |Phi_k| = sqrt(CRE^2 + CIM^2) (a bin with |Phi_k| = 0 gives
Phat_k = 0),

  G[i] = (1 / 250) sum_{k = 6}^{255} Re(Phat_k exp(-j 2 pi k i / (1023 . 8)))

Sign: when the right ear is the left ear d samples later, G peaks at tau = +d -- the rule of "Spatial", IPD positive when the right
ear is late.

Pick.  The ITD is the tau_i that maximises G itself, not |G|; among equal maxima the smallest |i| wins, then the negative one (the
column reordering of lags_from_corr), so a G of zeros picks 0.  It is reported in microseconds, tau . 62.5: a grid step is 7.8125 us.
`peak` is that maximum: it lies in [-1, 1] and tends to 1 for one coherent source.  A signal with no bin of the band at |Phi_k| > 0 has
itd and peak NaN.

Result.  ITD_ORDER = (itd, itd_est, itd_mix, itd_err, itd_err_base, itd_erri, peak, peak_est, peak_mix): itd is the target's,
itd_err = |itd_est - itd|, itd_err_base = |itd_mix - itd|, itd_erri = itd_err_base - itd_err, all in us.  "itd_whole" [R, 9] and
"itd_track" [R, M, 9], float64 on the device, and "itd_gcc" [R, 1 + M, 3, 257]: the functions themselves, the whole recording first.

Method.  m2h_score_itd (csrc/score_itd.hip) computes the tile sums straight from the waveforms: the folded transform of "Spectral" on
the exact fp32 matrix instruction, only the lower 256 bins of it, the four fp32 values of a bin converted to fp64 before they are
multiplied, no frame or spectrum ever in memory.  m2h_score_windows adds the tiles; m2h_itd_gcc normalises a row's band once, in fp64,
and adds the bins of every lag in ascending k with twiddles from itd_table(), the index (k i) mod 8184 reduced in integers;
itd_from_gcc picks, element-wise in torch float64.  The tile sums take 12 KB per recording and second, so recordings go in groups whose
tile sums stay under `max_corr_bytes` (a single recording above it goes alone); they are independent, so grouping changes no bit.  No
host synchronisation, and no copy from the host apart from the two tables on a Scorer's first itd call.  Not done: sub-grid
interpolation of the peak, a caller-chosen band or lag range, an ITD per frequency band.

STOI.  score(..., stoi=True) adds the short-time objective intelligibility of the estimate (Taal et al. 2011) and its extended form
ESTOI (Jensen & Taal 2016), with the mixture as baseline, per window and over the whole recording; every other number is unchanged by a
bit.  It is the published algorithm with the conventions of the widely used Python package, quirks included.  The tile must be 16000
(a tile is then exactly 10000 resampled samples): any other tile is a ValueError that names it, before any launch.

Constants.  FS = 10000, N_FRAME = 256, HOP = 128, NFFT = 512; 15 third-octave bands; a segment is N = 30 frames; BETA = -15 dB, so the
clip factor is 1 + 10^(15/20); dynamic range 40 dB; EPS = 2^-52; the window is w = hanning(258)[1:-1], 256 values.

Signals.  Per (r, c) the three signals of "Spectral" for the same C, with the same align=D rule: the clean signal
x = references[r, target_r, c], the estimate y, the baseline b (C = 1: 0.5 (mixture[r, 0] + mixture[r, 1]) formed in float32, C = 2:
mixture[r, c]); the region is [D, L - D) and the estimate is read at ITS OWN EAR's whole-recording lag, clamped to [-D, D].  Each
signal is converted to 10 kHz by this project's resampler (m2h.audio.resample: up / down = 5 / 8, the table of design(16000, 10000);
scipy.signal.resample_poly(x, 5, 8, padtype="constant") to the resampler's accuracy); Lr = L - 2 D samples give L10 = ceil(Lr 5 / 8).

Ranges.  The whole recording is the range [0, L10) of the 10 kHz signals; window m of score_plan / align_plan is the range
[m hop 10000, min((m hop + window) 10000, L10)).  Every range is analysed on its own by the three steps below, so stoi_track[..., m, :]
is, by construction, what the whole-recording analysis gives on that slice of the 10 kHz signals (stoi_plan() returns the ranges).

Step 1, silent frames.  Frames start at i = 0, 128, ... < n - 256, n the range's length: the end is EXCLUSIVE, so when n - 256 is a
multiple of 128 the last full frame is not taken.  The energy of frame f is e_f = 20 log10(|w x_f|_2 + EPS), from the clean signal only;
frame f is kept iff e_f > max_f e_f - 40.  The K kept frames of x, y and b -- one mask for all three -- are windowed by w and
overlap-added at hop 128: three signals of (K - 1) 128 + 256 samples.

Step 2, envelopes.  These signals are framed again by the same exclusive rule, which gives K - 1 frames; each is windowed by w again and
transformed at 512 points.  With f_k = k FS / 512 the band edges are the bins nearest to 150 2^((2 j -+ 1) / 6) Hz, j = 0 .. 14; the
half-open bin ranges are [7,9) [9,11) [11,14) [14,17) [17,22) [22,27) [27,34) [34,43) [43,55) [55,69) [69,87) [87,109) [109,138)
[138,174) [174,219), and the envelope is X[j, t] = sqrt(sum over the band's bins of |S|^2).

Step 3, segments.  For every m = 30 .. K - 1 take the 15 x 30 blocks X (clean) and Y (processed), columns [m - 30, m).
  STOI:  per band row alpha = |X_row| / (|Y_row| + EPS);  Y' = min(alpha Y, (1 + 10^0.75) X);  each row's mean is removed from X and from
         Y';  each row is divided by (its norm + EPS);  d_m = sum X Y' / 15;  STOI is the mean of d_m over the segments.
  ESTOI: X and Y are normalised by rows (mean removed, divided by norm + EPS), then by columns the same way;  d_m = sum X Y / 30;  ESTOI
         is the mean of d_m over the segments.

Choices where the package is arbitrary: a range with fewer than 30 envelope frames (K < 31) gives NaN (the package returns 1e-5 and
warns), and so does a range whose clean signal has max_f |w x_f| = 0.

Result.  STOI_ORDER = (stoi, estoi, stoi_base, estoi_base, stoii, estoii): base is the same with b as the processed signal, the
improvements are estimate minus base.  "stoi_whole" [R, C, 6] and "stoi_track" [R, C, M, 6] float64, and "stoi_frames" [R, C, 1 + M]
int64: the kept-frame count K of the whole recording, then of every window.  m2h_stoi_resample (csrc/score_stoi.hip) reads the
three signals in place and writes them at 10 kHz with the resampler's own chain of operations (the same bits as Resampler(16000, 10000)
on copies); m2h_stoi_ranges does steps 1 .. 3 for the whole recording and every window in the same five launches: frame energies in fp64
from fp32 products, the mask and its scan, the envelopes (gather through the kept-frame list, overlap-add, the packed transform of
fft_lds.h in LDS, band sums in fp64 -- no frame, no overlap-added signal and no spectrum in memory) and the segments in fp64.  K stays
on the device: no host synchronisation, and no copy from the host apart from three small tables on a Scorer's first stoi call.  No
atomics, fixed summation orders: a recording's bits do not depend on the batch around it, on strides or on alignment.

BSS.  score(..., bss=T) adds the number most separation papers call plain SDR: BSS-eval's SDR, SIR and SAR (Vincent et al. 2006), in which
the estimate is projected on the references through a time-invariant distortion filter of T taps before anything is compared, so an
estimate that carries a short FIR of the target (an early reflection, a codec's response) is not punished as if it were noise.  It is
mir_eval.separation.bss_eval_sources for one target without permutation search, with the filter timing of museval v4: one filter set
from the whole recording, window numbers from that filter's components.  T is a Python int in 1 .. 512 (None, the default: off); a bool,
a float or a value outside the range is a TypeError / ValueError that names the value, before any launch.  Every other number is
unchanged by a bit.

Signals.  Per recording r and channel c the signals are those of "Spectral", taken raw, no mean removed: s_0 .. s_{S-1} =
references[r, :, c] with the target j = target_r, x = estimate[r, c], and the baseline b = 0.5f (mixture[r, 0] + mixture[r, 1]) formed
in float32 for C = 1, mixture[r, c] for C = 2.  With align=D the region is [D, L - D) and x is read lag[r, c] samples later, clamped to
[-D, D], exactly as m2h_score_spectral reads it.  Lr is the region's length; every signal counts as zero outside the region -- no real
sample outside it is used -- so an aligned call equals the unaligned call on hand-cut slices.  N = Lr + T - 1.

  c_ik[d] = sum_t s_i[t] s_k[t + d]      d = -(T-1) .. T-1
  p_i[a]  = sum_t s_i[t] x[t + a]        a = 0 .. T-1                (q_i the same with b)
  G[(i,a),(k,b)] = c_ik[a - b]           (S T square, symmetric, block-Toeplitz: the Gram matrix of the shifted references)
  G h = p  (joint filters h [S, T])      G_jj g = p_j  (the target alone, g [T])
  s_t[n] = sum_a g[a] s_j[n - a]         P[n] = sum_i sum_a h_i[a] s_i[n - a]       n = 0 .. N-1, x zero-extended
  sdr = 10 log10(|s_t|^2 / |x - s_t|^2)  sir = 10 log10(|s_t|^2 / |P - s_t|^2)      sar = 10 log10(|P|^2 / |x - P|^2)

and the same with b in place of x, with its own h and g.  BSS_ORDER = (sdr, sir, sar, sdr_base, sir_base, sar_base, sdri, siri, sari),
the improvements estimate minus baseline.  The kernel sums one-sided lags: co[i, k, d] = sum_t s_i[t] v_k[t + d], d = 0 .. T - 1, for
v = (s_0 .. s_{S-1}, x, b); c_ik[d] is co[i, k, d] for d >= 0 and co[k, i, -d] for d < 0 when i <= k, and c_ki[d] = c_ik[-d], so G is
symmetric by construction.

Tiles and windows are score_plan's / align_plan's.  Tile j owns the output samples n in [j tile, (j + 1) tile) of [0, Lr); the last tile
also owns the tail [Lr, N).  A tile's ten sums are |s_t|^2, |x - s_t|^2, |P - s_t|^2, |P|^2, |x - P|^2 and the five of the baseline; a
window's sums are its tiles' sums in tile order (m2h_score_windows), the whole recording's are all J.  The result gains "bss_whole"
[R, C, 9] and "bss_track" [R, C, M, 9], float64; the track uses the whole recording's filters.

Degenerate input.  Lr >= S T is required (below that the normal equations are rank-deficient): a ValueError that names the values,
before any launch.  A reference whose whole-recording energy c_ii[0] is 0 is left out: its block becomes the identity, its right-hand
side 0 and its filter 0 (the rule of metrics_from_gram).  A silent target gives nine NaN; a factorisation that reports failure gives
NaN for that (r, c) only.  Otherwise IEEE rules apply (a perfect estimate gives +inf, a window without tiles NaN); no non-negative
quantity is formed as a difference.

Method.  m2h_bss_corr (csrc/score_bss.hip) writes co per tile in fp64 -- every product of two fp32 samples exact, the sums in an order
fixed by the recording alone, reads across the tile border but never past the region -- and m2h_score_windows adds the tiles; recordings
go in groups whose tile correlations stay under `max_corr_bytes`.  bss_filters builds G by index gather and factorises ONE (r, c) at a
time with torch.linalg.cholesky_ex + cholesky_solve in float64 on the device (never one batched call: the batch must not change a
recording's bits); the joint system, the target-alone system and both right-hand sides share the factorisations.  m2h_bss_project
applies the filters and writes the ten sums of every tile, no component signal ever stored, and bss_from_sums does the rest.  The
Scorer's own code makes no host synchronisation; what the library's factorisation does is recorded in DESIGN.md 8.11.
"""
import operator
from types import SimpleNamespace

import torch

from .. import ops
from .twiddles import device_twiddles
from ..common.eval_metrics import EPS, METRIC_ORDER

DEFAULT_TILE = 16000
MAX_SOURCES = 6
MAX_ALIGN = 8192             # the largest `align`, in samples
ALIGN_NFFT = 32768           # the correlation's transform: tile + 2 align samples must fit
DEFAULT_MAX_CORR_BYTES = 1 << 30
_NAN = float("nan")
SPECTRAL_ORDER = ("stft_l2", "stft_l2_complex", "sc", "stft_l2_base", "stft_l2_complex_base", "sc_base", "stft_l2i", "stft_l2_complexi")
SPECTRAL_TILE = 16000        # spectral=True: one second, the Separator's segment
SPECTRAL_BINS, SPECTRAL_FRAMES, SPECTRAL_NFFT = 512, 32, 1023
SPATIAL_ORDER = ("ild_err", "ipd_err", "ic_err", "ild_err_base", "ipd_err_base", "ic_err_base", "ild_erri", "ipd_erri", "ic_erri")
SPATIAL_BANDS = 32           # spatial=True: bands of 16 bins, band j = bins 16 j .. 16 j + 15
SPATIAL_IPD_BANDS = 6        # the phase error is taken over the bands 0 .. 5: bins below 96, about 1.5 kHz
ITD_ORDER = ("itd", "itd_est", "itd_mix", "itd_err", "itd_err_base", "itd_erri", "peak", "peak_est", "peak_mix")
ITD_BINS = (6, 256)          # itd=True: the band k_lo <= k < k_hi of GCC-PHAT, about 94 Hz to 4 kHz
ITD_MAX_LAG = 16             # samples: +-1 ms
ITD_UPSAMPLE = 8             # lags of 1 / 8 sample: 7.8125 us
ITD_LAGS = 2 * ITD_MAX_LAG * ITD_UPSAMPLE + 1
ITD_US_PER_STEP = 1e6 / (16000 * ITD_UPSAMPLE)
STOI_ORDER = ("stoi", "estoi", "stoi_base", "estoi_base", "stoii", "estoii")
STOI_TILE = 16000            # stoi=True: a tile is exactly STOI_FS resampled samples
STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT, STOI_BANDS, STOI_SEGMENT = 10000, 256, 128, 512, 15, 30
BSS_ORDER = ("sdr", "sir", "sar", "sdr_base", "sir_base", "sar_base", "sdri", "siri", "sari")
BSS_MAX_TAPS = 512           # bss=T: the longest distortion filter
# The metric families, in the order summarize() and score.py report them.  A row: (key prefix; metric order; rows per recording ("binaural")
# instead of per channel; the windows that enter the track's mean and median -- "active": the target has energy, "both": active in both
# ears, "finite": no NaN in the window's row --; the family's extra result keys as (key, whether summarize() carries it too)).
FAMILIES = (("", METRIC_ORDER, False, "active", ()),
            ("spectral_", SPECTRAL_ORDER, False, "active", ()),
            ("spatial_", SPATIAL_ORDER, True, "both", (("spatial_cues", False),)),
            ("itd_", ITD_ORDER, True, "both", (("itd_gcc", False),)),
            ("stoi_", STOI_ORDER, False, "finite", (("stoi_frames", True),)),
            ("bss_", BSS_ORDER, False, "active", ()))


def score_plan(L, tile=DEFAULT_TILE, window=1, hop=1):
    """Pure Python: the tiles and windows of one score.

    -> {"L", "tile", "window", "hop", "J", "M", "tiles": [(j0, j1)] per window, "samples": [(t0, t1)] per window}; window m holds the tiles
    j0 <= j < j1 and the samples t0 <= t < t1 (n = t1 - t0; an empty window has j0 == j1 and t0 == t1)."""
    vals = []
    for name, v in (("L", L), ("tile", tile), ("window", window), ("hop", hop)):
        try:
            vals.append(operator.index(v))
        except TypeError:
            raise TypeError("m2h.Scorer: %s must be an int, got %r" % (name, v))
        if isinstance(v, bool) or vals[-1] < 1:
            raise ValueError("m2h.Scorer: %s must be at least 1, got %r" % (name, v))
    L, tile, window, hop = vals
    J = -(-L // tile)
    M = 1 if J <= window else -(-(J - window) // hop) + 1
    tiles = [(min(m * hop, J), min(m * hop + window, J)) for m in range(M)]
    return {"L": L, "tile": tile, "window": window, "hop": hop, "J": J, "M": M, "tiles": tiles,
            "samples": [(min(j0 * tile, L), min(j1 * tile, L)) for j0, j1 in tiles]}


def align_plan(L, D, tile=DEFAULT_TILE, window=1, hop=1):
    """Pure Python: the tiles and windows of one aligned score (module docstring, "Alignment").

    -> score_plan(L - 2 D, tile, window, hop) plus "offset": D, with "samples" moved by D into coordinates of the input ("L" stays the
    region's length L - 2 D).  Raises on D outside 1 .. 8192, tile + 2 D > 32768 and L < 2 D + 2."""
    try:
        d = operator.index(D)
    except TypeError:
        raise TypeError("m2h.Scorer: align must be an int or None, got %r" % (D,))
    if isinstance(D, bool) or not 1 <= d <= MAX_ALIGN:
        raise ValueError("m2h.Scorer: align must be in 1 .. %d samples, got %r" % (MAX_ALIGN, D))
    L = score_plan(L, tile, window, hop)["L"]                                           # raises on L, tile, window, hop
    if L < 2 * d + 2:
        raise ValueError("m2h.Scorer: L = %d samples; align = %d needs at least 2 * %d + 2 = %d" % (L, d, d, 2 * d + 2))
    plan = score_plan(L - 2 * d, tile, window, hop)
    if plan["tile"] + 2 * d > ALIGN_NFFT:
        raise ValueError("m2h.Scorer: tile + 2 align = %d + 2 * %d = %d exceeds the transform's %d points" % (plan["tile"], d, plan["tile"] + 2 * d, ALIGN_NFFT))
    plan["offset"] = d
    plan["samples"] = [(t0 + d, t1 + d) for t0, t1 in plan["samples"]]
    return plan


def stoi_frames(n):
    """the frames of a range of n samples at 10 kHz: starts 0, 128, ... < n - 256 (the end is exclusive)"""
    return max(0, -(-(n - STOI_FRAME) // STOI_HOP))


def stoi_plan(plan):
    """Pure Python: the ranges of stoi=True for a score_plan / align_plan with tile = 16000 (module docstring, "STOI").

    -> {"L10", "ranges": [(start, end)] at 10 kHz, the whole recording first and then the plan's M windows, "slots": the first frame slot of
    every range in m2h_stoi_ranges' work buffers (a window owns "per_window" of them), "total": their count (at least 1)}."""
    if plan["tile"] != STOI_TILE:
        raise ValueError("m2h.Scorer: stoi=True needs tile = %d (one second), got %d" % (STOI_TILE, plan["tile"]))
    L10 = -(-plan["L"] * 5 // 8)
    ranges = [(0, L10)] + [(min(m * plan["hop"] * STOI_FS, L10), min((m * plan["hop"] + plan["window"]) * STOI_FS, L10)) for m in range(plan["M"])]
    per_window = stoi_frames(min(plan["window"] * STOI_FS, L10))
    slots = [0] + [stoi_frames(L10) + m * per_window for m in range(plan["M"])]
    return {"L10": L10, "ranges": ranges, "slots": slots, "per_window": per_window,
            "total": max(1, stoi_frames(L10) + plan["M"] * per_window)}


def stoi_window():
    """w = hanning(258)[1:-1] rounded to float32, numpy [256]"""
    import numpy as np
    return np.hanning(STOI_FRAME + 2)[1:-1].astype(np.float32)


def lags_from_corr(c):
    """c [..., 2 D + 1] float64, column d + D the correlation at lag d -> the lag of largest |c| as int32 [...]: among equal maxima the
    smallest |d|, then the negative one (the columns reordered as 0, -1, +1, -2, +2, ... and the first maximum taken), so all zeros give
    0.  Torch on c's device; no synchronisation."""
    if not isinstance(c, torch.Tensor) or c.dtype != torch.float64:
        raise TypeError("m2h.Scorer: a correlation must be a float64 torch tensor, got %s" % (c.dtype if isinstance(c, torch.Tensor) else type(c).__name__))
    K = c.shape[-1] if c.dim() else 0
    if K < 1 or K % 2 == 0:
        raise ValueError("m2h.Scorer: a correlation holds 2 D + 1 lags, not %d" % K)
    D = K // 2
    i = torch.arange(K, device=c.device, dtype=torch.int64)
    half = (i + 1) // 2
    lag = torch.where(i % 2 == 1, -half, half)                                          # 0, -1, +1, -2, +2, ...
    first = torch.argmax(c.abs().index_select(-1, lag + D), dim=-1)                     # the first of equal maxima
    return lag[first].to(torch.int32)


def gram_signals(K):
    """N of a Gram row of K = N + N(N+1)/2 numbers (4 <= N <= 9)."""
    for N in range(4, MAX_SOURCES + 4):
        if N + N * (N + 1) // 2 == K:
            return N
    raise ValueError("m2h.Scorer: a Gram row holds N + N(N+1)/2 numbers for N = S + 3 in 4 .. 9, not %d" % K)


def _count(n, device):
    """n as a float64 tensor on `device` (a number becomes a fill: no copy from the host)"""
    if isinstance(n, torch.Tensor):
        return n.to(device=device, dtype=torch.float64)
    return torch.full((), float(n), dtype=torch.float64, device=device)


def _dot(a, b):
    """sum_k a[..., k] b[..., k], k in order: element-wise operations only, so a row's result does not depend on the batch around it"""
    acc = a[..., 0] * b[..., 0]
    for k in range(1, a.shape[-1]):
        acc = acc + a[..., k] * b[..., k]
    return acc


def solve_pivoted(A, Y):
    """A [..., S, S], Y [..., S, Q] -> (X [..., S, Q] with A X = Y, singular [...] bool).

    Gaussian elimination with partial pivoting, the LU arithmetic of torch.linalg.solve_ex, written in element-wise torch operations:
    every matrix is reduced by the same operations in the same order whatever the batch holds, which a library's batched solver does
    not promise (it may pick another algorithm at another batch size), and the Scorer's numbers are bit for bit those of the
    recording or the window scored alone.  `singular` is solve_ex's info != 0: a pivot that is exactly 0; X is then meaningless."""
    S = A.shape[-1]
    M = torch.cat([A, Y], dim=-1)
    rows = [M[..., i, :] for i in range(S)]
    singular = torch.zeros(A.shape[:-2], dtype=torch.bool, device=A.device)
    for k in range(S):
        for i in range(k + 1, S):                                                      # the first row of largest |entry| becomes the pivot row
            swap = (rows[i][..., k].abs() > rows[k][..., k].abs())[..., None]
            rows[k], rows[i] = torch.where(swap, rows[i], rows[k]), torch.where(swap, rows[k], rows[i])
        zero = rows[k][..., k] == 0
        singular = singular | zero
        pivot = torch.where(zero, torch.ones_like(rows[k][..., k]), rows[k][..., k])
        for i in range(k + 1, S):
            rows[i] = rows[i] - (rows[i][..., k] / pivot)[..., None] * rows[k]
        rows[k] = rows[k] / pivot[..., None]
    for k in reversed(range(S)):
        for i in range(k):
            rows[i] = rows[i] - rows[i][..., k:k + 1] * rows[k]
    return torch.stack([row[..., S:] for row in rows], dim=-2), singular


def metrics_from_gram(gram, n, target, C):
    """The eleven metrics from sums and Gram matrices (module docstring), in torch float64 on gram's device.

    gram   [R, C, ..., K] float64 in m2h_score_gram's layout (K = N + N(N+1)/2; signals s_0 .. s_{S-1}, est_c, mix_l, mix_r);
    n      the sample count: a number, or a tensor that broadcasts against gram.shape[:-1];
    target an int, or an integer tensor [R] on gram's device;
    C      1 (the baseline is the mean of the mixture's mean-removed channels) or 2 (axis 1 is the ear; the baseline is that ear's mixture).
    -> [R, C, ..., 11] float64 in eval_metrics.METRIC_ORDER."""
    if not isinstance(gram, torch.Tensor) or gram.dtype != torch.float64:
        raise TypeError("m2h.Scorer: gram must be a float64 torch tensor, got %s" % (gram.dtype if isinstance(gram, torch.Tensor) else type(gram).__name__))
    if C not in (1, 2) or gram.dim() < 3 or gram.shape[1] != C:
        raise ValueError("m2h.Scorer: gram must be [R, C, ..., K] with C = %r in {1, 2}, got a tensor of shape %s" % (C, tuple(gram.shape)))
    N = gram_signals(gram.shape[-1])
    S = N - 3
    dev, batch = gram.device, gram.shape[:-1]
    R = batch[0]
    sums = gram[..., :N]
    iu = torch.triu_indices(N, N, device=dev)
    G = gram.new_zeros(batch + (N, N))
    G[..., iu[0], iu[1]] = gram[..., N:]
    G[..., iu[1], iu[0]] = gram[..., N:]
    n = _count(n, dev).expand(batch)
    Gc = G - sums[..., :, None] * sums[..., None, :] / n[..., None, None]              # <a_i - mean, a_k - mean>

    if isinstance(target, torch.Tensor):
        if target.dtype not in (torch.int32, torch.int64) or tuple(target.shape) != (R,) or target.device != dev:
            raise TypeError("m2h.Scorer: a tensor `target` must be [R] = [%d] int32 or int64 on %s" % (R, dev))
        t = target.to(torch.int64).view((R,) + (1,) * (len(batch) - 1))
        row_t = torch.take_along_dim(Gc, t[..., None, None].expand(batch + (1, N)), dim=-2).squeeze(-2)
        pick = lambda v: torch.take_along_dim(v, t[..., None].expand(batch + (1,)), dim=-1).squeeze(-1)   # noqa: E731
    else:
        t = int(target)
        if not 0 <= t < S:
            raise ValueError("m2h.Scorer: target = %d is not one of the %d references" % (t, S))
        row_t = Gc[..., t, :]
        pick = lambda v: v[..., t]                                                                      # noqa: E731
    ss = pick(row_t)                                                                   # <s, s>
    P = Gc[..., :S, :S]
    keep = torch.diagonal(P, dim1=-2, dim2=-1) > 0                                      # sources with energy in this window
    keep2 = keep[..., :, None] & keep[..., None, :]
    Pk = torch.where(keep2, P, torch.zeros_like(P))
    A = Pk + torch.diag_embed((~keep).to(torch.float64))                                # the reduced normal equations, padded by ones
    valid = (ss > 0) & (n >= 2)
    A = torch.where(valid[..., None, None], A, torch.eye(S, dtype=torch.float64, device=dev).expand_as(A))

    def first(gx, xx):
        """scale_bss_eval_helper (:16-40) for a signal x given <x, a_i> (gx [..., N]) and <x, x>, all centred; and refs^T (x - alpha s)"""
        sx = pick(gx)
        alpha = sx / ss
        noise = torch.clamp(xx - 2.0 * sx + ss, min=0.0)                                # |x - s|^2
        snr = 10.0 * torch.log10(ss / noise)
        signal = alpha * alpha * ss                                                     # |alpha s|^2
        res = torch.clamp(xx - alpha * sx, min=0.0)                                     # |x - alpha s|^2
        si_sdr = 10.0 * torch.log10(signal / res)
        srr = -10.0 * torch.log10((1.0 - 1.0 / alpha) ** 2)
        sd_sdr = snr + 10.0 * torch.log10(alpha ** 2)
        rhs = torch.where(keep & valid[..., None], gx[..., :S] - alpha[..., None] * row_t[..., :S], torch.zeros_like(Pk[..., 0]))
        return (si_sdr, sd_sdr, snr, srr), signal, res, rhs

    def second(signal, res, rhs, b0):
        """:45-55: the projection's two norms as quadratic forms"""
        b = torch.where(keep, b0 + EPS, torch.zeros_like(rhs))
        Pb = Pk[..., :, 0] * b[..., 0:1]
        for k in range(1, S):
            Pb = Pb + Pk[..., :, k] * b[..., k:k + 1]
        bPb = _dot(b, Pb)
        interf = torch.clamp(bPb, min=0.0)                                              # |refs b|^2
        artif = torch.clamp(res - 2.0 * _dot(b, rhs) + bPb, min=0.0) + n * (EPS * EPS)  # |x - alpha s - refs b + EPS|^2
        nan = torch.full_like(ss, _NAN)
        return torch.where(singular, nan, 10.0 * torch.log10(signal / interf)), torch.where(singular, nan, 10.0 * torch.log10(signal / artif))

    e, l, r = S, S + 1, S + 2
    parts = [first(Gc[..., e, :], Gc[..., e, e])]
    if C == 1:
        parts.append(first(0.5 * (Gc[..., l, :] + Gc[..., r, :]), 0.25 * (Gc[..., l, l] + 2.0 * Gc[..., l, r] + Gc[..., r, r])))
    else:
        parts.append(first(torch.stack([Gc[:, 0, ..., l, :], Gc[:, 1, ..., r, :]], dim=1), torch.stack([Gc[:, 0, ..., l, l], Gc[:, 1, ..., r, r]], dim=1)))
    x, singular = solve_pivoted(A, torch.stack([parts[0][3], parts[1][3]], dim=-1))     # one elimination, both right-hand sides
    both = []
    for q, ((si_sdr, sd_sdr, snr, srr), signal, res, rhs) in enumerate(parts):
        si_sir, si_sar = second(signal, res, rhs, x[..., q])
        both.append((si_sdr, si_sir, si_sar, sd_sdr, snr, srr))
    est, base = both
    out = torch.stack(list(est) + [est[0] - base[0], est[3] - base[3], est[4] - base[4], est[1] - base[1], est[2] - base[2]], dim=-1)
    return torch.where(valid[..., None], out, torch.full_like(out, _NAN))


def target_energy(gram, n, target):
    """The target's centred energy per Gram row (> 0: the window is `active`)."""
    N = gram_signals(gram.shape[-1])
    batch = gram.shape[:-1]
    n = _count(n, gram.device).expand(batch)
    energy = []
    for s in range(N - 3):                                                              # the diagonal entry of source s: N + idx(s, s)
        energy.append(gram[..., N + s * N - s * (s - 1) // 2] - gram[..., s] * gram[..., s] / n)
    energy = torch.stack(energy, dim=-1)
    if isinstance(target, torch.Tensor):
        t = target.to(torch.int64).view((batch[0],) + (1,) * len(batch[1:]))
        return torch.take_along_dim(energy, t[..., None].expand(batch + (1,)), dim=-1).squeeze(-1)
    return energy[..., int(target)]


def spectral_table():
    """m2h_score_spectral's transform table (include/m2h.h), numpy float32 [32, 128, 2, 64]: the window folded into the DFT rows,
    t[bt, ks, 0, l] = w[n] cos(2 pi k n / 1023), t[bt, ks, 1, l] = -w[n] sin(2 pi k n / 1023) with n = 4 ks + (l >> 4),
    k = 16 bt + (l & 15), w the periodic Hann window rounded to float32; built in float64 (the angle reduced in integers) and rounded
    once.  Rows n = 1 .. 511 serve their mirror images 1023 - n too: w and cos are even and sin is odd about 1023 / 2, and w[0] = 0."""
    import numpy as np
    N, nb = SPECTRAL_NFFT, SPECTRAL_BINS
    n, k = np.arange(nb), np.arange(nb)
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N)).astype(np.float32).astype(np.float64)
    ang = 2.0 * np.pi * ((k[:, None] * n[None, :]) % N) / N                             # [k, n]
    t = np.stack([w * np.cos(ang), -w * np.sin(ang)])                                   # [q, k, n]
    t = t.reshape(2, nb // 16, 16, nb // 4, 4).transpose(1, 3, 0, 4, 2)                 # [q, bt, k & 15, ks, n & 3] -> [bt, ks, q, n & 3, k & 15]
    return np.ascontiguousarray(t.reshape(nb // 16, nb // 4, 2, 64).astype(np.float32))


def spectral_from_sums(sums, Q):
    """The eight spectral numbers (module docstring, "Spectral") from the seven sums, element-wise in torch float64 on sums' device.

    sums [..., 7] float64; Q the tile count: a number, or a tensor that broadcasts against sums.shape[:-1] -> [..., 8] in SPECTRAL_ORDER."""
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64:
        raise TypeError("m2h.Scorer: spectral sums must be a float64 torch tensor, got %s" % (sums.dtype if isinstance(sums, torch.Tensor) else type(sums).__name__))
    if sums.dim() < 1 or sums.shape[-1] != 7:
        raise ValueError("m2h.Scorer: spectral sums hold 7 numbers per row, got a tensor of shape %s" % (tuple(sums.shape),))
    den = 2.0 * SPECTRAL_BINS * SPECTRAL_FRAMES * _count(Q, sums.device).expand(sums.shape[:-1])
    l2, l2c, sc = sums[..., 3] / den, sums[..., 4] / den, torch.sqrt(sums[..., 3] / sums[..., 0])
    l2b, l2cb, scb = sums[..., 5] / den, sums[..., 6] / den, torch.sqrt(sums[..., 5] / sums[..., 0])
    return torch.stack([l2, l2c, sc, l2b, l2cb, scb, l2b - l2, l2cb - l2c], dim=-1)


def spatial_from_sums(sums):
    """The interaural cues and their nine errors (module docstring, "Spatial") from band sums, element-wise in torch float64 on sums' device;
    the bands are added by element-wise additions of slices in a fixed pairwise order (never a library reduction, which may pick another
    order at another batch size), so a row's result does not depend on the batch around it.

    sums [..., 3, 32, 4] float64 (signal G, E, B; band; PL, PR, CRE, CIM) -> (metrics [..., 9] in SPATIAL_ORDER,
    cues [..., 3, 32, 3]: ILD in dB, IPD in rad, IC; IEEE rules apply in a band without energy)."""
    import math
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64:
        raise TypeError("m2h.Scorer: spatial sums must be a float64 torch tensor, got %s" % (sums.dtype if isinstance(sums, torch.Tensor) else type(sums).__name__))
    if sums.dim() < 3 or tuple(sums.shape[-3:]) != (3, SPATIAL_BANDS, 4):
        raise ValueError("m2h.Scorer: spatial sums hold [3, %d, 4] numbers per row, got a tensor of shape %s" % (SPATIAL_BANDS, tuple(sums.shape),))
    pl, pr, cre, cim = sums[..., 0], sums[..., 1], sums[..., 2], sums[..., 3]           # [..., 3, 32]
    ild = 10.0 * torch.log10(pl / pr)
    ipd = torch.atan2(cim, cre)
    ic = torch.hypot(cre, cim) / torch.sqrt(pl * pr)
    has = (pl > 0) & (pr > 0)
    w = pl[..., 0, :] + pr[..., 0, :]                                                   # the target's band energy [..., 32]

    def mean(d, ok, bands):
        a = torch.stack([w * d, w])[..., :bands]                                        # numerator and denominator terms [2, ..., bands]
        a = torch.where(ok[..., :bands], a, torch.zeros_like(a))
        n = bands
        while n > 1:                                                                    # halves added onto each other; an odd one out is carried
            h = n // 2
            a = torch.cat([a[..., :h] + a[..., h:2 * h], a[..., 2 * h:n]], dim=-1)
            n = a.shape[-1]
        return a[0, ..., 0] / a[1, ..., 0]                                              # 0 / 0: no valid band is NaN

    def errors(x):
        ok = (w > 0) & has[..., 0, :] & has[..., x, :]
        d = ipd[..., x, :] - ipd[..., 0, :]
        d = d - (2.0 * math.pi) * torch.ceil((d - math.pi) / (2.0 * math.pi))          # wrapped to (-pi, pi]
        return [mean((ild[..., x, :] - ild[..., 0, :]).abs(), ok, SPATIAL_BANDS), mean(d.abs(), ok, SPATIAL_IPD_BANDS),
                mean((ic[..., x, :] - ic[..., 0, :]).abs(), ok, SPATIAL_BANDS)]

    e, b = errors(1), errors(2)
    return torch.stack(e + b + [b[k] - e[k] for k in range(3)], dim=-1), torch.stack([ild, ipd, ic], dim=-1)


def itd_table():
    """m2h_itd_gcc's twiddles (include/m2h.h), numpy float64 [8184, 2]: t[q] = (cos, sin)(2 pi q / 8184), 8184 = 1023 . ITD_UPSAMPLE.  The
    kernel reads entry (k i) mod 8184 for bin k and lag i / 8 samples: the angle is reduced in integers, never as a float."""
    import numpy as np
    P = SPECTRAL_NFFT * ITD_UPSAMPLE
    ang = 2.0 * np.pi * (np.arange(P) % P) / P
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=-1))


def itd_has_band(sums):
    """sums [..., 256, 2] float64 (CRE, CIM per bin) -> [...] bool: some bin of the band ITD_BINS has |Phi_k| > 0, by m2h_itd_gcc's test"""
    band = sums[..., ITD_BINS[0]:ITD_BINS[1], :]
    return (torch.sqrt(band[..., 0] * band[..., 0] + band[..., 1] * band[..., 1]) > 0).any(dim=-1)


def itd_from_gcc(g, has=None):
    """The pick and the nine numbers of "ITD" (module docstring), element-wise in torch float64 on g's device; no synchronisation.

    g [..., 3, 257] float64: GCC-PHAT of the target, the estimate and the mixture, column i + 128 the lag of i / 8 samples;
    has [..., 3] bool or None: the signal has a bin in the band (False: its itd and peak are NaN) -> [..., 9] in ITD_ORDER.
    The lag is the one of largest g -- not |g| --; among equal maxima the smallest |i|, then the negative one (the columns reordered as
    0, -1, +1, -2, +2, ... and the first maximum taken, as in lags_from_corr), so all zeros give 0."""
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float64:
        raise TypeError("m2h.Scorer: a GCC-PHAT function must be a float64 torch tensor, got %s" % (g.dtype if isinstance(g, torch.Tensor) else type(g).__name__))
    if g.dim() < 2 or tuple(g.shape[-2:]) != (3, ITD_LAGS):
        raise ValueError("m2h.Scorer: GCC-PHAT functions hold [3, %d] numbers per row, got a tensor of shape %s" % (ITD_LAGS, tuple(g.shape),))
    H = ITD_LAGS // 2
    i = torch.arange(ITD_LAGS, device=g.device, dtype=torch.int64)
    half = (i + 1) // 2
    lag = torch.where(i % 2 == 1, -half, half)                                          # 0, -1, +1, -2, +2, ...
    ordered = g.index_select(-1, lag + H)
    first = torch.argmax(ordered, dim=-1, keepdim=True)                                 # the first of equal maxima
    peak = torch.take_along_dim(ordered, first, dim=-1).squeeze(-1)                     # [..., 3]
    itd = lag[first.squeeze(-1)].to(torch.float64) * ITD_US_PER_STEP
    if has is not None:
        nan = torch.full_like(peak, _NAN)
        itd, peak = torch.where(has, itd, nan), torch.where(has, peak, nan)
    err, base = (itd[..., 1] - itd[..., 0]).abs(), (itd[..., 2] - itd[..., 0]).abs()
    return torch.stack([itd[..., 0], itd[..., 1], itd[..., 2], err, base, base - err, peak[..., 0], peak[..., 1], peak[..., 2]], dim=-1)


def bss_filters(corr, target):
    """The distortion filters of "BSS" (module docstring) from the whole-recording one-sided correlations, torch float64 on corr's device.

    corr [R, C, S, S + 2, T] float64 (m2h_bss_corr's layout, tiles added); target an int or R ints (host)
    -> (h [R, C, 2, S + 1, T]: per right-hand side (estimate, baseline) the joint filters and, in slot S, the target-alone filter;
        ok [R, C] bool: the target has energy and both factorisations succeeded).
    One (r, c) at a time, so that a recording's bits do not depend on the batch; no host synchronisation of its own."""
    if not isinstance(corr, torch.Tensor) or corr.dtype != torch.float64:
        raise TypeError("m2h.Scorer: correlations must be a float64 torch tensor, got %s" % (corr.dtype if isinstance(corr, torch.Tensor) else type(corr).__name__))
    if corr.dim() != 5 or corr.shape[3] != corr.shape[2] + 2:
        raise ValueError("m2h.Scorer: correlations must be [R, C, S, S + 2, T], got a tensor of shape %s" % (tuple(corr.shape),))
    R, C, S, _, T = corr.shape
    dev = corr.device
    target = [int(target)] * R if isinstance(target, int) else [int(t) for t in target]
    a = torch.arange(T, device=dev, dtype=torch.int64)
    idx = (T - 1) + a[:, None] - a[None, :]                                             # G[(i, a), (k, b)] = c_ik[a - b]
    eye4 = (torch.eye(S, dtype=torch.float64, device=dev)[:, None, :, None] * torch.eye(T, dtype=torch.float64, device=dev)[None, :, None, :])
    h = torch.empty((R, C, 2, S + 1, T), dtype=torch.float64, device=dev)
    ok = torch.empty((R, C), dtype=torch.bool, device=dev)
    for r in range(R):
        j = target[r]
        for c in range(C):
            co = corr[r, c]
            two = co.new_empty((S, S, 2 * T - 1))                                       # c_ik[d] at index d + T - 1
            for i in range(S):
                for k in range(i, S):
                    row = torch.cat([co[k, i].flip(0)[:-1], co[i, k]])
                    two[i, k] = row
                    if k > i:
                        two[k, i] = row.flip(0)
            keep = torch.stack([co[i, i, 0] for i in range(S)]) > 0                     # references with energy
            G = torch.where(keep[:, None, None, None] & keep[None, None, :, None], two[:, :, idx].permute(0, 2, 1, 3), eye4)
            rhs = torch.where(keep[:, None, None], co[:, S:].permute(0, 2, 1), torch.zeros((), dtype=torch.float64, device=dev))    # [S, T, 2]
            chol, info = torch.linalg.cholesky_ex(G.reshape(S * T, S * T))
            h[r, c, :, :S] = torch.cholesky_solve(rhs.reshape(S * T, 2), chol).t().reshape(2, S, T)
            chol_j, info_j = torch.linalg.cholesky_ex(two[j, j][idx])
            h[r, c, :, S] = torch.cholesky_solve(co[j, S:].t().contiguous(), chol_j).t()
            ok[r, c] = keep[j] & (info == 0) & (info_j == 0)
    return h, ok


def bss_from_sums(sums, ok=None):
    """The nine BSS numbers (module docstring, "BSS") from the ten sums, element-wise in torch float64 on sums' device.

    sums [..., 10] float64; ok: a bool tensor that broadcasts against sums.shape[:-1] (False: nine NaN) -> [..., 9] in BSS_ORDER."""
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64:
        raise TypeError("m2h.Scorer: bss sums must be a float64 torch tensor, got %s" % (sums.dtype if isinstance(sums, torch.Tensor) else type(sums).__name__))
    if sums.dim() < 1 or sums.shape[-1] != 10:
        raise ValueError("m2h.Scorer: bss sums hold 10 numbers per row, got a tensor of shape %s" % (tuple(sums.shape),))
    db = lambda num, den: 10.0 * torch.log10(num / den)                                 # noqa: E731
    e = [db(sums[..., 0], sums[..., 1]), db(sums[..., 0], sums[..., 2]), db(sums[..., 3], sums[..., 4])]
    b = [db(sums[..., 5], sums[..., 6]), db(sums[..., 5], sums[..., 7]), db(sums[..., 8], sums[..., 9])]
    out = torch.stack(e + b + [e[k] - b[k] for k in range(3)], dim=-1)
    return out if ok is None else torch.where(ok[..., None], out, torch.full_like(out, _NAN))


def _whole_then_track(tiles, plan, lead=2):
    """tiles [R, C, J, ...] (lead = 2) or [R, J, ...] (lead = 1) float64, contiguous -> the same with 1 + M in place of J: all J tiles added
    in tile order, then the plan's M windows"""
    J, M = plan["J"], plan["M"]
    flat = tiles if (lead, tiles.dim()) == (2, 4) else tiles.view(tiles.shape[0], tiles.shape[1] if lead == 2 else 1, J, -1)
    both = torch.cat([ops.score_windows(flat, 1, J, 1), ops.score_windows(flat, M, plan["window"], plan["hop"])], dim=2)
    return both if flat is tiles else both.view(tiles.shape[:lead] + (1 + M,) + tiles.shape[lead + 1:])


def _rows(v, r0, r1):
    """the recordings r0 .. r1 - 1 of a per-recording argument: a tensor is sliced; one int for all (a target) or None (no lag) is passed on"""
    return v[r0:r1] if isinstance(v, torch.Tensor) else v


def _cat(groups):
    """the groups' results as one tensor (a single group as it is: no copy)"""
    return groups[0] if len(groups) == 1 else torch.cat(groups)


class Scorer:
    def __init__(self, device, max_corr_bytes=DEFAULT_MAX_CORR_BYTES):
        if isinstance(max_corr_bytes, bool) or int(max_corr_bytes) < 1:
            raise ValueError("m2h.Scorer: max_corr_bytes must be positive, got %r" % (max_corr_bytes,))
        self.device = torch.device(device)
        self.max_corr_bytes = int(max_corr_bytes)   # align, bss, itd: recordings are processed in groups whose tile buffers stay under this
        self._twiddles = self._dft = self._itd = self._stoi = None     # the device tables, each filled by _table on its first use
        self._timing = None          # tools/score_bench.py: a list that receives (stage, event) marks

    def _table(self, slot, make):
        """the device table kept in the attribute `slot`: make() on the first call (the one copy from the host), the same object afterwards"""
        if getattr(self, slot) is None:
            setattr(self, slot, make())
        return getattr(self, slot)

    def _twiddle_table(self):
        """the transform's [2, 16384, 2] table on the device (m2h.audio.twiddles), copied from the host once"""
        return self._table("_twiddles", lambda: device_twiddles(self.device, ALIGN_NFFT))

    def _spectral_table(self):
        """spectral_table() on the device, copied from the host once"""
        return self._table("_dft", lambda: torch.from_numpy(spectral_table()).to(self.device))

    def _itd_table(self):
        """itd_table() on the device, copied from the host once"""
        return self._table("_itd", lambda: torch.from_numpy(itd_table()).to(self.device))

    def _stoi_tables(self):
        """(the 16 kHz -> 10 kHz polyphase table [5, 33], the window [256], the 512-point transform's twiddles) on the device, copied from the
        host once"""
        def make():
            from .resample import design, polyphase_table
            import numpy as np
            up, _, _, taps = design(STOI_TILE, STOI_FS)
            return (torch.from_numpy(polyphase_table(taps.astype(np.float32), up)).to(self.device), torch.from_numpy(stoi_window()).to(self.device),
                    device_twiddles(self.device, STOI_NFFT))
        return self._table("_stoi", make)

    def _groups(self, R, bytes_per_recording):
        """[(r0, r1)]: the R recordings in groups whose tile buffers stay under max_corr_bytes (a single recording above it goes alone)"""
        step = max(1, self.max_corr_bytes // bytes_per_recording)
        return [(r0, min(r0 + step, R)) for r0 in range(0, R, step)]

    def _stoi_ranges(self, plan, sp):
        """m2h_stoi_ranges' table [1 + M, 3] int64 of stoi_plan's ranges, built on the device: fills and aranges, no copy from the host"""
        dev, M, L10 = self.device, plan["M"], sp["L10"]
        m = torch.arange(M, device=dev, dtype=torch.int64)
        table = torch.empty((1 + M, 3), dtype=torch.int64, device=dev)
        table[0, 0].fill_(0)
        table[0, 1].fill_(L10)
        table[0, 2].fill_(0)
        table[1:, 0] = torch.clamp(m * (plan["hop"] * STOI_FS), max=L10)
        table[1:, 1] = torch.clamp((m * plan["hop"] + plan["window"]) * STOI_FS, max=L10)
        table[1:, 2] = sp["slots"][1] + m * sp["per_window"]
        return table

    def _mark(self, stage):
        if self._timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.device))
            self._timing.append((stage, ev))

    def _check(self, estimate, references, mixture, target, tile, window, hop, align=None, spectral=False, spatial=False, stoi=False, bss=None,
               itd=False):
        for name, t in (("estimate", estimate), ("references", references), ("mixture", mixture)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("m2h.Scorer: %s must be a torch tensor, got %s" % (name, type(t).__name__))
            if t.dtype != torch.float32:
                raise TypeError("m2h.Scorer: %s must be float32, got %s" % (name, t.dtype))
        if references.dim() not in (3, 4):
            raise ValueError("m2h.Scorer: references must be [R, S, L] or [R, S, C, L], got a tensor of shape %s" % (tuple(references.shape),))
        if estimate.dim() not in (2, 3):
            raise ValueError("m2h.Scorer: estimate must be [R, L] or [R, C, L], got a tensor of shape %s" % (tuple(estimate.shape),))
        if mixture.dim() != 3 or mixture.shape[1] != 2:
            raise ValueError("m2h.Scorer: mixture must be [R, 2, L], got a tensor of shape %s" % (tuple(mixture.shape),))
        refs = references if references.dim() == 4 else references.unsqueeze(2)
        est = estimate if estimate.dim() == 3 else estimate.unsqueeze(1)
        R, S, C, L = refs.shape
        if C not in (1, 2):
            raise ValueError("m2h.Scorer: references have C = %d channels; 1 or 2 are supported" % C)
        if est.shape[1] != C:
            raise ValueError("m2h.Scorer: references have C = %d channels and the estimate has %d" % (C, est.shape[1]))
        if not 1 <= S <= MAX_SOURCES:
            raise ValueError("m2h.Scorer: S = %d reference sources; 1 .. %d are supported" % (S, MAX_SOURCES))
        if R < 1 or est.shape[0] != R or mixture.shape[0] != R:
            raise ValueError("m2h.Scorer: references, estimate and mixture hold R = %d, %d and %d recordings; one R >= 1 is required"
                             % (R, est.shape[0], mixture.shape[0]))
        if L < 1 or est.shape[2] != L or mixture.shape[2] != L:
            raise ValueError("m2h.Scorer: references, estimate and mixture are L = %d, %d and %d samples long; one L >= 1 is required"
                             % (L, est.shape[2], mixture.shape[2]))
        for name, t in (("estimate", estimate), ("references", references), ("mixture", mixture)):
            if L > 1 and t.stride(-1) != 1:
                raise ValueError("m2h.Scorer: the last stride of %s is %d; 1 is required (the scorer makes no hidden copy)" % (name, t.stride(-1)))
        if isinstance(target, torch.Tensor):
            if target.is_cuda:
                raise TypeError("m2h.Scorer: target must be host integers (its range is checked before any launch), got a tensor on %s" % (target.device,))
            target = target.tolist()
        given = target
        try:
            target = operator.index(given) if not isinstance(given, bool) else None
        except TypeError:
            try:
                target = [operator.index(t) for t in given]
            except TypeError:
                target = None
        if target is None:
            raise TypeError("m2h.Scorer: target must be an int or R ints, got %r" % (given,))
        if not isinstance(target, int) and len(target) != R:
            raise ValueError("m2h.Scorer: target must be an int or R = %d ints, got %d of them" % (R, len(target)))
        for t in ([target] if isinstance(target, int) else target):
            if not 0 <= t < S:
                raise ValueError("m2h.Scorer: target %d is not one of the S = %d references (0 .. %d)" % (t, S, S - 1))
        if not isinstance(target, int) and len(set(target)) == 1:
            target = target[0]
        plan = score_plan(L, tile, window, hop) if align is None else align_plan(L, align, tile, window, hop)      # raises on tile, window, hop, align
        if spatial and C != 2:
            raise ValueError("m2h.Scorer: spatial=True compares the two ears and needs C = 2 channels, got C = %d" % C)
        if not isinstance(itd, bool):
            raise TypeError("m2h.Scorer: itd must be a bool, got %r" % (itd,))
        if itd and C != 2:
            raise ValueError("m2h.Scorer: itd=True compares the two ears and needs C = 2 channels, got C = %d" % C)
        for name, on in (("spatial", spatial), ("spectral", spectral), ("stoi", stoi), ("itd", itd)):
            if on and plan["tile"] != SPECTRAL_TILE:
                raise ValueError("m2h.Scorer: %s=True needs tile = %d (one second), got %d" % (name, SPECTRAL_TILE, plan["tile"]))
        if bss is not None:
            if isinstance(bss, bool) or not isinstance(bss, int):
                raise TypeError("m2h.Scorer: bss must be an int (the filter length in taps) or None, got %r" % (bss,))
            if not 1 <= bss <= BSS_MAX_TAPS:
                raise ValueError("m2h.Scorer: bss must be in 1 .. %d taps, got %r" % (BSS_MAX_TAPS, bss))
            if plan["L"] < S * bss:
                raise ValueError("m2h.Scorer: bss = %d taps and S = %d references need at least S * bss = %d scored samples, got %d: the normal "
                                 "equations would be rank-deficient" % (bss, S, S * bss, plan["L"]))
        for name, t in (("estimate", estimate), ("references", references), ("mixture", mixture)):
            if not t.is_cuda or t.device != self.device:
                raise ValueError("m2h.Scorer: %s must live on %s, got %s; the scorer has no CPU path" % (name, self.device, t.device))
        return refs, est, target, plan

    def score(self, estimate, references, mixture, target=0, tile=DEFAULT_TILE, window=1, hop=1, align=None, spectral=False, spatial=False,
              stoi=False, bss=None, itd=False):
        """-> {"whole": [R, C, 11], "track": [R, C, M, 11], "active": [R, C, M] bool, "plan": score_plan(...)}; float64 on the device, in
        eval_metrics.METRIC_ORDER; no host synchronisation.  With align=D (an int, the largest lag searched in samples) the estimate is
        aligned to its target first: also "lag": [R, C] int32 and "lag_track": [R, C, M] int32 on the device, and "plan" is
        align_plan(...).  With spectral=True (tile must be 16000) also "spectral_whole": [R, C, 8] and "spectral_track": [R, C, M, 8],
        float64 in SPECTRAL_ORDER.  With spatial=True (two channels, tile must be 16000) also "spatial_whole": [R, 9] and
        "spatial_track": [R, M, 9], float64 in SPATIAL_ORDER, and the cues themselves, "spatial_cues": [R, M, 3, 32, 3] (signal target /
        estimate / mixture, band, ILD / IPD / IC).  With stoi=True (tile must be 16000) also "stoi_whole": [R, C, 6] and "stoi_track":
        [R, C, M, 6], float64 in STOI_ORDER, and "stoi_frames": [R, C, 1 + M] int64, the kept-frame count of the whole recording and of
        every window.  With bss=T (an int, the distortion filter's taps, 1 .. 512) also "bss_whole": [R, C, 9] and "bss_track": [R, C, M, 9],
        float64 in BSS_ORDER.  With itd=True (two channels, tile must be 16000) also "itd_whole": [R, 9] and "itd_track": [R, M, 9], float64
        in ITD_ORDER (microseconds and peak heights), and the GCC-PHAT functions themselves, "itd_gcc": [R, 1 + M, 3, 257] (the whole
        recording first; signal target / estimate / mixture; the lags i / 8 samples, i = -128 .. 128).  The module docstring holds the
        definition."""
        refs, est, targets, plan = self._check(estimate, references, mixture, target, tile, window, hop, align, spectral, spatial, stoi, bss, itd)
        with torch.cuda.device(self.device):
            target = targets                                                            # host integers (bss_filters); on the device:
            if not isinstance(targets, int):                                            # R small fills: no copy from the host
                target = torch.empty((len(targets),), dtype=torch.int64, device=self.device)
                for r, t in enumerate(targets):
                    target[r].fill_(t)
            # what every stage takes: the signals, the target on the device and on the host, the plan, the region's offset D, the taps of
            # bss=T; `lag` [R, C] int32 once _stage_align has run and `m`, the windows' first tiles [M] int64, once _stage_eleven has
            call = SimpleNamespace(refs=refs, est=est, mixture=mixture, target=target, targets=targets, plan=plan, D=plan.get("offset", 0), taps=bss,
                                   lag=None, m=None)
            self._mark("start")
            out = self._stage_align(call) if align is not None else {}
            eleven = self._stage_eleven(call)
            for on, stage in ((spectral, self._stage_spectral), (spatial, self._stage_spatial), (stoi, self._stage_stoi),
                              (bss is not None, self._stage_bss), (itd, self._stage_itd)):
                if on:
                    out.update(stage(call))
        out.update(eleven)                                                              # (their keys come last)
        return out

    def _stage_align(self, call):
        """align=D ("Alignment"): the lags of every recording and channel, whole and per window, as the keys lag and lag_track; sets call.lag"""
        R, _, C, _ = call.refs.shape
        plan, D, tw = call.plan, call.D, self._twiddle_table()
        lags = []
        for r0, r1 in self._groups(R, C * plan["J"] * (2 * D + 1) * 8):
            ct = ops.align_corr(call.refs[r0:r1], call.est[r0:r1], _rows(call.target, r0, r1), plan["tile"], D, tw)     # [r, C, J, 2 D + 1]
            self._mark("align_corr")
            lags.append(lags_from_corr(_whole_then_track(ct, plan)))
            del ct
            self._mark("lag_pick")
        lags = _cat(lags)                                                               # [R, C, 1 + M]: whole, then the track
        call.lag = lags[:, :, 0].contiguous()
        return {"lag": call.lag, "lag_track": lags[:, :, 1:]}

    def _stage_eleven(self, call):
        """the eleven numbers as the keys whole, track, active and plan; sets call.m"""
        plan, dev, C = call.plan, self.device, call.refs.shape[2]
        M, tile, window, hop, Ls = (plan[k] for k in ("M", "tile", "window", "hop", "L"))      # Ls: the scored samples per row
        if call.lag is None:
            tiles = ops.score_gram(call.refs, call.est, call.mixture, tile)             # [R, C, J, K]
        else:
            tiles = ops.score_gram_lag(call.refs, call.est, call.mixture, tile, call.lag, call.D)
        self._mark("score_gram")
        gram = _whole_then_track(tiles, plan)
        call.m = m = torch.arange(M, device=dev, dtype=torch.int64) * hop
        n = (torch.clamp((m + window) * tile, max=Ls) - torch.clamp(m * tile, max=Ls)).to(torch.float64)
        n = torch.cat([torch.full((1,), float(Ls), dtype=torch.float64, device=dev), n])
        scores = metrics_from_gram(gram, n, call.target, C)
        active = target_energy(gram[:, :, 1:], n[1:], call.target) > 0
        self._mark("metrics")
        return {"whole": scores[:, :, 0], "track": scores[:, :, 1:], "active": active, "plan": plan}

    def _stage_spectral(self, call):
        """spectral=True ("Spectral"): the keys spectral_whole and spectral_track"""
        J, window, dev = call.plan["J"], call.plan["window"], self.device
        sums = ops.score_spectral(call.refs, call.est, call.mixture, call.target, self._spectral_table(), call.lag, call.D)     # [R, C, J, 7]
        self._mark("score_spectral")
        sums = _whole_then_track(sums, call.plan)
        q = (torch.clamp(call.m + window, max=J) - torch.clamp(call.m, max=J)).to(torch.float64)
        spec = spectral_from_sums(sums, torch.cat([torch.full((1,), float(J), dtype=torch.float64, device=dev), q]))
        self._mark("spectral_metrics")
        return {"spectral_whole": spec[:, :, 0], "spectral_track": spec[:, :, 1:]}

    def _stage_spatial(self, call):
        """spatial=True ("Spatial"): the keys spatial_whole, spatial_track and spatial_cues"""
        sums = ops.score_spatial(call.refs, call.est, call.mixture, call.target, self._spectral_table(), call.lag, call.D)      # [R, J, 3, 32, 4]
        self._mark("score_spatial")
        spat, cues = spatial_from_sums(_whole_then_track(sums, call.plan, lead=1))
        self._mark("spatial_metrics")
        return {"spatial_whole": spat[:, 0], "spatial_track": spat[:, 1:], "spatial_cues": cues[:, 1:]}

    def _stage_stoi(self, call):
        """stoi=True ("STOI"): the keys stoi_whole, stoi_track and stoi_frames"""
        table, win, tw = self._stoi_tables()
        sp = stoi_plan(call.plan)
        x10 = ops.stoi_resample(call.refs, call.est, call.mixture, call.target, table, call.lag, call.D)                        # [R, C, 3, L10]
        self._mark("stoi_resample")
        st = ops.stoi_ranges(x10, self._stoi_ranges(call.plan, sp), sp["total"], win, tw)
        self._mark("stoi_ranges")
        return {"stoi_whole": st["out"][:, :, 0], "stoi_track": st["out"][:, :, 1:], "stoi_frames": st["kept"][..., 0].to(torch.int64)}

    def _stage_bss(self, call):
        """bss=T ("BSS"), T = call.taps: the keys bss_whole and bss_track"""
        R, S, C, _ = call.refs.shape
        plan, T, J, tile = call.plan, call.taps, call.plan["J"], call.plan["tile"]
        corr = []
        for r0, r1 in self._groups(R, C * J * S * (S + 2) * T * 8):
            ct = ops.bss_corr(call.refs[r0:r1], call.est[r0:r1], call.mixture[r0:r1], tile, T, _rows(call.lag, r0, r1), call.D)   # [r, C, J, S, S + 2, T]
            corr.append(ops.score_windows(ct.view(r1 - r0, C, J, S * (S + 2) * T), 1, J, 1).view(r1 - r0, C, S, S + 2, T))
            del ct
        self._mark("bss_corr")
        h, ok = bss_filters(_cat(corr), call.targets)
        self._mark("bss_solve")
        sums = ops.bss_project(call.refs, call.est, call.mixture, call.target, h, tile, call.lag, call.D)                       # [R, C, J, 10]
        self._mark("bss_project")
        b9 = bss_from_sums(_whole_then_track(sums, plan), ok[:, :, None])
        self._mark("bss_metrics")
        return {"bss_whole": b9[:, :, 0], "bss_track": b9[:, :, 1:]}

    def _stage_itd(self, call):
        """itd=True ("ITD"): the keys itd_whole, itd_track and itd_gcc"""
        dft, tab = self._spectral_table(), self._itd_table()
        gcc, has = [], []
        for r0, r1 in self._groups(call.refs.shape[0], call.plan["J"] * 3 * ITD_BINS[1] * 2 * 8):
            sums = ops.score_itd(call.refs[r0:r1], call.est[r0:r1], call.mixture[r0:r1], _rows(call.target, r0, r1), dft, _rows(call.lag, r0, r1),
                                 call.D)                                                # [r, J, 3, 256, 2]
            self._mark("score_itd")
            sums = _whole_then_track(sums, call.plan, lead=1)                           # [r, 1 + M, 3, 256, 2]
            self._mark("itd_windows")
            gcc.append(ops.itd_gcc(sums, tab, *ITD_BINS))                               # [r, 1 + M, 3, 257]
            has.append(itd_has_band(sums))
            del sums
            self._mark("itd_gcc")
        gcc = _cat(gcc)
        nine = itd_from_gcc(gcc, _cat(has))
        self._mark("itd_metrics")
        return {"itd_whole": nine[:, 0], "itd_track": nine[:, 1:], "itd_gcc": gcc}


def summarize(result):
    """Host-side summary of Scorer.score's result for one call, as Python lists (one synchronisation): {"metrics", "whole": [R][C][11],
    "track_mean", "track_median": over the active windows ([R][C][11], NaN without any), "active_windows": [R][C]}, and for every other family
    of FAMILIES that the result holds the same four keys under its prefix ("spectral_metrics", "spectral_whole", ...), the mean and median over
    that family's windows; spatial and itd are per recording, [R][9]; stoi=True results also carry "stoi_frames" [R][C][1 + M]."""
    import numpy as np
    active = result["active"].cpu().numpy()
    out = {}
    for prefix, order, binaural, windows, extras in FAMILIES:
        if prefix + "whole" not in result:
            continue
        whole, track = result[prefix + "whole"].cpu().numpy(), result[prefix + "track"].cpu().numpy()
        keep = active if windows == "active" else active.all(axis=1) if windows == "both" else ~np.isnan(track).any(axis=-1)
        mean, median = _mean_median(track, keep)
        out.update({prefix + "metrics": list(order), prefix + "whole": whole.tolist(), prefix + "track_mean": mean.tolist(),
                    prefix + "track_median": median.tolist()})
        if not prefix:
            out["active_windows"] = active.sum(axis=-1).tolist()
        out.update({key: result[key].cpu().tolist() for key, carried in extras if carried})
    return out


def _mean_median(track, keep):
    """track [..., M, K] and keep [..., M] bool, numpy -> (mean, median) [..., K] of every row's kept windows, NaN where a row keeps none"""
    import numpy as np
    mean, median = (np.full(track.shape[:-2] + track.shape[-1:], np.nan) for _ in range(2))
    with np.errstate(all="ignore"):
        for i in np.ndindex(keep.shape[:-1]):
            rows = track[i][keep[i]]
            if rows.shape[0]:
                mean[i], median[i] = rows.mean(axis=0), np.median(rows, axis=0)
    return mean, median
