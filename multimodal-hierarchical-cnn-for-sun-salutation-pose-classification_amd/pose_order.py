"""Pose-order decoding on the device: the best path through the steps of the pose sequence, and the rounds it makes
(csrc/pose_order.hip).  PoseTimeline smooths and debounces, but to it the twelve steps of a Sun Salutation are twelve unrelated
labels: its label may go from step 3 to step 7 and back, and it cannot tell the first Hasta Uttanasana of a round from the
second.  Here the STATES of a hidden-Markov chain are the steps, each emitting one class, and a transition table says which
step may follow which.  The reference has no such step.  In the video loop it sits between the timeline and the annotator:

    state_class, trans = cyclic_prior(step_classes, stay=prob_score(0.9), advance=prob_score(0.1))
    decoder = PoseOrderDecoder(state_class, trans, device, class_names=class_names)
    posterior = PosePosterior(state_class, trans, device, class_names=class_names)
    for frames, landmarks, detected in video:                       # chunks of any length
        probs, _, _ = predict(model(pre(frames), pose(landmarks, detected)))
        pred, _, stable, rows = timeline.update(probs, smoothed=True)
        path, path_class = decoder.decode(rows)                     # nothing read back
        rounds += decoder.cycles(path)                              # int64 [streams], on the device
        confidence = posterior.confidence(posterior.smooth(rows), path)   # how sure the chain is of the step it drew
        out = annotator.draw(frames, landmarks, detected, path_class, confidence)

Scores are integers: an emission is log2 p in units of 1/256 bit, read off the float's bit pattern (`prob_score` is the same
rule on the host), transitions are int32 in [-65536, 0].  So every output is the same bits on every run, and a stream handed
over in any split into calls gives the filtered states, emissions and carry of one call; the last call's path is the one-call
path on its frames, earlier calls' paths are the best given what had been seen by then.  include/qtcnn.h states the rule.
Calls of up to TILE = 64 frames are one launch of one wave per stream; longer calls are cut into tiles whose (max, +) products
are formed in parallel (five launches, seven above 32 tiles; a workspace that grows on demand).  Limits: S <= 64 states,
C <= 64 classes, 2^20 frames per call.

PosePosterior (csrc/pose_posterior.hip) gives the marginals of the same chain: posterior[f][j], the probability of step j at
frame f given every frame up to the end of the call (forward-backward), filtered[f][j] given the frames up to f alone, the
posterior summed by class on request, and the evidence in bits.  The rule is in log2 (an all -65536 table would underflow any scaled
probability), every sum runs in a fixed order, and whatever grows with the frame count is a double.  Calls of up to 64 frames are
one launch, and there a split into calls changes no bit of filtered, of the evidence total or of the carry; longer calls go
through tile products in the (L, +) semiring (three launches) and differ from the frame-by-frame rule by f32 rounding.

PoseOrderLearner (csrc/pose_posterior.hip, csrc/pose_prior.hip) fits the table that the two of them take, by Baum-Welch on the
device: the E-step is the posterior's forward-backward with the pairwise posteriors xi taken out of the backward step and summed
over the frames into float64 accumulators in a fixed order, the M-step turns the counts into int32 scores.

    learner = PoseOrderLearner(state_class, trans, device, pseudo_count=0.0)    # trans: the shape to start from
    for it in range(iterations):
        learner.zero()
        for probs in videos:                      # f32 [B, n, C] or [n, C], whole videos: predict's or the timeline's rows
            learner.accumulate(probs)             # E-step, nothing read back
        learner.update()                          # M-step on the device; learner.trans / learner.init are the new tables
    bits, frames = learner.totals()               # the one host sync: evidence of the last E-step, frames seen
    decoder.load_tables(learner.trans, learner.init); posterior.load_tables(learner.trans, learner.init)

`fit(videos, iterations)` is that loop, `accumulate_paths(path)` adds the hard counts of state paths (a decoder's `path` for
Viterbi training, or labelled steps), `tables()` returns numpy tables for saving.  An entry that starts at -65536 stays there.

PoseLagSmoother and PoseLagDecoder (qt_pose_lag_smooth in csrc/pose_posterior.hip, qt_pose_lag_decode in csrc/pose_order.hip)
are the two above for a loop that hands over a frame or a few per call: `push` returns the answer for the frames `lag` frames
ago given everything up to now (the posterior over a window of lag + 1 frames, the path walked back from the filtered state lag
frames later), a fixed delay behind the camera whose cost per step does not grow with the video.  The history of the last `lag`
frames travels between calls in two carry buffers that the object swaps; for any split of a stream into pushes, flush on the
last, the outputs are the bits of one push.

    smoother = PoseLagSmoother(state_class, trans, device, lag=16, streams=16)
    lagdec = PoseLagDecoder(state_class, trans, device, lag=16, streams=16)
    for rows in live:                                               # f32 [streams, 1, C]: one frame per stream
        first, lagged = smoother.push(rows)                         # frames first .. first + lagged.shape[1] - 1 (none while warming up)
        _, lag_path = lagdec.push(rows)
        confidence = smoother.confidence(lagged, lag_path)          # draw frame `first` from the ring of delayed frames
    first, lagged = smoother.push(rows[:, :0], flush=True)          # the last lag frames, at the end of the video

PoseDurationDecoder (csrc/pose_duration.hip) is the decoder with hold durations, for a whole video in hand.  The chain above
knows of a hold only one `stay` score per state, so every hold length is geometric and its most likely length is one frame: a
two-frame visit to the next step and back, or a step skipped because its three frames scored no better than staying, cost it
little, and they are what SegmentMeter's Edit and F1@IoU punish.  Here a segment is a pair (step, length), a table dur int32
[S, D] scores every length 1 .. D <= 128 per step (a longer hold is several segments joined by trans[j][j]), and the best
segmentation is found jointly with the step order (explicit-duration, semi-Markov Viterbi).  dur_open scores the first and the
last segment of a video, which the video cuts off: by default the suffix maximum of dur, so that a hold whose start or end lies
outside the video is not charged for being short.  Videos of different lengths go in one call (`lengths`); frames beyond a
video's end get path -1.  Integers throughout: the same bits on every run.  In the evaluation loop it takes the place of
`decoder.decode`:

    dur = hold_prior(S, D=64, shortest=4, longest=48)               # or duration_prior(counts) from labelled tracks, below
    durdec = PoseDurationDecoder(state_class, trans, dur, device, streams=B, class_names=class_names)
    for rows, labels, lengths in videos:                            # f32 [B, frames, C], int64 [B, frames], int32 [B]
        path, path_class, start = durdec.decode(rows, lengths=lengths, start=True)    # nothing read back
        rounds += durdec.cycles(path)
        meter.update(path_class, labels, lengths=lengths)           # SegmentMeter
        held = torch.arange(rows.shape[1], device=device) - start   # "held for n frames", for the caption
    counts = durdec.count_durations(step_labels, lengths)           # int64 [S, D] on the device: run lengths of labelled steps
    dur = duration_prior(counts.cpu().numpy())                      # the table fitted to them

PoseDurationPosterior (csrc/pose_duration_posterior.hip) gives the marginals of that chain, what PosePosterior gives under the
plain one: the probability of every step at every frame given the whole video (explicit-duration forward-backward), the same
summed by class, begin[f][j], the probability that a hold of step j begins at frame f (its sum over the frames is the expected
number of holds, and so of rounds), the evidence in bits, and the expected duration counts that fit `dur` softly.  It takes the
decoder's tables, emissions and `lengths`.  A level is a double (it falls by up to 288 bits a frame), the terms inside a log2-sum
are f32, every sum runs in a fixed order: the same bits on every run, alone or in a batch.

    durpost = PoseDurationPosterior(state_class, trans, dur, device, streams=B, class_names=class_names)
    for rows, lengths in videos:
        path, path_class = durdec.decode(rows, lengths=lengths)
        posterior, begin, bits = durpost.smooth(rows, lengths=lengths, begin=True, evidence=True)    # nothing read back
        confidence = durpost.confidence(posterior, path)            # 0 beyond a video's end
        holds = durpost.holds(begin)                                # float64 [B, S]: expected holds per step
        durpost.expected_durations(rows, lengths)                   # adds into durpost.counts, float64 [S, D]
    dur = expected_duration_prior(durpost.counts.cpu().numpy())     # the soft counterpart of duration_prior; durpost.zero()

PoseDurationLagDecoder (csrc/pose_duration_lag.hip) is PoseDurationDecoder for a loop that hands over a frame or a few per call,
as PoseLagDecoder is PoseOrderDecoder's: `push` returns, for the frames `lag` frames ago, the step and (start=True) the first frame
of its hold that PoseDurationDecoder would give on the stream up to now, a fixed delay behind the camera at a cost per step that
does not grow with the video.  The forward pass takes two maxima per frame, the closed one that the recurrence goes on from and
the open one that scores the stream as if it were cut here (dur_open); the last D rows of the forward pass and the last `lag` rows
of back-pointers travel between calls in two carry buffers that the object swaps.  Integers throughout, absolute int64 scores (a
stream may run for 2^36 frames); for any split of a stream into pushes, flush on the last, the outputs are the bits of one push.

    livedur = PoseDurationLagDecoder(state_class, trans, dur, device, lag=16, streams=16)
    for rows in live:                                               # f32 [streams, 1, C]: one frame per stream
        first, lag_path, lag_start = livedur.push(rows, start=True)     # frames first .. first + lag_path.shape[1] - 1
        held = first + torch.arange(lag_path.shape[1], device=device) - lag_start      # "held for n frames"
    first, lag_path, lag_start = livedur.push(rows[:, :0], flush=True, start=True)     # the last lag frames

PoseDurationLagSmoother (csrc/pose_duration_lag_posterior.hip) gives the fixed-lag posteriors with durations, what
PoseLagSmoother gives under the plain chain: `push` returns, for the frames `lag` frames ago, the row of PoseDurationPosterior's
posterior (and on request its class row and its begin row) on the stream up to now, bit for bit, and for every new frame the
lag-0 row and the evidence in bits.  The forward step is PoseDurationPosterior's with a closed and an open level per frame; every
emitted frame then gets a backward sweep of its own over its at most lag + 1 frames, a workgroup each, so a split into pushes
changes no bit.  lagged_begin is the probability that a hold begins at a frame given only `lag` frames of look-ahead: what a
loop needs to announce "next pose" once.  Levels are absolute float64, so a stream may run for 2^20 frames (9.7 hours at
30 fps); `reset()` starts a new one.

    livepost = PoseDurationLagSmoother(state_class, trans, dur, device, lag=16, streams=16)
    for rows in live:
        first, lag_path = livedur.push(rows)
        _, lagged, lagged_begin = livepost.push(rows, begin=True)       # nothing read back
        confidence = livepost.confidence(lagged, lag_path)              # "Pose: X (0.93)", lag frames behind the camera
    first, lagged = livepost.push(rows[:, :0], flush=True)              # the last lag frames

PoseDurationLearner (csrc/pose_duration_prior.hip) fits the tables that these four take, trans, init and dur jointly, to whole
videos whose frames carry class probabilities only: Baum-Welch for the explicit-duration chain, on the device.  PoseOrderLearner's
tables do not fit here: it learns the plain chain, where trans[j][j] means "stay one more frame", while here that entry joins two
segments of one step.  The E-step is PoseDurationPosterior's kernel in a second mode (the same sweeps: its evidence and its
expected duration counts are that kernel's bits), which in its backward step also sums xi_f[i][j], the probability that a hold of
i ends and a hold of j begins at frame f, into float64 registers, one lane per entry, in a fixed order; a second small launch adds
the videos' partials in order.  The M-step turns the three counts into int32 scores on the device (trans and init by
PoseOrderLearner's rule, dur by `expected_duration_prior`'s, dur_open as the suffix maximum) and nothing is read back:

    learner = PoseDurationLearner(state_class, trans, dur, device, dur_pseudo_count=0.01)    # the shapes to start from
    for it in range(iterations):
        learner.zero()
        for probs, lengths in videos:             # f32 [B, n, C] and int32 [B] or None: ragged batches of whole videos
            learner.accumulate(probs, lengths)    # E-step, nothing read back
        learner.update()                          # M-step; learner.trans / .init / .dur / .dur_open are the new tables
    bits, frames = learner.totals()               # the one host sync: evidence of the last E-step, frames seen
    for user in (durdec, durpost, livedur, livepost):
        user.load_tables(learner.trans, learner.init, learner.dur, learner.dur_open)    # device to device, no host sync

`fit(videos, iterations)` is that loop, `accumulate_paths(path, start)` adds hard counts (PoseDurationDecoder.decode's path and
start for Viterbi training: its segments, a join of one step with itself counting on the diagonal; or labelled steps without
start: their runs), `tables()` returns numpy tables for saving.  An entry of trans or dur that starts at -65536 stays there.
Start from a normalised dur (every row's 2^(dur / 256) summing to one, e.g. uniform at rint(-256 log2 D)): the evidence then
compares across iterations from the first on.  If self-joins are not wanted, start with trans[j][j] = -65536: with an allowed
diagonal a hold decomposes into one-frame segments joined by trans[j][j], which is the plain chain again, and the fitted dur says
nothing.  On seeded tracks with holds of 9 frames (tests/test_pose_duration_prior_cpu.py) four iterations from a uniform dur
raise the evidence at every step and move every step's most likely length to 9.

Not built for the chain with durations: D > 128, true minus infinity (a forbidden length is -65536), videos split across calls
in the learner, expected duration counts from a live stream, re-referenced levels for streams beyond 2^20 frames.

Not built: ragged batches (per-sequence lengths) and videos split across calls in PoseOrderLearner, learning emissions (they are the
network's), tying rows, true minus-infinity (forbidden) transitions, S > 64, bf16 probabilities, a second level of the
posterior's scan; for the fixed-lag pair: sliding-window products that share work between neighbouring windows (f32 (L, +) is
not associative: the split contract would break), a tiled forward pass, streams that advance by different counts.  There is no
torch fallback: CPU tensors and other dtypes raise QtError.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._abi import PoseDurationDesc, PoseDurationLagDesc, PoseLagDesc, PoseOrderDesc, bind  # noqa: F401  (<module>.bind is _abi.bind)
from ._lib import QtError

TILE = 64                   # QT_POSE_ORDER_TILE
GROUP = 32                  # PO_GROUP: tiles per group of the two-level scan
MAX_STATES = 64             # QT_POSE_ORDER_MAX_STATES
MAX_CLASSES = 64            # QT_POSE_ORDER_MAX_CLASSES
MAX_FRAMES = 1 << 20
LAG_MAX = 63                # QT_POSE_LAG_MAX
DUR_MAX = 128               # QT_POSE_DUR_MAX
MAX_STREAM_FRAMES = 1 << 36  # qt_pose_duration_lag_decode: seen + frames (absolute int64 scores)
MAX_SMOOTH_STREAM_FRAMES = 1 << 20  # qt_pose_duration_lag_smooth: seen + frames (absolute float64 levels)
SCORE_FLOOR = -8192         # q of NaN and of everything below 2^-32
TRANS_FLOOR = -65536
# rint(256 log2(1 + (2 i + 1) / 512)), i = 0 .. 255: the table of csrc/pose_chain.h
LOG2_TABLE = (
      1,   2,   4,   5,   6,   8,   9,  11,  12,  13,  15,  16,  18,  19,  20,  22,
     23,  24,  26,  27,  28,  30,  31,  32,  34,  35,  36,  38,  39,  40,  42,  43,
     44,  45,  47,  48,  49,  50,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,
     64,  65,  66,  68,  69,  70,  71,  72,  74,  75,  76,  77,  78,  80,  81,  82,
     83,  84,  85,  86,  88,  89,  90,  91,  92,  93,  94,  95,  97,  98,  99, 100,
    101, 102, 103, 104, 105, 106, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 131, 132, 133, 134,
    135, 136, 137, 138, 139, 140, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162, 163, 163, 164,
    165, 166, 167, 168, 169, 170, 171, 172, 173, 173, 174, 175, 176, 177, 178, 179,
    180, 181, 182, 182, 183, 184, 185, 186, 187, 188, 189, 189, 190, 191, 192, 193,
    194, 195, 195, 196, 197, 198, 199, 200, 200, 201, 202, 203, 204, 205, 205, 206,
    207, 208, 209, 210, 210, 211, 212, 213, 214, 214, 215, 216, 217, 218, 218, 219,
    220, 221, 222, 222, 223, 224, 225, 226, 226, 227, 228, 229, 229, 230, 231, 232,
    233, 233, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 242, 242, 243, 244,
    245, 245, 246, 247, 248, 248, 249, 250, 251, 251, 252, 253, 253, 254, 255, 256)


def scan_trip_tiles(num_states):
    """products the tiled route's scan stages at a time (16 KB of LDS, at most 16): a call of more than
    (scan_trip_tiles + 1) * TILE frames makes it stage more than once"""
    return max(1, min(16, 4096 // (num_states * num_states)))


def posterior_scan_trip_tiles(num_states):
    """products the posterior's scan (csrc/pose_posterior.hip) stages at a time, the decoder's figure: its forward sweep goes
    through tiles - 1 products and so does its backward sweep, so a call of more than (posterior_scan_trip_tiles + 1) * TILE
    frames makes both stage more than once"""
    return scan_trip_tiles(num_states)


def prob_score(p):
    """The emission rule q on the host: f32 values (any shape) -> int64 scores, log2 p in units of 1/256 bit from the bit
    pattern; NaN and everything below 2^-32 give -8192, 1 and above 0.  For a `stay` or `advance` taken from a probability."""
    a = np.asarray(p, dtype=np.float32)
    b = np.ascontiguousarray(a).view(np.uint32).astype(np.int64)
    table = np.array(LOG2_TABLE, np.int64)
    out = 256 * ((b >> 23) - 127) + table[(b >> 15) & 255]
    out = np.where(b >= (127 << 23), 0, out)
    out = np.where((b >> 31 != 0) | (b > 0x7F800000) | (b < ((127 - 32) << 23)), SCORE_FLOOR, out)
    out = out.astype(np.int64).reshape(a.shape)
    return int(out) if out.ndim == 0 else out


def _int_in(who, name, v, lo, hi=None, numpy=True, what=None):
    """v as an int where it is an integer (no bool; numpy's too where `numpy`) in lo .. hi (hi None: no upper bound); `what`
    words the range where "an integer in lo .. hi" does not"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer) if numpy else int) or int(v) < lo or \
            (hi is not None and int(v) > hi):
        what = what or (f"an integer >= {lo}" if hi is None else f"an integer in {lo} .. {hi}")
        raise ValueError(f"{who}: {name} must be {what} (got {v!r})")
    return int(v)


_DTYPE_NAMES = {torch.float32: "f32", torch.int32: "int32", torch.int64: "int64"}
_NO_FALLBACK = "; there is no CPU or torch fallback"
_NUMBERS = (int, float)


def _check_device_tensor(what, name, t, device, dtype, shape=None, tail=""):
    """t must be a tensor of `dtype` on `device` (and of `shape` where one is given)"""
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or \
            (shape is not None and tuple(t.shape) != tuple(shape)):
        dims = "" if shape is None else f" {list(shape)}"
        raise QtError(f"{what}: {name} must be an {_DTYPE_NAMES[dtype]} tensor{dims} on {device}{tail}")


def _check_pseudo(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) < float("inf"):
        raise ValueError(f"{who}: {name} must be a finite number >= 0 (got {v!r})")
    return float(v)


def _score(name, v, optional=False):
    if v is None and optional:
        return None
    return _int_in("cyclic_prior", name, v, TRANS_FLOOR, 0)


def cyclic_prior(step_classes, stay, advance, skip=None, other=TRANS_FLOOR, wrap=True):
    """(state_class int32 [S], trans int32 [S, S]) of a left-to-right cycle over the steps, on the host, integers in and out:
    trans[s][s] = stay, trans[s][s+1 mod S] = advance, trans[s][s+2 mod S] = skip where given, `other` everywhere else.  Without
    `wrap` the last steps do not lead back to the first.  Where S is so small that two of them name one entry, stay wins over
    advance and advance over skip."""
    classes = [int(c) for c in step_classes]
    S = len(classes)
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"cyclic_prior: {S} steps; 1 .. {MAX_STATES} are handled")
    if any(c < 0 for c in classes):
        raise ValueError("cyclic_prior: a step's class is negative")
    stay, advance, other = _score("stay", stay), _score("advance", advance), _score("other", other)
    skip = _score("skip", skip, optional=True)
    trans = np.full((S, S), other, np.int32)
    for s in range(S):
        for step, value in ((2, skip), (1, advance), (0, stay)):
            if value is None or (s + step >= S and not wrap):
                continue
            trans[s, (s + step) % S] = value
    return np.array(classes, np.int32), trans


def _dur_shape(who, S, D):
    return _int_in(who, "S", S, 1, MAX_STATES), _int_in(who, "D", D, 1, DUR_MAX)


def duration_prior(counts, pseudo_count=1.0):
    """dur int32 [S, D] from run-length counts [S, D] (PoseDurationDecoder.count_durations, integers), on the host:
    prob_score of (counts + pseudo_count) / the row's sum of them, as f32.  A row without any count and without a pseudo-count
    scores the floor -8192 everywhere."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.dtype.kind not in "iu" or not 1 <= c.shape[0] <= MAX_STATES or not 1 <= c.shape[1] <= DUR_MAX or \
            (c < 0).any():
        raise ValueError(f"duration_prior: counts must be [S <= {MAX_STATES}, D <= {DUR_MAX}] integers >= 0 (got shape "
                         f"{c.shape}, {c.dtype})")
    return _counts_to_scores("duration_prior", c.astype(np.float64), pseudo_count)


def _counts_to_scores(who, counts, pseudo_count):
    """the rule both duration priors share: checked float64 counts [S, D] -> int32 scores"""
    r = counts + _check_pseudo(who, "pseudo_count", pseudo_count)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (r / r.sum(axis=1, keepdims=True)).astype(np.float32)
    return prob_score(p).astype(np.int32)


def expected_duration_prior(counts, pseudo_count=1.0):
    """dur int32 [S, D] from expected duration counts [S, D] (PoseDurationPosterior.expected_durations, float64), on the host:
    `duration_prior`'s rule for counts that are not integers.  Refused: anything but a real floating or integer array
    [S <= 64, D <= 128], a negative, NaN or infinite count, a pseudo_count that is not a finite number >= 0."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.dtype.kind not in "fiu" or not 1 <= c.shape[0] <= MAX_STATES or not 1 <= c.shape[1] <= DUR_MAX:
        raise ValueError(f"expected_duration_prior: counts must be [S <= {MAX_STATES}, D <= {DUR_MAX}] real numbers (got shape "
                         f"{c.shape}, {c.dtype})")
    c = c.astype(np.float64)
    if not np.isfinite(c).all() or (c < 0).any():
        raise ValueError("expected_duration_prior: counts must be finite and >= 0")
    return _counts_to_scores("expected_duration_prior", c, pseudo_count)


def hold_prior(S, D, shortest, longest, inside=0, outside=TRANS_FLOOR):
    """dur int32 [S, D] of the simple box: `inside` for shortest <= d <= longest, `outside` for every other length"""
    S, D = _dur_shape("hold_prior", S, D)
    shortest, longest = _int_in("hold_prior", "shortest", shortest, 1), _int_in("hold_prior", "longest", longest, 1)
    if shortest > longest:
        raise ValueError(f"hold_prior: shortest = {shortest} > longest = {longest}")
    inside, outside = _score("inside", inside), _score("outside", outside)
    d = np.arange(1, D + 1)
    row = np.where((d >= shortest) & (d <= longest), inside, outside).astype(np.int32)
    return np.tile(row, (S, 1))


def geometric_durations(stay, S, D):
    """dur int32 [S, D] with dur[j][d - 1] = (d - 1) * stay: with trans[j][j] = stay the plain chain's implied durations (a hold
    split into segments costs what it costs inside one)"""
    S, D = _dur_shape("geometric_durations", S, D)
    stay = _score("stay", stay)
    if (D - 1) * stay < TRANS_FLOOR:
        raise ValueError(f"geometric_durations: (D - 1) * stay = {(D - 1) * stay} is below {TRANS_FLOOR}")
    return np.tile((np.arange(D, dtype=np.int64) * stay).astype(np.int32), (S, 1))


class _PoseTables:
    """what every owner of the chain's tables shares: the checked tables in device memory (state_class, trans, init or None),
    a workspace that grows on demand, and the checks of a `probs` argument"""
    _empty_with_flush = False                    # the fixed-lag pair: a push may bring no frames

    def __init__(self, state_class, trans, device, streams=1, init=None, class_names=None, **own):
        who = type(self).__name__
        sc, tr, init, self.class_names = _check_tables(who, state_class, trans, init, streams, class_names)
        self.num_states, self.streams = int(sc.shape[0]), streams
        init = self._check_own(who, init, **own)
        device = torch.device(device)
        if device.type != "cuda":
            raise QtError(f"{who} lives on an AMD GPU (device must be cuda:N); no CPU fallback")
        self.state_class = torch.from_numpy(sc.astype(np.int32)).to(device)
        self.trans = torch.from_numpy(np.ascontiguousarray(tr, np.int32)).to(device)
        self.init = None if init is None else torch.from_numpy(init.astype(np.int32)).to(device)
        self.device = self.trans.device
        self._workspace = None

    def _check_own(self, who, init):
        """a subclass's own constructor arguments (`own`), checked before anything goes to the device; returns init (numpy or
        None)"""
        return init

    def _room(self, query, desc):
        """(pointer, bytes) of a workspace of at least what `query` asks for `desc`; (None, 0) where it asks for none"""
        need = int(query(ctypes.byref(desc)))
        if need and (self._workspace is None or self._workspace.numel() < need):
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return (_lib.ptr(self._workspace), self._workspace.numel()) if need else (None, 0)

    def _call(self, name, desc, *args, workspace=None):
        """the entry point `name` on this object's device and torch's current stream: `desc` (a descriptor, passed by
        reference, or the leading number of an entry point without one), then `args` (tensors as their addresses, None and
        numbers as they are), then, where `workspace` names the size query, the workspace and its size, then the stream"""
        L = _lib.lib()
        room = self._room(getattr(L, workspace), desc) if workspace else ()
        args = [a if a is None or a.__class__ in _NUMBERS else a.data_ptr() for a in args]   # (this runs once per live frame)
        with torch.cuda.device(self.device):
            _lib.check(getattr(L, name)(desc if desc.__class__ is int else ctypes.byref(desc), *args, *room, _lib.stream_ptr()),
                       name)

    def _check_probs(self, what, probs, allow_empty=False):
        """probs f32 [streams, frames, C], or [frames, C] when there is one stream, on this object's device -> (probs as
        [streams, frames, C] with rows the kernels can walk, flat, frames, C)"""
        _check_probs_tensor(what, probs, self.device)
        B = self.streams
        flat = probs.dim() == 2
        if flat and B == 1:
            probs = probs.unsqueeze(0)
        if probs.dim() != 3 or probs.shape[0] != B or not 1 <= probs.shape[2] <= MAX_CLASSES or \
                (probs.shape[1] < 1 and not allow_empty):
            want = f"C <= {MAX_CLASSES} and frames >= 1, or 0 with flush" if self._empty_with_flush else \
                f"frames >= 1 and C <= {MAX_CLASSES}"
            raise QtError(f"{what}: probs must be [{B}, frames, C]{' or [frames, C]' if B == 1 else ''} with {want} "
                          f"(got {list(probs.shape)})")
        return (_check_probs_rows(what, probs), flat) + tuple(probs.shape[1:])


class _PoseStreams(_PoseTables):
    """the owners of streams (each has a `reset`): they take a learner's tables"""

    def load_tables(self, trans, init=None):
        """a learner's tables (int32 tensors on this device) copied into this object's own, device to device and without a host
        sync; every stream starts anew.  init None: no init from here on.  (Values are clamped by the kernels as they are read:
        checking them here would need a host sync.)"""
        S = self.num_states
        _load_tables(self, f"{type(self).__name__}.load_tables", (("trans", trans, (S, S)), ("init", init, (S,))))
        return self.reset()


def _replace_optional(current, new):
    """an optional table after a load: None for `new` None, a copy of its own where there was none, else copied in place"""
    if new is None:
        return None
    if current is None:
        return new.detach().clone().contiguous()
    current.copy_(new)
    return current


def _load_tables(self, who, specs):
    """checks `specs`, (name, int32 tensor on this device or None, shape) with trans first (required) and init second, and
    copies those two into the object's own"""
    for name, t, shape in specs:
        if t is not None or name == "trans":
            _check_device_tensor(who, name, t, self.device, torch.int32, shape)
    self.trans.copy_(specs[0][1])
    self.init = _replace_optional(self.init, specs[1][1])


def _cycles(who, self, path, wrap_from, wrap_to, before=None):
    """how often `path` goes from wrap_from to wrap_to between adjacent frames, `before` [streams] standing in front of it"""
    S, B = self.num_states, self.streams
    wrap_from = S - 1 if wrap_from is None else wrap_from
    for name, v in (("wrap_from", wrap_from), ("wrap_to", wrap_to)):
        _int_in(who, name, v, 0, S - 1, numpy=False, what=f"a state 0 .. {S - 1}")
    _check_device_tensor(who, "path", path, self.device, torch.int64)
    if path.dim() == 1 and B == 1:
        path = path.unsqueeze(0)
    if path.dim() != 2 or path.shape[0] != B or path.shape[1] < 1:
        raise QtError(f"{who}: path must be [{B}, frames] (got {list(path.shape)})")
    if before is None:
        return ((path[:, :-1] == wrap_from) & (path[:, 1:] == wrap_to)).sum(dim=1)
    return ((torch.cat([before[:, None], path[:, :-1]], dim=1) == wrap_from) & (path == wrap_to)).sum(dim=1)


def _confidence(who, self, rows, path, rows_name, path_name, pad=False):
    """`rows` f32 [..., S] at the states of `path` int64 [...]; pad: 0 where path is -1"""
    _check_device_tensor(who, rows_name, rows, self.device, torch.float32)
    _check_device_tensor(who, path_name, path, self.device, torch.int64)
    if rows.shape[:-1] != path.shape or rows.shape[-1] != self.num_states:
        raise QtError(f"{who}: {rows_name} {list(rows.shape)} and {path_name} {list(path.shape)} do not belong together "
                      f"({self.num_states} states)")
    if not pad:
        return rows.gather(-1, path.unsqueeze(-1)).squeeze(-1)
    at = rows.gather(-1, path.clamp_min(0).unsqueeze(-1)).squeeze(-1)
    return torch.where(path >= 0, at, torch.zeros_like(at))


def _path_batch(what, path):
    """a checked int64 tensor as [B, frames] with B, frames >= 1, within the frame limit"""
    if path.dim() == 1:
        path = path.unsqueeze(0)
    if path.dim() != 2 or path.shape[0] < 1 or path.shape[1] < 1:
        raise QtError(f"{what}: path must be [B, frames] or [frames] with B, frames >= 1 (got {list(path.shape)})")
    if path.shape[0] * path.shape[1] > MAX_FRAMES:
        raise QtError(f"{what}: {path.shape[0] * path.shape[1]} frames; at most {MAX_FRAMES} are handled in one call")
    return path


def _check_probs_tensor(what, probs, device):
    if not isinstance(probs, torch.Tensor):
        raise QtError(f"{what}: probs must be a tensor")
    if probs.device.type != "cuda" or probs.device != device:
        raise QtError(f"{what}: probs must be on {device} (got {probs.device}); there is no CPU or torch fallback")
    if probs.dtype != torch.float32:
        raise QtError(f"{what}: f32 probabilities only (got {probs.dtype})")


def _check_probs_rows(what, probs):
    """probs [B, frames, C] of a checked shape: the frame limit, then unit stride within a row and one stride between rows"""
    B, T, C = probs.shape
    if B * T > MAX_FRAMES:
        raise QtError(f"{what}: {B * T} frames; at most {MAX_FRAMES} are handled in one call")
    probs = probs.detach()
    if T and (probs.stride(2) != 1 or probs.stride(1) < C or (B > 1 and probs.stride(0) != T * probs.stride(1))):
        probs = probs.contiguous()
    return probs


class PoseOrderDecoder(_PoseStreams):
    """The decoder of `streams` videos (or camera feeds): the tables, the carry int64 [streams, S + 2] = (frames_seen,
    score_offset, delta[S]), each stream's last path state, and a workspace that grows on demand, all in device memory.
    `decode` and `cycles` launch kernels and read nothing back.  See the module text."""

    def __init__(self, state_class, trans, device, streams=1, init=None, class_names=None):
        super().__init__(state_class, trans, device, streams, init, class_names)
        device = self.device
        self._state_class64 = self.state_class.to(torch.int64)
        self.carry = torch.zeros(streams, self.num_states + 2, dtype=torch.int64, device=device)
        self._last = torch.full((streams,), -1, dtype=torch.int64, device=device)    # the last decode's last state; -1: none
        self._before = self._last                                                    # the same of the decode before it

    def reset(self):
        """every stream starts anew (no host sync)"""
        self.carry.zero_()
        self._last = torch.full_like(self._last, -1)
        self._before = self._last
        return self

    def decode(self, probs, filtered=False, emissions=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on the decoder's device: predict's
        probabilities or the timeline's smoothed rows.  Returns (path int64, path_class int64), each [streams, frames] (or
        [frames]): the best state per frame and the class it emits, which is what FrameAnnotator.draw takes as `pred`;
        with filtered=True the causal states int64 as a third, with emissions=True the scores int32 [..., S] as the last."""
        probs, flat, T, C = self._check_probs("PoseOrderDecoder.decode", probs)
        B, S = self.streams, self.num_states
        lead = (T,) if flat else (B, T)
        dev = self.device
        path = torch.empty(lead, dtype=torch.int64, device=dev)
        filt = torch.empty(lead, dtype=torch.int64, device=dev) if filtered else None
        emis = torch.empty(lead + (S,), dtype=torch.int32, device=dev) if emissions else None
        self._call("qt_pose_order_decode", PoseOrderDesc(B, T, C, S), probs, probs.stride(1), self.state_class, self.trans,
                   self.init, self.carry, path, filt, emis, workspace="qt_pose_order_workspace_bytes")
        self._before, self._last = self._last, path.view(B, T)[:, -1].clone()
        out = (path, self._state_class64[path])
        if filtered:
            out += (filt,)
        if emissions:
            out += (emis,)
        return out

    def cycles(self, path, wrap_from=None, wrap_to=0):
        """int64 [streams], on the device and without a host sync: how often `path` (a decode's, [streams, frames] or [frames])
        goes from state wrap_from (default S - 1) to state wrap_to between adjacent frames.  `decode` keeps the last state of
        the call before it, so with the latest decode's path a wrap that falls on the call boundary is counted: call it once
        per decode.  Plain torch."""
        return _cycles("PoseOrderDecoder.cycles", self, path, wrap_from, wrap_to, self._before)


class _PoseDurationTables(_PoseTables):
    """what the owners of a duration table share: the chain's tables, dur and dur_open int32 [S, D] checked and in device
    memory (dur_open: "suffix_max", built here on the host, a table of its own, or None for dur itself), and the check of a
    `lengths` argument"""

    def __init__(self, state_class, trans, dur, device, streams=1, init=None, dur_open="suffix_max", class_names=None):
        super().__init__(state_class, trans, device, streams, init, class_names, dur=dur, dur_open=dur_open)
        dur, dur_open = self._dur_host
        del self._dur_host
        self.max_duration = int(dur.shape[1])
        self.dur = torch.from_numpy(np.ascontiguousarray(dur, np.int32)).to(self.device)
        self.dur_open = None if dur_open is None else torch.from_numpy(np.ascontiguousarray(dur_open, np.int32)).to(self.device)

    def _check_own(self, who, init, dur, dur_open):
        S = self.num_states

        def table(name, t):
            t = np.asarray(t)
            if t.ndim != 2 or t.shape[0] != S or not 1 <= t.shape[1] <= DUR_MAX or t.dtype.kind not in "iu":
                raise ValueError(f"{who}: {name} must be [{S}, D] integers with D in 1 .. {DUR_MAX} (got shape {t.shape}, "
                                 f"{t.dtype})")
            if (t < TRANS_FLOOR).any() or (t > 0).any():
                raise ValueError(f"{who}: {name} holds a score outside {TRANS_FLOOR} .. 0")
            return t

        dur = table("dur", dur)
        if isinstance(dur_open, str):
            if dur_open != "suffix_max":
                raise ValueError(f"{who}: dur_open must be 'suffix_max', a table or None (got {dur_open!r})")
            dur_open = np.maximum.accumulate(dur[:, ::-1], axis=1)[:, ::-1].copy()     # (a copy: no negative stride, at D = 1 either)
        elif dur_open is not None:
            dur_open = table("dur_open", dur_open)
            if dur_open.shape != dur.shape:
                raise ValueError(f"{who}: dur_open is {list(dur_open.shape)}, dur {list(dur.shape)}")
        self._dur_host = (dur, dur_open)
        return init

    def _tables(self):
        """the five tables in the order every stream entry point takes them"""
        return self.state_class, self.trans, self.init, self.dur, self.dur_open

    def _check_lengths(self, what, lengths, B):
        if lengths is None:
            return None
        _check_device_tensor(what, "lengths", lengths, self.device, torch.int32, (B,))
        return lengths.detach().contiguous()

    def load_tables(self, trans, init=None, dur=None, dur_open=None):
        """a PoseDurationLearner's tables (int32 tensors on this device) copied into this object's own, device to device and
        without a host sync.  init None: no init from here on; dur None: the current dur and dur_open stay; dur_open None with a
        dur: dur itself scores the cut segments from here on.  An owner of streams starts them anew.  (Values are clamped by the
        kernels as they are read: checking them here would need a host sync.)"""
        who, S, D = f"{type(self).__name__}.load_tables", self.num_states, self.max_duration
        if dur is None and dur_open is not None:
            raise QtError(f"{who}: a dur_open without a dur")
        _load_tables(self, who, (("trans", trans, (S, S)), ("init", init, (S,)), ("dur", dur, (S, D)), ("dur_open", dur_open, (S, D))))
        if dur is not None:
            self.dur.copy_(dur)
            self.dur_open = _replace_optional(self.dur_open, dur_open)
        reset = getattr(self, "reset", None)
        return reset() if reset else self


class PoseDurationDecoder(_PoseDurationTables):
    """The decoder with hold durations of `streams` whole videos: the chain's tables, dur and dur_open int32 [S, D] and a
    workspace that grows on demand, all in device memory.  dur_open: "suffix_max" (built here, on the host), a table of its
    own, or None for dur itself.  Nothing is carried between calls; `decode`, `cycles` and `count_durations` launch kernels
    and read nothing back.  See the module text."""

    def __init__(self, state_class, trans, dur, device, streams=1, init=None, dur_open="suffix_max", class_names=None):
        super().__init__(state_class, trans, dur, device, streams, init, dur_open, class_names)
        self._state_class64 = self.state_class.to(torch.int64)

    def decode(self, probs, lengths=None, start=False, score=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on the decoder's device, whole videos;
        lengths: int32 [streams] on the device, or None when every video has `frames` frames (a value outside 1 .. frames is
        clamped into it).  Returns (path int64, path_class int64), each [streams, frames] (or [frames]): the step per frame and
        the class it emits, -1 for both beyond a video's end; with start=True the first frame of the segment a frame lies in,
        int64 of the same shape, with score=True the best score int64 [streams] as the last."""
        what = "PoseDurationDecoder.decode"
        probs, flat, T, C = self._check_probs(what, probs)
        B, S = self.streams, self.num_states
        lengths = self._check_lengths(what, lengths, B)
        lead = (T,) if flat else (B, T)
        dev = self.device
        path = torch.empty(lead, dtype=torch.int64, device=dev)
        first = torch.empty(lead, dtype=torch.int64, device=dev) if start else None
        best = torch.empty(B, dtype=torch.int64, device=dev) if score else None
        self._call("qt_pose_duration_decode", PoseDurationDesc(B, T, C, S, self.max_duration), probs, probs.stride(1),
                   *self._tables(), lengths, path, first, best, workspace="qt_pose_duration_workspace_bytes")
        path_class = torch.where(path >= 0, self._state_class64[path.clamp_min(0)], path)
        return (path, path_class) + tuple(t for t in (first, best) if t is not None)

    def cycles(self, path, wrap_from=None, wrap_to=0):
        """int64 [streams], on the device and without a host sync: how often `path` (a decode's, [streams, frames] or [frames])
        goes from state wrap_from (default S - 1) to state wrap_to between adjacent frames; whole videos, so nothing is kept
        between calls.  Plain torch."""
        return _cycles("PoseDurationDecoder.cycles", self, path, wrap_from, wrap_to)

    def count_durations(self, path, lengths=None):
        """int64 [S, D] on the device: the run lengths of state paths, for `duration_prior`.  path: int64 [B, n] or [n] on the
        decoder's device (any B): a decode's path, a PoseOrderDecoder's, or labelled steps; lengths: int32 [B] or None.  A run
        longer than D counts in column D - 1, a video's first and last run are cut by the video and not counted, an entry
        outside 0 .. S - 1 ends a run and counts nowhere.  Counts of further batches add up (integers)."""
        what = "PoseDurationDecoder.count_durations"
        S, D = self.num_states, self.max_duration
        _check_device_tensor(what, "path", path, self.device, torch.int64, tail=_NO_FALLBACK)
        path = _path_batch(what, path)
        B, T = path.shape
        lengths = self._check_lengths(what, lengths, B)
        path = path.detach()
        if path.stride(1) != 1 or (B > 1 and path.stride(0) < T):
            path = path.contiguous()
        out = torch.zeros(S, D, dtype=torch.int64, device=self.device)
        self._call("qt_pose_duration_count", PoseDurationDesc(B, T, 1, S, D), path, path.stride(0) if B > 1 else T, lengths, out)
        return out


def _check_tables(who, state_class, trans, init, streams, class_names):
    """the argument checks that PoseOrderDecoder makes, for a second owner of the same tables"""
    sc = np.asarray(state_class)
    if sc.ndim != 1 or not 1 <= sc.shape[0] <= MAX_STATES or sc.dtype.kind not in "iu":
        raise ValueError(f"{who}: state_class must be 1 .. {MAX_STATES} integers (got shape {sc.shape}, {sc.dtype})")
    S = int(sc.shape[0])
    if (sc < 0).any() or (sc >= MAX_CLASSES).any():
        raise ValueError(f"{who}: state_class holds a class outside 0 .. {MAX_CLASSES - 1}")
    tr = np.asarray(trans)
    if tr.shape != (S, S) or tr.dtype.kind not in "iu":
        raise ValueError(f"{who}: trans must be [{S}, {S}] integers (got shape {tr.shape}, {tr.dtype})")
    if (tr < TRANS_FLOOR).any() or (tr > 0).any():
        raise ValueError(f"{who}: trans holds a score outside {TRANS_FLOOR} .. 0")
    if init is not None:
        init = np.asarray(init)
        if init.shape != (S,) or init.dtype.kind not in "iu" or (init < TRANS_FLOOR).any() or (init > 0).any():
            raise ValueError(f"{who}: init must be [{S}] integers in {TRANS_FLOOR} .. 0")
    _int_in(who, "streams", streams, 1, MAX_FRAMES, numpy=False)
    if class_names is not None:
        class_names = [str(c) for c in class_names]
        if len(class_names) <= int(sc.max()):
            raise ValueError(f"{who}: {len(class_names)} class names, but a state emits class {int(sc.max())}")
    return sc, tr, init, class_names


class PosePosterior(_PoseStreams):
    """The posterior marginals of `streams` videos over the decoder's chain: the tables, the carry float64 [streams, S + 2] =
    (frames_seen, evidence_total in bits, a_last[S]) and a workspace that grows on demand, all in device memory.  `smooth`
    launches kernels and reads nothing back.  See the module text."""

    def __init__(self, state_class, trans, device, streams=1, init=None, class_names=None):
        super().__init__(state_class, trans, device, streams, init, class_names)
        self.carry = torch.zeros(streams, self.num_states + 2, dtype=torch.float64, device=self.device)

    def reset(self):
        """every stream starts anew (no host sync)"""
        self.carry.zero_()
        return self

    def smooth(self, probs, filtered=False, by_class=False, evidence=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on this object's device: predict's
        probabilities or the timeline's smoothed rows.  Returns posterior f32 [streams, frames, S] (or [frames, S]): the
        probability of every step at every frame given all frames up to the end of this call; then, as asked and in this order,
        filtered f32 of the same shape (given the frames up to each one alone), the class posterior f32 [..., C] and the
        call's evidence in bits, float64 [streams].  A tuple when anything beyond the posterior is asked for."""
        probs, flat, T, C = self._check_probs("PosePosterior.smooth", probs)
        B, S = self.streams, self.num_states
        lead = (T,) if flat else (B, T)
        dev = self.device
        post = torch.empty(lead + (S,), dtype=torch.float32, device=dev)
        filt = torch.empty(lead + (S,), dtype=torch.float32, device=dev) if filtered else None
        cls = torch.empty(lead + (C,), dtype=torch.float32, device=dev) if by_class else None
        ev = torch.empty(B, dtype=torch.float64, device=dev) if evidence else None
        self._call("qt_pose_posterior", PoseOrderDesc(B, T, C, S), probs, probs.stride(1), self.state_class, self.trans, self.init,
                   self.carry, post, filt, cls, ev, workspace="qt_pose_posterior_workspace_bytes")
        out = (post,) + tuple(t for t in (filt, cls, ev) if t is not None)
        return out[0] if len(out) == 1 else out

    def confidence(self, posterior, path):
        """f32 [streams, frames] (or [frames]): the posterior at the states of `path` (a decode's, int64), which is what
        FrameAnnotator.draw takes as `confidence` beside the path's class.  Plain torch, nothing read back."""
        return _confidence("PosePosterior.confidence", self, posterior, path, "posterior", "path")


class PoseDurationPosterior(_PoseDurationTables):
    """The posterior marginals of `streams` whole videos over PoseDurationDecoder's chain (csrc/pose_duration_posterior.hip):
    the same checked tables, a float64 [S, D] accumulator of expected duration counts and a workspace that grows on demand, all
    in device memory.  Nothing is carried between calls; no call reads anything back or synchronises.  See the module text."""

    def __init__(self, state_class, trans, dur, device, streams=1, init=None, dur_open="suffix_max", class_names=None):
        super().__init__(state_class, trans, dur, device, streams, init, dur_open, class_names)
        self.counts = torch.zeros(self.num_states, self.max_duration, dtype=torch.float64, device=self.device)

    def zero(self):
        """clears the accumulator of `expected_durations` (no host sync)"""
        self.counts.zero_()
        return self

    def _run(self, what, probs, lengths, post, cls, begin, ev, counts):
        B, T, C = probs.shape
        self._call("qt_pose_duration_posterior", PoseDurationDesc(B, T, C, self.num_states, self.max_duration), probs,
                   probs.stride(1), *self._tables(), lengths, post, cls, begin, ev, counts,
                   workspace="qt_pose_duration_posterior_workspace_bytes")

    def smooth(self, probs, lengths=None, by_class=False, begin=False, evidence=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on this object's device, whole videos;
        lengths: int32 [streams] on the device, or None (a value outside 1 .. frames is clamped into it).  Returns posterior f32
        [streams, frames, S] (or [frames, S]): the probability of every step at every frame given the whole video; then, as
        asked and in this order, the class posterior f32 [..., C], begin f32 [..., S] (the probability that a hold of step j
        begins at frame f) and the evidence in bits, float64 [streams].  Rows beyond a video's end are zeros.  A tuple when
        anything beyond the posterior is asked for."""
        what = "PoseDurationPosterior.smooth"
        probs, flat, T, C = self._check_probs(what, probs)
        B, S = self.streams, self.num_states
        lengths = self._check_lengths(what, lengths, B)
        lead = (T,) if flat else (B, T)
        dev = self.device
        post = torch.empty(lead + (S,), dtype=torch.float32, device=dev)
        cls = torch.empty(lead + (C,), dtype=torch.float32, device=dev) if by_class else None
        beg = torch.empty(lead + (S,), dtype=torch.float32, device=dev) if begin else None
        ev = torch.empty(B, dtype=torch.float64, device=dev) if evidence else None
        self._run(what, probs, lengths, post, cls, beg, ev, None)
        out = (post,) + tuple(t for t in (cls, beg, ev) if t is not None)
        return out[0] if len(out) == 1 else out

    def confidence(self, posterior, path):
        """f32 [streams, frames] (or [frames]): the posterior at the states of `path` (PoseDurationDecoder.decode's, int64),
        0 where path is -1 (beyond a video's end).  Plain torch, nothing read back."""
        return _confidence("PoseDurationPosterior.confidence", self, posterior, path, "posterior", "path", pad=True)

    def holds(self, begin):
        """float64 [streams, S]: the sum of `begin` (a smooth's, [streams, frames, S] or [frames, S]) over the frames, the
        expected number of holds of every step, and so of rounds.  Plain torch, nothing read back."""
        who = "PoseDurationPosterior.holds"
        _check_device_tensor(who, "begin", begin, self.device, torch.float32)
        if begin.dim() == 2 and self.streams == 1:
            begin = begin.unsqueeze(0)
        if begin.dim() != 3 or begin.shape[0] != self.streams or begin.shape[2] != self.num_states:
            raise QtError(f"{who}: begin must be [{self.streams}, frames, {self.num_states}] (got {list(begin.shape)})")
        return begin.sum(dim=1, dtype=torch.float64)

    def expected_durations(self, probs, lengths=None):
        """adds the expected duration counts of these videos (probs and lengths as for `smooth`) into the float64 [S, D]
        accumulator on the device and returns it: the soft counterpart of PoseDurationDecoder.count_durations, for
        `expected_duration_prior`.  Only the segments that the video does not cut count.  `zero()` clears it."""
        what = "PoseDurationPosterior.expected_durations"
        probs, _, _, _ = self._check_probs(what, probs)
        lengths = self._check_lengths(what, lengths, self.streams)
        self._run(what, probs, lengths, None, None, None, None, self.counts)
        return self.counts


def _check_lag(who, lag):
    _int_in(who, "lag", lag, 0, LAG_MAX)


class _LagState:
    """what the fixed-lag objects share beside their tables: the lag, the count of frames seen (on the host: all streams advance
    together) and the two carry buffers that are swapped after every push"""
    _empty_with_flush = True

    def _lag_init(self, lag, carry_query, desc):
        """desc: the descriptor of one frame, which `carry_query` takes"""
        self.lag, self.seen = int(lag), 0
        nbytes = getattr(_lib.lib(), carry_query)(ctypes.byref(desc))
        self._carry = [torch.zeros(nbytes, dtype=torch.uint8, device=self.device) for _ in range(2)]  # [0]: the next call's carry_in

    def reset(self):
        """every stream starts anew (no host sync; the carry is not read at a stream's first frame)"""
        self.seen = 0
        return self

    def _span(self, T, flush):
        """(first, count) of the frames that a push of T frames emits"""
        first = max(0, self.seen - self.lag)
        return first, (self.seen + T if flush else max(0, self.seen + T - self.lag)) - first

    def _carries(self):
        """(carry_in or None at a stream's start, carry_out)"""
        return (self._carry[0] if self.seen else None), self._carry[1]

    def _advance(self, T):
        self.seen += T
        self._carry.reverse()


class _PoseLag(_LagState, _PoseStreams):
    """what PoseLagSmoother and PoseLagDecoder share: the tables, the fixed-lag state and a workspace that grows on demand"""
    _carry_query = None

    def __init__(self, state_class, trans, device, lag, streams=1, init=None, class_names=None):
        super().__init__(state_class, trans, device, streams, init, class_names, lag=lag)
        self._lag_init(lag, self._carry_query, PoseLagDesc(streams, 1, 1, self.num_states, int(lag), 0, 0))

    def _check_own(self, who, init, lag):
        _check_lag(who, lag)
        return init

    def _probs(self, what, probs, flush):
        probs, flat, T, C = self._check_probs(what, probs, allow_empty=flush)
        first, count = self._span(T, flush)
        desc = PoseLagDesc(self.streams, T, C, self.num_states, self.lag, int(bool(flush)), self.seen)
        return probs, flat, T, C, first, count, desc


class PoseLagSmoother(_PoseLag):
    """Fixed-lag posteriors of `streams` live videos over the decoder's chain: `push` takes the new frames and returns the
    posterior of the frames `lag` frames ago given everything up to now.  Nothing is read back.  See the module text."""
    _carry_query = "qt_pose_lag_smooth_carry_bytes"

    def push(self, probs, flush=False, by_class=False, filtered=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on this object's device; frames may be 0
        with flush.  Returns (first_frame, lagged f32 [streams, count, S] (or [count, S])), then as asked the class posterior
        f32 [..., count, C] and the causal rows of the new frames f32 [..., frames, S]: lagged[:, k] belongs to frame
        first_frame + k of the stream, count is frames once the stream is `lag` frames old, 0 before, and with flush also the
        frames still pending."""
        probs, flat, T, C, first, count, desc = self._probs("PoseLagSmoother.push", probs, flush)
        B, S, dev = self.streams, self.num_states, self.device
        lead = (lambda n: (n,)) if flat else (lambda n: (B, n))
        lagged = torch.empty(lead(count) + (S,), dtype=torch.float32, device=dev)
        cls = torch.empty(lead(count) + (C,), dtype=torch.float32, device=dev) if by_class else None
        filt = torch.empty(lead(T) + (S,), dtype=torch.float32, device=dev) if filtered else None
        self._call("qt_pose_lag_smooth", desc, probs if T else None, probs.stride(1) if T else C, self.state_class, self.trans,
                   self.init, *self._carries(), lagged if count else None, cls if count else None, filt if T else None, None,
                   workspace="qt_pose_lag_smooth_workspace_bytes")
        self._advance(T)
        return (first, lagged) + tuple(t for t in (cls, filt) if t is not None)

    def confidence(self, lagged, lag_path):
        """f32 [streams, count] (or [count]): the lagged posterior at the states of `lag_path` (a PoseLagDecoder's push of the
        same frames, int64).  Plain torch, nothing read back."""
        return _confidence("PoseLagSmoother.confidence", self, lagged, lag_path, "lagged", "lag_path")


class PoseLagDecoder(_PoseLag):
    """Fixed-lag paths of `streams` live videos: `push` takes the new frames and returns, for the frames `lag` frames ago, the
    state on the best path that ends at the newest frame.  The joined lag_path is what PoseOrderDecoder.cycles counts rounds
    on.  Nothing is read back.  See the module text."""
    _carry_query = "qt_pose_lag_decode_carry_bytes"

    def push(self, probs, flush=False, filtered=False):
        """probs as PoseLagSmoother.push.  Returns (first_frame, lag_path int64 [streams, count] (or [count])), then with
        filtered=True the causal states of the new frames int64 [..., frames]."""
        probs, flat, T, C, first, count, desc = self._probs("PoseLagDecoder.push", probs, flush)
        B, dev = self.streams, self.device
        lead = (lambda n: (n,)) if flat else (lambda n: (B, n))
        path = torch.empty(lead(count), dtype=torch.int64, device=dev)
        filt = torch.empty(lead(T), dtype=torch.int64, device=dev) if filtered else None
        self._call("qt_pose_lag_decode", desc, probs if T else None, probs.stride(1) if T else C, self.state_class, self.trans,
                   self.init, *self._carries(), path if count else None, filt if T else None,
                   workspace="qt_pose_lag_decode_workspace_bytes")
        self._advance(T)
        return (first, path) + ((filt,) if filtered else ())


class PoseDurationLagDecoder(_LagState, _PoseDurationTables):
    """Fixed-lag paths with hold durations of `streams` live videos (csrc/pose_duration_lag.hip): `push` takes the new frames
    and returns, for the frames `lag` frames ago, the step and the start of its hold that PoseDurationDecoder would give on the
    stream up to now.  The tables are PoseDurationDecoder's; the count of frames seen lives on the host (all streams advance
    together), the two carry buffers are swapped after every push.  Nothing is read back.  See the module text."""

    def __init__(self, state_class, trans, dur, device, lag, streams=1, init=None, dur_open="suffix_max", class_names=None):
        _check_lag(type(self).__name__, lag)
        super().__init__(state_class, trans, dur, device, streams, init, dur_open, class_names)
        self._lag_init(lag, "qt_pose_duration_lag_carry_bytes",
                       PoseDurationLagDesc(streams, 1, 1, self.num_states, self.max_duration, int(lag), 0, 0))

    def push(self, probs, flush=False, start=False, filtered=False, score=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on this object's device; frames may be 0
        with flush.  Returns (first_frame, lag_path int64 [streams, count] (or [count])), then as asked and in this order
        lag_start int64 of the same shape (the first frame of the hold a frame lies in, counted from the stream's start), the
        causal end states of the new frames int64 [..., frames] and the best score of the stream cut after each new frame,
        int64 [..., frames]: lag_path[:, k] belongs to frame first_frame + k of the stream, count is frames once the stream is
        `lag` frames old, 0 before, and with flush also the frames still pending."""
        what = "PoseDurationLagDecoder.push"
        probs, flat, T, C = self._check_probs(what, probs, allow_empty=flush)
        B, dev = self.streams, self.device
        if self.seen + T > MAX_STREAM_FRAMES:
            raise QtError(f"{what}: frame {self.seen + T} of a stream; at most {MAX_STREAM_FRAMES} are handled")
        first, count = self._span(T, flush)
        desc = PoseDurationLagDesc(B, T, C, self.num_states, self.max_duration, self.lag, int(bool(flush)), self.seen)
        lead = (lambda n: (n,)) if flat else (lambda n: (B, n))
        path = torch.empty(lead(count), dtype=torch.int64, device=dev)
        begin = torch.empty(lead(count), dtype=torch.int64, device=dev) if start else None
        filt = torch.empty(lead(T), dtype=torch.int64, device=dev) if filtered else None
        best = torch.empty(lead(T), dtype=torch.int64, device=dev) if score else None
        self._call("qt_pose_duration_lag_decode", desc, probs if T else None, probs.stride(1) if T else C, *self._tables(),
                   *self._carries(), path if count else None, begin if count else None, filt if T else None,
                   best if T else None, workspace="qt_pose_duration_lag_workspace_bytes")
        self._advance(T)
        return (first, path) + tuple(t for t in (begin, filt, best) if t is not None)


class PoseDurationLagSmoother(_LagState, _PoseDurationTables):
    """Fixed-lag posteriors with hold durations of `streams` live videos (csrc/pose_duration_lag_posterior.hip): `push` takes
    the new frames and returns, for the frames `lag` frames ago, the rows that PoseDurationPosterior.smooth would give on the
    stream up to now, bit for bit.  The tables are PoseDurationDecoder's; the count of frames seen lives on the host (all
    streams advance together), the two carry buffers are swapped after every push.  Nothing is read back.  See the module
    text."""

    def __init__(self, state_class, trans, dur, device, lag, streams=1, init=None, dur_open="suffix_max", class_names=None):
        _check_lag(type(self).__name__, lag)
        super().__init__(state_class, trans, dur, device, streams, init, dur_open, class_names)
        self._lag_init(lag, "qt_pose_duration_lag_smooth_carry_bytes",
                       PoseDurationLagDesc(streams, 1, 1, self.num_states, self.max_duration, int(lag), 0, 0))

    def push(self, probs, flush=False, by_class=False, begin=False, filtered=False, evidence=False):
        """probs: f32 [streams, frames, C], or [frames, C] when there is one stream, on this object's device; frames may be 0
        with flush.  Returns (first_frame, lagged f32 [streams, count, S] (or [count, S])), then as asked and in this order the
        class posterior f32 [..., count, C], lagged_begin f32 [..., count, S] (the probability that a hold of step j begins at
        that frame, given `lag` frames of look-ahead), the lag-0 rows of the new frames f32 [..., frames, S] and the evidence in
        bits of the stream cut after each new frame, float64 [..., frames]: lagged[:, k] belongs to frame first_frame + k of the
        stream, count is frames once the stream is `lag` frames old, 0 before, and with flush also the frames still pending."""
        what = "PoseDurationLagSmoother.push"
        probs, flat, T, C = self._check_probs(what, probs, allow_empty=flush)
        B, S, dev = self.streams, self.num_states, self.device
        if self.seen + T > MAX_SMOOTH_STREAM_FRAMES:
            raise QtError(f"{what}: frame {self.seen + T} of a stream; at most {MAX_SMOOTH_STREAM_FRAMES} are handled "
                          f"(reset() starts a new stream)")
        first, count = self._span(T, flush)
        desc = PoseDurationLagDesc(B, T, C, S, self.max_duration, self.lag, int(bool(flush)), self.seen)
        lead = (lambda n: (n,)) if flat else (lambda n: (B, n))
        lagged = torch.empty(lead(count) + (S,), dtype=torch.float32, device=dev)
        cls = torch.empty(lead(count) + (C,), dtype=torch.float32, device=dev) if by_class else None
        beg = torch.empty(lead(count) + (S,), dtype=torch.float32, device=dev) if begin else None
        filt = torch.empty(lead(T) + (S,), dtype=torch.float32, device=dev) if filtered else None
        ev = torch.empty(lead(T), dtype=torch.float64, device=dev) if evidence else None
        self._call("qt_pose_duration_lag_smooth", desc, probs if T else None, probs.stride(1) if T else C, *self._tables(),
                   *self._carries(), lagged if count else None, cls if count else None, beg if count else None,
                   filt if T else None, ev if T else None, workspace="qt_pose_duration_lag_smooth_workspace_bytes")
        self._advance(T)
        return (first, lagged) + tuple(t for t in (cls, beg, filt, ev) if t is not None)

    def confidence(self, lagged, lag_path):
        """f32 [streams, count] (or [count]): the lagged posterior at the states of `lag_path` (a PoseDurationLagDecoder's push
        of the same frames, int64).  Plain torch, nothing read back."""
        return _confidence("PoseDurationLagSmoother.confidence", self, lagged, lag_path, "lagged", "lag_path")

    def holds(self, lagged_begin):
        """float64 [streams, S]: the sum of `lagged_begin` (a push's, [streams, count, S] or [count, S]) over its frames, the
        expected number of holds of every step that begin in them.  Plain torch, nothing read back."""
        who = "PoseDurationLagSmoother.holds"
        _check_device_tensor(who, "lagged_begin", lagged_begin, self.device, torch.float32)
        if lagged_begin.dim() == 2 and self.streams == 1:
            lagged_begin = lagged_begin.unsqueeze(0)
        if lagged_begin.dim() != 3 or lagged_begin.shape[0] != self.streams or lagged_begin.shape[2] != self.num_states:
            raise QtError(f"{who}: lagged_begin must be [{self.streams}, count, {self.num_states}] "
                          f"(got {list(lagged_begin.shape)})")
        return lagged_begin.sum(dim=1, dtype=torch.float64)


class _Learner:
    """what the two learners share: the loop of `fit`, `totals`, the checks of whole videos and of state paths, and the start
    vector that learn_init writes out"""
    def _learned_init(self, init):
        if init is None and self.learn_init:
            init = np.zeros(self.num_states, np.int32)          # the start vector of zeros, written out
        return init

    def _videos(self, what, probs):
        """probs f32 [B, n, C] or [n, C] on this device -> [B, n, C] with rows the kernels can walk"""
        _check_probs_tensor(what, probs, self.device)
        if probs.dim() == 2:
            probs = probs.unsqueeze(0)
        if probs.dim() != 3 or probs.shape[0] < 1 or probs.shape[1] < 1 or not 1 <= probs.shape[2] <= MAX_CLASSES:
            raise QtError(f"{what}: probs must be [B, frames, C] or [frames, C] with B, frames >= 1 and C <= {MAX_CLASSES} "
                          f"(got {list(probs.shape)})")
        return _check_probs_rows(what, probs)

    def _fit_args(self, video):
        """an item of `fit`'s videos as the arguments of `accumulate`"""
        return (video,)

    def fit(self, videos, iterations):
        """`iterations` rounds of zero / accumulate every video / update, with no host synchronisation; `videos` is a sequence
        (it is walked once per round) of what `accumulate` takes: probs f32 [B, n, C] or [n, C] and, for the learner with hold
        durations, also pairs (probs, lengths).  The accumulators are left as the last E-step made them: `totals` gives the
        evidence under the tables BEFORE the last update."""
        _int_in(f"{type(self).__name__}.fit", "iterations", iterations, 0, numpy=False)
        videos = [self._fit_args(v) for v in videos]
        for _ in range(iterations):
            self.zero()
            for args in videos:
                self.accumulate(*args)
            self.update()
        return self

    def totals(self):
        """(evidence in bits, frames) of what has been accumulated since `zero`: the one host sync"""
        bits, frames = self._totals.cpu().tolist()
        return bits, int(frames)


class PoseOrderLearner(_Learner, _PoseTables):
    """Baum-Welch for the decoder's chain, on the device: the transition table (and, with learn_init, the start scores) fitted
    to videos whose frames carry class probabilities only.  `accumulate` is the E-step of one video or of a batch of videos of
    equal length (qt_pose_prior_expect adds the expected transition counts onto float64 accumulators in a fixed order),
    `accumulate_paths` adds the hard counts of given state paths (a decoder's path for Viterbi training, or labelled steps),
    `update` is the M-step.  An entry of the initial table at -65536 is forbidden and stays there; `pseudo_count` is added to
    every allowed count.  Nothing is read back but by `totals` and `tables`.  See the module text."""

    def __init__(self, state_class, trans, device, init=None, pseudo_count=0.0, learn_init=False, class_names=None):
        self.learn_init = bool(learn_init)
        super().__init__(state_class, trans, device, 1, init, class_names, pseudo_count=pseudo_count)
        S, device = self.num_states, self.device
        self.pseudo_count = float(pseudo_count)
        self.allowed = (self.trans > TRANS_FLOOR).to(torch.int32)
        self.counts = torch.zeros(S, S, dtype=torch.float64, device=device)
        self.start_counts = torch.zeros(S, dtype=torch.float64, device=device)
        self._totals = torch.zeros(2, dtype=torch.float64, device=device)

    def _check_own(self, who, init, pseudo_count):
        _check_pseudo(who, "pseudo_count", pseudo_count)
        return self._learned_init(init)

    def zero(self):
        """the accumulators to zero, before an E-step (no host sync)"""
        self.counts.zero_(), self.start_counts.zero_(), self._totals.zero_()
        return self

    def accumulate(self, probs):
        """E-step of whole videos: probs f32 [B, n, C], or [n, C] for one, on the learner's device (predict's rows or the
        timeline's smoothed rows).  Adds onto counts, start_counts and the totals; nothing is read back."""
        probs = self._videos("PoseOrderLearner.accumulate", probs)
        B, T, C = probs.shape
        self._call("qt_pose_prior_expect", PoseOrderDesc(B, T, C, self.num_states), probs, probs.stride(1), self.state_class,
                   self.trans, self.init, self.counts, self.start_counts, self._totals, workspace="qt_pose_prior_workspace_bytes")
        return self

    def accumulate_paths(self, path):
        """hard counts: path int64 [B, n] or [n] on the learner's device, whole videos; a state outside 0 .. S - 1 (a label
        that is missing) takes its transitions out.  The frames are counted, the evidence is not touched."""
        what = "PoseOrderLearner.accumulate_paths"
        _check_device_tensor(what, "path", path, self.device, torch.int64, tail=_NO_FALLBACK)
        path = _path_batch(what, path).detach().contiguous()
        B, T = path.shape
        self._call("qt_pose_prior_count_paths", PoseOrderDesc(B, T, 1, self.num_states), path, self.counts, self.start_counts,
                   self._totals, workspace="qt_pose_prior_workspace_bytes")
        return self

    def update(self):
        """M-step on the device, in place: self.trans (and with learn_init self.init) are the new int32 tables"""
        init = self.init if self.learn_init else None
        self._call("qt_pose_prior_update", self.num_states, self.counts, self.start_counts, self.allowed, self.pseudo_count,
                   self.trans, init, self.trans, init)
        return self

    def tables(self):
        """numpy (state_class int32 [S], trans int32 [S, S], init int32 [S] or None), for saving (a host sync)"""
        return (self.state_class.cpu().numpy(), self.trans.cpu().numpy(), None if self.init is None else self.init.cpu().numpy())


class PoseDurationLearner(_Learner, _PoseDurationTables):
    """Baum-Welch for the chain with hold durations, on the device (csrc/pose_duration_prior.hip): trans, dur and, with
    learn_init, the start scores fitted jointly to whole videos whose frames carry class probabilities only.  `accumulate` is the
    E-step of one video or of a ragged batch (qt_pose_duration_prior_expect adds the expected transition, start and duration
    counts onto float64 accumulators in a fixed order), `accumulate_paths` adds the hard counts of given segmentations, `update`
    is the M-step.  Entries of the initial trans and dur at -65536 are forbidden and stay there; `pseudo_count` is added to
    every allowed transition count, `dur_pseudo_count` to every allowed duration count.  dur_open "suffix_max": the M-step
    rewrites dur_open on the device; a table of its own or None is left as given.  Nothing is read back but by `totals` and
    `tables`.  See the module text."""

    def __init__(self, state_class, trans, dur, device, init=None, dur_open="suffix_max", pseudo_count=0.0, dur_pseudo_count=1.0,
                 learn_init=False, class_names=None):
        who = type(self).__name__
        self.learn_init = bool(learn_init)
        self.pseudo_count = _check_pseudo(who, "pseudo_count", pseudo_count)
        self.dur_pseudo_count = _check_pseudo(who, "dur_pseudo_count", dur_pseudo_count)
        self._learn_open = isinstance(dur_open, str)
        super().__init__(state_class, trans, dur, device, 1, init, dur_open, class_names)
        S, D, device = self.num_states, self.max_duration, self.device
        self.allowed = (self.trans > TRANS_FLOOR).to(torch.int32)
        self.dur_allowed = (self.dur > TRANS_FLOOR).to(torch.int32)
        self.counts = torch.zeros(S, S, dtype=torch.float64, device=device)
        self.start_counts = torch.zeros(S, dtype=torch.float64, device=device)
        self.dur_counts = torch.zeros(S, D, dtype=torch.float64, device=device)
        self._totals = torch.zeros(2, dtype=torch.float64, device=device)

    def _check_own(self, who, init, dur, dur_open):
        return self._learned_init(super()._check_own(who, init, dur, dur_open))

    def zero(self):
        """the accumulators to zero, before an E-step (no host sync)"""
        self.counts.zero_(), self.start_counts.zero_(), self.dur_counts.zero_(), self._totals.zero_()
        return self

    def accumulate(self, probs, lengths=None):
        """E-step of whole videos: probs f32 [B, n, C], or [n, C] for one, on the learner's device (predict's rows or the
        timeline's smoothed rows); lengths int32 [B] on the device, or None when every video has n frames (a value outside
        1 .. n is clamped into it).  Adds onto counts, start_counts, dur_counts and the totals; nothing is read back."""
        what = "PoseDurationLearner.accumulate"
        probs = self._videos(what, probs)
        B, T, C = probs.shape
        lengths = self._check_lengths(what, lengths, B)
        self._call("qt_pose_duration_prior_expect", PoseDurationDesc(B, T, C, self.num_states, self.max_duration), probs,
                   probs.stride(1), *self._tables(), lengths, self.counts, self.start_counts, self.dur_counts, self._totals,
                   workspace="qt_pose_duration_prior_workspace_bytes")
        return self

    def accumulate_paths(self, path, start=None, lengths=None):
        """hard counts: path int64 [B, n] or [n] on the learner's device, whole videos, and start int64 of the same shape or
        None, lengths int32 [B] or None.  With start (PoseDurationDecoder.decode's) the segments are the decoder's, and two
        segments of one step count on the diagonal of trans; without it they are the runs of path (labelled steps).  A step
        outside 0 .. S - 1 (a label that is missing) counts nowhere.  The frames are counted, the evidence is not touched."""
        what = "PoseDurationLearner.accumulate_paths"
        _check_device_tensor(what, "path", path, self.device, torch.int64, tail=_NO_FALLBACK)
        if start is not None:
            _check_device_tensor(what, "start", start, self.device, torch.int64, tail=_NO_FALLBACK)
            if start.shape != path.shape:
                raise QtError(f"{what}: start {list(start.shape)} and path {list(path.shape)} do not belong together")
        path = _path_batch(what, path)
        B, T = path.shape
        lengths = self._check_lengths(what, lengths, B)
        path = path.detach().contiguous()
        start = None if start is None else start.detach().reshape(B, T).contiguous()
        self._call("qt_pose_duration_prior_count_paths", PoseDurationDesc(B, T, 1, self.num_states, self.max_duration), path,
                   start, T, lengths, self.counts, self.start_counts, self.dur_counts, self._totals,
                   workspace="qt_pose_duration_prior_workspace_bytes")
        return self

    def update(self):
        """M-step on the device, in place: self.trans, self.dur (with learn_init self.init, with dur_open "suffix_max"
        self.dur_open) are the new int32 tables"""
        init = self.init if self.learn_init else None
        dur_open = self.dur_open if self._learn_open else None
        self._call("qt_pose_duration_prior_update", self.num_states, self.max_duration, self.counts, self.start_counts,
                   self.dur_counts, self.allowed, self.dur_allowed, self.pseudo_count, self.dur_pseudo_count, self.trans, init,
                   self.dur, self.trans, init, self.dur, dur_open)
        return self

    def _fit_args(self, video):
        probs, lengths = video if isinstance(video, (tuple, list)) else (video, None)
        return probs, lengths

    def tables(self):
        """numpy (state_class int32 [S], trans int32 [S, S], init int32 [S] or None, dur int32 [S, D], dur_open int32 [S, D] or
        None), for saving (a host sync)"""
        host = lambda t: None if t is None else t.cpu().numpy()
        return (host(self.state_class), host(self.trans), host(self.init), host(self.dur), host(self.dur_open))
