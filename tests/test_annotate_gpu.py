"""Annotated frames on the GPU (csrc/annotate.hip, <pkg>/annotate.py): qt_annotate_u8 through the C ABI against the integer
rule of tests/_annotate_ref.py, every output byte equal, every buffer between the guard bands of tests/_guard.py; then
FrameAnnotator.draw without a host read, fed by `predict`."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _annotate_ref as R
from _guard import Guard
from _util import pkg

pytestmark = pytest.mark.gpu
SHAPES = ((1, 37, 53), (2, 64, 80), (3, 240, 320))      # 159-byte rows: every row unaligned; one tile; 19 tiles per frame
MODES = ("skeleton", "caption", "both")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _style(H, W):
    # the caption starts inside the frame and runs off its right and bottom edges
    return R.Style(origin=(W - 30, H - 6))


@functools.lru_cache(maxsize=None)
def _case(shape, mode, fill="random"):
    """the operands of one call and what the rule makes of them: computed once, shared, never written"""
    B, H, W = shape
    atlas, widths = R.make_atlas()
    C = atlas.shape[0] - 14
    frames = R.make_frames(B, H, W, seed=H + W) if fill == "random" else np.full((B, H, W, 3), fill, np.uint8)
    case = dict(frames=frames, style=_style(H, W))
    if mode in ("skeleton", "both"):
        lm = R.make_landmarks(B, seed=W)
        lm[0], edge_seg = R.edge_landmarks(H, W)       # borders, coincident ends, the three directions, 16383 / 16384, NaN, inf
        case.update(landmarks=lm, segments=np.concatenate([edge_seg, R.default_segments()]))
        assert len(case["segments"]) <= R.MAX_SEGMENTS
        if B > 2:
            case["detected"] = np.array([1, 0, 7][:B], np.uint8)
    if mode in ("caption", "both"):
        case.update(pred=np.array([0, C, 3][:B], np.int64), confidence=np.array([0.995, 0.5, np.nan][:B], np.float32),
                    atlas=atlas, widths=widths)
    want = R.annotate(**case)
    assert (want != frames).any()
    for v in list(case.values()) + [want]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case, want


def _desc(M, case, B, H, W):
    s = case["style"]
    three = lambda c: (ctypes.c_ubyte * 3)(*c)
    atlas = case.get("atlas")
    return M.AnnotateDesc(B, H, W, 0 if case.get("segments") is None else len(case["segments"]), s.min_visibility,
                          s.thick_major, s.thick_minor, s.radius_hi, s.radius_lo, three(s.line_hi), three(s.line_lo),
                          three(s.point_hi), three(s.point_lo), 0 if atlas is None else atlas.shape[0] - 14,
                          0 if atlas is None else atlas.shape[1], 0 if atlas is None else atlas.shape[2], s.origin[0],
                          s.origin[1], three(s.caption_colour))


def run(dev, case, out_fill=0xFF, in_place=False, off_out=0, off_src=0, n_segments=None):
    """qt_annotate_u8 through ctypes, every operand between guard bands: out (or the frames drawn on in place) must keep
    its bands, every input its bytes.  Returns out as numpy."""
    M, Lm = pkg("annotate"), pkg("_lib")
    L = Lm.lib()
    G = Guard(dev)
    frames = torch.tensor(case["frames"])            # (a copy: the shared arrays are read-only)
    B, H, W, _ = frames.shape
    if in_place:
        out = src = G.output("frames drawn on in place", frames.shape, torch.uint8, fill=out_fill, offset=off_out, written=False)
        out.copy_(frames)
    else:
        src = G.input("frames", frames, offset=off_src)
        out = G.output("out", frames.shape, torch.uint8, fill=out_fill, offset=off_out, written=False)
    t = {k: G.input(k, None if case.get(k) is None else torch.tensor(case[k]))
         for k in ("landmarks", "detected", "segments", "pred", "confidence", "atlas", "widths")}
    desc = _desc(M, case, B, H, W)
    if n_segments is not None:
        desc.n_segments = n_segments
    Lm.check(L.qt_annotate_u8(ctypes.byref(desc), Lm.ptr(src), Lm.ptr(t["landmarks"]), Lm.ptr(t["detected"]),
                              Lm.ptr(t["segments"]), Lm.ptr(t["pred"]), Lm.ptr(t["confidence"]), Lm.ptr(t["atlas"]),
                              Lm.ptr(t["widths"]), Lm.ptr(out), Lm.stream_ptr()), "qt_annotate_u8")
    G.check()
    return out.cpu().numpy()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at frame / row / column {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])].tolist()}, want {want[tuple(bad[0])].tolist()}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_byte_equals_the_rule(shape, mode):
    dev = _dev()
    case, want = _case(shape, mode)
    got = run(dev, case, out_fill=0xFF)
    _same(got, want, f"{shape} {mode}")
    print(f"{shape} {mode}: {int((want != case['frames']).any(axis=-1).sum())} pixels drawn")
    _same(run(dev, case, out_fill=0x00), got, "a second run, out filled with zeros")        # the same bits, bands intact
    _same(run(dev, case, in_place=True), got, "in place")
    _same(run(dev, case, in_place=True, out_fill=0x00, off_out=3), got, "in place, 3 bytes off")
    for fill in (0x00, 0xFF):                         # a stray 0xFF would hide in 0xFF frames or bands, a stray 0x00 would not
        flat, flat_want = _case(shape, mode, fill)
        for out_fill in (0x00, 0xFF):
            _same(run(dev, flat, out_fill=out_fill), flat_want, f"{shape} {mode} frames of {fill:#x}, out of {out_fill:#x}")
        _same(run(dev, flat, in_place=True), flat_want, f"{shape} {mode} frames of {fill:#x} in place")


@pytest.mark.parametrize("off_out,off_src", [(1, 1), (2, 3), (3, 0), (0, 2)])
def test_at_any_alignment(off_out, off_src):
    """out's address decides where a frame's 16-byte groups start; frames at another address modulo 16 are read bytewise"""
    dev = _dev()
    for shape in SHAPES[:2]:
        case, want = _case(shape, "both")
        _same(run(dev, case, off_out=off_out, off_src=off_src), want, f"{shape} out + {off_out}, frames + {off_src}")
        _same(run(dev, case, out_fill=0x00, off_out=off_out, off_src=off_src), want, f"{shape} likewise, out of zeros")


def test_a_frame_alone_equals_the_frame_in_its_batch():
    dev = _dev()
    for shape in SHAPES[1:]:
        case, want = _case(shape, "both")
        for b in range(shape[0]):
            one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) and k not in ("segments", "atlas", "widths") else v)
                   for k, v in case.items()}
            _same(run(dev, one), want[b:b + 1], f"{shape} frame {b} alone")


def test_caption_cases():
    """every class of caption in one batch: widths of gw, 0 and gw + 1, pred of -1 and C, confidence at 0, 0.005, 0.995, 1 and
    NaN; then the origin off each edge, and a caption without confidence"""
    dev = _dev()
    atlas, widths = R.make_atlas()
    C, gh, gw = atlas.shape[0] - 14, atlas.shape[1], atlas.shape[2]
    assert widths[0] == gw and widths[1] == 0 and widths[2] == gw + 1
    B, H, W = 8, 37, 53
    pred = np.array([0, 1, 2, 3, 4, -1, C, 3], np.int64)
    conf = np.array([0.0, 0.005, 0.995, 1.0, np.nan, 0.5, 0.5, 0.25], np.float32)
    assert [R.confidence_digits(c) for c in conf[:5]] == [(0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), None]
    frames = R.make_frames(B, H, W, seed=5)
    for origin in ((2, 3), (W - 30, H - 6), (-7, -4), (W - 1, H - 1), (W, 0), (0, H), (-200, 3), (3, -gh)):
        for confidence in (conf, None):
            case = dict(frames=frames, pred=pred, confidence=confidence, atlas=atlas, widths=widths, style=R.Style(origin=origin))
            want = R.annotate(**case)
            _same(run(dev, case), want, f"origin {origin}")
            _same(run(dev, case, in_place=True, off_out=1), want, f"origin {origin} in place")
            untouched = [5, 6] + ([1, 2] if confidence is None else [])
            assert all(np.array_equal(want[b], frames[b]) for b in untouched)
    assert not np.array_equal(R.annotate(frames=frames, pred=pred, confidence=conf, atlas=atlas, widths=widths)[1], frames[1])


def test_styles_and_small_frames():
    """the widest strokes the ABI takes, an empty segment list, frames smaller than one 16-pixel group"""
    dev = _dev()
    atlas, widths = R.make_atlas()
    wide = R.Style(thick_major=15, thick_minor=1, radius_hi=15, radius_lo=1, min_visibility=0.5, origin=(1, 1))
    for (B, H, W) in ((2, 37, 53), (1, 3, 5), (2, 1, 16), (1, 1, 1), (1, 130, 33)):
        lm = R.make_landmarks(B, seed=H * W)
        case = dict(frames=R.make_frames(B, H, W, seed=W), landmarks=lm, segments=R.default_segments(), pred=np.arange(B),
                    confidence=np.full(B, 0.75, np.float32), atlas=atlas, widths=widths, style=wide)
        want = R.annotate(**case)
        _same(run(dev, case, off_out=1), want, f"{(B, H, W)} wide strokes")
        _same(run(dev, case, in_place=True), want, f"{(B, H, W)} wide strokes in place")
        # the discs alone: n_segments = 0 (an empty table has no address, so one unused row is handed over)
        discs = dict(case, pred=None, confidence=None, atlas=None, widths=None)
        want = R.annotate(**dict(discs, segments=np.zeros((0, 3), np.uint8)))
        _same(run(dev, dict(discs, segments=np.zeros((1, 3), np.uint8)), n_segments=0), want, f"{(B, H, W)} discs only")


def _annotator(P, style, atlas, widths, **kw):
    return P.FrameAnnotator(atlas=(torch.from_numpy(atlas.copy()), torch.from_numpy(widths.copy())), caption_origin=style.origin, **kw)


def test_draw_reads_nothing_back_and_takes_predict():
    """random logits -> predict -> draw with no host read in between, under set_sync_debug_mode("error")"""
    dev = _dev()
    P = pkg()
    atlas, widths = R.make_atlas()
    C = atlas.shape[0] - 14
    B, H, W = 4, 64, 80
    style = R.Style(origin=(4, 40))
    frames_np, lm_np = R.make_frames(B, H, W, seed=11), R.make_landmarks(B, seed=12)
    det_np = np.array([1, 1, 0, 1], np.uint8)
    frames, lm, det = (torch.from_numpy(a).to(dev) for a in (frames_np, lm_np, det_np))
    logits = torch.randn(B, C, generator=torch.Generator().manual_seed(3)).to(dev)
    annotator = _annotator(P, style, atlas, widths)
    _, confidence, pred = P.predict(logits)      # first launches outside the guarded region (code-object load, table upload)
    annotator.draw(frames, lm, det, pred, confidence)
    work = frames.clone()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, confidence, pred = P.predict(logits)
        out = annotator.draw(frames, lm, det, pred, confidence)
        same = annotator.draw(work, lm, det, pred, confidence, out=work)
        bones = annotator.draw(frames, lm, det.bool())
        text = annotator.draw(frames, pred=pred)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert same is work and out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, 3)
    ref = dict(frames=frames_np, atlas=atlas, widths=widths, style=style)
    bone_args = dict(landmarks=lm_np, detected=det_np, segments=R.default_segments())
    cap_args = dict(pred=pred.cpu().numpy(), confidence=confidence.cpu().numpy())
    assert ((cap_args["pred"] >= 0) & (cap_args["pred"] < C)).all()
    _same(out.cpu().numpy(), R.annotate(**ref, **bone_args, **cap_args), "predict -> draw")
    _same(work.cpu().numpy(), out.cpu().numpy(), "draw in place")
    _same(bones.cpu().numpy(), R.annotate(**ref, **bone_args), "skeleton only")
    _same(text.cpu().numpy(), R.annotate(**ref, pred=cap_args["pred"]), "class caption only")
    assert torch.equal(frames.cpu(), torch.from_numpy(frames_np))
    # clips [B,T,H,W,3] are frames with two leading dimensions; RGB frames take the colours reversed
    clip = annotator.draw(frames.view(2, 2, H, W, 3), lm.view(2, 2, 33, 4), det.view(2, 2), pred.view(2, 2), confidence.view(2, 2))
    assert tuple(clip.shape) == (2, 2, H, W, 3) and torch.equal(clip.view(B, H, W, 3), out)
    rgb = _annotator(P, style, atlas, widths, channel_order="rgb").draw(frames.flip(-1).contiguous(), lm, det, pred, confidence)
    assert torch.equal(rgb.flip(-1), out)


def test_errors_on_the_device():
    dev = _dev()
    P = pkg()
    atlas, widths = R.make_atlas()
    a = _annotator(P, R.Style(), atlas, widths)
    frames = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    lm = torch.zeros(2, 33, 4, device=dev)
    pred = torch.zeros(2, dtype=torch.int64, device=dev)
    for bad in (dict(), dict(landmarks=lm.cpu()), dict(landmarks=lm[:1]), dict(landmarks=lm.double()), dict(pred=pred.int()),
                dict(pred=pred[:1]), dict(confidence=torch.zeros(2, device=dev)), dict(detected=torch.ones(2, dtype=torch.uint8, device=dev)),
                dict(landmarks=lm, detected=torch.ones(3, dtype=torch.uint8, device=dev)), dict(landmarks=lm, out=frames[:1]),
                dict(pred=pred, confidence=torch.zeros(2, dtype=torch.float64, device=dev))):
        with pytest.raises(P.QtError):
            a.draw(frames, **bad)
    with pytest.raises(P.QtError, match="atlas"):
        P.FrameAnnotator().draw(frames, pred=pred)
    with pytest.raises(P.QtError, match="frames"):
        a.draw(frames[..., :2], lm)
