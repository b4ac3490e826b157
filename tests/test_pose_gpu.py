"""The pose vector on the GPU (csrc/pose.hip, <pkg>/pose.py): qt_pose_features against the float64 rule and the derived
bound of tests/_pose_ref.py on the fixture and on seeded random rows, at the sizes where the row-to-lane mapping, the LDS
staging and the heads and tails of the 188-byte rows can go wrong, every imputation mode on both sources, and the models
fed by it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _pose_ref as R
from _util import ROOT, pkg, rel_err

pytestmark = pytest.mark.gpu
POISON = 12345.0
TILE = 32          # rows per workgroup (PF_ROWS of csrc/pose.hip)
MODES = {"raw": R.RAW, "zero": R.ZERO, "class_mean": R.CLASS_MEAN, "standardize": R.STANDARDIZE}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_features.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def random_rows():
    """the seeded random rows and their reference, computed once and shared (never written)"""
    lm = R.make_landmarks(R.ROWS, R.SEED)
    ref, bound, excluded = R.features(lm)
    for a in (lm, ref, bound, excluded):
        a.setflags(write=False)
    return lm, ref, bound, excluded


@functools.lru_cache(maxsize=None)
def mixed_rows():
    """the fixture's rows (NaN features, a row without a pose) followed by 60 random ones"""
    g = fixture()
    lm = np.concatenate([g["landmarks"], R.make_landmarks(60, seed=11)])
    det = np.concatenate([g["detected"], np.ones(60, np.uint8)])
    ref, bound, excluded = R.features(lm, det)
    for a in (lm, det, ref, bound):
        a.setflags(write=False)
    return lm, det, ref, bound


@functools.lru_cache(maxsize=None)
def tables():
    """K = 3 class tables with one std below 1e-6, and labels with two outside [0, 3)"""
    rng = np.random.default_rng(21)
    means = rng.standard_normal((3, 47)).astype(np.float32) * 20
    stds = (0.5 + 1.5 * rng.random((3, 47))).astype(np.float32)
    stds[1, 40] = np.float32(1e-7)
    stds[2, 3] = np.float32(0.0)
    return means, stds


def labels_for(rows, rows_per_label=1):
    n = rows // rows_per_label
    lab = np.random.default_rng(rows).integers(0, 3, n).astype(np.int64)
    if n > 9:
        lab[5], lab[9] = 3, -1
    return lab


def run(dev, rows, mode=R.RAW, lm=None, det=None, raw=None, labels=None, means=None, stds=None, rows_per_label=1, shift=0,
        in_place=False):
    """qt_pose_features through ctypes.  The output starts `shift` floats into its buffer (shift 1, 2, 3: a head of 3, 2, 1
    single floats) between poisoned floats that must stay as they are; the inputs must not be written."""
    M, Lm = pkg("pose"), pkg("_lib")
    L = Lm.lib()
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)      # (a copy: the shared arrays are read-only)
    d_lm, d_det, d_lab, d_mean, d_std = t(lm), t(det), t(labels), t(means), t(stds)
    n = rows * 47
    buf = torch.full((64 + shift + n + 64,), POISON, device=dev)
    out = buf[64 + shift:64 + shift + n]
    if raw is not None:
        if in_place:
            out.copy_(torch.from_numpy(np.array(raw)).reshape(-1))
            d_raw = out
        else:
            d_raw = t(np.asarray(raw).reshape(-1))
    else:
        d_raw = None
    keep = [None if x is None else x.clone() for x in (d_lm, d_det, None if in_place else d_raw, d_lab, d_mean, d_std)]
    desc = M.PoseDesc(rows, mode, rows_per_label, 0 if means is None else int(means.shape[0]))
    Lm.check(L.qt_pose_features(ctypes.byref(desc), Lm.ptr(d_lm), Lm.ptr(d_det), Lm.ptr(d_raw), Lm.ptr(d_lab), Lm.ptr(d_mean),
                                Lm.ptr(d_std), Lm.ptr(out), Lm.stream_ptr()), "qt_pose_features")
    torch.cuda.synchronize()
    assert bool((buf[:64 + shift] == POISON).all()) and bool((buf[64 + shift + n:] == POISON).all()), "written outside the output"
    for now, was in zip((d_lm, d_det, None if in_place else d_raw, d_lab, d_mean, d_std), keep):
        if now is not None:
            assert torch.equal(now.view(torch.uint8), was.view(torch.uint8)), "an input was written"
    return out.cpu().numpy().reshape(rows, 47)


def test_fixture_rows_raw():
    dev = _dev()
    g = fixture()
    ref, bound, excluded = R.features(g["landmarks"], g["detected"])
    got = run(dev, ref.shape[0], lm=g["landmarks"], det=g["detected"])
    assert not excluded.any()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions"
    assert np.array_equal(np.isnan(got), np.isnan(g["features"])), "NaN positions of the reference's own output"
    worst = R.compare(got, ref, bound, "fixture")
    print(f"fixture: largest error / bound {worst:.3f}")


def test_random_rows_raw_within_bound():
    dev = _dev()
    lm, ref, bound, excluded = random_rows()
    assert not excluded.any()
    got = run(dev, R.ROWS, lm=lm)
    worst = R.compare(got, ref, bound, "4096 random rows")
    per_col = np.abs(got - ref).max(axis=0)
    print(f"4096 random rows: largest error / bound {worst:.3f}; largest angle error {per_col[33:41].max():.2e} degrees "
          f"(bound {bound[:, 33:41].max():.2e})")


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("rows", [1, TILE - 1, TILE, TILE + 1, 63, 64, 65, 257])
def test_sizes_and_output_alignments(rows, shift):
    """1 row; one workgroup's rows, one fewer, one more; 63 / 64 / 65; 257 (a last tile of one row); the output at every
    address modulo 16.  The rows are the first of the 4096: within their bound, and the very bits they have in the batch."""
    dev = _dev()
    lm, ref, bound, _ = random_rows()
    got = run(dev, rows, lm=lm[:rows], shift=shift)
    R.compare(got, ref[:rows], bound[:rows], f"{rows} rows, shift {shift}")
    whole = run(dev, 300, lm=lm[:300])
    assert got.tobytes() == whole[:rows].tobytes()
    # the stored-vector source over the same extents
    again = run(dev, rows, mode=R.RAW, raw=whole[:rows], shift=shift)
    assert again.tobytes() == whole[:rows].tobytes()          # mode raw: the identity, NaNs included


def test_a_row_alone_and_the_same_bits_on_every_run():
    dev = _dev()
    lm, det, ref, bound = mixed_rows()
    first = run(dev, lm.shape[0], lm=lm, det=det)
    second = run(dev, lm.shape[0], lm=lm, det=det)
    assert first.tobytes() == second.tobytes()
    for r in (0, 37, 64, 70, lm.shape[0] - 1):
        alone = run(dev, 1, lm=lm[r:r + 1], det=det[r:r + 1])
        assert alone.tobytes() == first[r:r + 1].tobytes(), r


@pytest.mark.parametrize("source", ["landmarks", "stored"])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_mode_on_both_sources(mode, source):
    dev = _dev()
    lm, det, ref, bound = mixed_rows()
    rows = lm.shape[0]
    means, stds = tables()
    labels = labels_for(rows)
    kw = dict(labels=labels, means=means, stds=stds) if mode in ("class_mean", "standardize") else {}
    if source == "landmarks":
        want, wb = R.impute(ref, bound, MODES[mode], labels, means, stds)
        got = run(dev, rows, MODES[mode], lm=lm, det=det, **kw)
    else:
        raw = run(dev, rows, lm=lm, det=det)                   # stored vectors: f32, NaNs included
        assert np.isnan(raw).any()
        want, wb = R.impute(raw, np.zeros_like(raw, dtype=np.float64), MODES[mode], labels, means, stds)
        got = run(dev, rows, MODES[mode], raw=raw, shift=1, **kw)
    worst = R.compare(got, want, wb, f"{mode} from {source}")
    print(f"{mode} from {source}: largest error / bound {worst:.3f}")
    if mode in ("class_mean", "standardize"):
        assert np.isnan(got[5]).all() and np.isnan(got[9]).all()        # labels 3 and -1
        assert not np.isnan(got[[4, 6, 8, 10]]).any()                   # their neighbours are untouched
    if mode == "standardize":
        assert (got[labels == 1, 40] == 0).all() and (got[labels == 2, 3] == 0).all()      # std < 1e-6
    if mode == "zero":
        assert not np.isnan(got).any() and (got[np.isnan(ref)] == 0).all()
    if mode == "raw":
        assert np.array_equal(np.isnan(got), np.isnan(ref))


def test_impute_in_place():
    dev = _dev()
    lm, det, ref, bound = mixed_rows()
    rows = lm.shape[0]
    means, stds = tables()
    labels = labels_for(rows)
    raw = run(dev, rows, lm=lm, det=det)
    apart = run(dev, rows, R.STANDARDIZE, raw=raw, labels=labels, means=means, stds=stds)
    for shift in (0, 3):
        same = run(dev, rows, R.STANDARDIZE, raw=raw, labels=labels, means=means, stds=stds, shift=shift, in_place=True)
        assert same.tobytes() == apart.tobytes()
    # and through the module
    P = pkg()
    pose = P.PoseFeatures("class_mean", torch.from_numpy(means).to(dev))
    t = torch.from_numpy(raw).to(dev)
    ret = pose.impute(t, torch.from_numpy(labels).to(dev), out=t)
    assert ret is t
    want, _ = R.impute(raw, np.zeros(raw.shape), R.CLASS_MEAN, labels, means)
    assert np.array_equal(np.nan_to_num(t.cpu().numpy(), nan=-777.0), np.nan_to_num(want, nan=-777.0).astype(np.float32))


def test_undetected_rows():
    dev = _dev()
    lm = R.make_landmarks(70, seed=4).copy()
    det = np.ones(70, np.uint8)
    det[[0, 31, 32, 69]] = 0
    lm[31] = np.nan                                           # not read where nothing was detected
    ref, bound, _ = R.features(lm, det)
    got = run(dev, 70, lm=lm, det=det)
    R.compare(got, ref, bound, "undetected rows")
    for r in (0, 31, 32, 69):
        assert not got[r, :33].any() and not np.signbit(got[r, :33]).any() and np.isnan(got[r, 33:]).all()
    assert got[[1, 30, 33, 68]].tobytes() == run(dev, 70, lm=lm)[[1, 30, 33, 68]].tobytes()
    zeroed = run(dev, 70, R.ZERO, lm=lm, det=det)
    assert not zeroed[[0, 31, 32, 69]].any()


def test_nan_coordinate_and_nan_visibility():
    dev = _dev()
    lm = R.make_landmarks(40, seed=6).copy()
    lm[[3, 7], 11, 3] = lm[[3, 7], 12, 3] = np.float32(0.9)      # two visible torso landmarks: column 46 is a number
    clean = run(dev, 40, lm=lm)
    lm[3, 13, 0] = np.nan          # left elbow x: the left elbow and shoulder angles
    lm[7, 11, 2] = np.nan          # left shoulder z: its angles, sw (so s = 1); not the 2-D torso features
    lm[9, 12, 3] = np.nan          # a NaN visibility is not visible
    lm[9, [11, 23, 24], 3] = 0.9
    ref, bound, _ = R.features(lm)
    got = run(dev, 40, lm=lm)
    R.compare(got, ref, bound, "NaN inputs")
    col = {n: i for i, n in enumerate(R.FEATURE_NAMES)}
    assert np.isnan(got[3, [col["LEFT_ELBOW_ANGLE"], col["LEFT_SHOULDER_ANGLE"]]]).all() and np.isnan(got[3]).sum() == 2
    assert np.isnan(got[7, [col["LEFT_ELBOW_ANGLE"], col["LEFT_SHOULDER_ANGLE"], col["LEFT_HIP_ANGLE"]]]).all()
    assert np.isfinite(got[7, 41:47]).all()
    assert np.isnan(got[9, col["LM12_visibility"]]) and np.isnan(got[9]).sum() == 1 and np.isfinite(got[9, 46])
    untouched = [r for r in range(40) if r not in (3, 7, 9)]
    assert got[untouched].tobytes() == clean[untouched].tobytes()


def test_sequences_take_one_label_each():
    dev = _dev()
    P = pkg()
    means, stds = tables()
    lm = R.make_landmarks(6, seed=8).copy()
    lm[1, 15, :3] = lm[1, 13, :3]                             # a NaN elbow in sequence 0
    lm[4, 15, :3] = lm[4, 13, :3]                             # and in sequence 1
    det = np.ones(6, np.uint8)
    det[5] = 0
    labels = np.array([2, 0], np.int64)
    ref, bound, _ = R.features(lm, det)
    dl = torch.from_numpy(lm.reshape(2, 3, 33, 4)).to(dev)
    dd = torch.from_numpy(det.reshape(2, 3)).to(dev)
    dlab = torch.from_numpy(labels).to(dev)
    for mode in ("class_mean", "standardize"):
        pose = P.PoseFeatures(mode, torch.from_numpy(means).to(dev), torch.from_numpy(stds).to(dev) if mode == "standardize" else None)
        got = pose.from_landmarks(dl, dd, dlab)
        assert tuple(got.shape) == (2, 3, 47) and got.dtype == torch.float32
        want, wb = R.impute(ref, bound, MODES[mode], labels, means, stds, rows_per_label=3)
        R.compare(got.cpu().numpy().reshape(6, 47), want, wb, f"[2,3,33,4] {mode}")
        assert not torch.isnan(got).any()
        again = pose.impute(P.PoseFeatures("raw").from_landmarks(dl, dd), dlab)
        assert torch.equal(again, got)
    assert float(got[0, 1, 33]) == 0.0                                # "standardize": the imputed mean becomes 0
    flat = P.PoseFeatures("zero").from_landmarks(dl.view(6, 33, 4), dd.view(6).bool())
    assert tuple(flat.shape) == (6, 47) and not torch.isnan(flat).any()
    with pytest.raises(P.QtError, match="labels"):
        pose.from_landmarks(dl, dd, torch.zeros(6, dtype=torch.int64, device=dev))
    with pytest.raises(P.QtError, match="labels"):
        pose.from_landmarks(dl, dd)


def test_fit_against_a_float64_loop():
    dev = _dev()
    P = pkg()
    rng = np.random.default_rng(31)
    raw = R.restated(R.make_landmarks(200, seed=31))
    raw[rng.random(raw.shape) < 0.15] = np.nan
    labels = rng.choice([0, 1, 3], 200).astype(np.int64)      # class 2 is empty
    raw[labels == 0, 46] = np.nan                             # an empty cell of a class that has rows
    means, stds = P.PoseFeatures.fit(torch.from_numpy(raw).to(dev), torch.from_numpy(labels).to(dev), 4)
    assert means.dtype == stds.dtype == torch.float32 and tuple(means.shape) == tuple(stds.shape) == (4, 47)
    wm, ws = np.zeros((4, 47)), np.ones((4, 47))
    for k in range(4):
        for c in range(47):
            vals = [float(v) for v in raw[labels == k, c] if not np.isnan(v)]
            if vals:
                wm[k, c], ws[k, c] = float(np.mean(vals)), float(np.std(vals)) + 1e-6
    assert (wm[2] == 0).all() and (ws[2] == 1).all() and wm[0, 46] == 0 and ws[0, 46] == 1
    # two float64 evaluations that differ in the order of their sums (<= 200 x 2^-53 of the largest term, 180), then one
    # rounding to f32
    for got, want in ((means.cpu().numpy(), wm), (stds.cpu().numpy(), ws)):
        assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 1e-10).all()


def test_quadtree_eval_forward_fed_by_the_kernel():
    dev = _dev()
    P, synth = pkg(), pkg("synth")
    g = fixture()
    case = {str(n): i for i, n in enumerate(g["cases"])}
    pick = [0, case["no_pose"], case["body_scale_below_0.05"], 1]
    lm, det = g["landmarks"][pick], g["detected"][pick]
    ref, bound = R.impute(*R.features(lm, det)[:2], R.ZERO)
    numerical = P.PoseFeatures("zero").from_landmarks(torch.from_numpy(lm).to(dev), torch.from_numpy(det).to(dev))
    R.compare(numerical.cpu().numpy(), ref, bound, "model input")
    model = P.QuadtreeCNN(12, compute_dtype=torch.float32)
    model.load_state_dict(synth.synth_state_dict(model))
    model = model.to(dev).eval()
    images = synth.synth_images(4, salt=5).to(dev)
    with torch.no_grad():
        got = model(images, numerical).cpu()
        want = model(images, torch.from_numpy(ref.astype(np.float32)).to(dev)).cpu()
    assert torch.isfinite(got).all()
    assert rel_err(got, want) <= 1e-3             # LOGIT_TOL of tests/test_model_gpu.py for the f32 build


def test_cnn_lstm_takes_the_sequence_result_as_it_is():
    dev = _dev()
    P, synth = pkg(), pkg("synth")
    B, T = 2, 3
    lm = R.make_landmarks(B * T, seed=9)
    numerical = P.PoseFeatures("zero").from_landmarks(torch.from_numpy(lm).view(B, T, 33, 4).to(dev))
    assert tuple(numerical.shape) == (B, T, 47) and numerical.is_contiguous()
    model = P.CnnLstm(12, sequence_length=T, dropout_rate=0.0, compute_dtype=torch.float32)
    model.load_state_dict(synth.synth_state_dict(model))
    model = model.to(dev).eval()
    images = synth.synth_images(B * T, salt=9).view(B, T, 3, 224, 224).to(dev)
    ref, _ = R.impute(*R.features(lm)[:2], R.ZERO)
    with torch.no_grad():
        got = model(images, numerical).cpu()
        want = model(images, torch.from_numpy(ref.astype(np.float32)).view(B, T, 47).to(dev)).cpu()
    assert tuple(got.shape) == (B, 12) and torch.isfinite(got).all()
    assert rel_err(got, want) <= 1e-3
