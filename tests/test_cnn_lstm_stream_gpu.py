"""CnnLstmStream on the GPU (sequence_stream.py, qt_plan_stream_forward / qt_plan_features of csrc/plan.hip), f32 and bf16
builds: per-frame logits against the reference's golden vectors (tests/golden/cnn_lstm_b2t3.npz) and against the model's own
eval() forward on the materialised windows, short windows at their own length, in one call and in two; the per-frame features
at a batch that is no multiple of seq_len; the video loop step -> softmax -> PoseTimeline.update under "no host
synchronisation"; refusals.

Tolerances: those of tests/test_cnn_lstm_gpu.py, restated: logits 1e-3 (f32 build) / 4e-2 (bf16 build), max|a-b| / max|b|.
"""
import ctypes

import pytest
import torch

from _util import pkg, rel_err

pytestmark = pytest.mark.gpu
LOGIT_TOL = {torch.float32: 1e-3, torch.bfloat16: 4e-2}
FUSED_TOL = {torch.float32: 1e-4, torch.bfloat16: 4e-2}
DTYPES = [torch.float32, torch.bfloat16]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _build(dt, T):
    P, synth = pkg(), pkg("synth")
    m = P.CnnLstm(12, sequence_length=T, dropout_rate=0.5, compute_dtype=dt)
    m.load_state_dict(synth.synth_state_dict(m))
    return m


def _inputs(S, n, salt, dev):
    synth = pkg("synth")
    x = synth.synth_images(S * n, salt=salt).view(S, n, 3, 224, 224).to(dev)
    f = synth.synth_pose_features(S * n, salt=salt).view(S, n, 47).to(dev)
    return x, f


@pytest.mark.parametrize("dt", DTYPES)
def test_third_frame_matches_reference_golden(dt, golden_cnn_lstm):
    dev = _dev()
    S, T = 2, 3
    x, f = _inputs(S, T, 7, dev)          # the inputs of test_cnn_lstm_matches_reference_golden
    m = _build(dt, T).to(dev).eval()
    stream = pkg().CnnLstmStream(m, streams=S)
    logits = stream.step(x, f)
    assert tuple(logits.shape) == (S, T, 12) and stream.seen == T
    err = rel_err(logits[:, T - 1].cpu(), golden_cnn_lstm["eval/logits"])
    print(f"{dt}: third-frame logits vs golden: {err:.3e}")
    assert err <= LOGIT_TOL[dt], err


@pytest.mark.parametrize("dt", DTYPES)
def test_every_frame_matches_the_model_on_its_window_in_one_call_and_in_two(dt):
    dev = _dev()
    S, T, N = 2, 3, 5
    x, f = _inputs(S, N, 21, dev)
    m = _build(dt, T).to(dev).eval()
    want = torch.empty(S, N, 12)
    with torch.no_grad():
        for g in range(N):                  # the model at sequence length min(T, g + 1)
            a = max(0, g - T + 1)
            want[:, g] = m(x[:, a:g + 1].contiguous(), f[:, a:g + 1].contiguous()).cpu()
    stream = pkg().CnnLstmStream(m, streams=S, window=T)
    one = stream.step(x, f).cpu()
    assert stream.seen == N
    stream.reset()
    assert stream.seen == 0
    two = torch.cat([stream.step(x[:, :2].contiguous(), f[:, :2].contiguous()),
                     stream.step(x[:, 2:].contiguous(), f[:, 2:].contiguous())], dim=1).cpu()
    assert stream.seen == N
    for name, got in (("one call", one), ("2 + 3", two)):
        for g in range(N):
            err = rel_err(got[:, g], want[:, g])
            print(f"{dt} {name} frame {g}: {err:.3e}")
            assert err <= LOGIT_TOL[dt], (name, g, err)
    # new weights: the carry holds products of the old W_ih, the stream starts over by itself
    with torch.no_grad():
        m.lstm.weight_ih_l0.mul_(1.0)
    stream.step(x[:, :1].contiguous(), f[:, :1].contiguous())
    assert stream.seen == 1


@pytest.mark.parametrize("dt", DTYPES)
def test_features_at_a_batch_that_is_no_multiple_of_seq_len(dt):
    dev = _dev()
    T = 3
    x, f = _inputs(2, T, 7, dev)
    m = _build(dt, T).to(dev).eval()
    with torch.no_grad():
        m(x, f)
    eng = m._engine
    fused = eng.buffer("fused", (eng.max_batch, 640))
    six = fused[:6].float().cpu()
    fused.fill_(float("nan"))
    L = pkg("_lib")
    lib = eng.L
    images, poses = x.view(6, 3, 224, 224)[:5].contiguous(), f.view(6, 47)[:5].contiguous()
    L.check(lib.qt_plan_features(eng.handle, eng.ws_ptr, eng._tensor_ptrs, L.ptr(images), L.ptr(poses), 5, L.stream_ptr()),
            "qt_plan_features")
    five = fused[:5].float().cpu()
    err = rel_err(five, six[:5])
    print(f"{dt}: fused rows at batch 5 vs batch 6: {err:.3e}")
    assert err <= FUSED_TOL[dt], err
    assert bool(torch.isnan(fused[5:6].float()).all())          # nothing beyond the batch is written
    # the plan refuses a backward after it: what it would read is gone
    grads = (ctypes.c_void_p * len(eng.names))()
    d = torch.zeros(2, 12, device=dev)
    assert eng.L.qt_plan_backward(eng.handle, eng.ws_ptr, eng._tensor_ptrs, grads, L.ptr(poses), L.ptr(d), 15,
                                  L.stream_ptr()) != 0


def test_video_loop_runs_without_host_synchronisation():
    dev = _dev()
    P = pkg()
    S, T = 2, 3
    x, f = _inputs(S, 4, 33, dev)
    m = _build(torch.bfloat16, T).to(dev).eval()
    stream = P.CnnLstmStream(m, streams=S)
    timeline = P.PoseTimeline(12, dev, streams=S, window=3, min_run=2)
    chunks = [(x[:, a:b].contiguous(), f[:, a:b].contiguous()) for a, b in ((0, 1), (1, 3), (3, 4))]
    # first launches outside the guarded region (plan, code-object load, workspaces)
    timeline.update(stream.step(x, f).softmax(-1), smoothed=True)
    stream.reset()
    timeline.reset()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = []
        for frames, poses in chunks:
            logits = stream.step(frames, poses)
            pred, confidence, stable, rows = timeline.update(logits.softmax(-1), smoothed=True)
            outs.append((logits, pred))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert stream.seen == 4
    logits = torch.cat([o[0] for o in outs], dim=1)
    assert tuple(logits.shape) == (S, 4, 12) and bool(torch.isfinite(logits).all())
    assert tuple(torch.cat([o[1] for o in outs], dim=1).shape) == (S, 4)


def test_refusals_on_the_device():
    dev = _dev()
    P = pkg()
    QtError = P.QtError
    with pytest.raises(TypeError, match="CnnLstm"):
        P.CnnLstmStream(P.QuadtreeCNN(12, pretrained=False).to(dev))
    m = _build(torch.bfloat16, 3).to(dev)
    stream = P.CnnLstmStream(m, streams=2)
    x, f = _inputs(2, 1, 3, dev)
    m.train()
    with pytest.raises(QtError, match="train"):
        stream.step(x, f)
    m.eval()
    with pytest.raises(QtError, match="no CPU"):
        stream.step(x.cpu(), f.cpu())
    with pytest.raises(QtError, match="float32"):
        stream.step(x.half(), f)
    with pytest.raises(ValueError, match="frames must be"):
        stream.step(x[:1], f[:1])
    assert stream.seen == 0
