"""CnnLstm stream, the parts that need no GPU: the plain loops of tests/_lstm_stream_ref.py against torch's nn.LSTM on
materialised windows (short windows included) and against themselves for every split of a stream into two and three calls,
the workspace-size condition, the C ABI's declarations, every host-side refusal of the new entry points (pointers that are
never dereferenced), the module's argument checks and exports."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _lstm_stream_ref as R
from _util import PKG, ROOT, pkg

QT_OK, QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = 0, -1, -3
P = ctypes.c_void_p
FAKE = 0x10000   # a 16-byte aligned address that is never dereferenced
STREAM = pkg("sequence_stream")   # the loops below restate ITS rule: without the module there is nothing to hold them to
assert STREAM.TILE == R.TILE and STREAM.MAX_WINDOW == 64 and STREAM.HIDDEN_SIZES == (256, 64)


def _lib():
    return pkg("_lib").lib()


def _last_error(L):
    return L.qt_last_error().decode()


@pytest.mark.parametrize("H,T", [(8, 1), (8, 4), (12, 6)])
def test_loops_match_torch_lstm_on_materialised_windows(H, T):
    S, frames, I = 2, 9, 5
    g = torch.Generator().manual_seed(3 + H)
    lstm = torch.nn.LSTM(I, H, num_layers=2, batch_first=True).double().eval()
    x = torch.randn(S, frames, I, generator=g, dtype=torch.float64)
    w = {"whh0": lstm.weight_hh_l0, "bhh0": lstm.bias_hh_l0, "wih1": lstm.weight_ih_l1, "bih1": lstm.bias_ih_l1,
         "whh1": lstm.weight_hh_l1, "bhh1": lstm.bias_hh_l1}
    w = {k: v.detach().numpy() for k, v in w.items()}
    rows = (x @ lstm.weight_ih_l0.t() + lstm.bias_ih_l0).detach().numpy()
    for seen, n in ((0, frames), (2, 5), (T - 1, 3), (T, 4)):
        n = min(n, frames - seen)
        got, carry = R.stream_forward(R.call_buffer(rows, seen, n, T), w, seen, n, T)
        for s in range(S):
            for f in range(n):
                gi = seen + f
                window = x[s:s + 1, max(0, gi - T + 1):gi + 1]          # the model at sequence length min(T, g + 1)
                with torch.no_grad():
                    want = lstm(window)[0][0, -1].numpy()
                assert np.abs(got[s, f] - want).max() <= 1e-12, (seen, s, f)
        for k in range(T - 1):
            gk = seen + n - (T - 1) + k
            assert np.array_equal(carry[:, k], rows[:, gk] if gk >= 0 else np.zeros_like(rows[:, 0]))


def test_every_split_of_a_stream_gives_the_bits_of_one_call():
    H, T, S, frames = 8, 4, 2, 20
    w = R.weights(H)
    rows = R.stream_rows(H, S, frames, "normal")
    whole_h, whole_c = R.run_calls(rows, w, [], T)
    assert np.isfinite(whole_h).all() and float(np.abs(whole_h).max()) > 1e-3
    cuts = [[a] for a in range(1, frames)] + [[a, b] for a, b in itertools.combinations(range(1, frames), 2)]
    assert len(cuts) == 19 + 171
    for cut in cuts:
        h, c = R.run_calls(rows, w, cut, T)
        assert R.bits(h) == R.bits(whole_h), cut
        assert R.bits(c) == R.bits(whole_c), cut
    # a stream alone and in a batch
    alone_h, alone_c = R.run_calls(rows[1:2], w, [7], T)
    assert R.bits(alone_h) == R.bits(whole_h[1:2]) and R.bits(alone_c) == R.bits(whole_c[1:2])


def test_f32_loops_follow_the_float64_loops_in_both_regimes():
    H, T, S, frames = 8, 4, 1, 10
    w = R.weights(H)
    for regime in ("normal", "saturated"):
        rows = R.stream_rows(H, S, frames, regime)
        buf = R.call_buffer(rows, 0, frames, T)
        h64, _ = R.stream_forward(buf, w, 0, frames, T, np.float64)
        h32, _ = R.stream_forward(buf, w, 0, frames, T, np.float32)
        assert h32.dtype == np.float32 and np.abs(h32 - h64).max() <= 1e-5, regime


def test_workspace_is_bounded_by_a_constant_times_the_input_products():
    """no buffer of size windows x T: at most a constant (here 1) times S (T - 1 + n) 4H floats, whatever T"""
    L = _lib()
    for H in (64, 256):
        for S, n, T in itertools.product((1, 3, 16), (1, 7, 8, 4096, 65536), (1, 2, 16, 64)):
            ws = L.qt_lstm_stream_workspace_bytes(S, n, T, H)
            assert ws <= 1 * S * (T - 1 + n) * 4 * H * 4, (H, S, n, T, ws)
    # the plan's: the input products themselves plus the kernel's
    eng = pkg("engine")
    desc = eng.PlanDesc(1, 64, 12, eng.QT_MODEL_CNN_LSTM, 0, 47, 0.5, 1e-5, 0.1, 4, 256)
    h = P()
    assert L.qt_plan_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    try:
        for S, n, T in ((1, 64, 16), (16, 1, 16), (3, 5, 1), (2, 19, 64)):
            want = S * (T - 1 + n) * 4 * 256 * 4 + L.qt_lstm_stream_workspace_bytes(S, n, T, 256)
            assert L.qt_plan_stream_workspace_bytes(h, S, n, T) == want
    finally:
        L.qt_plan_destroy(h)


def test_header_declares_the_entry_points_and_the_tile():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    for name in ("qt_lstm_stream_workspace_bytes", "qt_lstm_stream_forward", "qt_lstm_stream_stage", "qt_plan_features",
                 "qt_plan_stream_workspace_bytes", "qt_plan_stream_forward"):
        assert re.search(r"\b%s\s*\(" % name, header), name
    tile = int(re.search(r"#define\s+QT_LSTM_STREAM_TILE\s+(\d+)", header).group(1))
    assert tile == R.TILE == pkg("sequence_stream").TILE
    assert "min(T, g + 1)" in header        # the rule is stated next to the LSTM block


def _stream_args(**kw):
    a = dict(xproj0=FAKE, whh0=FAKE, bhh0=FAKE, wih1=FAKE, bih1=FAKE, whh1=FAKE, bhh1=FAKE, hlast=FAKE, carry=FAKE + 0x100000,
             ws=None, ws_bytes=0, seen=0, S=1, n=4, T=4, H=256)
    a.update(kw)
    return [a[k] for k in ("xproj0", "whh0", "bhh0", "wih1", "bih1", "whh1", "bhh1", "hlast", "carry", "ws", "ws_bytes",
                           "seen", "S", "n", "T", "H")] + [None]


def test_lstm_stream_forward_refusals():
    L = _lib()
    for kw in (dict(H=188), dict(H=128), dict(H=0), dict(T=0), dict(T=65), dict(T=-1)):
        assert L.qt_lstm_stream_forward(*_stream_args(**kw)) == QT_ERR_UNSUPPORTED, kw
        assert "qt_lstm_stream_forward" in _last_error(L)
    for kw in (dict(S=0), dict(n=0), dict(n=-3), dict(seen=-1), dict(xproj0=None), dict(whh0=None), dict(bhh0=None),
               dict(wih1=None), dict(bih1=None), dict(whh1=None), dict(bhh1=None), dict(hlast=None),
               dict(carry=FAKE), dict(xproj0=FAKE + 4), dict(whh1=FAKE + 8), dict(carry=FAKE + 0x100004),
               dict(S=1 << 30, n=1 << 30)):
        assert L.qt_lstm_stream_forward(*_stream_args(**kw)) == QT_ERR_INVALID_ARG, kw
        assert "qt_lstm_stream_forward" in _last_error(L)


def test_lstm_stream_stage_refusals():
    L = _lib()
    assert L.qt_lstm_stream_stage(FAKE, FAKE, FAKE, 1, 4, 4, 188, None) == QT_ERR_UNSUPPORTED
    assert L.qt_lstm_stream_stage(FAKE, FAKE, FAKE, 1, 4, 65, 64, None) == QT_ERR_UNSUPPORTED
    for args in ((None, FAKE, FAKE, 1, 4, 4, 64), (FAKE, None, FAKE, 1, 4, 4, 64), (FAKE, FAKE, None, 1, 4, 4, 64),
                 (FAKE, FAKE, FAKE, 0, 4, 4, 64), (FAKE, FAKE, FAKE, 1, 0, 4, 64), (FAKE, FAKE + 4, FAKE, 1, 4, 4, 64)):
        assert L.qt_lstm_stream_stage(*args, None) == QT_ERR_INVALID_ARG, args
        assert "qt_lstm_stream_stage" in _last_error(L)


def _plan(L, kind, batch=8):
    eng = pkg("engine")
    desc = eng.PlanDesc(1, batch, 12, kind, 0, 47, 0.5, 1e-5, 0.1, 4, 256)
    h = P()
    assert L.qt_plan_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    return h


def test_plan_entry_points_refuse_other_models_and_bad_arguments():
    L = _lib()
    ALIGNED = 0x100000
    assert L.qt_plan_features(None, ALIGNED, FAKE, FAKE, FAKE, 4, None) == QT_ERR_INVALID_ARG
    assert L.qt_plan_stream_forward(None, ALIGNED, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE + 64, FAKE, 1 << 30, 0, 1, 4, 4,
                                    None) == QT_ERR_INVALID_ARG
    for kind in (0, 1, 2):
        h = _plan(L, kind)
        try:
            assert L.qt_plan_features(h, ALIGNED, FAKE, FAKE, FAKE, 4, None) == QT_ERR_UNSUPPORTED
            assert "not a CnnLstm" in _last_error(L)
            assert L.qt_plan_stream_forward(h, ALIGNED, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE + 64, FAKE, 1 << 30, 0, 1, 4, 4,
                                            None) == QT_ERR_UNSUPPORTED
            assert "not a CnnLstm" in _last_error(L)
            assert L.qt_plan_stream_workspace_bytes(h, 1, 4, 4) == 0
        finally:
            L.qt_plan_destroy(h)
    h = _plan(L, 3)
    try:
        big = L.qt_plan_stream_workspace_bytes(h, 2, 4, 4)
        assert big == 2 * 7 * 1024 * 4

        def fwd(ws=ALIGNED, tensors=FAKE, image=FAKE, numerical=FAKE, logits=FAKE, cin=FAKE, cout=FAKE + 64, sws=FAKE,
                sws_bytes=big, seen=0, S=2, n=4, T=4):
            return L.qt_plan_stream_forward(h, ws, tensors, image, numerical, logits, cin, cout, sws, sws_bytes, seen, S, n, T,
                                            None)
        for kw in (dict(T=0), dict(T=65)):
            assert fwd(**kw) == QT_ERR_UNSUPPORTED, kw
        for kw in (dict(ws=None), dict(tensors=None), dict(image=None), dict(numerical=None), dict(logits=None),
                   dict(sws=None), dict(cin=None), dict(cout=None), dict(cout=FAKE), dict(S=0), dict(n=0), dict(seen=-1),
                   dict(S=3), dict(sws_bytes=big - 1), dict(ws=ALIGNED + 16), dict(sws=FAKE + 4)):
            assert fwd(**kw) == QT_ERR_INVALID_ARG, kw
            assert "qt_plan_stream_forward" in _last_error(L)
        for args in ((None, FAKE, FAKE, FAKE, 4), (ALIGNED, None, FAKE, FAKE, 4), (ALIGNED, FAKE, None, FAKE, 4),
                     (ALIGNED, FAKE, FAKE, None, 4), (ALIGNED, FAKE, FAKE, FAKE, 0), (ALIGNED, FAKE, FAKE, FAKE, 9),
                     (ALIGNED + 16, FAKE, FAKE, FAKE, 4)):
            assert L.qt_plan_features(h, *args, None) == QT_ERR_INVALID_ARG, args
            assert "qt_plan_features" in _last_error(L)
    finally:
        L.qt_plan_destroy(h)


def test_module_checks_its_arguments_without_a_gpu():
    Pk = pkg()
    QtError = Pk.QtError
    assert Pk.CnnLstmStream is pkg("sequence_stream").CnnLstmStream and "CnnLstmStream" in Pk.__all__
    with pytest.raises(TypeError, match="CnnLstm"):
        Pk.CnnLstmStream(Pk.StandardResNetCNN(12, pretrained=False))
    m = Pk.CnnLstm(12, sequence_length=3, pretrained=False)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="window"):
            Pk.CnnLstmStream(m, window=bad)
    with pytest.raises(ValueError, match="streams"):
        Pk.CnnLstmStream(m, streams=0)
    st = Pk.CnnLstmStream(m, streams=2)
    assert st.window == 3 and st.seen == 0
    frames, poses = torch.zeros(2, 1, 3, 224, 224), torch.zeros(2, 1, 47)
    m.train()
    with pytest.raises(QtError, match="train"):
        st.step(frames, poses)
    m.eval()
    with pytest.raises(QtError, match="no CPU"):
        st.step(frames, poses)                   # CPU tensors: there is no torch fallback
    assert st.seen == 0
