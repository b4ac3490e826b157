"""Pose-order decoding, the parts that need no GPU: the table and q of tests/_pose_order_ref.py against their formulas, hand-
written cases of the rule, every split of a stream into two and three calls, a float64 Viterbi on a well-separated input, the
tiled algorithm restated in integers against the loops, the C ABI's declaration and every host-side refusal (pointers that are
never dereferenced), the module's argument checks, the exports and the documents."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import _pose_order_ref as R
from _util import PKG, ROOT, pkg, pose_chain_header

QT_ERR_INVALID_ARG, QT_ERR_UNSUPPORTED = -1, -3
F32 = np.float32


def test_log2_table_is_its_formula():
    i = np.arange(256, dtype=np.float64)
    exact = 256.0 * np.log2(1.0 + (2.0 * i + 1.0) / 512.0)
    assert np.abs(exact - np.floor(exact) - 0.5).min() > 1e-3                  # no entry within 10^-3 of a half
    assert np.rint(exact).astype(int).tolist() == list(R.LOG2_TABLE)
    assert R.LOG2_TABLE[:4] == (1, 2, 4, 5) and R.LOG2_TABLE[-4:] == (253, 254, 255, 256)
    M = pkg("pose_order")
    assert tuple(M.LOG2_TABLE) == R.LOG2_TABLE
    body = re.search(r"PC_LOG2\[256\] = \{(.*?)\};", pose_chain_header(), re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", body)] == list(R.LOG2_TABLE)


def test_q_at_its_edges():
    one, low = F32(1.0), F32(2.0 ** -32)
    assert [R.q(x) for x in (np.nan, -np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-42, np.nextafter(low, F32(0)))] == [-8192] * 8
    assert [R.q(x) for x in (np.inf, 1.0, 1.5, 3e38)] == [0] * 4
    assert R.q(low) == 256 * -32 + 1 and R.q(np.nextafter(low, one)) == 256 * -32 + 1
    assert R.q(np.nextafter(one, F32(0))) == -256 + 256 == 0
    assert R.q(0.5) == -256 + 1 and R.q(0.25) == -512 + 1 and R.q(0.75) == -256 + R.LOG2_TABLE[128] == -106
    values = np.array([np.nan, -0.0, 0.0, 1e-42, low, 0.3, 0.5, 1.0, np.inf, -np.inf, 2.0], F32)
    M = pkg("pose_order")
    assert R.q_array(values).tolist() == [R.q(v) for v in values] == M.prob_score(values).tolist()
    assert M.prob_score(0.5) == -255 and isinstance(M.prob_score(0.5), int) and M.prob_score(values.reshape(1, -1)).shape == (1, 11)


def test_q_stays_within_a_unit_and_a_quarter_of_the_logarithm():
    rng = np.random.default_rng(2024)
    p = (2.0 ** rng.uniform(-32, 0, 100_000)).astype(F32)
    p = p[(p >= F32(2.0 ** -32)) & (p < 1)]
    assert p.size > 99_000
    err = np.abs(R.q_array(p) - 256.0 * np.log2(p.astype(np.float64)))
    assert err.max() <= 1.25
    assert [R.q(v) for v in p[:500]] == R.q_array(p[:500]).tolist()


def _one(probs, sc, trans, init=None, carry=None):
    return R.decode(np.asarray(probs, F32)[None], np.asarray(sc), np.asarray(trans), init, carry)


def test_a_cycle_does_not_visit_a_wrong_state():
    """3 states in a cycle; the raw argmax says 0 0 0 2 1 1 1 2 2: frame 3 is a flicker the prior does not follow.  Staying in 0
    for it or advancing to 1 score alike there (0.3 each, one advance either way): psi's lowest index keeps state 0"""
    hi, lo = 0.8, 0.1
    rows = [[hi, lo, lo]] * 3 + [[0.3, 0.3, 0.4]] + [[lo, hi, lo]] * 3 + [[lo, lo, hi]] * 2
    sc, trans = R.cyclic_prior([0, 1, 2], -30, -300)
    path, filtered, em, carry = _one(rows, sc, trans)
    assert np.argmax(np.asarray(rows), axis=1).tolist() == [0, 0, 0, 2, 1, 1, 1, 2, 2]
    assert path[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2] and filtered[0, 3] == 0
    assert 2 not in path[0, :7].tolist()
    assert em[0, 0].tolist() == [R.q(F32(hi)), R.q(F32(lo)), R.q(F32(lo))] and carry[0, 0] == 9 and carry[0, 2:].max() == 0
    assert R.cycles(path, 2, 0)[0].tolist() == [0]
    twice = np.concatenate([path, path], axis=1)
    assert R.cycles(twice, 2, 0)[0].tolist() == [1]
    counts, last = R.cycles(path, 2, 0)
    assert last.tolist() == [2] and R.cycles(path, 2, 0, last)[0].tolist() == [1]      # the wrap on the call boundary


def test_ties_go_to_the_lower_index():
    # every probability alike, trans all zero: psi is 0 everywhere, the end state is 0
    path, filtered, _, carry = _one(np.full((5, 3), 0.25), [0, 1, 2], np.zeros((3, 3), int))
    assert path[0].tolist() == [0] * 5 and filtered[0].tolist() == [0] * 5 and carry[0].tolist() == [5, 5 * R.q(0.25), 0, 0, 0]
    # predecessors 1 and 2 tie for every state and beat 0: psi says 1; all three states tie for the end: 0
    trans = np.array([[-90, -90, -90], [-20, -20, -20], [-20, -20, -20]])
    path, filtered, _, _ = _one([[0.5, 0.5, 0.5]] * 2, [0, 1, 2], trans, np.zeros(3, int))
    assert filtered[0].tolist() == [0, 0] and path[0].tolist() == [1, 0]
    # states 1 and 2 tie for the end above state 0: 1
    path, filtered, _, _ = _one([[0.25, 0.5, 0.5]] * 2, [0, 1, 2], trans, np.zeros(3, int))
    assert filtered[0].tolist() == [1, 1] and path[0].tolist() == [1, 1]


def test_a_class_that_two_states_emit():
    """steps 0 1 0 2 of three classes: the two states of class 0 are told apart by what comes before and after"""
    sc, trans = R.cyclic_prior([0, 1, 0, 2], -30, -400)
    lead = [0] * 4 + [1] * 4 + [0] * 4 + [2] * 4 + [0] * 3
    rows = np.full((len(lead), 3), 0.1)
    rows[np.arange(len(lead)), lead] = 0.8
    path, _, em, _ = _one(rows, sc, trans)
    assert path[0].tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [0] * 3
    assert (em[0, :, 0] == em[0, :, 2]).all()
    assert sc[path[0]].tolist() == lead and R.cycles(path, 3, 0)[0].tolist() == [1]


def test_every_split_of_a_stream_gives_the_bits_of_one_call():
    T, C = 40, 5
    probs = R.make_probs(3, 1, T, C, run=4)
    probs[0, 7] = np.nan
    probs[0, 20] = 0.0
    probs[0, 30:33] = F32(0.2)
    sc, trans = R.cyclic_prior([0, 1, 2, 3, 4, 2], -30, -500, skip=-2500)
    init = np.array([0, -100, -200, -300, -400, -500])
    whole = R.decode(probs, sc, trans, init)
    assert len(set(whole[0][0].tolist())) >= 5 and (whole[0] != whole[1]).any()      # smoothing differs from filtering
    cuts = [[a] for a in range(1, T)] + [[a, b] for a, b in itertools.combinations(range(1, T), 2)]
    assert len(cuts) == 39 + 741
    for cut in cuts:
        path, filtered, em, carry, last = R.decode_split(probs, sc, trans, init, cut)
        assert R.bits(filtered) == R.bits(whole[1]) and R.bits(em) == R.bits(whole[2]) and R.bits(carry) == R.bits(whole[3]), cut
        assert R.bits(last) == R.bits(whole[0][:, cut[-1]:]), cut


def test_float64_viterbi_finds_the_same_path():
    T, C = 60, 6
    rng = np.random.default_rng(8)
    lead = (np.arange(T) // 5) % C
    probs = rng.uniform(0.01, 0.05, (T, C))
    probs[np.arange(T), lead] = rng.uniform(0.6, 0.8, T)
    probs[[12, 33], lead[[12, 33]]] = 0.02                     # two frames where the right class is weak
    probs = probs.astype(F32)
    sc, trans = R.cyclic_prior(range(C), -38, -850)
    want = R.decode_float64(probs, sc, trans)
    path = R.decode(probs[None], sc, trans)[0]
    assert path[0].tolist() == want.tolist() == lead.tolist()


def test_the_tiled_form_equals_the_loops():
    for seed, (B, T, C, S) in enumerate([(2, 23, 5, 6), (1, 23, 3, 3), (2, 23, 12, 12)]):
        probs = R.make_probs(40 + seed, B, T, C, run=3)
        probs[0, 5] = np.nan
        probs[-1, 11:14] = F32(0.25)
        sc, trans = R.cyclic_prior([s % C for s in range(S)], -30, -600, skip=-3000, other=-20000)
        init = -np.arange(S) * 37
        for trans_used in (trans, np.zeros_like(trans)):
            for carry in (None, np.array([[9, -1234] + [-((7 * s * s) % 900) for s in range(S)]] * B, np.int64)):
                want = R.decode(probs, sc, trans_used, init, carry)
                for tile, group in ((1, R.GROUP), (2, R.GROUP), (5, R.GROUP), (R.TILE, R.GROUP), (1, 4), (2, 3), (5, 2), (1, 1)):
                    got = R.tiled(probs, sc, trans_used, init, carry, tile=tile, group=group)
                    for name, w, g in zip(("path", "filtered", "emissions", "carry"), want, got):
                        assert w.dtype == g.dtype and R.bits(w) == R.bits(g), (B, T, S, tile, group, name)


def test_cyclic_prior():
    M = pkg("pose_order")
    sc, trans = M.cyclic_prior([3, 1, 4, 1], -10, -20, skip=-30, other=-99)
    assert sc.dtype == np.int32 and trans.dtype == np.int32 and sc.tolist() == [3, 1, 4, 1]
    assert trans.tolist() == [[-10, -20, -30, -99], [-99, -10, -20, -30], [-30, -99, -10, -20], [-20, -30, -99, -10]]
    assert M.cyclic_prior([0, 1, 2], -1, -2, wrap=False)[1].tolist() == [[-1, -2, -65536], [-65536, -1, -2], [-65536, -65536, -1]]
    assert M.cyclic_prior([0], -1, -2, skip=-3)[1].tolist() == [[-1]] and M.cyclic_prior([0, 1], -1, -2, skip=-3)[1].tolist() == [[-1, -2], [-2, -1]]
    for args in (([3, 1, 4, 1], -10, -20, -30, -99), ([0, 1, 2], -1, -2, None, -65536, False), ([0, 1], -1, -2, -3), (list(range(12)), -38, -850)):
        a, b = M.cyclic_prior(*args), R.cyclic_prior(*args)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    for bad in (dict(stay=1), dict(stay=-65537), dict(advance=-1.5), dict(advance=True), dict(skip=3), dict(other=-70000)):
        with pytest.raises(ValueError):
            M.cyclic_prior(**{"step_classes": [0, 1, 2], "stay": -1, "advance": -2, **bad})
    with pytest.raises(ValueError):
        M.cyclic_prior([], -1, -2)
    with pytest.raises(ValueError):
        M.cyclic_prior(list(range(65)), -1, -2)
    with pytest.raises(ValueError):
        M.cyclic_prior([0, -1], -1, -2)


def test_constants_are_the_kernels_and_the_modules():
    M = pkg("pose_order")
    assert (M.TILE, M.MAX_STATES, M.MAX_CLASSES, M.MAX_FRAMES, M.SCORE_FLOOR, M.TRANS_FLOOR) == \
        (R.TILE, R.MAX_STATES, R.MAX_CLASSES, R.MAX_FRAMES, R.SCORE_FLOOR, R.TRANS_FLOOR)
    src = pose_chain_header() + open(os.path.join(ROOT, PKG, "csrc", "pose_order.hip")).read()
    const = lambda name: int(re.search(rf"constexpr int {name} = (-?\d+);", src).group(1))
    assert (const("PC_TILE"), const("PC_MAX_S"), const("PC_MAX_C"), const("PC_FLOOR"), const("PC_TRANS_FLOOR")) == \
        (R.TILE, R.MAX_STATES, R.MAX_CLASSES, R.SCORE_FLOOR, R.TRANS_FLOOR)
    assert M.GROUP == const("PO_GROUP") == R.GROUP
    for S in (1, 2, 3, 11, 12, 13, 16, 17, 45, 46, 63, 64):
        assert M.scan_trip_tiles(S) == R.scan_trip_tiles(S) == max(1, min(const("PO_SCAN_MAX_TILES"), const("PO_SCAN_INTS") // (S * S)))
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert (define("QT_POSE_ORDER_TILE"), define("QT_POSE_ORDER_MAX_STATES"), define("QT_POSE_ORDER_MAX_CLASSES")) == \
        (R.TILE, R.MAX_STATES, R.MAX_CLASSES)
    # the kernel's range: 64 v + r fits 32 bits 64 frames below the lowest start it keeps
    low = -const_shift(src)
    assert 64 * (low - R.TILE * (65536 + 8192) - 65536) > -2 ** 31


def const_shift(src):
    return 1 << int(re.search(r"constexpr int PO_LOW = -\(1 << (\d+)\);", src).group(1))


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "qtcnn.h")).read()
    declared = set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.path.join(ROOT, PKG, "libqtcnn_hip.so"))
    for symbol in ("qt_pose_order_workspace_bytes", "qt_pose_order_decode"):
        assert symbol in declared and hasattr(lib, symbol), symbol
    M = pkg("pose_order")
    fields = re.search(r"typedef struct qt_pose_order_desc \{(.*?)\} qt_pose_order_desc;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields)
    assert re.findall(r"\b(\w+)\s*;", fields) == [n for n, _ in M.PoseOrderDesc._fields_]
    assert all(t is ctypes.c_int for _, t in M.PoseOrderDesc._fields_)
    P = pkg()
    assert P.PoseOrderDecoder is M.PoseOrderDecoder and P.cyclic_prior is M.cyclic_prior and P.prob_score is M.prob_score
    assert {"PoseOrderDecoder", "cyclic_prior", "prob_score"} <= set(P.__all__)


def _lib():
    M = pkg("pose_order")
    L = pkg("_lib").lib()
    return M, L


def test_workspace_query():
    M, L = _lib()
    q = lambda *a: L.qt_pose_order_workspace_bytes(ctypes.byref(M.PoseOrderDesc(*a)))
    for frames in (1, 2, R.TILE):
        assert q(3, frames, 12, 12) == 0
    B, T, S = 3, 2 * R.TILE + 3, 12
    tiles = 3
    assert q(B, T, 12, S) == B * (tiles * S * 8 + (tiles - 1) * S * S * 4 + tiles * 4 + T * S + tiles * S)
    T, tiles, groups = 33 * R.TILE, 33, 2                                      # above a group of 32 tiles the scan has two levels
    assert q(B, T, 12, S) == B * (tiles * S * 8 + groups * S * 8 + (tiles - 1) * S * S * 4 + (groups - 1) * S * S * 4 + tiles * 4 +
                                  T * S + tiles * S)
    assert q(1, R.TILE + 1, 64, 64) == 2 * 64 * 8 + 64 * 64 * 4 + 2 * 4 + 65 * 64 + 2 * 64
    assert q(0, 100, 12, 12) == 0 and q(1, 100, 12, 65) == 0 and L.qt_pose_order_workspace_bytes(None) == 0


def test_decode_argument_checks_need_no_device():
    """every refusal comes before the first device call: the pointers are never dereferenced"""
    M, L = _lib()
    D = lambda batch=2, frames=100, C=12, S=12: M.PoseOrderDesc(batch, frames, C, S)
    probs, sc, trans, init, carry, path, filt, em, ws = (0x10000000 * k for k in range(1, 10))
    good = dict(probs=probs, ld=12, sc=sc, trans=trans, init=init, carry=carry, path=path, filt=filt, em=em, ws=ws, ws_bytes=1 << 24)

    def call(desc, **kw):
        a = {**good, **kw}
        return L.qt_pose_order_decode(ctypes.byref(desc), a["probs"], a["ld"], a["sc"], a["trans"], a["init"], a["carry"],
                                      a["path"], a["filt"], a["em"], a["ws"], a["ws_bytes"], None)

    def refused(rc, word, status=QT_ERR_INVALID_ARG):
        assert rc == status and word in L.qt_last_error(), (rc, L.qt_last_error())

    refused(L.qt_pose_order_decode(None, probs, 12, sc, trans, init, carry, path, filt, em, ws, 1 << 24, None), b"null descriptor")
    for batch in (0, -3):
        refused(call(D(batch=batch)), b"batch")
    for frames in (0, -1):
        refused(call(D(frames=frames)), b"frames")
    for C in (0, -1, 65):
        refused(call(D(C=C), ld=70), b"num_classes")
    for S in (0, -1, 65):
        refused(call(D(S=S)), b"num_states")
    refused(call(D(), ld=11), b"ld")
    for name in ("probs", "sc", "trans", "carry", "path"):
        refused(call(D(), **{name: None}), b"null")
    for name, off in (("probs", 2), ("sc", 1), ("trans", 3), ("init", 2), ("em", 1), ("carry", 4), ("path", 4), ("filt", 4), ("ws", 4)):
        refused(call(D(), **{name: good[name] + off}), b"aligned")
    need = L.qt_pose_order_workspace_bytes(ctypes.byref(D()))
    assert need > 0
    refused(call(D(), ws_bytes=need - 1), b"workspace")
    refused(call(D(), ws_bytes=0), b"workspace")
    refused(call(D(), ws=None), b"workspace")
    rows = 2 * 100
    for out, nbytes in (("carry", 2 * 14 * 8), ("path", rows * 8), ("filt", rows * 8), ("em", rows * 12 * 4), ("ws", need)):
        refused(call(D(), **{out: probs + (rows * 12 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: probs - nbytes + 8}), b"overlap")
        refused(call(D(), **{out: sc + 40}), b"overlap")
        refused(call(D(), **{out: trans + (144 - 2) * 4}), b"overlap")
        refused(call(D(), **{out: init}), b"overlap")
    refused(call(D(), ld=16, path=probs + (199 * 16 + 10) * 4), b"overlap")
    refused(call(D(), filt=path + 8), b"overlap")
    refused(call(D(batch=1 << 10, frames=(1 << 10) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    refused(call(D(batch=1, frames=(1 << 20) + 1)), b"frames", QT_ERR_UNSUPPORTED)
    # the short route asks for no workspace: a null one is not refused for being null (the next check is reached)
    refused(call(D(frames=R.TILE), ws=None, ws_bytes=0, path=None), b"null path")


def test_module_argument_checks_need_no_device():
    P = pkg()
    sc, trans = P.cyclic_prior(range(4), -10, -100)
    for bad in (dict(state_class=[]), dict(state_class=list(range(65)), trans=np.zeros((65, 65), int)), dict(state_class=[0, 1, 2, 64]),
                dict(state_class=[0, -1, 2, 3]), dict(state_class=np.zeros(4)), dict(trans=trans[:3]), dict(trans=trans.astype(float)),
                dict(trans=trans - 65536), dict(trans=-trans), dict(init=[0, 0, 0]), dict(init=np.array([0, 0, 0, 1])),
                dict(init=np.zeros(4)), dict(streams=0), dict(streams=True), dict(streams=2.0), dict(class_names=["a", "b", "c"])):
        with pytest.raises(ValueError):
            P.PoseOrderDecoder(**{"state_class": sc, "trans": trans, "device": "cuda:0", **bad})
    with pytest.raises(P.QtError, match="AMD GPU"):      # no torch fallback
        P.PoseOrderDecoder(sc, trans, "cpu")


def test_the_documents_speak_of_the_pose_order():
    for doc, word in (("DESIGN.md", "Pose order"), ("DESIGN.md", "(max, +)"), ("INTEGRATION.md", "decoder.decode("),
                      ("README.md", "PoseOrderDecoder"), ("EXPERIMENTS.md", "Pose order"),
                      (os.path.join(PKG, "timeline.py"), "pose_order.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
