"""One internal buffer of the plan workspace running into the next (tests/_plan_gaps.py): every plan model, at the batches where
the plan changes kernel routes, through eval forwards, two train steps and a forward on the re-packed operands, on a workspace
whose regions lie 1 MiB apart with 0xFF in between -- gaps intact after every call, every result finite and equal to a plain
twin's.  The sizes of the regions come from layout_workspace() in csrc/plan.hip, the rows and bytes written from the kernels
the plan picks at that batch: this is where the two meet.

Default QTCNN_* switches and stream schedule.  Batches (conv_pt.hip / conv_s2.hip: `batch < 16`, 7x7 maps `batch % 4`):
  2    the generic tile everywhere
  4    QuadtreeCNN only: the quadrant head's 4 x 4 = 16 region images put its conv on conv_pt (qt_pt_eligible counts
       pt_images() = M / 49 images against 16), everything else on the generic tile
  16   conv_pt / qt_conv_s2_pair at every stage
  18   those at 28x28 / 14x14, the 7x7 stage back on the generic tile
  48   more than 1024 partial rows in the backward: the merged stride-2 data gradient on conv_pt emits 32 rows per image, the
       data-gradient epilogues of layer1 one per 128 pixels (1176), so qt_bn_bwd_finalize first folds them 64:1 into the spare
       rows behind (fold_partial in elementwise.hip: `rows <= 1024`; qt_stats_capacity_rows) -- the `+ 8` and the fold rows of
       the three `stats_*` scratches.  (The stem's forward statistics fold from 11 images on.)
  5 of 18   rows sized by the run batch inside regions sized by the plan batch
Mistakes made on purpose stay on the CPU (tests/test_plan_gaps_cpu.py)."""
import pytest
import torch

from _guard import POISON, Guard
from _plan_gaps import GAP_BYTES, PlanGaps, compare_twins, plan_guard_gap, plan_run, region_table
from _util import pkg

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SEQ = 4   # frames per CnnLstm sequence (the reference's SEQ_LEN)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(kind, dt, plan_batch, gap):
    """`kind` on the GPU in train mode with its engine for plan_batch built under guard gap `gap`"""
    P, synth = pkg(), pkg("synth")
    dev = _dev()
    kw = dict(dropout_rate=0.0, compute_dtype=dt, max_batch=plan_batch)
    if kind == "standard":
        m = P.StandardResNetCNN(12, **kw)
    elif kind == "attention":
        m = P.AttentionHierarchicalCNN(12, **kw)
    elif kind == "cnn_lstm":
        m = P.CnnLstm(12, sequence_length=SEQ, **kw)
        m._seq_len_bound = SEQ      # what forward() sets before it builds the engine
    elif kind in ("image_only", "numerical_only"):   # frozen backbone, as in test_frozen_backbone_modes_*
        m = P.QuadtreeCNN(12, mode=kind, freeze_backbone=True, **kw)
    else:
        m = P.QuadtreeCNN(12, **kw)
    m.load_state_dict(synth.synth_state_dict(m))
    m = m.to(dev).train()
    with plan_guard_gap(gap):
        eng = m._ensure_engine(plan_batch, dev)
    assert eng.max_batch == plan_batch
    return m


def _data(kind, batch, salt=5):
    synth = pkg("synth")
    dev = _dev()
    x, f = synth.synth_images(batch, salt=salt), synth.synth_pose_features(batch, salt=salt)
    if kind == "cnn_lstm":      # inputs as in tests/test_cnn_lstm_gpu.py: [sequences][frames]...
        x, f = x.view(batch // SEQ, SEQ, 3, 224, 224), f.view(batch // SEQ, SEQ, 47)
    y = synth.synth_labels(x.shape[0], 12, salt=salt)
    return x.to(dev), f.to(dev), y.to(dev)


ROWS = [
    # kind, dtype, plan batch, run batch, d(loss)/d(image)
    ("quadtree", BF16, 2, 2, False),
    ("quadtree", BF16, 4, 4, False),
    ("quadtree", BF16, 16, 16, False),
    ("quadtree", BF16, 18, 18, False),
    ("quadtree", BF16, 48, 48, False),
    ("quadtree", F32, 2, 2, False),         # the f32 build gives every 3x3 a slice of the `dw` region
    ("quadtree", F32, 16, 16, False),
    ("image_only", BF16, 2, 2, False),      # layouts without the numerical branch ...
    ("numerical_only", BF16, 2, 2, False),  # ... or without the image buffers
    ("standard", BF16, 2, 2, False),        # no quadrant head, fused_ld 512
    ("standard", BF16, 16, 16, False),
    ("attention", BF16, 2, 2, False),       # gbase_tmp2, the attention.* buffers
    ("attention", BF16, 16, 16, False),
    ("cnn_lstm", BF16, 8, 8, False),        # the LSTM buffers: 2 sequences of 4 frames
    ("cnn_lstm", BF16, 16, 16, False),      # 4 sequences
    ("quadtree", BF16, 16, 16, True),       # qt_plan_backward_dx / qt_stem_dgrad
    ("quadtree", BF16, 18, 5, False),
]


def _id(row):
    kind, dt, plan_batch, batch, dx = row
    return f"{kind}-{'bf16' if dt == BF16 else 'f32'}-{batch}" + (f"of{plan_batch}" if batch != plan_batch else "") + \
        ("-dx" if dx else "")


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_plan_gaps_stay_intact(row):
    kind, dt, plan_batch, batch, dx = row
    dev = _dev()
    plain, gapped = _model(kind, dt, plan_batch, 0), _model(kind, dt, plan_batch, GAP_BYTES)
    guard = Guard(dev)
    gaps = PlanGaps(gapped, guard)
    # the same regions as the plain twin's, GAP_BYTES apart
    names = [(n, b) for n, _, b in gaps.table]
    assert names == [(n, b) for n, _, b in region_table(plain._engine.L, plain._engine.handle)]
    assert gaps.ws.numel() == plain._engine.workspace_bytes + len(names) * GAP_BYTES
    assert all(hi - lo >= GAP_BYTES for _, _, lo, hi in gaps.gaps)
    gaps.check()
    data = _data(kind, batch)
    # (small = 1: the first image, or the first sequence of CnnLstm)
    want, got = plan_run([plain, gapped], [torch.cuda.synchronize, gaps.check], share_grads=(dt == F32), data=data,
                         small=1, image_grad=dx)
    assert ("plain/grad/image" in got) == dx
    # the launches wrote into this workspace: the classifier's input is no longer the fill
    (off, size), = [(o, b) for n, o, b in gaps.table if n == "fused"]
    assert not bool((gaps.ws[off:off + size] == POISON).all())
    compare_twins(want, got, dt)
