#!/usr/bin/env python3
"""Generate tests/golden/seq_windows.npz by RUNNING THE REFERENCE's own two window scripts on the CPU, on temporary directories
(developer aid; no test and no GPU run reads the reference checkout).

    python tests/golden/make_seq_windows_golden.py <path of the reference checkout>

Imports by path and drives, without restating either loop:
  "sqn process/create_sequential_dataset.py"      create_dataset_sequences() on small feature CSVs, frame maps and label CSVs
      (pandas as it is; the annotated images are absent, the script only warns).  SEQUENCE_LENGTH is set to 4, the stride is
      the script's own 1.  Frames without a label (no entry in the label CSV, or the string "nan") are dropped by the script
      before it windows.  Read back: dataset_metadata.json (clip, start index, label) and every sequence's features.npy.
  "cnn+lstm/prepare_sequential_dataset.py"        process_view_sequence() per clip on tiny PNGs and stored 47-float .npy rows,
      with SEQ_LEN 4 and STRIDE 2, `torchvision.transforms` stubbed in sys.modules and a transform that returns one zero.
      One label string is left out of class_to_idx: a last frame of an unknown class.  Read back: every .pt file's start
      index (from its name), label and numerical_sequence.
Only data is written.  Column 0 of every numerical row is the frame's number in the table as given (before the reference's
filtering), so the stored rows say which frames each window was made of.  Keys, for rule in ("uniform", "last"):
  <rule>_T, <rule>_stride, <rule>_num_classes
  <rule>_labels [N] int64, <rule>_lengths [C]     per-frame labels and clip lengths AFTER the reference's own filtering
  <rule>_rows [N,F]                               the frames' numerical rows, same filtering
  <rule>_starts [W] int32, <rule>_window_labels [W] int64     in the reference's order
  <rule>_stored [W,T,F]                           features.npy / numerical_sequence as the reference stored them
  uniform_labels_given [M], uniform_lengths_given [C], uniform_rows_given [M,F]   before the filtering, -1 = no label
  clips                                           clip names with what each is for
"""
import importlib.util
import io
import json
import os
import re
import sys
import tempfile
import types
import contextlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T = 4
FEATURE_COLUMNS = ["FRAME_NUMBER", "LEFT_ELBOW_ANGLE", "DIST_LR_WRIST_NORM", "LM0_vx_px", "TORSO_VAR_XY_RATIO"]


def load(checkout, relative, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(checkout, *relative))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def uniform_clips():
    """(name, labels): a label string per frame, None = no entry in the label CSV, "nan" = the string the script filters"""
    A, B, C = "Tadasana", "Bhujangasana", "Padahastasana"
    return [
        ("clip_00_shorter_than_T", [A] * 3),
        ("clip_01_exactly_T", [B] * 4),
        ("clip_02_T_plus_1", [C] * 5),
        ("clip_03_label_change_mid_clip", [A] * 5 + [B] * 5),                       # starts 0, 1, 5, 6
        ("clip_04_unlabelled_frames_bridged", [A] * 3 + [None, "nan"] + [A] * 3),     # six frames remain: starts 0, 1, 2
        ("clip_05_unlabelled_between_classes", [C, C, C, C, None, B, B, B, B, None]),
        ("clip_06_no_labelled_frame", [None] * 4),                                  # skipped by the script altogether
        ("clip_07_changes_every_three", [A] * 3 + [B] * 3 + [C] * 3),                # no window
    ]


def run_uniform(checkout, rng):
    import pandas as pd
    ref = load(checkout, ("sqn process", "create_sequential_dataset.py"), "_reference_create_sequential_dataset")
    ref.SEQUENCE_LENGTH = T
    cases = uniform_clips()
    given_labels, given_rows, number = [], [], 0
    with tempfile.TemporaryDirectory() as tmp:
        processed, renamed, final = (os.path.join(tmp, d) for d in ("processed", "renamed", "final"))
        label_rows = []
        for name, labels in cases:
            os.makedirs(os.path.join(processed, "train", f"{name}_annotated_images"))
            os.makedirs(os.path.join(renamed, "train", name))
            rows, frame_map = [], []
            for t, label in enumerate(labels):
                values = rng.integers(0, 4096, len(FEATURE_COLUMNS)) / 64.0     # (short decimals: the CSV gives them back exactly)
                values[rng.random(len(FEATURE_COLUMNS)) < 0.2] = np.nan
                values[0] = number
                new, long = f"frame_{t:05d}.jpg", f"{name}_mp4-{t:04d}_jpg.rf.{number:08x}.jpg"
                rows.append({"clip_id": name, "frame_index": t, "original_image_filename": new,
                             **dict(zip(FEATURE_COLUMNS, values)), "annotated_image_path": f"{name}/{new}"})
                frame_map.append({"new_filename": new, "original_filename": long})
                if label is not None:
                    label_rows.append({"filename": long, "label": label})
                given_labels.append(label)
                given_rows.append(values)
                number += 1
            # the script sorts by frame_index itself: hand the frames over in reverse
            pd.DataFrame(rows[::-1]).to_csv(os.path.join(processed, "train", f"{name}_features.csv"), index=False)
            pd.DataFrame(frame_map).to_csv(os.path.join(renamed, "train", name, f"{name}_frame_map.csv"), index=False)
        csv = os.path.join(tmp, "labels.csv")
        pd.DataFrame(label_rows).to_csv(csv, index=False)
        with contextlib.redirect_stdout(io.StringIO()):
            ref.create_dataset_sequences(processed, [csv], renamed, final)
        meta = json.load(open(os.path.join(final, "dataset_metadata.json")))
        stored = [np.load(os.path.join(final, m["path"], "features.npy")) for m in meta]
    classes = {m["class_label_string"]: m["class_label_int"] for m in meta}
    names = sorted({l for _, labels in cases for l in labels if l not in (None, "nan")})
    assert all(classes[n] == names.index(n) for n in classes), "the script numbers the sorted label strings"
    # the table after the script's filtering, from the inputs; that the script saw it the same way is checked on what it stored
    kept = [l not in (None, "nan") for l in given_labels]
    lengths_given = [len(labels) for _, labels in cases]
    bounds = np.concatenate([[0], np.cumsum(lengths_given)])
    lengths = [int(np.sum(kept[a:b])) for a, b in zip(bounds[:-1], bounds[1:])]
    begin = dict(zip((name for name, _ in cases), np.concatenate([[0], np.cumsum(lengths)])[:-1]))
    rows = np.array(given_rows)[kept]
    labels = np.array([names.index(l) for l, k in zip(given_labels, kept) if k], dtype=np.int64)
    starts = np.array([begin[m["source_clip_name"]] + m["start_frame_index"] for m in meta], dtype=np.int32)
    stored = np.stack(stored)
    assert stored.shape == (len(meta), T, len(FEATURE_COLUMNS))
    for s, rows_stored in zip(starts, stored):
        assert np.array_equal(rows_stored, rows[s:s + T], equal_nan=True), "a stored window is T consecutive filtered frames"
    return {
        "uniform_T": T, "uniform_stride": 1, "uniform_num_classes": len(names),
        "uniform_labels": labels, "uniform_lengths": np.array(lengths, dtype=np.int64), "uniform_rows": rows,
        "uniform_starts": starts, "uniform_window_labels": np.array([m["class_label_int"] for m in meta], dtype=np.int64),
        "uniform_stored": stored,
        "uniform_labels_given": np.array([names.index(l) if l in names else -1 for l in given_labels], dtype=np.int64),
        "uniform_lengths_given": np.array(lengths_given, dtype=np.int64), "uniform_rows_given": np.array(given_rows),
    }, [name for name, _ in cases]


def last_clips():
    A, B, X = "Tadasana", "Bhujangasana", "Unlisted pose"
    return [
        ("video_clip_001", "shorter_than_T", [A] * 3),
        ("video_clip_002", "exactly_T", [B] * 4),
        ("video_clip_003", "T_plus_1", [A] * 5),                                   # stride 2: start 0 only
        ("video_clip_004", "odd_remainder", [A, B, A, B, A, B, A]),                # starts 0, 2; frame 6 is in no window
        ("video_clip_005", "label_change_mid_clip", [A] * 5 + [B] * 5),            # starts 0, 2, 4, 6: the last frame decides
        ("video_clip_006", "last_frame_of_unknown_class", [A, A, A, X, B, X, B, B, B]),   # start 0 ends on X, 2 on X, 4 on B
        ("video_clip_007", "label_with_spaces", [" " + A + " "] * 6),              # the script strips it
    ]


def run_last(checkout, rng):
    import torch
    from PIL import Image
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    ref = load(checkout, ("cnn+lstm", "prepare_sequential_dataset.py"), "_reference_prepare_sequential_dataset")
    ref.SEQ_LEN, ref.STRIDE = T, 2
    cases = last_clips()
    class_to_idx = {"Bhujangasana": 0, "Tadasana": 1}
    rows, labels, lengths, starts, window_labels, stored = [], [], [], [], [], []
    number = 0
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out")
        for clip, what, clip_labels in cases:
            frames = []
            for t, label in enumerate(clip_labels):
                row = rng.random(47).astype(np.float32)
                row[rng.random(47) < 0.2] = np.nan
                row[0] = number
                png, npy = os.path.join(tmp, f"{clip}_{t}.png"), os.path.join(tmp, f"{clip}_{t}.npy")
                Image.fromarray(np.full((2, 2, 3), t, np.uint8)).save(png)
                np.save(npy, row)
                frames.append({"frame_idx": 10 * t, "img_path": png, "npy_path": npy, "label": label})
                rows.append(row)
                labels.append(class_to_idx.get(label.strip(), -1))
                number += 1
            begin = sum(lengths)
            lengths.append(len(clip_labels))
            saved = ref.process_view_sequence(clip, "01", frames[::-1], out, "train", class_to_idx,
                                              lambda image: torch.zeros(1))      # (the script sorts by frame_idx itself)
            found = []
            for root, _, files in os.walk(out):
                for f in files:
                    m = re.fullmatch(rf"{clip}_view_01_seq_(\d+)\.pt", f)
                    if m:
                        found.append((int(m.group(1)), os.path.join(root, f)))
            assert len(found) == saved
            for i, path in sorted(found):
                item = torch.load(path)
                starts.append(begin + i)
                window_labels.append(int(item["label"]))
                stored.append(item["numerical_sequence"].numpy())
    rows, stored = np.stack(rows), np.stack(stored)
    for s, rows_stored in zip(starts, stored):
        assert np.array_equal(rows_stored, rows[s:s + T], equal_nan=True)
    return {
        "last_T": T, "last_stride": 2, "last_num_classes": len(class_to_idx),
        "last_labels": np.array(labels, dtype=np.int64), "last_lengths": np.array(lengths, dtype=np.int64), "last_rows": rows,
        "last_starts": np.array(starts, dtype=np.int32), "last_window_labels": np.array(window_labels, dtype=np.int64),
        "last_stored": stored,
    }, [f"{clip}_{what}" for clip, what, _ in cases]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    rng = np.random.default_rng(20240607)
    uniform, uniform_names = run_uniform(sys.argv[1], rng)
    last, last_names = run_last(sys.argv[1], rng)
    out = os.path.join(HERE, "seq_windows.npz")
    np.savez_compressed(out, **uniform, **last, clips=np.array(uniform_names + last_names))
    print(f"{out}: {len(uniform['uniform_starts'])} uniform windows of {len(uniform['uniform_labels'])} frames, "
          f"{len(last['last_starts'])} last-label windows of {len(last['last_labels'])} frames, {os.path.getsize(out)} bytes")
    print("uniform starts", uniform["uniform_starts"].tolist(), "labels", uniform["uniform_window_labels"].tolist())
    print("last starts", last["last_starts"].tolist(), "labels", last["last_window_labels"].tolist())


if __name__ == "__main__":
    main()
