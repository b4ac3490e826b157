"""The inventory of capped grid-stride launches (tests/_grid_caps.py), without a GPU: every chosen shape does what its row
claims (some walkers take one trip more than the others; the pair loops at three totals: body entered by some, tail taken by
some, back edge taken by some), the table has one row per `qt_grid_for(` call site of csrc/*.hip, every test a row names
exists, the periodic cases cannot hide a wrong trip offset, no case needs more than 4 GiB.  trips() is held against the loops
walked index by index and against the path tables the stem and pool3d tests already have."""
import os
import re

import pytest

import _grid_caps as G
import _pool3d_bounds as Pb
import _stem_bounds as Sb

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(r, c) for r in G.ROWS for c in r["cases"]]
_id = lambda rc: f"{rc[0]['kernel']}-{'-'.join(f'{k}{v}' for k, v in rc[1]['shape'].items())}"


def _holds(row, case, total=None):
    t = G.trips(case["total"] if total is None else total, G.block_of(row, case), row["cap"], row["loop"], row["unit"])
    if not t["grid"] == row["cap"]:
        return False
    want = case["want"]
    if row["loop"] != "pair":
        return want == "some" and t["crossed"]
    if want == "pair_some":      # between 1 and 2 strides: only some walkers enter the pair body
        return t["k"] == 1 and t["pair_body"] == (True, True)
    if want == "tail_some":      # between 2 and 3: all enter it, some take the tail, none the back edge
        return t["k"] == 2 and t["pair_body"] == (True, False) and t["tail"] == (True, True) and t["back_edge"] == (False, True)
    return want == "back_edge" and t["k"] >= 3 and t["back_edge"] == (True, True)


@pytest.mark.parametrize("rc", CASES, ids=_id)
def test_the_chosen_shape_does_what_the_row_claims(rc):
    row, case = rc
    assert _holds(row, case), G.case_trips(row, case)
    # .. and the check can fail: the same row one item under its cap, and at exactly one stride
    full = row["cap"] * G.block_of(row, case)
    assert not _holds(row, case, full) and not _holds(row, case, full - 1)
    assert case["bytes"] <= G.GIB4, case["bytes"]


@pytest.mark.parametrize("row", [r for r in G.ROWS if r["loop"] == "pair"], ids=lambda r: r["kernel"])
def test_pair_rows_have_their_three_totals(row):
    have = {c["want"] for c in row["cases"]}
    if row["kernel"] == "stem_bn_bwd_sums_light_kernel":   # the middle one is B = 11 of the stem tests: the table names it
        assert have == {"back_edge"} and "B = 11" in row["note"] and Sb.paths(11)["light_tail"]
        for B in range(1, 11):     # not capped: the stride is the number of 8-channel groups, the total twice that
            assert Sb.sums_rows(B) < 1024 and B * 56 * 56 * 16 == 2 * Sb.sums_rows(B) * 256
        assert Sb.sums_rows(11) == 1024
        t = G.trips(11 * 56 * 56 * 16, 256, 1024, "pair")
        assert t["k"] == 2 and t["tail"] == (True, True) and t["back_edge"] == (False, True)
    else:
        assert have == {"pair_some", "tail_some", "back_edge"}


def test_one_row_per_call_site():
    """a capped launch cannot be added without a row: the count of one identifier in each source, read as text"""
    sites = G.call_sites()
    rows = {}
    for r in G.ROWS:
        if r["site"]:
            rows[r["file"]] = rows.get(r["file"], 0) + 1
    assert sites == rows, (sites, rows)
    assert set(sites) == {"elementwise.hip", "attention.hip", "lstm.hip", "pack.hip", "lstm_stream.hip", "video3d.hip", "metrics.hip",
                          "scores.hip"}
    for name in ("stem_bwd_rows", "stem_sums_rows"):      # the hand-written caps have rows as well
        assert any(name in r["total"] for r in G.ROWS if not r["site"])
    assert sum(r["not_reached"] is not None for r in G.ROWS) <= G.NOT_REACHED_MAX


def _defined(module, test):
    return re.search(rf"^def {re.escape(test)}\(", open(os.path.join(HERE, module + ".py")).read(), re.M) is not None


def test_every_named_test_exists():
    gpu = open(os.path.join(HERE, "test_grid_caps_gpu.py")).read()
    named = set()
    for r in G.ROWS:
        if r["not_reached"] is not None:
            continue
        if r["covered_by"]:
            module, test = re.match(r"(\w+)::(\w+)", r["covered_by"]).groups()
            assert _defined(module, test), r["covered_by"]
        else:
            assert _defined("test_grid_caps_gpu", r["gpu_test"]), r["gpu_test"]
            named.add(r["gpu_test"])
    assert set(re.findall(r"^def (test_\w+)\(", gpu, re.M)) == named      # and no GPU test without a row
    # the shapes the covering tests use are the table's
    import _bounds as Bd
    import _head_bounds as Hb
    assert (Bd.LARGE_M, Bd.LARGE_C) == (G.LARGE_M, 64) and Hb.REGION_LARGE == (335, 2, 196, 128)
    assert (262145, 8) in Hb.BN_SHAPES and (300000, 8) in Hb.BN_SHAPES and 11 in Sb.BATCHES
    assert (256, 256, 184, 192) in Pb.PACK_ELEMENT and Pb.pack_kernel(256, 256, 184, 192, 0) == "element"


@pytest.mark.parametrize("rc", [rc for rc in CASES if rc[1]["period"]], ids=_id)
def test_a_period_cannot_hide_a_wrong_trip_offset(rc):
    row, case = rc
    t = G.case_trips(row, case)
    assert not G.period_hidden(t["stride"], case["total"], case["period"])
    assert t["stride"] % case["period"] != 0 and case["period"] < case["total"]
    # .. and the check can fail: a period that divides the stride is refused
    assert G.period_hidden(t["stride"], case["total"], t["stride"] // 4)


def test_the_slab_sizes_are_prime():
    for p in (G.PRIME, G.QUAD_SLAB, G.STEM_SLAB):
        assert p > 1 and all(p % d for d in range(2, int(p ** 0.5) + 1))


@pytest.mark.parametrize("loop", ["plain", "pair"])
@pytest.mark.parametrize("total", [1, 255, 256, 511, 512, 513, 700, 1024, 1025, 1300, 1536, 1537, 1800, 2048, 2049, 2500])
def test_trips_equals_the_loop_walked_index_by_index(loop, total):
    """cap 2 x block 256: a stride of 512 items"""
    t = G.trips(total, 256, 2, loop)
    items, pairs, tail = G.simulate(total, t["stride"], loop)
    assert int(items.sum()) == total
    assert int((items == t["k"] + 1).sum()) == t["walkers_k1"] and int((items == t["k"]).sum()) == t["walkers_k"]
    if loop == "pair":
        assert t["pair_body"] == (bool((pairs >= 1).any()), bool((pairs < 1).any()))
        assert t["back_edge"] == (bool((pairs >= 2).any()), bool((pairs < 2).any()))
        assert t["tail"] == (bool(tail.any()), bool((~tail).any()))


def test_trips_agrees_with_the_path_tables_of_the_stem_and_pool3d_tests():
    for B in (1, 3, 6, 11, 16):
        p = Sb.paths(B)
        if Sb.sums_rows(B) == 1024:    # (below the cap the light kernel's grid is not the one its own total would give)
            t = G.trips(B * 56 * 56 * 16, 256, 1024, "pair")
            assert t["grid"] == 1024 and p["light_tail"] == t["tail"][0]
        else:
            assert not p["light_tail"]
        t = G.trips(B * 56 * 56 * 8, 256, 1024)
        assert p["sums_capped"] == (G.trips(B * 56 * 56 * 8, 256, 1024)["k"] >= 1 and t["grid"] == 1024)
        assert p["reduce_capped"] == (G.grid_for(B * 112 * 112 * 8, 256, 2048) == 2048 and B * 112 * 112 * 8 > 2048 * 256)
        assert G.grid_for(B * 112 * 112 * 8, 256, 2048) == Sb.reduce_rows(B)
    for total in (1, 4096 * 256, 4096 * 256 + 1, Pb.pack_total(256, 192, 0)):
        assert Pb.grid_strided(total) == (G.trips(total, 256, Pb.PACK_GRID_CAP)["k"] >= 1 and total > Pb.PACK_GRID_CAP * 256)
    assert Pb.pool_grid(G.POOL3D["T"] * G.POOL3D["B"] * 24 * 8) == Pb.POOL_GRID_CAP
