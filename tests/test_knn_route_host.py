"""ops.knn_route, the one route rule of the neighbour search, over a table of plain facts (no GPU, no bank objects): one row
per distinct outcome, and the rows in which two callers answer differently for the same bank and search.  The callers'
policies: nw_knn passes no gates (and so a ShardedBank, which asks no rule of its own: it always calls nw_knn); KNN.indices
and NWNet.get_neighbors pass size_gate and need_n4."""
import pytest

from nwhead_amd import ops

F32 = dict(precision="fp32", packed=False, split=True, sorted_copy=False, shape=(40, 64), pad=0, width=64, B=3, k=5)
F16 = dict(precision="fp16", packed=True, split=False, sorted_copy=False, shape=(40, 192), pad=0, width=192, B=3, k=5)
GATES = dict(size_gate=True, need_n4=True)
BIG = dict(B=4096, shape=(1 << 16, 64))      # a (B, N) score matrix of 1 GiB: the size gate's threshold

ROWS = [
    # ---- nw_knn (no gates)
    ("fused", F32, {}),
    ("fused", F32, dict(matches=True)),
    ("matrix: another tensor", F32, dict(matches=False), "matrix"),
    ("matrix: k > 32", F32, dict(k=33), "matrix"),
    ("matrix: class-sorted copy", F32, dict(sorted_copy=True), "matrix"),
    ("matrix: norms only", F32, dict(split=False, shape=(40, 40), width=40), "matrix"),
    ("matrix: N <= 25", F32, dict(shape=(25, 64)), "matrix"),
    ("matrix: no queries", F32, dict(B=0), "matrix"),
    ("matrix: width does not pad to the bank's", F32, dict(width=60), "matrix"),
    ("matrix: the size rule picks the fp32 kernel", F32, dict(use_split=False), "matrix"),
    ("fused: N % 4 != 0 without need_n4", F32, dict(shape=(42, 64)), "fused"),
    ("fused: padded queries", F32, dict(shape=(40, 96), pad=24, width=72), "fused"),
    ("fp16 bank, fp32 search", F16, {}, "matrix"),
    ("rounded", F16, dict(search_precision="fp16"), "rounded"),
    ("rounded: padded queries", F16, dict(search_precision="fp16", pad=92, width=100), "rounded"),
    ("rounded asked of an fp32 bank", F32, dict(search_precision="fp16"), "fused"),
    ("rounded: norms only", F16, dict(search_precision="fp16", packed=False, shape=(20, 192)), "matrix"),
    ("rounded: class-sorted copy", F16, dict(search_precision="fp16", sorted_copy=True), "matrix"),
    ("rounded: k > 32", F16, dict(search_precision="fp16", k=33), "matrix"),
    ("rounded: width", F16, dict(search_precision="fp16", width=100), "matrix"),
    # ---- KNN.indices / NWNet.get_neighbors (size_gate, need_n4): the same banks, other answers
    ("gated: small score matrix", F32, GATES, None),
    ("gated: at the threshold", F32, dict(GATES, **BIG), "fused"),
    ("gated: one query below it", F32, dict(GATES, B=4095, shape=(1 << 16, 64)), None),
    ("gated: k > 32 stays the caller's", F32, dict(GATES, k=33, **BIG), None),
    ("gated: N % 4 != 0 stays the caller's", F32, dict(GATES, B=4096, shape=((1 << 16) + 2, 64)), None),
    ("gated: norms only, nw_knn's nw_topk ranks", F32, dict(GATES, split=False, **BIG), "matrix"),
    ("gated: fp16 bank, fp32 search", F16, dict(GATES, B=4096, shape=(1 << 16, 192)), "matrix"),
    ("gated: the rounded search has no size gate", F16, dict(GATES, search_precision="fp16"), "rounded"),
    ("gated: ... and no N % 4 rule", F16, dict(GATES, search_precision="fp16", shape=(42, 192)), "rounded"),
    ("gated: rounded refused (k > 32)", F16, dict(GATES, search_precision="fp16", k=33), None),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_route(row):
    name, base, change = row[:3]
    want = row[3] if len(row) > 3 else "fused"
    assert ops.knn_route(**dict(base, **change)) == want


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_size_rule_only_turns_fused_into_matrix(row):
    """What knn_route_for relies on to ask the library's size rule only after a "fused" answer."""
    facts = dict(row[1], **row[2])
    with_split, without = ops.knn_route(**dict(facts, use_split=True)), ops.knn_route(**dict(facts, use_split=False))
    assert without == ("matrix" if with_split == "fused" else with_split)


def test_every_outcome_has_a_row():
    assert {(r[3] if len(r) > 3 else "fused") for r in ROWS} == {"rounded", "fused", "matrix", None}


def test_gate_follows_the_module_threshold(monkeypatch):
    """The size gate reads ops.KNN_FUSED_MIN_SCORE_BYTES when asked (tests and tools patch it)."""
    assert ops.knn_route(**F32, **GATES) is None
    monkeypatch.setattr(ops, "KNN_FUSED_MIN_SCORE_BYTES", 0)
    assert ops.knn_route(**F32, **GATES) == "fused"
    assert ops.knn_route(**dict(F32, k=33), **GATES) is None


def test_rounded_refusal_is_the_route_rule():
    """knn_rounded_refusal (the text nw_knn(rounded=True) raises with) and the "rounded" route are one rule."""
    class Bank:
        precision, packed, sorted_rows, shape, pad = "fp16", object(), None, (40, 192), 0
    assert ops.knn_rounded_refusal(Bank, 5, 192) is None
    assert "k = 33 > 32" in ops.knn_rounded_refusal(Bank, 33, 192)
    assert "width 100" in ops.knn_rounded_refusal(Bank, 5, 100)
    Bank.packed = None
    assert "norms-only" in ops.knn_rounded_refusal(Bank, 5, 192)
