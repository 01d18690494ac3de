"""The stage loop and the tile start of the 256-query persistent kernel (fused_f16p12.h, pvar 3) at the stage counts and
tile sequences that its instruction order depends on.  The kernel issues a stage's held pair of MFMAs right behind the stage
barrier with the stage's first reads between them, spreads the later reads under the MFMAs and keeps byte addresses that
move from ring slot to ring slot; none of that may change a bit, so:

  * split form: pvar 3 bit-equal to pvar 2 (fused_f16p.h, the kernel it is derived from) at d = 128, 160, 224 -- 4, 5 and 7
    stages: an even count (the single-stage tail) and odd counts (no tail), first-stage ring slots 1, 2, 1 after one tile --
    with a ragged last query tile and a ragged last support tile, on 8 workgroups (many tiles per workgroup);
  * run tables: a workgroup's consecutive tiles have 1, 2, 3 and more than 3 runs in turn (the table entries are loaded
    under the tile's first stage), with the tables in the bank and with tables built by the launch into a scratch buffer
    filled with 0xFF, so an entry read past the tables' end would show;
  * half-precision rows (HALF) against the fp64 oracle on the rounded operands, bound of test_half_bank_gpu.py;
  * the candidate form (CAND, nw_knn_f16) under the conditions of test_knn_half_gpu.py;
  * two calls give the same bits.

Shapes.  B = 300, N = 4 * 128 * 8 + 80 is the small ragged shape.  A split-operand forward of that size does NOT take a
persistent kernel (plan_fused in fused.hip asks for 4 * CUs 64-query tiles and 1024 tiles), whatever NW_PVAR says; the half
and candidate forms always do.  The split-form cases therefore run at that shape (it stays equal, by the other kernel) AND
at B = 1030, N = 7757 (5 query tiles, the last with 6 rows; 61 support tiles, the last with 77 rows), the smallest shape of
test_persistent_schedule_gpu.py, where the library's own plan is asserted to be the persistent kernel of the forced variant.

Every forward writes its partials through a scratch buffer filled with 0xFF (tests/ws_poison.py) into a poisoned row.
"""
import os

import numpy as np
import pytest
import torch

import ws_poison
from persistent_schedule import BS, assert_persistent, decode, n_local
from test_half_bank_gpu import _round_rows
from test_knn_half_gpu import _check, _scores64

pytestmark = pytest.mark.gpu

RTOL = 1e-5
C = 200
SMALL = (300, 4 * 128 * 8 + 80)
LARGE = (1030, 7757)
WGS = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from nwhead_amd import _lib
    _lib.check(_lib.load().nw_device_check(), "nw_device_check")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


@pytest.fixture(scope="module")
def O():
    from oracle import nw_oracle
    return nw_oracle


@pytest.fixture
def pvar():
    """set(v) forces the persistent kernel's tile variant; the knob is unset again after the test."""
    from nwhead_amd import _lib
    _lib.load()
    before = os.environ.get("NW_PVAR")

    def set_(v):
        os.environ["NW_PVAR"] = str(v)
        _lib.sync_knobs()

    yield set_
    if before is None:
        os.environ.pop("NW_PVAR", None)
    else:
        os.environ["NW_PVAR"] = before
    _lib.sync_knobs()


def _inputs(B, N, d, dev):
    g = torch.Generator().manual_seed(1000 * B + N + d)
    q = (torch.randn(B, d, generator=g) * 0.7).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    return q, s, g


def _ls(kind, dev):
    return torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev) if kind == "clip" else None


RUNS = {1: (128,), 2: (50, 78), 3: (40, 40, 48), 5: (20, 20, 30, 30, 28)}


def _stepped_labels(N):
    """Class-sorted labels; support tile t has RUNS[...][(t + t // 8) % 4] runs, so the tiles t, t + 8, t + 16, ... that
    one workgroup walks have 1, 2, 3 and 5 runs in turn.  Returns (labels, runs per tile)."""
    cats = (1, 2, 3, 5)
    y, c, per_tile = [], 0, []
    for t in range(-(-N // BS)):
        lens = RUNS[cats[(t + t // 8) % 4]]
        for n in lens:
            y.append(torch.full((n,), c, dtype=torch.int64))
            c += 1
    y = torch.cat(y)[:N]
    assert int(y.max()) < C
    per_tile = [len(torch.unique_consecutive(y[a:a + BS])) for a in range(0, N, BS)]
    return y, per_tile


def _forward(dev, ops, q, s, sy, bank, kind, wgs=WGS):
    """One forward on `wgs` workgroups: partials through a poisoned scratch buffer into a poisoned row, then the merge."""
    B, (N, d) = q.shape[0], s.shape
    need = ws_poison.fwd_workspace_bytes(B, N, d, C)
    ws_poison.poison_cached_workspaces()
    L = 2 * B + B * C
    packed = ws_poison.poisoned_workspace(4 * L, dev).view(torch.float32)
    ws = ws_poison.poisoned_workspace(need, dev)
    ops.nw_partials_into(packed, q, s, sy, C, kind, _ls(kind, dev), ws=ws, cache=bank, persistent_wgs=wgs)
    out = ops.nw_merge(packed.view(1, L), B, C)
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all(), "partials: a slot was not written (or holds poison read from the workspace)"
    assert out.shape == (B, C) and torch.isfinite(out).all()
    return out


def _p3_and_p2(dev, ops, pvar, q, s, sy, bank, kind):
    B, (N, d) = q.shape[0], s.shape
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    outs = {}
    for v in (2, 3):
        pvar(v)
        if (B, N) == LARGE:
            assert assert_persistent(B, N, d, cus, variant=v, wgs=WGS).workgroups == WGS
        outs[v] = _forward(dev, ops, q, s, sy, bank, kind).clone()
    assert torch.equal(outs[3], outs[2]), \
        f"{(outs[3] != outs[2]).sum().item()} of {outs[3].numel()} differ, max |diff| {(outs[3] - outs[2]).abs().max().item():.3e}"
    return outs[3]


# ------------------------------------------------------------------------------------------------ split form: pvar 3 == pvar 2
@pytest.mark.parametrize("kind", ["euclidean", "cosine"])
@pytest.mark.parametrize("sorted_labels", [True, False], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("d", [128, 160, 224])
@pytest.mark.parametrize("B,N", [SMALL, LARGE], ids=["small", "large"])
def test_split_form_equals_the_128_query_kernel(dev, ops, pvar, B, N, d, sorted_labels, kind):
    q, s, g = _inputs(B, N, d, dev)
    sy = torch.arange(N) % C
    sy = (sy.sort().values if sorted_labels else sy[torch.randperm(N, generator=g)]).to(dev)
    bank = ops.SplitBank(s)            # no tables in the bank: the launch builds them (shuffled: ~128 runs per tile)
    assert bank.split is not None and bank.tables is None
    _p3_and_p2(dev, ops, pvar, q, s, sy, bank, kind)


# ----------------------------------------------------------------------------------- run counts that change from tile to tile
@pytest.mark.parametrize("tables", ["bank", "launch"])
@pytest.mark.parametrize("d", [128, 160])
def test_run_counts_change_between_consecutive_tiles(dev, ops, pvar, d, tables):
    B, N = LARGE
    sy, per_tile = _stepped_labels(N)
    n_stiles, n_qtiles = len(per_tile), -(-B // 256)
    assert set(per_tile[:-1]) == {1, 2, 3, 5}
    # the one workgroup of XCD 0 (8 workgroups): its list, decoded by the model of the kernel's tile order (group size 4)
    walk = [per_tile[decode(L, 0, n_stiles, n_qtiles, 4)[1]] for L in range(n_local(n_stiles, n_qtiles, 0))]
    changes = {(a, b) for a, b in zip(walk[:-1], walk[1:]) if a != b}
    assert {(1, 2), (2, 3), (3, 5), (5, 1)} <= changes, changes
    q, s, _ = _inputs(B, N, d, dev)
    sy = sy.to(dev)
    bank = ops.SplitBank(s)
    if tables == "bank":
        bank.build_tables(sy)
        assert bank.tables is not None
    out = _p3_and_p2(dev, ops, pvar, q, s, sy, bank, "euclidean")
    # once more, through freshly poisoned buffers: nothing came from a table entry or a partial of the call before
    assert torch.equal(_forward(dev, ops, q, s, sy, bank, "euclidean"), out)


# --------------------------------------------------------------------------------------------------------- half-precision rows
@pytest.mark.parametrize("kind", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [192, 320])
def test_half_form_against_the_oracle_on_rounded_operands(dev, ops, O, d, kind):
    B, N = SMALL
    q, s, _ = _inputs(B, N, d, dev)
    sy = _stepped_labels(N)[0].to(dev)
    bank = ops.SplitBank(s, labels=sy, precision="fp16")
    assert bank.packed is not None and bank.split is None and bank.pad == 0 and bank.tables is not None
    out = _forward(dev, ops, q, s, sy, bank, kind)
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]
    ref = torch.cat([O.nw_head_f64(q_r[a:a + 16], s_r, sy, C, kind) for a in range(0, B, 16)])
    smax = O.scores_f64(q_r[:64], s_r, kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
    atol = max(3e-5, 3e-6 * smax)
    print(f"half d {d} {kind}: max|err| {(out.double() - ref).abs().max().item():.3e} (atol {atol:.1e})")
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=atol)


# -------------------------------------------------------------------------------------------------------------- candidate form
def test_candidate_form(dev, ops, O):
    (B, N), d, k = SMALL, 192, 8
    q, s, _ = _inputs(B, N, d, dev)
    bank = ops.SplitBank(s, precision="fp16")
    assert bank.packed is not None and bank.sorted_rows is None
    res = [ops.nw_knn(q, bank, k, "euclidean", None, return_values=True, rounded=True, persistent_wgs=w) for w in (WGS, WGS, 0)]
    torch.cuda.synchronize()
    _check(res[0][0], res[0][1], _scores64(O, q, s, "euclidean"), k)
    for idx, val in res[1:]:
        assert torch.equal(idx, res[0][0]) and torch.equal(val.view(torch.int32), res[0][1].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- reproducibility
def test_two_calls_give_the_same_bits(dev, ops, pvar):
    B, N = LARGE
    d = 224
    q, s, g = _inputs(B, N, d, dev)
    sy = (torch.arange(N) % C)[torch.randperm(N, generator=g)].to(dev)
    bank = ops.SplitBank(s)
    pvar(3)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert_persistent(B, N, d, cus, variant=3, wgs=WGS)
    a = _forward(dev, ops, q, s, sy, bank, "euclidean").clone()
    b = _forward(dev, ops, q, s, sy, bank, "euclidean")
    assert torch.equal(a, b)
