"""The tile turnaround of the 256-query persistent kernel (fused_f16p12.h, pvar 3): what it carries from one tile of a
workgroup's list to the next and what it makes once per tile.  The kernel issues tile T + 1's first eight fragment reads
from tile T's epilogue, decodes the tile order with reciprocals made once per launch, and takes the per-support-row score
factors from LDS, where a loader wave has made them from the tile's header (the distance kinds read them one 16-row block
ahead).  None of that may change a bit, and the cases also guard what a further step in this direction would touch (a tile
record loaded ahead of its tile, run sums by whole blocks):

  1. split form: pvar 3 bit-equal to pvar 2 (fused_f16p.h), every score kind, d = 96, 128, 160, 224 (3, 4, 5, 7 stages: the
     shortest tile, an even count with the single-stage tail, odd counts), at B = 1030, N = 7757 (the library's own plan is
     asserted persistent) and at B = 300, N = 4 * 128 * 8 + 80;
  2. a workgroup's consecutive tiles have 1, 2, 3, 5, 2 and 3 runs in turn, with run boundaries inside a 16-row block
     (rows 50; 69) and on a block's edge (rows 64; 32, 80): tile T's epilogue must use tile T's run count and boundaries, not
     the ones already loaded for tile T + 1.  Tables from the bank, and tables built by the launch into poisoned scratch;
  3. the ends of a workgroup's list, on half-precision rows (which always take this kernel) against the fp64 oracle on the
     rounded operands with the bound of test_half_bank_gpu.py: N = 3 * 128 and N = 128 on 8 workgroups (fewer than 8 support
     tiles: every tile is in the leftover part of the order, seven XCD lists are empty, one has three tiles or one; the last
     tile has no successor) and N = 128 * 8 * 2 + 5 (the last support tile has 5 rows);
  4. row scales and norms that differ from row to row by orders of magnitude, and rows of exactly zero norm: bit-equal to
     pvar 2, every score kind (the normalised kinds divide by max(|x|, eps));
  5. the candidate form (nw_knn_f16) under the conditions of test_knn_half_gpu.py at d = 192 and 256;
  6. two calls give the same bits.

Every forward runs on 8 workgroups (each walks many tiles) and writes its partials through a scratch buffer filled with
0xFF (tests/ws_poison.py) into a poisoned row.
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

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
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
    g = torch.Generator().manual_seed(1000 * B + N + d + 17)
    q = (torch.randn(B, d, generator=g) * 0.7).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    return q, s, g


def _ls(kind, dev):
    return torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev) if kind == "clip" else None


# run lengths of a 128-row support tile: boundaries inside a 16-row block (50; 69) and on a block's edge (64; 32, 80)
RUNS = ((128,), (50, 78), (40, 40, 48), (20, 20, 30, 30, 28), (64, 64), (32, 37, 59))


def _stepped_labels(N):
    """Class-sorted labels; support tile t has the runs RUNS[(t + 5 * (t // 8)) % 6], so the tiles t, t + 8, t + 16, ... that
    one workgroup walks have 1, 2, 3, 5, 2, 3 runs in turn.  Returns (labels, runs per tile)."""
    y, c = [], 0
    for t in range(-(-N // BS)):
        for n in RUNS[(t + 5 * (t // 8)) % len(RUNS)]:
            y.append(torch.full((n,), c, dtype=torch.int64))
            c += 1
    y = torch.cat(y)[:N]
    assert int(y.max()) < C
    return y, [len(torch.unique_consecutive(y[a:a + BS])) for a in range(0, N, BS)]


def _forward(dev, ops, q, s, sy, bank, kind, finite=True):
    """One forward on 8 workgroups: partials through a poisoned scratch buffer into a poisoned row, then the merge.
    Returns (log-probabilities, the packed partials)."""
    B, (N, d) = q.shape[0], s.shape
    need = ws_poison.fwd_workspace_bytes(B, N, d, C)
    ws_poison.poison_cached_workspaces()
    L = 2 * B + B * C
    packed = ws_poison.poisoned_workspace(4 * L, dev).view(torch.float32)
    ws = ws_poison.poisoned_workspace(need, dev)
    ops.nw_partials_into(packed, q, s, sy, C, kind, _ls(kind, dev), ws=ws, cache=bank, persistent_wgs=WGS)
    out = ops.nw_merge(packed.view(1, L), B, C)
    torch.cuda.synchronize()
    assert out.shape == (B, C)
    if finite:
        assert torch.isfinite(packed).all(), "partials: a slot was not written (or holds poison read from the workspace)"
        assert torch.isfinite(out).all()
    return out.clone(), packed.clone()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _p3_and_p2(dev, ops, pvar, q, s, sy, bank, kind, finite=True):
    """pvar 3 and pvar 2 give the same bits (partials and log-probabilities); returns pvar 3's log-probabilities."""
    B, (N, d) = q.shape[0], s.shape
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res = {}
    for v in (2, 3):
        pvar(v)
        if (B, N) == LARGE:
            assert assert_persistent(B, N, d, cus, variant=v, wgs=WGS).workgroups == WGS
        res[v] = _forward(dev, ops, q, s, sy, bank, kind, finite)
    for a, b, what in zip(res[3], res[2], ("log-probabilities", "partials")):
        assert _same_bits(a, b), f"{what}: {(a.view(torch.int32) != b.view(torch.int32)).sum().item()} of {a.numel()} differ"
    return res[3][0]


# ---------------------------------------------------------------------------------------------- 1. split form: pvar 3 == pvar 2
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [96, 128, 160, 224])
@pytest.mark.parametrize("B,N", [SMALL, LARGE], ids=["small", "large"])
def test_split_form_equals_the_128_query_kernel(dev, ops, pvar, B, N, d, kind):
    q, s, _ = _inputs(B, N, d, dev)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    bank = ops.SplitBank(s)            # no tables in the bank: the launch builds them
    assert bank.split is not None and bank.tables is None
    _p3_and_p2(dev, ops, pvar, q, s, sy, bank, kind)


# --------------------------------------------------------------------------------- 2. run counts that change from tile to tile
@pytest.mark.parametrize("tables", ["bank", "launch"])
@pytest.mark.parametrize("d", [128, 160])
def test_each_tile_uses_its_own_run_table_entries(dev, ops, pvar, d, tables):
    B, N = LARGE
    sy, per_tile = _stepped_labels(N)
    n_stiles, n_qtiles = len(per_tile), -(-B // 256)
    # the one workgroup of XCD 0 (8 workgroups): its list, decoded by the model of the kernel's tile order (group size 4)
    walk = [per_tile[decode(L, 0, n_stiles, n_qtiles, 4)[1]] for L in range(n_local(n_stiles, n_qtiles, 0))]
    changes = {(a, b) for a, b in zip(walk[:-1], walk[1:]) if a != b}
    assert {(1, 2), (2, 3), (3, 5), (5, 2), (3, 1)} <= changes, changes
    q, s, _ = _inputs(B, N, d, dev)
    sy = sy.to(dev)
    bank = ops.SplitBank(s)
    if tables == "bank":
        bank.build_tables(sy)
        assert bank.tables is not None
    _p3_and_p2(dev, ops, pvar, q, s, sy, bank, "euclidean")


# ------------------------------------------------------------------------------------------- 3. the ends of a workgroup's list
@pytest.mark.parametrize("kind", ["euclidean", "cosine"])
@pytest.mark.parametrize("N", [3 * 128, 128, 128 * 8 * 2 + 5])
def test_list_ends_on_half_precision_rows(dev, ops, O, N, kind):
    B, d = 256, 192
    q, s, _ = _inputs(B, N, d, dev)
    sy = _stepped_labels(N)[0].to(dev)
    bank = ops.SplitBank(s, labels=sy, precision="fp16")
    assert bank.packed is not None and bank.split is None and bank.pad == 0 and bank.tables is not None
    out, _ = _forward(dev, ops, q, s, sy, bank, kind)
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]
    ref = torch.cat([O.nw_head_f64(q_r[a:a + 64], s_r, sy, C, kind) for a in range(0, B, 64)])
    smax = O.scores_f64(q_r[:64], s_r, kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
    atol = max(3e-5, 3e-6 * smax)
    print(f"half N {N} {kind}: max|err| {(out.double() - ref).abs().max().item():.3e} (atol {atol:.1e})")
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=atol)


# --------------------------------------------------------------------------------------- 4. wild row scales, rows of zero norm
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("labels", ["sorted", "shuffled"])
def test_row_factors_over_orders_of_magnitude(dev, ops, pvar, kind, labels):
    (B, N), d = LARGE, 128
    q, s, g = _inputs(B, N, d, dev)
    s = s * (10.0 ** (6 * torch.rand(N, 1, generator=g) - 3)).to(dev)      # 1e-3 .. 1e3, row by row
    q = q * (10.0 ** (4 * torch.rand(B, 1, generator=g) - 2)).to(dev)
    s[torch.randperm(N, generator=g)[:40].to(dev)] = 0.0                   # rows of exactly zero norm, several per tile pair
    s[N - 1] = 0.0
    q[torch.randperm(B, generator=g)[:7].to(dev)] = 0.0
    sy = torch.arange(N) % C
    sy = (sy.sort().values if labels == "sorted" else sy[torch.randperm(N, generator=g)]).to(dev)
    bank = ops.SplitBank(s)
    assert bank.split is not None
    # far rows underflow to probability 0 and the log-probabilities may be -inf: the bits are compared, whatever they are
    _p3_and_p2(dev, ops, pvar, q, s, sy, bank, kind, finite=False)


# ----------------------------------------------------------------------------------------------------------- 5. candidate form
@pytest.mark.parametrize("kind", ["euclidean", "dotproduct"])
@pytest.mark.parametrize("d", [192, 256])
def test_candidate_form(dev, ops, O, d, kind):
    (B, N), k = SMALL, 8
    q, s, _ = _inputs(B, N, d, dev)
    bank = ops.SplitBank(s, precision="fp16")
    assert bank.packed is not None and bank.sorted_rows is None
    res = [ops.nw_knn(q, bank, k, kind, None, return_values=True, rounded=True, persistent_wgs=w) for w in (WGS, WGS, 0)]
    torch.cuda.synchronize()
    _check(res[0][0], res[0][1], _scores64(O, q, s, kind), k)
    for idx, val in res[1:]:
        assert torch.equal(idx, res[0][0]) and _same_bits(val, res[0][1])


# ---------------------------------------------------------------------------------------------------------- 6. reproducibility
def test_two_calls_give_the_same_bits(dev, ops, pvar):
    (B, N), d = LARGE, 160
    q, s, _ = _inputs(B, N, d, dev)
    sy = _stepped_labels(N)[0].to(dev)
    bank = ops.SplitBank(s)
    pvar(3)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert_persistent(B, N, d, cus, variant=3, wgs=WGS)
    a = _forward(dev, ops, q, s, sy, bank, "euclidean")
    b = _forward(dev, ops, q, s, sy, bank, "euclidean")   # through freshly poisoned buffers
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
