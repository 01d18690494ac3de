"""The tile schedule of the persistent split-fp16 kernels (fused_f16p.h: NW_PVAR 0, 1, 2; fused_f16p12.h: NW_PVAR 3) away
from its defaults, every call through a scratch buffer filled with 0xFF (tests/ws_poison.py).

Which workgroup runs which tile, in which ring slot and header buffer, follows from n_cu = workgroups / 8 (the
`persistent_wgs` option, which ShardedBank sets to CUs - 8 on every multi-rank run), the query-group size (NW_QG; pvar 3
takes half of it), n_stiles / 8 and n_stiles % 8, n_qtiles, and nk = d / 32 (PersistentTiles::decode() and, in
persistent_loader(), set_tile() and issue_next() of persistent_pipe.h; the consumer loop of both files).  The tests:

  a  schedule invariance: per-tile arithmetic depends on (qt, st) only (the k rotation is st % nk) and the merge adds in a
     fixed order, so every (persistent_wgs, NW_QG) setting gives the default setting's BITS;
  b  ring residues: d / 32 = 3..8 and 16 (every residue mod the 3-slot rings of pvar 1 / 3 and mod the 4-slot rings of
     pvar 0 / 2), at the default schedule and with 8 workgroups (many tiles per workgroup: the slot and header counters
     wrap many times), against the fp64 oracle;
  c  edges of the order: fewer than 8 support tiles (no full round, no groups), n_stiles = 0, 1, 7 mod 8, one tile per
     workgroup, one tile more than workgroups on one XCD, XCDs that own no query tile of the leftover part;
  d  the persistent kernel against the one-workgroup-per-tile kernel (NW_NO_PERSISTENT=1), both against the oracle.  The
     two are NOT compared for equality: with more than three runs per tile fused_epilogue (fused_impl.h) sums a run in
     four MFMA chains that it adds at the end, epilogue_p / epilogue_p12 in one chain;
  e  (test_persistent_schedule_model.py, on the CPU) the Python model of decode() in tests/persistent_schedule.py: it
     documents the order and checks the MODEL, not the kernel.

Calls go through ops.nw_partials_into(..., ws=poisoned, persistent_wgs=w) + ops.nw_merge (nw_head does not expose
persistent_wgs), or through ShardedBank with its `_ws` poisoned.  Run tables come from a bank that holds them
(SplitBank.build_tables / ShardedBank: bank_tables_take) or are built by the launch (launch_run_tables).  Label modes:
"sorted" (class-sorted, tables in the bank), "shuffled" (a SplitBank built WITH the shuffled labels: it keeps a
class-sorted copy, which is what the call then passes) and "shuffled_nolabels" (a bank built without labels: ~128 runs per
tile reach the kernel, tables built by the launch).

Bound against the oracle: that of test_hip_parity.py::test_persistent_many_tiles.  Every GPU test asserts that its shape
takes the persistent kernel, twice: by the documented rule (plan_fused in fused.hip: at least 4 * CUs 64-query tiles, d >= 96,
d % 32 == 0; pick_rs, which picks the 128-support tile the persistent kernel needs, asks for 1024 of them whatever the
device) and by the library's own answer for the shape (persistent_schedule.assert_persistent: nw_debug_fwd_plan with the
device's CU count; with the forced tile variant once NW_PVAR is set).
"""
import os

import numpy as np
import pytest
import torch

import ws_poison
from persistent_schedule import BS, EDGES, assert_persistent, edge_shape, n_local, workgroups

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
PVARS = (0, 1, 2, 3)
RTOL = 1e-5
C = 200


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


_KNOB_VARS = ("NW_PVAR", "NW_QG", "NW_NO_PERSISTENT")


@pytest.fixture
def knobs():
    """set(pvar=, qg=, no_persistent=) forces the library's diagnostic knobs (None: unset); all are restored after the test."""
    from nwhead_amd import _lib
    _lib.load()
    before = {k: os.environ.get(k) for k in _KNOB_VARS}

    def set_(pvar=None, qg=None, no_persistent=None):
        for k, v in zip(_KNOB_VARS, (pvar, qg, no_persistent)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(int(v))
        _lib.sync_knobs()

    yield set_
    for k, v in before.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    _lib.sync_knobs()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _wgs(spec, cus):
    return {"cus-8": cus - 8, "cus+8": cus + 8}.get(spec) or int(spec)


def _assert_persistent(dev, B, N, d):
    cus = _cus(dev)
    tiles = ((B + 63) // 64) * ((N + BS - 1) // BS)
    assert tiles >= 4 * cus and tiles >= 1024 and d >= 96 and d % 32 == 0, \
        f"B={B} N={N} d={d}: {tiles} 64-query tiles do not take the persistent kernel on {cus} CUs"
    assert_persistent(B, N, d, cus)


_CASES = {}


def _case(dev, ops, B, N, d, kind, labels):
    """Seeded inputs and the banks of one (shape, kind, label mode), kept for the tests that share them."""
    key = (B, N, d, kind, labels)
    c = _CASES.get(key)
    if c is not None:
        return c
    if len(_CASES) >= 8:
        _CASES.clear()
    g = torch.Generator().manual_seed(1000 * B + N + d)
    q = (torch.randn(B, d, generator=g) * 0.7).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = torch.arange(N) % C
    sy = (sy.sort().values if labels == "sorted" else sy[torch.randperm(N, generator=g)]).to(dev)
    ls = torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev) if kind == "clip" else None
    c = dict(B=B, N=N, d=d, kind=kind, labels=labels, q=q, s=s, sy=sy, ls=ls, ref=None, sharded=None)
    if labels == "shuffled":                  # the bank sorts: the call passes its class-sorted copy, tables in the bank
        bank = ops.SplitBank(s, labels=sy)
        assert bank.sorted_rows is not None and bank.tables is not None
        c.update(bank=bank, s_call=bank.sorted_rows, sy_call=bank.sorted_labels)
    else:
        bank = ops.SplitBank(s)
        if labels == "sorted":
            bank.build_tables(sy)
            assert bank.tables is not None
        else:
            assert labels == "shuffled_nolabels" and bank.tables is None
        c.update(bank=bank, s_call=s, sy_call=sy)
    assert bank.split is not None
    _CASES[key] = c
    return c


def _forward(dev, ops, c, wgs=0, sharded=False):
    """One forward through poisoned buffers: partials into a poisoned row with a poisoned workspace, then the merge."""
    B, N, d = c["B"], c["N"], c["d"]
    need = ws_poison.fwd_workspace_bytes(B, N, d, C)
    # The buffer this call uses is the explicit poisoned one below.  The shared cache is poisoned as well so that nothing can
    # come from it; it may rightly be empty here, so the byte count is not asserted (where the cache IS the buffer in use,
    # assert it: see test_persistent_p12_gpu.py).
    ws_poison.poison_cached_workspaces()
    L = 2 * B + B * C
    packed = ws_poison.poisoned_workspace(4 * L, dev).view(torch.float32)
    assert torch.isnan(packed).all()
    if sharded:                                # the shipped sharded path (one rank here): the bank's own tables and buffer
        from nwhead_amd.sharded import ShardedBank
        sb = c["sharded"]
        if sb is None:
            sb = c["sharded"] = ShardedBank(c["s"], c["sy"], C, c["kind"], c["ls"])
            assert sb.cache is not None and sb.cache.split is not None and sb.cache.tables is not None and sb.CL == C
        sb.persistent_wgs = int(wgs)
        sb._ws = ws_poison.poisoned_workspace(need, dev)
        sb._partial(packed, c["q"])
        assert sb._ws.numel() == need          # (a larger need would have replaced the poisoned buffer)
        out = sb._merge(packed.view(1, L), B)
    else:
        ws = ws_poison.poisoned_workspace(need, dev)
        ops.nw_partials_into(packed, c["q"], c["s_call"], c["sy_call"], C, c["kind"], c["ls"], ws=ws, cache=c["bank"],
                             persistent_wgs=int(wgs))
        out = ops.nw_merge(packed.view(1, L), B, C)
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all(), "partials: a slot was not written (or holds poison read from the workspace)"
    assert out.shape == (B, C) and torch.isfinite(out).all()
    return out


def _oracle(O, c):
    """O.nw_head_f64 on the device, in row chunks (its direct-difference form builds a (rows, N, d) fp64 tensor), and the
    absolute bound of test_persistent_many_tiles."""
    if c["ref"] is None:
        rows = max(1, min(256, 60_000_000 // (c["N"] * c["d"])))
        q, s, sy, kind = c["q"], c["s"], c["sy"], c["kind"]
        ref = torch.cat([O.nw_head_f64(q[a:a + rows], s, sy, C, kind) for a in range(0, len(q), rows)])
        smax = O.scores_f64(q[:64], s, kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
        c["ref"] = (ref.cpu().numpy(), max(3e-5, 3e-6 * smax))
    return c["ref"]


def _assert_oracle(O, c, out, what=""):
    ref, atol = _oracle(O, c)
    got = out.cpu().numpy()
    print(f"{what} max|err| {np.abs(got - ref).max():.3e} (atol {atol:.1e})")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=atol)


# ---- a: schedule invariance
# (B, N, kind): ragged B and N, 61 support tiles (61 % 8 = 5), ~39 rows per class: more than three runs per tile;
#               37 / 19 / 10 query tiles of 64 / 128 / 256 rows: no multiple of a swept group size above 1 (1, 2, 3, 8, 13,
#               64; halved for pvar 3: 4, 6, 32), 102 support tiles (102 % 8 = 6), 65 rows per class: 2-3 runs per tile
SHAPES_A = [(1030, 7757, "euclidean"), (2330, 13000, "cosine")]
# (persistent_wgs, NW_QG); None = unset.  CUs + 8 must be ignored, 100 is rounded down to 96.
SETTINGS = [("8", 1), ("8", 64), ("cus-8", None), ("cus-8", 13), ("0", 2), ("64", 3), ("100", 8), ("cus+8", 13)]
_DEFAULT_OUT = {}


@pytest.mark.parametrize("wgs,qg", SETTINGS, ids=[f"wgs={w}-qg={'default' if g is None else g}" for w, g in SETTINGS])
@pytest.mark.parametrize("labels", ["sorted", "shuffled", "shuffled_nolabels"])
@pytest.mark.parametrize("B,N,kind", SHAPES_A, ids=[f"B{b}-N{n}" for b, n, _ in SHAPES_A])
@pytest.mark.parametrize("pvar", PVARS, ids=[f"pvar{v}" for v in PVARS])
def test_schedule_invariance(dev, ops, knobs, pvar, B, N, kind, labels, wgs, qg):
    d = 96
    _assert_persistent(dev, B, N, d)
    cus = _cus(dev)
    w = _wgs(wgs, cus)
    n_wg, n_wg0 = workgroups(pvar, cus, w), workgroups(pvar, cus, 0)
    if wgs in ("0", "cus+8"):
        assert n_wg == n_wg0                   # ignored
    else:
        assert 8 <= n_wg < n_wg0 and n_wg % 8 == 0
    c = _case(dev, ops, B, N, d, kind, labels)
    key = (pvar, B, N, labels)
    if key not in _DEFAULT_OUT:
        if len(_DEFAULT_OUT) >= 4:
            _DEFAULT_OUT.clear()
        knobs(pvar=pvar)
        _DEFAULT_OUT[key] = _forward(dev, ops, c).clone()
    knobs(pvar=pvar, qg=qg)
    assert assert_persistent(B, N, d, cus, variant=pvar, wgs=w).workgroups == n_wg
    # the sharded bank's setting goes through the sharded bank (class-sorted, as precompute() builds it)
    out = _forward(dev, ops, c, wgs=w, sharded=(wgs == "cus-8" and labels == "sorted"))
    ref = _DEFAULT_OUT[key]
    assert torch.equal(out, ref), \
        f"{(out != ref).sum().item()} of {out.numel()} differ, max |diff| {(out - ref).abs().max().item():.3e}"


# ---- b: ring residues
DS = [96, 128, 160, 192, 224, 256, 512]


@pytest.mark.parametrize("wgs", ["0", "8"], ids=["wgs=0", "wgs=8"])
@pytest.mark.parametrize("d", DS, ids=[f"d{d}" for d in DS])
@pytest.mark.parametrize("pvar", PVARS, ids=[f"pvar{v}" for v in PVARS])
def test_ring_residues(dev, ops, O, knobs, pvar, d, wgs):
    B, N = 1030, 7757                          # 17 / 9 / 5 query tiles x 61 support tiles: 65-130 tiles per workgroup of 8
    _assert_persistent(dev, B, N, d)
    kind = KINDS[(d // 32) % len(KINDS)]
    labels = "shuffled_nolabels" if d in (160, 224) else "sorted"
    c = _case(dev, ops, B, N, d, kind, labels)
    knobs(pvar=pvar)
    assert_persistent(B, N, d, _cus(dev), variant=pvar)
    out = _forward(dev, ops, c, wgs=_wgs(wgs, _cus(dev)))
    _assert_oracle(O, c, out, f"pvar {pvar} d {d} wgs {wgs} {kind}:")


# ---- c: order edges
@pytest.mark.parametrize("edge", EDGES)
def test_order_edges(dev, ops, O, knobs, edge):
    cus = _cus(dev)
    B, N = edge_shape(edge, cus)
    d = 96
    _assert_persistent(dev, B, N, d)
    n_stiles, nq3 = -(-N // BS), -(-B // 256)
    lists3 = [n_local(n_stiles, nq3, x) for x in range(8)]
    n_cu3 = workgroups(3, cus, 0) // 8
    if edge == "fewer_than_8_stiles":
        assert n_stiles < 8
    elif edge.startswith("stiles_"):
        assert n_stiles % 8 == int(edge[7])
    elif edge == "one_tile_per_wg":
        assert sum(lists3) == n_stiles * nq3 == workgroups(3, cus, 0) and lists3 == [n_cu3] * 8
    elif edge == "one_more_tile_than_wgs_on_one_xcd":
        assert lists3 == [n_cu3 + 1] + [n_cu3] * 7
    else:
        assert n_stiles % 8 and [(nq3 - x + 7) >> 3 for x in range(8)] == [1, 1, 0, 0, 0, 0, 0, 0]
    kind = KINDS[EDGES.index(edge) % len(KINDS)]
    c = _case(dev, ops, B, N, d, kind, "sorted")
    outs = {}
    for pvar in PVARS:
        knobs(pvar=pvar)
        assert_persistent(B, N, d, cus, variant=pvar)
        outs[pvar] = _forward(dev, ops, c).clone()
    for pvar in PVARS:
        _assert_oracle(O, c, outs[pvar], f"{edge} B {B} N {N} pvar {pvar} {kind}:")
    # the 256-query kernel does the 128-query kernel's arithmetic, element for element
    assert torch.equal(outs[3], outs[2]), f"max |diff| {(outs[3] - outs[2]).abs().max().item():.3e}"


# ---- d: persistent against one workgroup per tile
_ONE_WG_PER_TILE = {}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pvar", PVARS, ids=[f"pvar{v}" for v in PVARS])
def test_persistent_and_one_workgroup_per_tile(dev, ops, O, knobs, pvar, kind):
    """NW_NO_PERSISTENT=1 takes nw_fused_kernel whatever NW_PVAR says, so that half runs once per kind and is held to the
    oracle once.  Nothing here observes which kernel ran: that the knob switches kernels shows only in the bits (printed,
    not asserted: the two epilogues are not required to differ either)."""
    B, N, d = 1030, 7757, 128
    _assert_persistent(dev, B, N, d)
    c = _case(dev, ops, B, N, d, kind, "sorted")
    if kind not in _ONE_WG_PER_TILE:
        knobs(no_persistent=1)
        _ONE_WG_PER_TILE[kind] = _forward(dev, ops, c).clone()
        _assert_oracle(O, c, _ONE_WG_PER_TILE[kind], f"{kind} one workgroup per tile:")
    knobs(pvar=pvar)
    assert_persistent(B, N, d, _cus(dev), variant=pvar)
    out_p = _forward(dev, ops, c).clone()
    _assert_oracle(O, c, out_p, f"{kind} pvar {pvar} persistent:")
    print(f"{kind} pvar {pvar}: {(out_p != _ONE_WG_PER_TILE[kind]).sum().item()} of {out_p.numel()} outputs differ in bits "
          "from the one-workgroup-per-tile kernel's")
