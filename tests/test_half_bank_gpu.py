"""The half-precision bank (ops.SplitBank(precision="fp16"), nw_pack_rows_f16, nw_fwd_opts.operand_form = 1).

Its contract: the fp16 head IS the existing head applied to fp16-rounded features -- a row x is rounded to
h * 2^-e with h = fp16_rn(x * 2^e), e = 14 - frexp-exponent(max|x|) (at most 126; 0 for an all-zero row), and the norms the
kernel uses are those of the rounded rows.  So the tests round queries and supports in torch (`_round_rows`) and hold
the result to the fp64 oracle ON THE ROUNDED OPERANDS with the bound of test_persistent_p12_gpu.py; one test bounds the
distance to the head of the unrounded features from the rounding itself.  Every forward runs through a scratch buffer
filled with 0xFF (tests/ws_poison.py).  The oracle is evaluated on the device, in row chunks.
"""
import ctypes

import numpy as np
import pytest
import torch

import ws_poison

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
RTOL = 1e-5
C = 200
# (B, N, d): one tile; two query tiles + a ragged last support tile, even stage count; 9 support tiles (the leftover part
# of the tile order) with an odd stage count; 5 support tiles, 7 stages
SHAPES = ((1, 26, 192), (257, 129, 256), (300, 1100, 192), (64, 640, 448))


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


def _pow2(e):
    """2^e as fp32, exactly, for an integer tensor e in [-126, 127] (built from the exponent field)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _round_rows(x):
    """The rounding rule of nw_pack_rows_f16 in torch: (h fp16, e int32, 2^-e fp32, rounded rows h * 2^-e fp32)."""
    mx = x.abs().amax(dim=1)
    _, ex = torch.frexp(mx)
    e = (14 - ex.to(torch.int32)).clamp(max=126)
    e = torch.where((mx > 0) & torch.isfinite(mx), e, torch.zeros_like(e))
    h = (x * _pow2(e)[:, None]).to(torch.float16)
    down = _pow2(-e)
    return h, e, down, h.float() * down[:, None]


def _oracle_rows(O, q, s, sy, kind, n_classes=C, rows=64):
    return torch.cat([O.nw_head_f64(q[a:a + rows], s, sy, n_classes, kind) for a in range(0, len(q), rows)])


def _atol(O, q, s, kind):
    smax = O.scores_f64(q[:64], s, kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
    return max(3e-5, 3e-6 * smax)


def _ls(kind, dev):
    return torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev) if kind == "clip" else None


def _sorted_labels(N):
    """Class-sorted labels whose runs give every 128-row tile one to three runs."""
    if N < 256:
        lens = [N // 3, N // 3, N - 2 * (N // 3)]
    else:
        lens, pat, k = [], (256, 64, 64, 64, 33, 120, 75), 0
        while sum(lens) < N:
            lens.append(pat[k % len(pat)])
            k += 1
    y = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate(lens)])[:N]
    per_tile = [len(torch.unique_consecutive(y[a:a + 128])) for a in range(0, N, 128)]
    assert 1 <= min(per_tile) and max(per_tile) <= 3, per_tile
    if N >= 640:
        assert set(per_tile) == {1, 2, 3}, per_tile
    assert int(y.max()) < C
    return y


def _inputs(B, N, d, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * B + N + d + seed)
    q = (torch.randn(B, d, generator=g) * 0.7).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    return q, s, g


def _poison(dev, B, N, d, n_classes=C):
    need = ws_poison.fwd_workspace_bytes(B, N, d, n_classes)
    assert ws_poison.poison_cached_workspaces(need, dev) >= need


# ------------------------------------------------------------------------------------------------------------ pack format
@pytest.mark.parametrize("rows,d", [(37, 192), (5, 4160)])   # 4160: past the kernel's rows-in-registers branch (2048)
def test_pack_format(dev, rows, d):
    from nwhead_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * torch.logspace(-3, 3, rows)[:, None]   # mixed signs, many row scales
    x[0] = 0.0                                                  # all-zero row: e = 0
    x[1] = torch.randn(d, generator=g) * 1e-30                  # e = 14 + 99 = 113 or so: scales far from 1
    x[2] = torch.randn(d, generator=g)
    x[2, d // 3] = 3e4                                          # one large entry: e = -1
    x[3, ::2] = 0.0
    x = x.to(dev)
    out = torch.full((rows, d), float("nan"), dtype=torch.float16, device=dev)
    sc = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    n2 = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.nw_pack_rows_f16(x.data_ptr(), out.data_ptr(), sc.data_ptr(), n2.data_ptr(), rows, d,
                                    torch.cuda.current_stream().cuda_stream), "nw_pack_rows_f16")
    torch.cuda.synchronize()
    h, e, down, back = _round_rows(x)
    assert int(e[0]) == 0 and int(e[2]) == -1 and 100 < int(e[1]) <= 126
    assert torch.equal(out.view(torch.int16), h.view(torch.int16))
    assert torch.equal(sc, down)
    ref = back.double().pow(2).sum(1)
    # row_norm2 is an fp32 output: the reference is the fp64 sum rounded to that format (the 1e-30 row's norm, ~1e-58, is
    # below fp32's range and rounds to zero in both); the all-zero row must give exactly zero
    ref32 = ref.float().double()
    assert float(ref32[0]) == 0.0 and float(n2[0]) == 0.0
    err = (n2.double() - ref32).abs()
    assert bool((err <= 1e-6 * ref32).all()), (err / ref32.clamp_min(1e-300)).max().item()
    assert float(ref32[2]) > 1e8 and float(ref32[3]) > 0


# ------------------------------------------------------------------------------------- parity with the oracle, rounded
def _labels(mode, N, g):
    if mode == "sorted":
        return _sorted_labels(N)
    if mode == "cycled":            # every row starts a run: more than three per tile, the indicator-MFMA path
        return torch.arange(N) % C
    assert mode == "shuffled"
    y = _sorted_labels(N)
    return y[torch.randperm(N, generator=g)]


@pytest.mark.parametrize("labels", ["sorted", "cycled", "shuffled"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_oracle_on_rounded_operands(dev, ops, O, kind, shape, labels):
    B, N, d = shape
    q, s, g = _inputs(B, N, d, dev)
    sy = _labels(labels, N, g).to(dev)
    # "cycled": a bank without labels, run tables built by the launch; the others: tables (and, for shuffled labels, a
    # class-sorted copy) inside the bank
    bank = ops.SplitBank(s, labels=None if labels == "cycled" else sy, precision="fp16")
    assert bank.packed is not None and bank.split is None and bank.packed.dtype == torch.float16
    assert bank.packed.shape == (N, d) and bank.pad == 0
    assert (bank.sorted_rows is not None) == (labels == "shuffled" and N > 1)
    assert (bank.tables is not None) == (labels != "cycled")
    ls = _ls(kind, dev)
    _poison(dev, B, N, d)
    out = ops.nw_head(q, s, sy, C, kind, ls, support_cache=bank)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]
    ref = _oracle_rows(O, q_r, s_r, sy, kind)
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=_atol(O, q_r, s_r, kind))


def test_label_outside_the_classes_contributes_nothing(dev, ops, O):
    """Labels >= n_classes, passed with a bank that holds no labels: such supports keep their softmax weight and feed no
    class -- the oracle's result for a wide enough one-hot, cut to the first n_classes columns."""
    B, N, d = SHAPES[3]
    n_classes = 150
    q, s, _ = _inputs(B, N, d, dev, seed=5)
    sy = (torch.arange(N) % C).to(dev)
    assert int(sy.max()) >= n_classes
    bank = ops.SplitBank(s, precision="fp16")
    _poison(dev, B, N, d, n_classes)
    out = ops.nw_head(q, s, sy, n_classes, "euclidean", support_cache=bank)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]
    ref = _oracle_rows(O, q_r, s_r, sy, "euclidean", n_classes=C)[:, :n_classes]
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=_atol(O, q_r, s_r, "euclidean"))


# ---------------------------------------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("kind", ["euclidean", "cosine"])
@pytest.mark.parametrize("d,padded", [(128, 192), (200, 256)])
def test_padded_widths(dev, ops, O, kind, d, padded):
    B, N = 70, 300
    q, s, _ = _inputs(B, N, d, dev, seed=9)
    sy = _sorted_labels(N).to(dev)
    bank = ops.SplitBank(s, labels=sy, precision="fp16")
    assert bank.pad == padded - d and bank.packed.shape == (N, padded) and bank.rows.shape == (N, padded)
    assert not bool(bank.packed[:, d:].any())
    _poison(dev, B, N, padded)
    out = ops.nw_head(q, s, sy, C, kind, support_cache=bank)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]      # zero columns change neither the row maxima nor any product
    ref = _oracle_rows(O, q_r, s_r, sy, kind)
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=_atol(O, q_r, s_r, kind))
    # the bank's norm2 stays that of the ORIGINAL rows (every other path reads it)
    np.testing.assert_allclose(bank.norm2.cpu().numpy(), s.double().pow(2).sum(1).cpu().numpy(), rtol=1e-5)


# ------------------------------------------------------------------------------- distance to the unrounded fp32 features
@pytest.mark.parametrize("kind", ["euclidean", "dotproduct"])
def test_derived_bound_against_unrounded_features(dev, ops, O, kind):
    """Rounding moves a vector v by at most 2^-11 |v| (every element by at most 2^-11 relative), so a euclidean score
    moves by at most 2^-11 (|q| + |s|) and a dot product by at most (2^-10 + 2^-22) |q| |s|; a log-softmax-sum moves by at
    most twice the largest score change.  1e-4 covers the kernel's own error and the 1e-12 inside the log for entries of
    probability above 1e-6."""
    B, N, d = 64, 640, 256
    g = torch.Generator().manual_seed(77)
    q = (torch.randn(B, d, generator=g) / d ** 0.5).to(dev)       # |v| ~ 1
    s = (torch.randn(N, d, generator=g) / d ** 0.5).to(dev)
    sy = (torch.arange(N) % C).to(dev)
    bank = ops.SplitBank(s, precision="fp16")
    _poison(dev, B, N, d)
    out = ops.nw_head(q, s, sy, C, kind, support_cache=bank).double()
    torch.cuda.synchronize()
    ref = _oracle_rows(O, q, s, sy, kind)
    qn, sn = q.double().norm(dim=1), s.double().norm(dim=1)
    if kind == "euclidean":
        dscore = 2.0 ** -11 * (qn + sn.max())
    else:
        dscore = (2.0 ** -10 + 2.0 ** -22) * qn * sn.max()
    bound = (2 * dscore + 1e-4)[:, None].expand_as(ref)
    live = ref > float(np.log(1e-6))
    assert int(live.sum()) > B                                    # the comparison is not empty
    err = (out - ref).abs()
    print(f"{kind}: max |out - ref| / bound = {(err[live] / bound[live]).max().item():.3f}, max |out - ref| = "
          f"{err[live].max().item():.3e}")
    assert bool((err[live] <= bound[live]).all()), (err[live] / bound[live]).max().item()


# --------------------------------------------------------------------------------------------------------------- partials
@pytest.mark.parametrize("kind", ["euclidean", "clip"])
def test_partials_of_two_shards_merge_to_the_single_bank_call(dev, ops, O, kind):
    B, N, d = SHAPES[2]
    cut = 500
    q, s, _ = _inputs(B, N, d, dev, seed=3)
    sy = _sorted_labels(N).to(dev)
    ls = _ls(kind, dev)
    whole = ops.SplitBank(s, labels=sy, precision="fp16")
    _poison(dev, B, N, d)
    single = ops.nw_head(q, s, sy, C, kind, ls, support_cache=whole).clone()
    parts = []
    for a, b in ((0, cut), (cut, N)):
        sa, ya = s[a:b].contiguous(), sy[a:b].contiguous()
        bank = ops.SplitBank(sa, labels=ya, precision="fp16")
        _poison(dev, B, b - a, d)
        parts.append(ops.nw_partials(q, sa, ya, C, kind, ls, support_cache=bank).reshape(-1).clone())
    merged = ops.nw_merge(torch.stack(parts), B, C)
    torch.cuda.synchronize()
    assert torch.isfinite(merged).all() and torch.isfinite(single).all()
    q_r, s_r = _round_rows(q)[3], _round_rows(s)[3]
    np.testing.assert_allclose(merged.cpu().numpy(), single.cpu().numpy(), rtol=RTOL, atol=_atol(O, q_r, s_r, kind))


def test_sharded_bank_passes_the_precision_through(dev, ops):
    from nwhead_amd.sharded import ShardedBank
    B, N, d = SHAPES[3]
    q, s, _ = _inputs(B, N, d, dev, seed=4)
    sy = _sorted_labels(N).to(dev)
    sb = ShardedBank(s, sy, C, precision="fp16")
    assert sb.cache.packed is not None and sb.cache.tables is not None
    direct = ops.nw_head(q, sb.feat, sb.y, C, support_cache=ops.SplitBank(sb.feat, labels=sb.y, precision="fp16"))
    assert torch.equal(sb.predict(q), direct)
    assert ShardedBank(s, sy, C).cache.packed is None


# ----------------------------------------------------------------------------------------------------------------- guards
def test_c_abi_refuses_what_form_1_does_not_cover(dev):
    from nwhead_amd import _lib
    lib = _lib.load()
    B, N, n_classes = 8, 100, 5
    op = _lib.fwd_opts(operand_form=1)
    stream = torch.cuda.current_stream().cuda_stream

    def call(d, scores=False, sup_b=0):
        q = torch.randn(B, d, device=dev)
        s = torch.randn(*((B, N, d) if sup_b else (N, d)), device=dev)
        sy = torch.zeros(N, dtype=torch.int64, device=dev)
        half = torch.zeros(N, d, dtype=torch.float16, device=dev)
        v = torch.ones(N, device=dev)
        out = torch.zeros(B, n_classes, device=dev)
        sc = torch.zeros(B, N, device=dev) if scores else None
        nbytes = lib.nw_fwd_workspace_bytes(B, N, d, n_classes)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        rc = lib.nw_fwd_f32(q.data_ptr(), s.data_ptr(), sy.data_ptr(), v.data_ptr(), half.data_ptr(), v.data_ptr(),
                            out.data_ptr(), None if sc is None else sc.data_ptr(), None, None, ws.data_ptr(), nbytes, B, N, d,
                            n_classes, 0, None, sup_b, 0, ctypes.addressof(op), stream)
        torch.cuda.synchronize()
        return rc

    assert call(256, scores=True) == -2
    assert call(128) == -2
    assert call(256, sup_b=1) == -2
    assert call(256) == 0


def test_other_paths_with_an_fp16_bank_are_the_fp32_paths(dev, ops, O):
    """return_weights and a call under autograd proceed as with a norms-only bank; nw_scores takes its non-split path."""
    B, N, d = 64, 640, 256
    q, s, _ = _inputs(B, N, d, dev, seed=6)
    sy = _sorted_labels(N).to(dev)
    bank = ops.SplitBank(s, labels=sy, precision="fp16")
    plain = ops.nw_head(q, s, sy, C)
    atol = _atol(O, q, s, "euclidean")
    half = ops.nw_head(q, s, sy, C, support_cache=bank)
    print(f"fp16 head against the fp32 head: max |diff| = {(half - plain).abs().max().item():.3e}, atol = {atol:.3e}")
    assert (half - plain).abs().max().item() > 2 * atol             # the comparisons below tell the two paths apart
    out_w, w = ops.nw_head(q, s, sy, C, return_weights=True, support_cache=bank)
    _, w_plain = ops.nw_head(q, s, sy, C, return_weights=True)
    np.testing.assert_allclose(out_w.cpu().numpy(), plain.cpu().numpy(), rtol=RTOL, atol=atol)
    np.testing.assert_allclose(w.cpu().numpy(), w_plain.cpu().numpy(), rtol=1e-4, atol=1e-7)
    qg = q.clone().requires_grad_(True)
    out_g = ops.nw_head(qg, s, sy, C, support_cache=bank)
    assert out_g.requires_grad
    np.testing.assert_allclose(out_g.detach().cpu().numpy(), plain.cpu().numpy(), rtol=RTOL, atol=atol)
    out_g.sum().backward()
    assert torch.isfinite(qg.grad).all()
    assert torch.equal(ops.nw_scores(q, s, "euclidean", support_cache=bank), ops.nw_scores(q, s, "euclidean"))
    out_i, infl = ops.nw_head_influence(q, s, sy, C, sy[:B], support_cache=bank)
    np.testing.assert_allclose(out_i.cpu().numpy(), plain.cpu().numpy(), rtol=RTOL, atol=atol)
    assert infl.shape == (B, N)


def test_small_banks_keep_norms_only(dev, ops):
    s = torch.randn(25, 192, device=dev)          # no tile kernel takes 25 supports or fewer
    bank = ops.SplitBank(s, precision="fp16")
    assert bank.packed is None and bank.split is None and bank.pad == 0
    with pytest.raises(ValueError):
        ops.SplitBank(s, precision="bf16")


# ------------------------------------------------------------------------------------------------------------------ NWNet
class _DS(torch.utils.data.Dataset):
    def __init__(self, data, targets, n_classes):
        self.data, self.targets, self.num_classes = data, list(targets), n_classes

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.data[i], self.targets[i]


def _net(**kw):
    import torch.nn as nn
    from conftest import T, load_golden
    from nwhead_amd.nwhead.nw import NWNet
    g = load_golden("g5_nwnet_plumbing.npz")
    n_classes = int(g["C"])
    ds = _DS(T(g["ds_data"]), g["ds_targets"].tolist(), n_classes)
    feat = nn.Sequential(nn.Flatten(), nn.Linear(48, 16))
    with torch.no_grad():
        feat[1].weight.copy_(T(g["w"]))
        feat[1].bias.copy_(T(g["b"]))
    net = NWNet(feat, n_classes, support_dataset=ds, feat_dim=16, n_shot=2, n_way=6, n_shot_full=7, n_shot_cluster=2,
                n_neighbors=3, device="cuda:0", cluster_backend="sklearn", **kw).to("cuda:0")
    net.eval()
    np.random.seed(1234)
    net.precompute()
    return net, T(g["xq"]).cuda(), n_classes


def test_nwnet_full_precision_fp16(dev, ops, O):
    net, xq, n_classes = _net(full_precision="fp16")
    bank = net.full_cache
    assert bank.precision == "fp16" and bank.packed is not None and bank.packed.shape[1] == 192
    with torch.no_grad():
        _poison(dev, len(xq), bank.shape[0], bank.shape[1], n_classes)
        out = net.predict(xq, "full")
        qfeat = net.featurizer(xq)
    torch.cuda.synchronize()
    q_r, s_r = _round_rows(qfeat)[3], _round_rows(net.full_feat)[3]
    ref = O.nw_head_f64(q_r, s_r, net.full_y, n_classes, "euclidean")
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=_atol(O, q_r, s_r, "euclidean"))
    # a bank rebuilt by predict() keeps the precision
    net.full_cache = None
    with torch.no_grad():
        again = net.predict(xq, "full")
    assert net.full_cache.precision == "fp16" and torch.equal(again, out)


def test_nwnet_default_is_the_fp32_grade_path(dev, ops):
    net, xq, n_classes = _net()
    assert net.full_precision == "fp32" and net.full_cache.precision == "fp32" and net.full_cache.packed is None
    with torch.no_grad():
        out = net.predict(xq, "full")
        qfeat = net.featurizer(xq)
        same = ops.nw_head(qfeat, net.full_feat, net.full_y, n_classes,
                           support_cache=ops.SplitBank(net.full_feat, labels=net.full_y, precision="fp32"))
    assert torch.equal(out, same)
    with pytest.raises(ValueError):
        from nwhead_amd.nwhead.nw import NWNet
        NWNet(net.featurizer, n_classes, full_precision="half")
