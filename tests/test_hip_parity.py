"""GPU parity: the HIP path, called through the C ABI (ctypes -> libnwhead_hip.so), against
  (1) the golden fixtures captured from the reference, (2) the CPU oracle on seeded inputs,
  (3) size-independent properties at BASELINE.json's full sizes.

Tolerance: BASELINE.json north_star = 1e-5 relative fp32 on the (B,C) log-probabilities.  Stated per
test as rtol=1e-5 plus an absolute floor of 1e-5 * |log(1e-12)| = 2.8e-4 only where entries are the
-27.63 "absent class" constant; elsewhere atol is 2e-5 (log-probs are O(1..30)).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import T, load_golden
import ws_poison

pytestmark = pytest.mark.gpu

KINDS = ("euclidean", "hypersphere_euclidean", "cosine", "dotproduct", "clip")
RTOL, ATOL = 1e-5, 2e-5


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


def _ls(dev):
    return torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float32, device=dev)


def close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(a.detach().cpu().numpy(), np.asarray(b), rtol=rtol, atol=atol)


# ------------------------------------------------------------------ golden fixtures
@pytest.mark.parametrize("kind", KINDS)
def test_g1_all_kernels_2d_3d(dev, ops, kind):
    g = load_golden("g1_k1_all_kernels.npz")
    C = int(g["C"])
    x, sx, sy = T(g["x"]).to(dev), T(g["sx"]).to(dev), T(g["sy"]).to(dev)
    ls = _ls(dev) if kind == "clip" else None
    close(ops.nw_head(x, sx, sy, C, kind, ls), g[f"out2d_{kind}"])
    close(ops.nw_head(x, T(g["sx3"]).to(dev), T(g["sy3"]).to(dev), C, kind, ls), g[f"out3d_{kind}"])
    if "euclidean" in kind:
        close(ops.nw_scores(x, sx, kind), g[f"scores2d_{kind}"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("N", [20, 25, 26])
def test_g2_cdist_regimes(dev, ops, N):
    g = load_golden("g2_cdist_regimes.npz")
    out = ops.nw_head(T(g[f"x_{N}"]).to(dev), T(g[f"sx_{N}"]).to(dev), T(g[f"sy_{N}"]).to(dev), int(g["C"]))
    close(out, g[f"out_{N}"])


@pytest.mark.parametrize("tag", ["n20", "n64"])
@pytest.mark.parametrize("kind", KINDS)
def test_g3_backward(dev, ops, tag, kind):
    g = load_golden("g3_backward.npz")
    C = int(g["C"])
    x = T(g[f"{tag}_x"]).to(dev).requires_grad_(True)
    sx = T(g[f"{tag}_sx"]).to(dev).requires_grad_(True)
    sy, t = T(g[f"{tag}_sy"]).to(dev), T(g[f"{tag}_t"]).to(dev)
    ls = _ls(dev).requires_grad_(True) if kind == "clip" else None
    out = ops.nw_head(x, sx, sy, C, kind, ls)
    F.nll_loss(out, t).backward()
    noisy = kind in ("euclidean", "hypersphere_euclidean") and tag == "n64"
    if noisy:
        # queries 0 and 3 sit exactly on a support row: in the matmul-form regime (N > 25) the
        # reference's distance there is sqrt(rounding residue) ~ 1e-3, not 0 -- a noise value of
        # the reference's own making.  Those two rows are held to 5e-3, the others to the bar.
        ok = [i for i in range(out.shape[0]) if i not in (0, 3)]
        close(out[ok], g[f"{tag}_{kind}_out"][ok])
        close(out, g[f"{tag}_{kind}_out"], rtol=1e-3, atol=5e-3)
    else:
        close(out, g[f"{tag}_{kind}_out"])
    gx_ref, gs_ref = g[f"{tag}_{kind}_gx"], g[f"{tag}_{kind}_gs"]
    gx, gs = x.grad.cpu().numpy(), sx.grad.cpu().numpy()
    if noisy:
        # D == 0 pairs (query 0 <-> support 1, query 3 <-> support N-1) in the matmul-form regime:
        # the reference divides by a rounding residue there, so those rows carry noise-sized
        # gradients in the reference itself -- compare every other row.
        N = gs.shape[0]
        qrows = [i for i in range(gx.shape[0]) if i not in (0, 3)]
        srows = [j for j in range(N) if j not in (1, N - 1)]
        gx, gx_ref, gs, gs_ref = gx[qrows], gx_ref[qrows], gs[srows], gs_ref[srows]
        tol = dict(rtol=2e-3, atol=2e-5)    # the two noisy pairs still leak into sum_j terms
    else:
        tol = dict(rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(gx, gx_ref, **tol)
    np.testing.assert_allclose(gs, gs_ref, **tol)
    if kind == "clip":
        np.testing.assert_allclose(ls.grad.cpu().numpy(), g[f"{tag}_{kind}_gls"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("kind", ["euclidean", "cosine", "hypersphere_euclidean", "dotproduct", "clip"])
@pytest.mark.parametrize("B,N,d,C", [(16, 5000, 512, 100), (3, 9001, 132, 7), (40, 300, 64, 1000)])
def test_per_query_supports_at_large_n(dev, ops, kind, B, N, d, C):
    """sx of shape (B, N, d) with labels (B, N) beyond the small-N regime: the streaming score kernel (16 lanes per support
    row) and the aggregation sliced over several workgroups per query, against fp64 (16 x 5000 x 512)."""
    from oracle import nw_oracle as O
    g = torch.Generator().manual_seed(B + N)
    q = torch.randn(B, d, generator=g)
    s = torch.randn(B, N, d, generator=g) * 0.7 + 0.1
    sy = torch.randint(0, C, (B, N), generator=g)
    ls = torch.tensor(2.3) if kind == "clip" else None
    out = ops.nw_head(q.to(dev), s.to(dev), sy.to(dev), C, kind, None if ls is None else ls.to(dev))
    out2 = ops.nw_head(q.to(dev), s.to(dev), sy.to(dev), C, kind, None if ls is None else ls.to(dev))
    assert torch.equal(out, out2)
    nb = min(B, 3)
    ref = torch.stack([O.nw_head_f64(q[b:b + 1], s[b], sy[b], C, kind, 2.3)[0] for b in range(nb)])
    np.testing.assert_allclose(out[:nb].cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=3e-5)
    sc = ops.nw_scores(q.to(dev), s.to(dev), kind, None if ls is None else ls.to(dev))
    ref_sc = torch.stack([O.scores_f64(q[b:b + 1], s[b], kind, 2.3)[0] for b in range(nb)])
    assert (sc[:nb].cpu().double() - ref_sc).abs().max().item() < 2e-5 * max(1.0, ref_sc.abs().max().item())


@pytest.mark.parametrize("tag", ["n20", "n64"])
def test_g3_backward_batched_support(dev, ops, tag):
    g = load_golden("g3_backward.npz")
    C = int(g["C"])
    x = T(g[f"{tag}_x"]).to(dev).requires_grad_(True)
    sx3 = T(g[f"{tag}_sx3"]).to(dev).requires_grad_(True)
    out = ops.nw_head(x, sx3, T(g[f"{tag}_sy3"]).to(dev), C)
    F.nll_loss(out, T(g[f"{tag}_t"]).to(dev)).backward()
    close(out, g[f"{tag}_out3"])
    np.testing.assert_allclose(x.grad.cpu().numpy(), g[f"{tag}_gx3"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(sx3.grad.cpu().numpy(), g[f"{tag}_gs3"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("B", [1, 4])
def test_g4_support_influence(dev, B):
    from nwhead_amd.util.metric import support_influence
    g = load_golden("g4_support_influence.npz")
    C = int(g["C"])
    sm, qy, w, sy = (T(g[f"b{B}_{k}"]).to(dev) for k in ("softmaxes", "qy", "w", "sy"))
    infl = support_influence(sm, F.one_hot(qy, C).float(), w, F.one_hot(sy, C).float()).cpu().numpy()
    ref = g[f"b{B}_infl"]
    assert infl.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(infl), np.isnan(ref))
    np.testing.assert_array_equal(np.isinf(infl), np.isinf(ref))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(infl[fin], ref[fin], rtol=1e-5, atol=1e-6)
    quirk = support_influence(sm, F.one_hot(qy, C).float(), w, F.one_hot(sy, C).float()[None].expand(B, -1, -1))
    assert tuple(quirk.shape) == tuple(g[f"b{B}_quirk_shape"])


def test_g7_shard_merge(dev, ops):
    g = load_golden("g7_shard_merge.npz")
    C, G = int(g["C"]), int(g["n_shards"])
    x, sx, sy = T(g["x"]).to(dev), T(g["sx"]).to(dev), T(g["sy"]).to(dev)
    N, B = len(sx), len(x)
    rows = [ops.nw_partials(x, sx[i * N // G:(i + 1) * N // G], sy[i * N // G:(i + 1) * N // G], C).view(-1)
            for i in range(G)]
    out = ops.nw_merge(torch.stack(rows), B, C)
    close(out, g["out"])
    close(out, ops.nw_head(x, sx, sy, C).cpu().numpy(), rtol=1e-6, atol=2e-6)     # sharded == unsharded


def test_g8_adversarial(dev, ops, O):
    g = load_golden("g8_adversarial.npz")
    C = int(g["C"])
    sy = T(g["sy"])
    far = ops.nw_head(T(g["xf"]).to(dev), T(g["sxf"]).to(dev), sy.to(dev), C)
    close(far, g["out_far"], rtol=1e-5, atol=1e-4)        # dist > 90: needs the max shift
    # large-norm / tiny-distance: the fp32 matmul form cancels; the reference itself is ~1e-4..1e-3
    # away from the fp64 truth, so grade against fp64 with the reference's own error as the bar.
    near = ops.nw_head(T(g["x"]).to(dev), T(g["sx"]).to(dev), sy.to(dev), C).cpu().double()
    truth = O.nw_head_f64(T(g["x"]), T(g["sx"]), sy, C)
    ref_err = np.abs(g["out_near"] - truth.numpy()).max()
    our_err = (near - truth).abs().max().item()
    assert our_err <= max(2.0 * ref_err, 5e-4), (our_err, ref_err)


# ------------------------------------------------------------------ oracle on seeded inputs
@pytest.mark.parametrize("B,N,d,C", [(64, 1000, 512, 200), (8, 64, 128, 10), (3, 27, 20, 4), (130, 333, 36, 7),
                                       (1, 4097, 256, 1000), (256, 2000, 512, 200)])
@pytest.mark.parametrize("kind", ["euclidean", "cosine"])
@pytest.mark.parametrize("dist", ["randn", "relu_like"])
def test_forward_vs_oracle(dev, ops, O, B, N, d, C, kind, dist):
    g = torch.Generator().manual_seed(B * 7 + N)
    if dist == "randn":
        q, s = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
    else:
        q, s = torch.rand(B, d, generator=g) * 2, torch.rand(N, d, generator=g) * 2
    sy = torch.randint(0, C, (N,), generator=g)
    out, w = ops.nw_head(q.to(dev), s.to(dev), sy.to(dev), C, kind, return_weights=True)
    ref64, w64 = O.nw_head_f64(q, s, sy, C, kind, return_weights=True)
    close(out, ref64.numpy(), rtol=RTOL, atol=3e-5)
    close(w, w64.numpy(), rtol=1e-4, atol=1e-8)
    if B * N * d <= 64 * 1000 * 512:                       # fp32 op-for-op restatement of the reference
        close(out, O.nw_head_f32(q, s, sy, C, kind).numpy(), rtol=RTOL, atol=3e-5)


def _out_and_lse(ops, q, s, sy, C):
    """The head's log-probabilities and the per-query log-sum-exp the same launch writes for the backward (the autograd
    node keeps it)."""
    out = ops.nw_head(q.clone().requires_grad_(True), s, sy, C)
    return out.detach(), out.grad_fn.saved_tensors[4]


@pytest.mark.parametrize("sorted_labels", [False, True])
def test_run_merge_with_more_classes_than_lds_holds_tables_for(dev, ops, O, sorted_labels):
    """The run merge keeps its per-class tables in LDS while C * 9 * 4 + 72 bytes fit in 150 KB (C <= 4265); past that
    nw_class_tables_kernel builds them once in the workspace and one workgroup per query reads them from there
    (nw_merge_runs_kernel<., 1, 2>).  4300 classes, 40 of them present: most classes have no entry, some have more than the
    four a table keeps (unsorted labels: found again by scanning the class's tiles)."""
    B, N, d, C = 8, 600, 32, 4300
    g = torch.Generator().manual_seed(4300)
    q, s = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
    present = torch.cat([torch.randperm(C - 2, generator=g)[:38] + 1, torch.tensor([0, C - 1])])
    sy = present[torch.randint(0, len(present), (N,), generator=g)]
    if sorted_labels:
        sy = sy.sort().values
    out, lse = _out_and_lse(ops, q.to(dev), s.to(dev), sy.to(dev), C)
    ref = O.nw_head_f64(q, s, sy, C)
    close(out, ref.numpy(), rtol=RTOL, atol=3e-5)
    close(lse, torch.logsumexp(O.scores_f64(q, s), dim=-1).numpy(), rtol=RTOL, atol=3e-5)
    close(ops.nw_head(q.to(dev), s.to(dev), sy.to(dev), C), ref.numpy(), rtol=RTOL, atol=3e-5)   # inference: no lse asked for
    if sorted_labels:   # the partials form of the same merge (nw_merge_runs_kernel<true, 1, 2>), once
        h = N // 2
        rows = torch.stack([ops.nw_partials(q.to(dev), s[a:b].to(dev), sy[a:b].to(dev), C).view(-1) for a, b in ((0, h), (h, N))])
        close(ops.nw_merge(rows, B, C), ref.numpy(), rtol=RTOL, atol=3e-5)


@pytest.mark.parametrize("N,n_ref", [(200, 512), (24576, 24)])
def test_run_merge_blocked_over_queries(dev, ops, O, N, n_ref):
    """From 512 queries up a merge workgroup takes 32 consecutive queries, or 16 once a query has 128 support tiles or more
    (24576 supports: 128 tiles of 192 rows, the tallest tile, and more of any other).  `n_ref` queries, spread over the
    workgroups and over the places inside one, against the fp64 oracle (its (B, N, d) cube of differences sets the count);
    every row sums to 1 + C * eps."""
    B, d, C = 512, 32, 10
    g = torch.Generator().manual_seed(N)
    q, s = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
    sy = torch.randint(0, C, (N,), generator=g)
    out, lse = _out_and_lse(ops, q.to(dev), s.to(dev), sy.to(dev), C)
    p = out.exp().sum(-1).cpu()
    assert torch.allclose(p, torch.full_like(p, 1 + C * 1e-12), atol=2e-5)
    rows = torch.arange(n_ref) * (B - 1) // (n_ref - 1)       # 0 ... B - 1; a stride of 22 walks through the places of a group
    close(out[rows.to(dev)], O.nw_head_f64(q[rows], s, sy, C).numpy(), rtol=RTOL, atol=3e-5)
    close(lse[rows.to(dev)], torch.logsumexp(O.scores_f64(q[rows], s), dim=-1).numpy(), rtol=RTOL, atol=3e-5)


def test_empty_and_ragged(dev, ops):
    C = 5
    q = torch.randn(4, 16, device=dev)
    out = ops.nw_head(q, torch.empty(0, 16, device=dev), torch.empty(0, dtype=torch.int64, device=dev), C)
    assert torch.allclose(out.cpu(), torch.full((4, C), float(np.log(np.float32(1e-12)))), atol=1e-5)
    assert ops.nw_head(torch.empty(0, 16, device=dev), torch.randn(7, 16, device=dev),
                       torch.zeros(7, dtype=torch.int64, device=dev), C).shape == (0, C)
    # odd feature dim -> generic kernel, single support, single class
    out = ops.nw_head(torch.randn(2, 13, device=dev), torch.randn(1, 13, device=dev),
                      torch.zeros(1, dtype=torch.int64, device=dev), 1)
    assert torch.allclose(out.cpu(), torch.zeros(2, 1), atol=1e-6)


def test_cpu_tensors_fail_loudly(ops):
    from nwhead_amd import NWHipError
    with pytest.raises(NWHipError):
        ops.nw_head(torch.randn(2, 8), torch.randn(30, 8), torch.zeros(30, dtype=torch.int64), 3)


# ------------------------------------------------------------------ properties at full size
def _t_inputs(dev, B=256, N=10000, d=512, C=200, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, d, generator=g).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    return q, s, sy, C


def test_full_size_properties(dev, ops, O):
    q, s, sy, C = _t_inputs(dev)
    out = ops.nw_head(q, s, sy, C)
    p = out.exp().sum(-1).cpu()
    assert torch.allclose(p, torch.full_like(p, 1 + C * 1e-12), atol=2e-5)       # rows sum to 1 + C*eps
    perm = torch.randperm(len(s), generator=torch.Generator().manual_seed(1)).to(dev)
    out_p = ops.nw_head(q, s[perm], sy[perm], C)                                 # support order is irrelevant
    close(out_p, out.cpu().numpy(), rtol=1e-5, atol=2e-5)
    # shard-merge associativity at 8 shards == unsharded
    B, N = q.shape[0], s.shape[0]
    rows = torch.stack([ops.nw_partials(q, s[i * N // 8:(i + 1) * N // 8], sy[i * N // 8:(i + 1) * N // 8], C).view(-1)
                        for i in range(8)])
    close(ops.nw_merge(rows, B, C), out.cpu().numpy(), rtol=1e-5, atol=2e-5)
    # a 32-query slice against the fp64 oracle (the full 256 x 10000 x 512 fp64 cube is 10 GB)
    ref = O.nw_head_f64(q[:32].cpu(), s.cpu(), sy.cpu(), C)
    close(out[:32], ref.numpy(), rtol=RTOL, atol=3e-5)


def test_influence_full_size(dev, ops, O):
    q, s, sy, C = _t_inputs(dev, B=64)
    out, w = ops.nw_head(q, s, sy, C, return_weights=True)
    qy = torch.randint(0, C, (64,), generator=torch.Generator().manual_seed(5)).to(dev)
    infl = ops.support_influence_idx(out.exp(), qy, w, sy).cpu()
    ref = O.support_influence_f32(out.exp().cpu(), F.one_hot(qy.cpu(), C).float(), w.cpu(), F.one_hot(sy.cpu(), C).float())
    np.testing.assert_array_equal(np.isfinite(infl.numpy()), np.isfinite(ref.numpy()))
    fin = np.isfinite(ref.numpy())
    np.testing.assert_allclose(infl.numpy()[fin], ref.numpy()[fin], rtol=1e-5, atol=1e-6)


def test_cached_support_norms(dev, ops, O):
    """predict('full') path: squared norms of the bank cached once (nw_row_norm2_f32) == in-kernel norms."""
    q, s, sy, C = _t_inputs(dev, B=96, N=3000)
    sn2 = ops.row_norm2(s)
    close(sn2, (s.double() ** 2).sum(-1).cpu().numpy(), rtol=1e-6, atol=1e-4)
    for kind in ("euclidean", "cosine", "hypersphere_euclidean"):
        a = ops.nw_head(q, s, sy, C, kind, support_norm2=sn2)
        b = ops.nw_head(q, s, sy, C, kind)
        close(a, b.cpu().numpy(), rtol=1e-5, atol=2e-5)
    ref = O.nw_head_f64(q[:32].cpu(), s.cpu(), sy.cpu(), C)
    close(ops.nw_head(q, s, sy, C, support_norm2=sn2)[:32], ref.numpy(), rtol=RTOL, atol=3e-5)


@pytest.mark.parametrize("kind", KINDS)
def test_split_fp16_fast_path(dev, ops, O, kind):
    """'full' inference fast path: bank prepared once (SplitBank: split-fp16 rows + scales + norms), dot
    products on the fp16 matrix cores.  Same bar as the fp32 path."""
    q, s, sy, C = _t_inputs(dev, B=96, N=3000)
    q = q * 3.0 + 0.5
    cache = ops.SplitBank(s)
    ls = _ls(dev) if kind == "clip" else None
    fast = ops.nw_head(q, s, sy, C, kind, ls, support_cache=cache)
    slow = ops.nw_head(q, s, sy, C, kind, ls)
    # dot-product scores are unbounded (|score| ~ 340 here, fp32 spacing 3e-5): the bar scales with them
    smax = O.scores_f64(q.cpu(), s.cpu(), kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
    atol = max(2e-5, 3e-6 * smax)
    close(fast, slow.cpu().numpy(), rtol=1e-5, atol=atol)
    ref = O.nw_head_f64(q[:32].cpu(), s.cpu(), sy.cpu(), C, kind)
    close(fast[:32], ref.numpy(), rtol=RTOL, atol=max(3e-5, 3e-6 * smax))
    # the fast path is at least as close to the fp64 truth as the fp32 matrix-core path
    e_fast = (fast[:32].cpu().double() - ref).abs().max().item()
    e_slow = (slow[:32].cpu().double() - ref).abs().max().item()
    assert e_fast <= 2.0 * e_slow + 1e-6, (e_fast, e_slow)


def test_split_fp16_dynamic_range(dev, ops, O):
    """rows whose magnitudes span 1e-4 .. 1e4 (per-row power-of-two scaling keeps fp16 in range)."""
    g = torch.Generator().manual_seed(3)
    B, N, d, C = 64, 2048, 128, 16
    scale_s = (10.0 ** torch.randint(-2, 3, (N, 1), generator=g).float())
    s = (torch.randn(N, d, generator=g) * scale_s).to(dev)
    q = (torch.randn(B, d, generator=g) * 10.0 ** torch.randint(-2, 3, (B, 1), generator=g).float()).to(dev)
    sy = (torch.arange(N) % C).sort().values.to(dev)
    cache = ops.SplitBank(s)
    for kind in ("euclidean", "cosine"):
        fast = ops.nw_head(q, s, sy, C, kind, support_cache=cache)
        ref = O.nw_head_f64(q.cpu(), s.cpu(), sy.cpu(), C, kind)
        close(fast, ref.numpy(), rtol=1e-5, atol=1e-4)


def test_split_rows_format(dev, ops):
    s = torch.randn(50, 64, device=dev) * 7
    c = ops.SplitBank(s)
    halves = c.split.view(torch.float16).view(50, 2, 2, 32).float()       # [row][chunk][h|l][32]
    rebuilt = (halves[:, :, 0] + halves[:, :, 1]).reshape(50, 64) * c.scale[:, None]
    # h + l reproduces x to 2^-23 of x, with an absolute floor (fp16 subnormals) far below the row's scale
    assert torch.allclose(rebuilt, s, rtol=3e-7, atol=3e-7 * s.abs().max().item())
    assert torch.allclose(c.norm2, (s * s).sum(-1), rtol=1e-6)
    e = torch.log2(c.scale)
    assert torch.equal(e, e.round())                                       # exact powers of two
    assert ops.SplitBank(torch.randn(5, 48, device=dev)).split is None     # d % 32 != 0: norms only


def test_class_window_merge(dev, ops):
    """Sharded exchange with class windows: shard g carries only [class_lo[g], class_lo[g] + CL) (labels
    shifted, C = CL in its partial forward); nw_merge_finalize scatters the windows back."""
    q, s, sy, C = _t_inputs(dev, B=64, N=4000)
    G, B, N = 8, q.shape[0], s.shape[0]
    bounds = [(i * N // G, (i + 1) * N // G) for i in range(G)]
    los = [int(sy[a:b].min()) for a, b in bounds]
    CL = max(int(sy[a:b].max()) - lo + 1 for (a, b), lo in zip(bounds, los))
    assert CL < C
    rows = torch.stack([ops.nw_partials(q, s[a:b], sy[a:b] - lo, CL).view(-1) for (a, b), lo in zip(bounds, los)])
    out = ops.nw_merge(rows, B, C, class_lo=torch.tensor(los, dtype=torch.int64, device=dev), c_local=CL)
    close(out, ops.nw_head(q, s, sy, C).cpu().numpy(), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("B,N,d,C,kind,sorted_labels", [
    (1000, 9000, 64, 37, "euclidean", False),     # d < 96: the one-workgroup-per-tile kernel (the persistent one needs three
                                                  # 32-column stages per tile); ragged B and N, ~128 runs per tile
    (520, 16500, 512, 200, "cosine", True),       # the bench's d, class-sorted bank (1-2 runs per tile)
    (1030, 8200, 96, 11, "dotproduct", True),
    (640, 14000, 128, 150, "euclidean", True),    # ~93 rows per class: 2-3 runs per 128-row tile (VALU run sums)
    (530, 9000, 160, 9, "hypersphere_euclidean", True),
    (515, 8300, 128, 40, "clip", False),
    (70, 140003, 96, 7, "euclidean", True),       # one (padded) 128-query tile, 1094 support tiles
    (129, 70001, 128, 3, "cosine", True),         # 129 queries: a 128-query tile plus a 1-row one
])
def test_persistent_many_tiles(dev, ops, O, B, N, d, C, kind, sorted_labels):
    """>= 4 tiles per CU with a SplitBank: the persistent kernel (fused_f16p.h: XCD-local tile walk, stage
    pipeline running across tile boundaries) and, from 512 queries up, the blocked merge -- against the
    fp64 oracle, for the final output and for the (m, den, num) partials."""
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(B, d, generator=g) * 0.7).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = torch.arange(N) % C
    sy = (sy.sort().values if sorted_labels else sy[torch.randperm(N, generator=g)]).to(dev)
    cache = ops.SplitBank(s)
    assert cache.split is not None
    ls = _ls(dev) if kind == "clip" else None
    # (the scratch buffer is never cleared: poisoned, so that a store the kernel forgets is not filled in by an earlier call)
    need = ws_poison.fwd_workspace_bytes(B, N, d, C)
    assert ws_poison.poison_cached_workspaces(need, dev) >= need
    out = ops.nw_head(q, s, sy, C, kind, ls, support_cache=cache)
    assert torch.isfinite(out).all()
    ref = O.nw_head_f64(q.cpu(), s.cpu(), sy.cpu(), C, kind)
    smax = O.scores_f64(q[:64].cpu(), s.cpu(), kind, O.CLIP_LOGIT_SCALE_INIT).abs().max().item()
    atol = max(3e-5, 3e-6 * smax)
    close(out, ref.numpy(), rtol=RTOL, atol=atol)
    # partials of two halves of the bank, merged == the whole
    h = N // 2
    rows = []
    for a, b in ((0, h), (h, N)):
        assert ws_poison.poison_cached_workspaces() >= need
        rows.append(ops.nw_partials(q, s[a:b], sy[a:b], C, kind, ls, support_cache=ops.SplitBank(s[a:b])).view(-1))
    rows = torch.stack(rows)
    assert torch.isfinite(rows).all()
    close(ops.nw_merge(rows, B, C), ref.numpy(), rtol=RTOL, atol=atol)


@pytest.mark.parametrize("variant", ["0", "1"])
def test_persistent_other_variants(dev, variant):
    """The library picks the persistent kernel's tile variant once per process (NW_PVAR unset: per launch);
    the variants that are not the default choice (0: 64-query tiles, one workgroup per CU; 1: two per CU) get
    a process of their own."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, NW_PVAR=variant)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_hip_parity.py"), "-q", "-x",
                        "-m", "gpu", "-k", "persistent_many_tiles and (cosine or dotproduct or 640)"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.parametrize("kind", KINDS)
def test_zero_rows_and_tiny_norms(dev, ops, O, kind):
    """All-zero query / support rows (F.normalize's eps branch for the cosine-type kernels, zero distance
    for the Euclidean ones) and rows of tiny norm, on the fp32 path and on the split-fp16 path."""
    g = torch.Generator().manual_seed(9)
    B, N, d, C = 40, 300, 64, 6
    q = torch.randn(B, d, generator=g)
    s = torch.randn(N, d, generator=g)
    q[3] = 0.0
    s[7] = 0.0
    s[8] *= 1e-20
    q[5] *= 1e-18
    s[100] = q[9]                                   # an exact duplicate: zero Euclidean distance
    sy = (torch.arange(N) % C).sort().values
    ls = _ls(dev) if kind == "clip" else None
    ref = O.nw_head_f64(q, s, sy, C, kind)
    qd, sd, syd = q.to(dev), s.to(dev), sy.to(dev)
    slow = ops.nw_head(qd, sd, syd, C, kind, ls)
    fast = ops.nw_head(qd, sd, syd, C, kind, ls, support_cache=ops.SplitBank(sd))
    assert torch.isfinite(slow).all() and torch.isfinite(fast).all()
    # the duplicate makes one Euclidean distance a difference of equal numbers (noise ~1e-3 in the matmul
    # form, as in torch's own cdist for N > 25): that query row gets the loose bar
    loose = np.zeros(B, dtype=bool)
    loose[9] = kind in ("euclidean", "hypersphere_euclidean")
    for out in (slow, fast):
        o = out.cpu().numpy()
        np.testing.assert_allclose(o[~loose], ref.numpy()[~loose], rtol=RTOL, atol=5e-5)
        np.testing.assert_allclose(o[loose], ref.numpy()[loose], rtol=1e-2, atol=5e-2)


def test_split_bank_sorts_unsorted_labels(dev, ops, O):
    """SplitBank(s, labels=...) with shuffled labels keeps a class-sorted copy and nw_head runs on it (same
    output); another label tensor, or a request for per-position weights, falls back to the plain path."""
    g = torch.Generator().manual_seed(13)
    B, N, d, C = 48, 3000, 64, 11
    q = torch.randn(B, d, generator=g).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = torch.randint(0, C, (N,), generator=g).to(dev)
    bank = ops.SplitBank(s, labels=sy)
    assert bank.sorted_rows is not None and bool((bank.sorted_labels[1:] >= bank.sorted_labels[:-1]).all())
    ref = O.nw_head_f64(q.cpu(), s.cpu(), sy.cpu(), C)
    close(ops.nw_head(q, s, sy, C, support_cache=bank), ref.numpy(), rtol=RTOL, atol=3e-5)
    other = sy.roll(1)                                            # a different label tensor: cache not applicable
    close(ops.nw_head(q, s, other, C, support_cache=bank), O.nw_head_f64(q.cpu(), s.cpu(), other.cpu(), C).numpy(),
          rtol=RTOL, atol=3e-5)
    out, w = ops.nw_head(q, s, sy, C, return_weights=True, support_cache=bank)
    close(out, ref.numpy(), rtol=RTOL, atol=3e-5)
    assert w.shape == (B, N) and torch.allclose(w.sum(-1).cpu(), torch.ones(B), atol=1e-5)
    rows = ops.nw_partials(q, s, sy, C, support_cache=bank).view(1, -1)
    close(ops.nw_merge(rows, B, C), ref.numpy(), rtol=RTOL, atol=3e-5)
    sorted_bank = ops.SplitBank(s, labels=sy.sort().values)      # already sorted: no copy
    assert sorted_bank.sorted_rows is None


def test_bank_beyond_4gb(dev, ops):
    """A bank of 4.5 GB (N = 2.2 M rows of 512 floats): the LDS-DMA loaders address rows relative to their
    tile, so nothing in the path is limited to 32-bit byte offsets.  Checked against an fp64 evaluation on
    the device in chunks (the CPU oracle would need the 9 GB fp64 bank)."""
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("needs ~20 GB of free HBM")
    g = torch.Generator(device=dev).manual_seed(5)
    B, N, d, C = 136, 2_150_000, 512, 50
    q = torch.randn(B, d, generator=g, device=dev)
    s = torch.randn(N, d, generator=g, device=dev)
    s[-3:] = q[:3] + 0.5 * torch.randn(3, d, generator=g, device=dev)   # the nearest neighbours sit in the LAST rows (beyond 4 GB)
    sy = (torch.arange(N, device=dev) * C // N)
    bank = ops.SplitBank(s, labels=sy)
    out = ops.nw_head(q, s, sy, C, support_cache=bank)            # 128-query tiles
    out16 = ops.nw_head(q[:16], s, sy, C, support_cache=bank)     # 64-query tiles, two workgroups per CU
    # fp64 reference for the first 16 queries, streamed over the bank
    nr = 16
    m = torch.full((nr,), -float("inf"), dtype=torch.float64, device=dev)
    num = torch.zeros(nr, C, dtype=torch.float64, device=dev)
    qd = q[:nr].double()
    for a0 in range(0, N, 430_000):
        sc = -torch.cdist(qd, s[a0:a0 + 430_000].double())
        mn = torch.maximum(m, sc.max(1).values)
        num *= torch.exp(m - mn)[:, None]
        num.index_add_(1, sy[a0:a0 + 430_000], torch.exp(sc - mn[:, None]))
        m = mn
    ref = torch.log(num / num.sum(1, keepdim=True) + 1e-12).cpu().numpy()
    close(out[:nr], ref, rtol=RTOL, atol=3e-5)
    close(out16, ref, rtol=RTOL, atol=3e-5)
    assert torch.isfinite(out).all() and (out.exp().sum(1) - 1).abs().max().item() < 1e-4
    del bank, s
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ weights / influences from the fused forward
# The smallest shape at which the three users of the forward workspace's tail meet: few queries over a long row (B <= 64,
# N >= 4096: the slice area is sized), split operands with the query-split launch (forced: the shape alone would take raw
# queries), and no lse_out of the caller's (weights / influences: the workspace's own lse slot).
TAIL_MEETS = (4, 4096, 64, 3)


@pytest.fixture
def tail_meets(request, dev):
    """True for the TAIL_MEETS case, which runs under NW_SPLIT_QUERIES=1 (restored afterwards) on a poisoned workspace."""
    import os
    from nwhead_amd import _lib
    B, N, d, C = (request.node.callspec.params[k] for k in "BNdC")
    if (B, N, d, C) != TAIL_MEETS:
        yield False
        return
    before = os.environ.get("NW_SPLIT_QUERIES")
    os.environ["NW_SPLIT_QUERIES"] = "1"
    _lib.sync_knobs()
    try:
        assert _lib.force_split(), "conftest pins NW_SPLIT_ALWAYS=1: below the size rule the bank's split rows are used with it only"
        assert _lib.fwd_plan(B, N, d, C, form="split", outputs="scores").split_queries
        assert _lib.fwd_layout(B, N, d, C).n_slices > 1
        yield True
    finally:
        if before is None:
            os.environ.pop("NW_SPLIT_QUERIES", None)
        else:
            os.environ["NW_SPLIT_QUERIES"] = before
        _lib.sync_knobs()


@pytest.mark.parametrize("B,N,d,C,cache", [(64, 10000, 512, 200, True), (37, 1001, 96, 7, False), (9, 300, 64, 5, True),
                                           (5, 20, 32, 4, False), TAIL_MEETS + (True,)])
def test_weights_from_the_fused_forward(dev, ops, O, tail_meets, B, N, d, C, cache):
    """return_weights=True: the tile kernel writes the scores where the weights go, one in-place pass normalises
    them with the merge's log-sum-exp (N > 25); N <= 25 keeps the two-kernel path.  `sweights` of util/metric.py:23."""
    g = torch.Generator().manual_seed(B + N)
    q, s = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
    sy = torch.randint(0, C, (N,), generator=g).sort().values
    qd, sd, syd = q.to(dev), s.to(dev), sy.to(dev)
    bank = ops.SplitBank(sd, syd) if cache else None
    if tail_meets:
        assert ws_poison.poison_cached_workspaces(min_bytes=ws_poison.fwd_workspace_bytes(B, N, d, C), device=dev) > 0
    out, w = ops.nw_head(qd, sd, syd, C, return_weights=True, support_cache=bank)
    if tail_meets:
        assert torch.isfinite(out).all() and torch.isfinite(w).all()
    ref, wref = O.nw_head_f64(q, s, sy, C, return_weights=True)
    close(out, ref.numpy(), rtol=RTOL, atol=3e-5)
    np.testing.assert_allclose(w.cpu().numpy(), wref.numpy(), rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(w.sum(-1).cpu().numpy(), 1.0, rtol=1e-5)
    # with gradients requested too (scores saved for the backward): weights from the saved scores
    qg = qd.clone().requires_grad_(True)
    out2, w2 = ops.nw_head(qg, sd, syd, C, return_weights=True)
    if tail_meets:
        assert torch.isfinite(out2).all() and torch.isfinite(w2).all()
    np.testing.assert_allclose(w2.detach().cpu().numpy(), wref.numpy(), rtol=2e-5, atol=1e-9)
    F.nll_loss(out2, torch.zeros(B, dtype=torch.int64, device=dev)).backward()
    assert torch.isfinite(qg.grad).all()


@pytest.mark.parametrize("B,N,d,C,cache", [(256, 10000, 512, 200, True), (33, 999, 64, 10, False), (4, 20, 16, 3, False),
                                           TAIL_MEETS + (True,)])
def test_forward_plus_influence_in_one_call(dev, ops, O, tail_meets, B, N, d, C, cache):
    """nw_fwd_influence_f32: util/metric.py:23-50 on the head's own outputs without a softmax-weight matrix, against
    the oracle's influence of the oracle's head (fp64 head, the reference's fp32 influence arithmetic)."""
    g = torch.Generator().manual_seed(7 * B + N)
    q, s = torch.randn(B, d, generator=g), torch.randn(N, d, generator=g)
    sy = (torch.arange(N) % C).sort().values
    qy = torch.randint(0, C, (B,), generator=g)
    qd, sd, syd = q.to(dev), s.to(dev), sy.to(dev)
    bank = ops.SplitBank(sd, syd) if cache else None
    if tail_meets:
        assert ws_poison.poison_cached_workspaces(min_bytes=ws_poison.fwd_workspace_bytes(B, N, d, C), device=dev) > 0
    out, infl = ops.nw_head_influence(qd, sd, syd, C, qy.to(dev), support_cache=bank)
    if tail_meets:
        assert torch.isfinite(out).all() and torch.isfinite(infl).all()
    rows = slice(0, min(B, 32))
    ref, wref = O.nw_head_f64(q[rows], s, sy, C, return_weights=True)
    close(out[rows], ref.numpy(), rtol=RTOL, atol=3e-5)
    iref = O.support_influence_f32(ref.exp().float(), F.one_hot(qy[rows], C).float(), wref.float(), F.one_hot(sy, C).float())
    got = infl[rows].cpu().numpy()
    # entries where the support carries most of its class's mass divide by a near-zero p - w: compare where the
    # denominator keeps at least 1e-3 of p (elsewhere a last-bit difference in p or w moves the value freely)
    p = ref.exp().float()[torch.arange(len(ref)), qy[rows]][:, None]
    ok = ((p - wref.float() * (sy[None, :] == qy[rows][:, None])) > 1e-3 * p).numpy() & np.isfinite(iref.numpy())
    np.testing.assert_allclose(got[ok], iref.numpy()[ok], rtol=2e-4, atol=2e-6)
    assert ok.mean() > 0.9
    # and the composite of the two separate calls gives the same numbers
    out2, w = ops.nw_head(qd, sd, syd, C, return_weights=True, support_cache=bank)
    comp = ops.support_influence_idx(out2.exp(), qy.to(dev), w, syd)[rows].cpu().numpy()
    np.testing.assert_allclose(got[ok], comp[ok], rtol=2e-4, atol=2e-6)
