"""ops.nw_knn / nw_knn_f32: the k nearest rows of a prepared bank without the (B,N) score matrix -- the tiles of the
split-fp16 score kernel select their k best scores in their epilogue (fused_impl.h, OUT_CAND), a second kernel takes the k
best of every query's candidates (topk.hip).

Exact tests: rows AND values equal nw_topk of the bank-route score matrix.  Below 2e8 multiply-adds that matrix comes from
the fp32 tile kernel and nw_knn goes through it too; NW_SPLIT_ALWAYS=1 puts both on the split kernel, which is where the
fused selection runs -- so every exact case runs under both settings, and one shape is large enough to take the fused
search without the switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops
    return ops


@pytest.fixture(params=[False, True], ids=["default", "split_always"])
def split_always(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    else:
        monkeypatch.delenv("NW_SPLIT_ALWAYS", raising=False)
    return request.param


def _data(dev, B, N, d, seed=None):
    g = torch.Generator().manual_seed(B * 7919 + N * 31 + d if seed is None else seed)
    return torch.randn(B, d, generator=g).to(dev), torch.randn(N, d, generator=g).to(dev)


def _parent(ops, q, s, bank, k, kind="euclidean", ls=None):
    return ops.nw_topk(ops.nw_scores(q, s, kind, ls, support_cache=bank), k, return_values=True)


def _fused_calls(ops, monkeypatch):
    """Counts the nw_knn_f32 launches: which route a call took."""
    from nwhead_amd import _lib
    lib = _lib.load()
    real = lib.nw_knn_f32
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name == "nw_knn_f32":
                return lambda *a: (calls.append(a[8:12]), real(*a))[1]
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy())
    return calls


@pytest.fixture
def launches(ops, monkeypatch):
    return _fused_calls(ops, monkeypatch)


def _check_exact(ops, q, s, bank, k, kind="euclidean", ls=None):
    idx, val = ops.nw_knn(q, bank, k, kind, ls, return_values=True, support=s)
    ridx, rval = _parent(ops, q, s, bank, k, kind, ls)
    assert idx.dtype == torch.int64 and idx.shape == (q.shape[0], k)
    assert torch.equal(idx, ridx)
    assert torch.equal(val, rval)
    assert torch.equal(ops.nw_knn(q, bank, k, kind, ls, support=s), ridx)       # without the values
    return idx


# a ragged query tile; a ragged last support tile; k larger than the rows of the last tile (4100 = 32 * 128 + 4); one tile
# only; many tiles; and one shape past 2e8 multiply-adds, fused without the switch
SHAPES = [(1, 400, 512), (37, 4100, 96), (130, 1000, 64), (64, 10000, 128), (200, 2048, 32), (256, 2048, 512)]


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("B,N,d", SHAPES)
def test_rows_and_values_equal_topk_of_the_bank_scores(dev, ops, split_always, monkeypatch, B, N, d, k):
    q, s = _data(dev, B, N, d)
    bank = ops.SplitBank(s)
    calls = _fused_calls(ops, monkeypatch)
    _check_exact(ops, q, s, bank, k)
    fused = split_always or B * N * d >= 2e8
    assert len(calls) == (2 if fused else 0), "the fused search runs exactly where the bank-route scores are the split kernel's"


@pytest.mark.parametrize("kind", ["euclidean", "cosine", "dotproduct", "hypersphere_euclidean"])
def test_score_kinds(dev, ops, split_always, launches, kind):
    q, s = _data(dev, 37, 4100, 96)
    _check_exact(ops, q, s, ops.SplitBank(s), 10, kind)
    assert bool(launches) == split_always


def test_clip_with_logit_scale(dev, ops, split_always, launches):
    q, s = _data(dev, 130, 1000, 64)
    ls = torch.tensor(2.5, device=dev)
    _check_exact(ops, q, s, ops.SplitBank(s), 10, "clip", ls)
    assert bool(launches) == split_always


@pytest.mark.parametrize("rs", [2, 4, 5, 6, 8, 10])
def test_every_tile_height(dev, ops, monkeypatch, rs):
    """pick_rs chooses by shape; NW_TILE_RS pins each height the launcher can take (the score call follows the same knob)."""
    from nwhead_amd import _lib
    monkeypatch.setenv("NW_SPLIT_ALWAYS", "1")
    monkeypatch.setenv("NW_TILE_RS", str(rs))
    _lib.sync_knobs()
    try:
        from nwhead_amd.ops import _WS_BYTES
        _WS_BYTES.clear()                      # sizes answered under another tile height
        q, s = _data(dev, 70, 16 * rs * 3 + 20, 64)
        bank = ops.SplitBank(s)
        for k in (1, 7, 32):
            _check_exact(ops, q, s, bank, k)
    finally:
        monkeypatch.delenv("NW_TILE_RS")
        _lib.sync_knobs()
        _WS_BYTES.clear()


def test_ties_keep_the_lowest_rows_in_order(dev, ops, split_always, launches):
    B, N, d = 8, 2048, 64                      # rows 100 / 101 share a tile under every tile height (32 .. 160 rows)
    q, s = _data(dev, B, N, d)
    s = s.clone()
    # The K chunks are walked in an order rotated by the support tile, so copies of a row in different tiles have their
    # dot products summed in different orders: of random floats they differ in the last bit and are no ties (under the
    # fp32 tile kernel the 40 copies below came out grouped by tile parity).  Small integers make every product and every
    # partial sum exact -- in fp32 and in the split form, whose row scale is a power of two -- whatever the order.
    g = torch.Generator().manual_seed(3)
    s[[100, 1919, 300]] = torch.randint(-3, 4, (3, d), generator=g).float().to(dev)
    s[101] = s[100]                            # a duplicate inside one tile
    s[1920] = s[1919]                          # ... across a tile boundary: 1920 is a multiple of every tile height
    copies = list(range(300, 300 + 40 * 11, 11))          # 40 copies of one row spread over three or more tiles
    s[copies] = s[300].clone()
    q[0], q[1], q[2] = s[100], s[1919], s[300]
    bank = ops.SplitBank(s)
    idx = _check_exact(ops, q, s, bank, 32)
    assert idx[0, :2].tolist() == [100, 101]
    assert idx[1, :2].tolist() == [1919, 1920]
    assert idx[2].tolist() == copies[:32]
    idx = _check_exact(ops, q, s, bank, 1)
    assert idx[:3, 0].tolist() == [100, 1919, 300]
    assert bool(launches) == split_always


def test_bank_of_padded_width(dev, ops, split_always, launches):
    q, s = _data(dev, 33, 1000, 100)
    bank = ops.SplitBank(s)
    assert bank.pad == 28 and bank.shape[1] == 128
    _check_exact(ops, q, s, bank, 10)
    assert bool(launches) == split_always


# ---- against fp64, independent of the score route (N % 4 != 0: there are no bank-route scores to compare with)
@pytest.mark.parametrize("B,N,d,k", [(33, 1001, 64, 10), (5, 27, 32, 20), (33, 1001, 64, 32), (5, 27, 32, 1)])
def test_against_fp64_distances(dev, ops, split_always, launches, B, N, d, k):
    q, s = _data(dev, B, N, d)
    idx, val = ops.nw_knn(q, ops.SplitBank(s), k, return_values=True, support=s)
    assert bool(launches) == split_always
    assert idx.shape == (B, k) and int(idx.min()) >= 0 and int(idx.max()) < N
    assert all(len(set(r)) == k for r in idx.tolist()), "rows are distinct"
    assert bool((val[:, 1:] <= val[:, :-1]).all()), "values are non-increasing"
    d64 = torch.cdist(q.double(), s.double())
    kth = torch.sort(d64, dim=1).values[:, k - 1:k]
    got = torch.gather(d64, 1, idx)
    # the project's score bound (3e-5 on every score): a returned row is at most that much past the k-th distance
    assert float((got - kth).max()) <= 3e-5
    assert float((val.double() + got).abs().max()) <= 3e-5


# ---- integration
def test_knn_indices_through_the_bank(dev, ops, split_always, monkeypatch):
    from nwhead_amd.nwhead.utils import KNN
    monkeypatch.setattr(ops, "KNN_FUSED_MIN_SCORE_BYTES", 0)        # the size gate of the callers: open
    q, s = _data(dev, 64, 4100, 96)
    labels = torch.arange(4100, device=dev) // 41
    knn = KNN(s, labels, 20)
    knn.bank = ops.SplitBank(s)
    sc = ops.nw_scores(q, s, "euclidean", support_cache=knn.bank)
    ref = torch.argsort(sc.cpu(), dim=-1, descending=True, stable=True)[:, :20]
    calls = _fused_calls(ops, monkeypatch)
    assert torch.equal(knn.indices(q).cpu(), ref)
    assert len(calls) == (1 if split_always else 0)
    sx, sy = knn(q)
    assert torch.equal(sx, s[ref.reshape(-1).to(dev)]) and torch.equal(sy, labels[ref.reshape(-1).to(dev)])


def test_callers_keep_the_score_matrix_below_the_size_gate(dev, ops, split_always, monkeypatch):
    """KNN.indices takes the fused search from a 1 GiB score matrix on: a small search is today's route, launch for launch."""
    from nwhead_amd.nwhead.utils import KNN
    assert not ops.knn_fused_pays(256, 50000) and not ops.knn_fused_pays(256, 400000)
    assert ops.knn_fused_pays(256, 1 << 20) and ops.knn_fused_pays(256, 2150000)
    q, s = _data(dev, 64, 4100, 96)
    knn = KNN(s, torch.zeros(4100, dtype=torch.int64, device=dev), 20)
    knn.bank = ops.SplitBank(s)
    calls = _fused_calls(ops, monkeypatch)
    sc = ops.nw_scores(q, s, "euclidean", support_cache=knn.bank)
    assert torch.equal(knn.indices(q), ops.nw_topk(sc, 20))
    assert not calls


def test_callers_leave_a_bank_of_odd_length_to_the_fp32_scores(dev, ops, monkeypatch):
    """N % 4 != 0 past 2e8 multiply-adds: nw_knn would rank the split kernel's scores, but KNN.indices has always ranked
    the fp32 scores kernel's there (no bank route for such N) and stays bit-identical: no fused launch."""
    from nwhead_amd.nwhead.utils import KNN
    monkeypatch.setattr(ops, "KNN_FUSED_MIN_SCORE_BYTES", 0)
    B, N, d = 256, 2050, 512
    assert B * N * d >= 2e8 and N % 4
    q, s = _data(dev, B, N, d)
    knn = KNN(s, torch.zeros(N, dtype=torch.int64, device=dev), 20)
    knn.bank = ops.SplitBank(s)
    calls = _fused_calls(ops, monkeypatch)
    ref = ops.nw_topk(ops.nw_scores(q, s, "euclidean"), 20)
    assert torch.equal(knn.indices(q), ref)
    assert not calls
    ops.nw_knn(q, knn.bank, 20, support=s)
    assert len(calls) == 1, "nw_knn itself does search such a bank fused"


def test_get_neighbors_with_k(dev, ops, split_always, monkeypatch):
    from nwhead_amd.nwhead.nw import NWNet
    monkeypatch.setattr(ops, "KNN_FUSED_MIN_SCORE_BYTES", 0)

    class DS(torch.utils.data.Dataset):
        def __init__(self):
            g = torch.Generator().manual_seed(5)
            self.x = torch.randn(400, 48, generator=g)
            self.targets = (torch.arange(400) % 10).tolist()

        def __len__(self):
            return 400

        def __getitem__(self, i):
            return self.x[i], self.targets[i]

    torch.manual_seed(0)
    net = NWNet(torch.nn.Linear(48, 64), 10, support_dataset=DS(), n_shot_full=40, device=dev).to(dev).eval()
    with torch.no_grad():
        net.precompute()
        x = torch.randn(9, 48, generator=torch.Generator().manual_seed(6)).to(dev)
        full = net.get_neighbors(x)
        assert full.shape == (9, 400)
        if net.full_cache.sorted_rows is not None:      # (labels that arrive unsorted: a bank of the rows as they stand)
            net.full_cache = ops.SplitBank(net.full_feat)
        calls = _fused_calls(ops, monkeypatch)
        assert torch.equal(net.get_neighbors(x, k=5), full[:, :5])
        assert len(calls) == (1 if split_always else 0), "the net's bank is found and searched fused"
        assert torch.equal(net.get_neighbors(x, k=40), full[:, :40])        # past 32: through the argsort
        assert len(calls) == (1 if split_always else 0)
        for bad in (0, 401):
            with pytest.raises(ops.NWHipError):
                net.get_neighbors(x, k=bad)


def test_fallbacks_return_the_parent_routes_rows(dev, ops, split_always, monkeypatch):
    q, s = _data(dev, 40, 2048, 64)
    calls = _fused_calls(ops, monkeypatch)
    _check_exact(ops, q, s, ops.SplitBank(s), 33)                              # k > 32
    shuffled = torch.randperm(2048, generator=torch.Generator().manual_seed(1)).to(dev) % 7
    bank = ops.SplitBank(s, labels=shuffled)
    assert bank.sorted_rows is not None
    _check_exact(ops, q, s, bank, 10)                                          # a class-sorted copy inside
    q2, s2 = _data(dev, 40, 2048, 40)
    bank = ops.SplitBank(s2)
    assert bank.split is None
    _check_exact(ops, q2, s2, bank, 10)                                        # norms only
    assert not calls


def test_bad_arguments_raise_like_nw_topk(dev, ops):
    q, s = _data(dev, 4, 100, 64)
    bank = ops.SplitBank(s)
    for k in (0, 101):
        with pytest.raises(ops.NWHipError):
            ops.nw_topk(ops.nw_scores(q, s, support_cache=bank), k)
        with pytest.raises(ops.NWHipError):
            ops.nw_knn(q, bank, k, support=s)
    with pytest.raises(ops.NWHipError):
        ops.nw_topk(torch.zeros(4, 100), 3)
    with pytest.raises(ops.NWHipError):
        ops.nw_knn(q.cpu(), bank, 3, support=s)
