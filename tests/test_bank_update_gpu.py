"""Rows of a prepared bank refreshed in place (split.hip: nw_bank_update_rows_f32; ops.SplitBank.update_rows,
NWNet.refresh_bank, the harness's --train_type bank).

After every update: (a) the updated fp32 rows equal the torch reference bit for bit -- for a blend
``m = torch.tensor(momentum, dtype=float32); m * old + (1 - m) * x`` in fp32 tensors; (b) every tensor of the bank equals that
of a fresh ``ops.SplitBank(support.clone(), labels, precision)``; (c) rows that no item names keep the bits of a clone taken
before; (d) ``bank.matches(support)`` holds and ``bank.tables`` is the same object.  All comparisons are of bit patterns
(integer views): stricter than torch.equal on floats, and NaN patterns compare like any other.

The recorded outputs of the three preparation entry points (tests/golden/bank_forms.npz, record_bank_forms.py) hold the
shapes 64 x 96 and 8 x 2080 for the split rows and the plain norms; nw_pack_rows_f16 refuses both widths (it takes multiples
of 64), so its records are 64 x 192 and 8 x 2112, and its refusal of the other two is checked."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BANK_TENSORS = ("split", "scale", "norm2", "packed", "packed_scale", "packed_norm2", "rows")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from nwhead_amd import ops as o
    return o


def bits(t):
    """The tensor's bit patterns (fp32 -> int32, fp16 -> int16)."""
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def bank_tensors(bank):
    return {k: getattr(bank, k) for k in BANK_TENSORS if getattr(bank, k) is not None}


def sorted_labels(N, C, dev):
    return (torch.arange(N, device=dev) * C) // N


def winners(rows, N):
    """{bank row: item} under the kernel's rule: rows outside [0, N) skipped, the last occurrence wins."""
    w = {}
    for i, r in enumerate(rows.tolist()):
        if 0 <= r < N:
            w[r] = i
    return w


def reference_rows(old, rows, x, momentum):
    """The support after the update, by torch ops in fp32 on the device."""
    ref = old.clone()
    w = winners(rows, old.shape[0])
    if w:
        r = torch.tensor(list(w.keys()), device=old.device)
        i = torch.tensor(list(w.values()), device=old.device)
        if momentum == 0:
            ref[r] = x[i]
        else:
            m = torch.tensor(momentum, dtype=torch.float32, device=old.device)
            ref[r] = m * old[r] + (1 - m) * x[i]
    return ref, w


def update_and_check(ops, bank, support, labels, precision, rows, x, momentum, what):
    """One update_rows call with the module's assertions (a) - (d)."""
    N = support.shape[0]
    old = support.clone()
    before = {k: v.clone() for k, v in bank_tensors(bank).items()}
    tables, writes = bank.tables, bank.writes
    ref, w = reference_rows(old, rows, x, momentum)
    bank.update_rows(support, rows, x, momentum)
    assert same_bits(support, ref), f"(a) fp32 rows: {what}"
    fresh = ops.SplitBank(support.clone(), labels, precision)
    got, want = bank_tensors(bank), bank_tensors(fresh)
    assert set(got) == set(want) and set(got) == set(before), what
    for k in want:
        assert same_bits(got[k], want[k]), f"(b) bank.{k} differs from a fresh bank's: {what}"
    untouched = torch.ones(N, dtype=torch.bool, device=support.device)
    if w:
        untouched[torch.tensor(list(w.keys()), device=support.device)] = False
    assert same_bits(support[untouched], old[untouched]), f"(c) support: {what}"
    for k, v in before.items():
        assert same_bits(got[k][untouched], v[untouched]), f"(c) bank.{k}: {what}"
    assert bank.matches(support) and bank.tables is tables and bank.writes == writes + 1, f"(d) {what}"


def make_rows(R, N, g, dev):
    """R bank rows: distinct while the bank has that many, else with repeats (the last one wins)."""
    r = torch.randperm(N, generator=g)[:R] if R <= N else torch.randint(0, N, (R,), generator=g)
    return r.to(dev)


# (feature width, precision, bank width): one chunk with most lanes idle; 96; two register slots; the last in-register
# width; the streaming path; a padded fp32 bank (s_user written), one whose feature width is no multiple of 4 (scalar loads
# of x); fp16 banks padded to the minimum width, to the next multiple of 64, and not padded
WIDTHS = [(32, "fp32", 32), (96, "fp32", 96), (512, "fp32", 512), (2048, "fp32", 2048), (2080, "fp32", 2080),
          (100, "fp32", 128), (70, "fp32", 96), (64, "fp16", 192), (200, "fp16", 256), (256, "fp16", 256)]


@pytest.mark.parametrize("width,precision,bank_width", WIDTHS)
def test_update_rows_matches_a_fresh_bank(ops, dev, width, precision, bank_width):
    N, C = 64, 6
    g = torch.Generator().manual_seed(1000 + width)
    support = torch.randn(N, width, generator=g).to(dev)
    labels = sorted_labels(N, C, dev)
    bank = ops.SplitBank(support, labels, precision)
    assert bank.shape == (N, bank_width) and bank.sorted_rows is None and bank.has_operand_rows
    assert (bank.rows is not None) == (bank_width != width)
    for R in (1, 5, 256):
        for momentum in (0.0, 0.5, 0.9):
            rows = make_rows(R, N, g, dev)
            x = (torch.randn(R, width, generator=g) * 3).to(dev)
            update_and_check(ops, bank, support, labels, precision, rows, x, momentum,
                             f"width {width} {precision} R={R} momentum={momentum}")
    assert bank.writes == 9


def test_update_rows_under_the_split_lbits_knob(ops, dev, monkeypatch):
    """The diagnostic knob that masks the low halves of the split rows applies to refreshed rows as to built ones."""
    from nwhead_amd import _lib
    N, C, width = 64, 6, 96
    g = torch.Generator().manual_seed(21)
    support = torch.randn(N, width, generator=g).to(dev)
    labels = sorted_labels(N, C, dev)
    full = ops.SplitBank(support.clone(), labels).split.clone()
    monkeypatch.setenv("NW_SPLIT_LBITS", "3")
    _lib.sync_knobs()
    try:
        bank = ops.SplitBank(support, labels)
        assert not same_bits(bank.split, full)                  # the knob is in force
        for momentum in (0.0, 0.9):
            rows = make_rows(5, N, g, dev)
            x = torch.randn(5, width, generator=g).to(dev)
            update_and_check(ops, bank, support, labels, "fp32", rows, x, momentum, f"split_lbits=3 momentum={momentum}")
    finally:
        monkeypatch.delenv("NW_SPLIT_LBITS")
        _lib.sync_knobs()


@pytest.mark.parametrize("precision,width", [("fp32", 96), ("fp16", 256)])
def test_update_rows_of_a_longer_bank_and_unaligned_x(ops, dev, precision, width):
    """N = 4100 (rows past 4096 are named); x at an address that is no multiple of 16 (scalar loads), int32 rows."""
    N, C, R = 4100, 11, 256
    g = torch.Generator().manual_seed(7)
    support = torch.randn(N, width, generator=g).to(dev)
    labels = sorted_labels(N, C, dev)
    bank = ops.SplitBank(support, labels, precision)
    rows = torch.cat([torch.tensor([N - 1, 4096, 0]), torch.randperm(N, generator=g)[:R - 3]]).to(dev)
    x = torch.randn(R, width, generator=g).to(dev)
    update_and_check(ops, bank, support, labels, precision, rows, x, 0.5, f"N=4100 {precision}")
    flat = torch.randn(5 * width + 1, generator=g).to(dev)
    x5 = flat[1:].view(5, width)
    assert x5.data_ptr() % 16 != 0 and x5.is_contiguous()
    for momentum in (0.0, 0.9):
        update_and_check(ops, bank, support, labels, precision, rows[:5].to(torch.int32), x5, momentum,
                         f"N=4100 {precision} unaligned x momentum={momentum}")


@pytest.mark.parametrize("precision,width", [("fp32", 96), ("fp32", 100), ("fp16", 200)])
@pytest.mark.parametrize("momentum", [0.0, 0.5])
def test_row_rule_last_occurrence_wins(ops, dev, precision, width, momentum):
    N, C = 64, 6
    g = torch.Generator().manual_seed(3)
    base = torch.randn(N, width, generator=g)
    labels = sorted_labels(N, C, dev)
    rows = torch.tensor([3, 7, 3, 3, -1, N, N + 5, 7], device=dev)
    x = torch.randn(8, width, generator=g).to(dev)              # distinct rows
    assert winners(rows, N) == {3: 3, 7: 7}
    s1, s2 = base.to(dev), base.to(dev)
    b1, b2 = ops.SplitBank(s1, labels, precision), ops.SplitBank(s2, labels, precision)
    update_and_check(ops, b1, s1, labels, precision, rows, x, momentum, f"row rule {precision} {width}")
    b2.update_rows(s2, rows, x, momentum)
    # row 3 took item 3 and row 7 item 7, blended ONCE with the old row
    m = torch.tensor(momentum, dtype=torch.float32, device=dev)
    old = base.to(dev)
    for r, i in ((3, 3), (7, 7)):
        want = x[i] if momentum == 0 else m * old[r] + (1 - m) * x[i]
        assert same_bits(s1[r], want)
    moved = (bits(s1) != bits(old)).any(dim=1).nonzero().flatten().tolist()
    assert moved == [3, 7]
    # two banks given the same call end with identical bits
    assert same_bits(s1, s2)
    t1, t2 = bank_tensors(b1), bank_tensors(b2)
    assert set(t1) == set(t2)
    for k in t1:
        assert same_bits(t1[k], t2[k]), k


@pytest.mark.parametrize("precision,width", [("fp32", 96), ("fp32", 2080), ("fp16", 256)])
def test_special_values(ops, dev, precision, width):
    """An all-zero new row, one whose largest magnitude is subnormal, one holding +inf: the forms still equal the
    constructor's (every branch of the scale rule).  With momentum 0, -0.0 and a NaN payload arrive unchanged."""
    N, C = 64, 6
    g = torch.Generator().manual_seed(11)
    support = torch.randn(N, width, generator=g).to(dev)
    labels = sorted_labels(N, C, dev)
    bank = ops.SplitBank(support, labels, precision)
    x = torch.randn(3, width, generator=g)
    x[0] = 0.0
    x[1] = torch.randn(width, generator=g) * 1e-41
    x[2, width // 2] = float("inf")
    assert 0 < x[1].abs().max() < 1.1754944e-38
    x = x.to(dev)
    rows = torch.tensor([5, 40, 63], device=dev)
    for momentum in (0.0, 0.5):
        update_and_check(ops, bank, support, labels, precision, rows, x, momentum, f"special values {precision} {width} m={momentum}")
    # bit-exact transport with momentum 0
    xi = torch.randn(2, width, generator=g).view(torch.int32)
    xi[0, 1] = -2 ** 31                     # -0.0
    xi[0, 5] = 0x7fc12345                   # a quiet NaN with a payload
    xi[1, 0] = -4194304 + 0x00777           # 0xffc00777: a negative NaN with a payload
    xs = xi.view(torch.float32).to(dev)
    r2 = torch.tensor([9, 10], device=dev)
    old = support.clone()
    bank.update_rows(support, r2, xs, 0.0)
    assert torch.equal(support[r2].view(torch.int32), xi.to(dev))
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[r2] = False
    assert same_bits(support[keep], old[keep])


def test_old_entry_points_keep_their_bits(ops, dev, golden):
    """nw_split_rows_f16x2, nw_pack_rows_f16 and nw_row_norm2_f32 against the outputs recorded from the library before
    their per-row arithmetic moved into shared functions."""
    from nwhead_amd import _lib
    lib = _lib.load()
    z = golden("bank_forms.npz")
    st = torch.cuda.current_stream(dev).cuda_stream

    def u32(name):
        return torch.from_numpy(z[name].view(np.int32)).to(dev)

    for name in ("a", "b"):
        x = torch.from_numpy(z[f"{name}_x"]).to(dev)
        rows, d = x.shape
        assert (rows, d) == {"a": (64, 96), "b": (8, 2080)}[name]
        split = torch.empty_like(x)
        scale, norm2, plain = (torch.empty(rows, device=dev) for _ in range(3))
        _lib.check(lib.nw_split_rows_f16x2(x.data_ptr(), split.data_ptr(), scale.data_ptr(), norm2.data_ptr(), rows, d, st),
                   "nw_split_rows_f16x2")
        _lib.check(lib.nw_row_norm2_f32(x.data_ptr(), plain.data_ptr(), rows, d, st), "nw_row_norm2_f32")
        assert torch.equal(split.view(torch.int32), u32(f"{name}_split"))
        assert torch.equal(scale, torch.from_numpy(z[f"{name}_scale"]).to(dev))
        assert torch.equal(norm2.view(torch.int32), u32(f"{name}_norm2"))
        assert torch.equal(plain.view(torch.int32), u32(f"{name}_rownorm2"))
        assert torch.equal(ops.row_norm2(x).view(torch.int32), u32(f"{name}_rownorm2"))
        packed = torch.empty(rows, d, dtype=torch.float16, device=dev)
        assert lib.nw_pack_rows_f16(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), norm2.data_ptr(), rows, d, st) \
            == int(z[f"{name}_pack_status"]) == -2
    for name in ("pa", "pb"):
        x = torch.from_numpy(z[f"{name}_x"]).to(dev)
        rows, d = x.shape
        packed = torch.empty(rows, d, dtype=torch.float16, device=dev)
        scale, norm2 = (torch.empty(rows, device=dev) for _ in range(2))
        _lib.check(lib.nw_pack_rows_f16(x.data_ptr(), packed.data_ptr(), scale.data_ptr(), norm2.data_ptr(), rows, d, st),
                   "nw_pack_rows_f16")
        assert torch.equal(packed.view(torch.int16), torch.from_numpy(z[f"{name}_packed"].view(np.int16)).to(dev))
        assert torch.equal(scale, torch.from_numpy(z[f"{name}_scale"]).to(dev))
        assert torch.equal(norm2.view(torch.int32), u32(f"{name}_norm2"))


def test_served_without_a_rebuild(ops, dev, monkeypatch):
    """After update_rows the head, the windowed head and the neighbour search run over the bank as it stands and equal the
    same calls over a freshly built bank bit for bit; no N-row nw_split_rows_f16x2 call is made on the way."""
    from nwhead_amd import _lib
    B, N, d, C = 130, 1000, 64, 10
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, d, generator=g).to(dev)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = sorted_labels(N, C, dev)
    bank = ops.SplitBank(s, sy)
    rows = torch.randperm(N, generator=g)[:256].to(dev)
    x = torch.randn(256, d, generator=g).to(dev)
    lo = torch.arange(B, device=dev) * 7
    window = (lo, lo + 1)

    lib = _lib.load()
    real = lib.nw_split_rows_f16x2
    split_rows = []

    class Spy:
        def __getattr__(self, name):
            if name == "nw_split_rows_f16x2":
                return lambda *a: (split_rows.append(a[4]), real(*a))[1]
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", Spy())
    bank.update_rows(s, rows, x, 0.5)
    head = ops.nw_head(q, s, sy, C, support_cache=bank)
    loo = ops.nw_head(q, s, sy, C, support_cache=bank, row_window=window, exclude=True)
    knn = ops.nw_knn(q, bank, 5)
    assert N not in split_rows
    monkeypatch.undo()

    s2 = s.clone()
    fresh = ops.SplitBank(s2, sy)
    assert same_bits(head, ops.nw_head(q, s2, sy, C, support_cache=fresh))
    assert same_bits(loo, ops.nw_head(q, s2, sy, C, support_cache=fresh, row_window=window, exclude=True))
    assert torch.equal(knn, ops.nw_knn(q, fresh, 5))
    assert torch.isfinite(head).all() and torch.isfinite(loo).all()


def test_guards(ops, dev):
    from nwhead_amd._lib import NWHipError
    B, N, d, C = 40, 200, 64, 5
    g = torch.Generator().manual_seed(9)
    s = torch.randn(N, d, generator=g).to(dev)
    sy = sorted_labels(N, C, dev)
    rows = torch.tensor([1, 2, 3], device=dev)
    x = torch.randn(3, d, generator=g).to(dev)
    # the bank head's backward recomputes the scores from the bank: refused once the bank has been written
    bank = ops.SplitBank(s, sy)
    q = torch.randn(B, d, generator=g).to(dev).requires_grad_()
    out = ops.nw_head_bank(q, s, sy, C, bank)
    bank.update_rows(s, rows, x)
    with pytest.raises(RuntimeError, match="update_rows"):
        out.sum().backward()
    ops.nw_head_bank(q, s, sy, C, bank).sum().backward()          # a forward after the update is served
    assert torch.isfinite(q.grad).all()
    # nw_head saves the support itself: torch's own in-place check
    s.requires_grad_()
    out = ops.nw_head(q, s, sy, C, support_cache=bank)
    bank.update_rows(s, rows, x, 0.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    # another tensor than the bank's
    with pytest.raises(ValueError):
        bank.update_rows(s.detach().clone(), rows, x)
    # unsorted labels: the bank's rows are a class-sorted copy, not the caller's
    s3 = torch.randn(N, d, generator=g).to(dev)
    unsorted = torch.arange(N, device=dev) % C
    b3 = ops.SplitBank(s3, unsorted)
    assert b3.sorted_rows is not None
    keep = s3.clone()
    with pytest.raises(NWHipError, match="class-sorted copy"):
        b3.update_rows(s3, rows, x)
    # 20 rows: norms only
    s4 = torch.randn(20, d, generator=g).to(dev)
    b4 = ops.SplitBank(s4, sorted_labels(20, C, dev), precision="fp16")
    assert not b4.has_operand_rows
    with pytest.raises(NWHipError, match="norms-only"):
        b4.update_rows(s4, rows, x)
    with pytest.raises(NWHipError, match="width"):
        bank.update_rows(s, rows, x[:, :32])
    assert same_bits(s3, keep) and b3.writes == 0 and b4.writes == 0


def _harness_net(dev):
    """NWNet as the harness builds it for its test: 'tiny' featurizer, procedural images, 6 classes x 20."""
    from nwhead_amd.data import build_datasets
    from nwhead_amd.nwhead.nw import NWNet
    from nwhead_amd.train import build_featurizer
    torch.manual_seed(1)
    train_ds, _ = build_datasets("synthetic", "./", 32, 20, 6, 1, 2.5)
    featurizer, feat_dim = build_featurizer("tiny", True)
    net = NWNet(featurizer, 6, support_dataset=train_ds, feat_dim=feat_dim, n_shot=2, device="cuda:0").to(dev)
    return net


def test_nwnet_refresh_bank(ops, dev):
    net = _harness_net(dev).eval()
    net.precompute()
    N = net.full_feat.shape[0]
    assert N == 120 and net.full_cache.writes == 0
    ds = net.support_eval.full_datasets[0]
    rows = torch.tensor([0, 17, 33, 64, 119, 5, 90, 41], device=dev)
    x = torch.stack([ds[i][0] for i in rows.tolist()]).float().to(dev)
    y = torch.tensor([int(ds[i][1]) for i in rows.tolist()], device=dev)
    old = net.full_feat.clone()
    cache = net.full_cache
    out = net.forward_bank(x, leave_out=rows)
    torch.nn.functional.nll_loss(out, y).backward()
    feats = net.bank_features.clone()
    assert net.bank_features.shape == (8, 64) and not net.bank_features.requires_grad
    net.refresh_bank(rows)
    assert net.bank_features is None
    assert net.full_cache is cache and cache.writes == 1 and cache.matches(net.full_feat)
    assert same_bits(net.full_feat[rows], feats)
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[rows] = False
    assert same_bits(net.full_feat[keep], old[keep])
    with torch.no_grad():
        served = net.predict(x, "full")
        assert net.full_cache is cache                       # not rebuilt: it still matches
        net.full_cache = None                                # predict builds a new bank from full_feat
        rebuilt = net.predict(x, "full")
    assert net.full_cache is not cache and net.full_cache.writes == 0
    assert same_bits(served, rebuilt)
    with pytest.raises(ops.NWHipError, match="forward_bank first"):
        net.refresh_bank(rows)
    net.refresh_bank(rows[:2], feats=feats[:2], momentum=0.5)
    assert net.full_cache.writes == 1


def test_harness_trains_in_bank_mode(tmp_path, dev):
    from nwhead_amd.train import Trainer, make_parser
    argv = ["--dataset", "synthetic", "--arch", "tiny", "--models_dir", str(tmp_path), "--batch_size", "40",
            "--lr", "0.05", "--num_epochs", "2", "--log_interval", "2", "--seed", "1", "--n_shot", "2",
            "--synthetic_classes", "6", "--synthetic_per_class", "20", "--synthetic_size", "32",
            "--synthetic_noise", "2.5", "--scheduler_milestones", "3", "--train_type", "bank"]
    tr = Trainer(make_parser().parse_args(argv))
    steps = len(tr.train_loader)
    assert steps == 3
    hist = tr.fit()
    assert [h["epoch"] for h in hist] == [1, 2]
    for h in hist:
        assert np.isfinite(h["loss:train"]) and np.isfinite(h["loss:val:full"])
    net = tr.network
    assert net.full_cache.matches(net.full_feat)
    assert net.full_cache.writes == steps
