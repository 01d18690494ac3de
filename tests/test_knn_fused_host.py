"""The fused neighbour search's host-side surface (no GPU): nw_knn_workspace_bytes / nw_knn_f32 are declared, exported and
bound; the workspace answer is small, non-decreasing in B, N and k, and zero exactly where nw_knn_f32 refuses the shape."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nwhead_hip.h")).read(), flags=re.S)


def _lib():
    from nwhead_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound():
    L = _lib()
    code = _code()
    assert re.search(r"\bsize_t\s+nw_knn_workspace_bytes\s*\(\s*int64_t\s+B\s*,\s*int64_t\s+N\s*,\s*int64_t\s+d\s*,\s*int64_t\s+k\s*\)",
                     code)
    m = re.search(r"\bint\s+nw_knn_f32\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["q", "s_split", "s_scale", "s_norm2", "idx_out", "val_out", "workspace", "workspace_bytes", "B", "N", "d",
                     "k", "kind", "logit_scale_dev", "stream"]
    assert os.path.exists(L.LIB_PATH), "run __graft_entry__.build() first"
    so = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(so, "nw_knn_workspace_bytes") and hasattr(so, "nw_knn_f32")
    res, args = L.SIGNATURES["nw_knn_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int64] * 4
    res, args = L.SIGNATURES["nw_knn_f32"]
    assert res is ctypes.c_int and len(args) == 15
    assert args[7] is ctypes.c_size_t and args[8:12] == [ctypes.c_int64] * 4 and args[12] is ctypes.c_int


def test_abi_version_stays_2():
    assert _lib().load().nw_abi_version() == 2
    assert "#define NW_ABI_VERSION 2" in _code()


def test_workspace_is_a_fraction_of_the_score_matrix():
    ws = _lib().load().nw_knn_workspace_bytes(256, 50000, 512, 10)
    assert 0 < ws < 256 * 50000 * 4 // 4


def test_workspace_is_monotone_in_B_N_and_k():
    """Also across the shapes at which the tile height changes (a taller tile means fewer candidate slots)."""
    lib = _lib().load()
    f = lib.nw_knn_workspace_bytes
    Ns = [26, 27, 32, 33, 100, 400, 1000, 1001, 1999, 2000, 2100, 4100, 8000, 10000, 16000, 20000, 32000, 33000, 50000, 400000]
    Bs = [1, 37, 64, 65, 130, 200, 256, 257, 512, 1000, 4096]
    ks = [1, 4, 5, 10, 20, 32]
    for d in (32, 512):
        tab = {(B, N, k): f(B, N, d, k) for B in Bs for N in Ns for k in ks}
        assert all((v > 0) == (k <= N) for (B, N, k), v in tab.items())      # k > N is no search: refused, no workspace
        for B in Bs:
            for N in Ns:
                for k in ks:
                    v = tab[(B, N, k)]
                    if k > N:
                        continue
                    for B2 in Bs[Bs.index(B) + 1:][:1]:
                        assert tab[(B2, N, k)] >= v, (B, B2, N, k, d)
                    for N2 in Ns[Ns.index(N) + 1:][:1]:
                        assert tab[(B, N2, k)] >= v, (B, N, N2, k, d)
                    for k2 in [x for x in ks[ks.index(k) + 1:][:1] if x <= N]:
                        assert tab[(B, N, k2)] >= v, (B, N, k, k2, d)
    # every N of one stretch where a smaller bank needs MORE slots than a larger one on taller tiles
    prev = 0
    for N in range(1900, 2300):
        v = f(256, N, 512, 10)
        assert v >= prev, N
        prev = v


def test_unsupported_shapes_have_no_workspace_and_are_refused():
    """Argument validation needs no device: the data pointers are never read on these paths."""
    lib = _lib().load()
    buf = (ctypes.c_float * 8)()
    p = (ctypes.addressof(buf) + 15) & ~15          # any non-null 16-byte aligned address

    def knn(B, N, d, k, kind=0, ws=p, ws_bytes=0, q=p, ls=None):
        return lib.nw_knn_f32(q, p, p, p, p, None, ws, ws_bytes, B, N, d, k, kind, ls, None)

    for B, N, d, k in ((4, 100, 64, 0), (4, 100, 64, 33), (4, 30, 64, 31), (4, 25, 32, 5), (4, 100, 48, 5), (4, 100, 0, 5),
                       (4, 100, 100, 5), (4, 1 << 30, 64, 5), (1 << 30, 100, 64, 5)):
        assert lib.nw_knn_workspace_bytes(B, N, d, k) == 0, (B, N, d, k)
        assert knn(B, N, d, k) == -2, (B, N, d, k)                     # NW_ERR_UNSUPPORTED
    assert lib.nw_knn_workspace_bytes(-1, 100, 64, 5) == 0 and knn(-1, 100, 64, 5) == -1
    assert knn(4, 100, 64, 5, kind=9) == -2                            # unknown score kind
    assert knn(4, 100, 64, 5, kind=4) == -1                            # CLIP without its logit scale
    assert knn(4, 100, 64, 5, q=None) == -1                            # null pointers
    assert knn(4, 100, 64, 5, q=p + 4) == -1                           # misaligned queries
    need = lib.nw_knn_workspace_bytes(4, 100, 64, 5)
    assert need > 0
    assert knn(4, 100, 64, 5, ws=None, ws_bytes=need) == -3            # NW_ERR_WORKSPACE
    assert knn(4, 100, 64, 5, ws=p, ws_bytes=need - 1) == -3
    assert lib.nw_knn_workspace_bytes(0, 100, 64, 5) == 0 and knn(0, 100, 64, 5) == 0   # nothing to do


def test_python_entry_refuses_what_it_cannot_search():
    import pytest
    import torch
    from nwhead_amd import ops
    with pytest.raises(ops.NWHipError):
        ops.nw_knn(torch.zeros(2, 32), None, 1)                       # a CPU tensor, before anything else


def test_size_rule_of_the_bank_route_scores_is_exported():
    """nw_knn follows the library's own rule for which tile kernel writes the bank-route scores of a shape."""
    L = _lib()
    assert re.search(r"\bint\s+nw_scores_use_split\s*\(\s*int64_t\s+B\s*,\s*int64_t\s+N\s*,\s*int64_t\s+d\s*\)", _code())
    f = L.load().nw_scores_use_split
    assert f(256, 2048, 512) == 1 and f(256, 10000, 512) == 1 and f(256, 50000, 512) == 1
    assert f(64, 10000, 128) == 0 and f(8, 2048, 64) == 0 and f(0, 1 << 20, 512) == 0
    assert f(1, 390625, 512) == 1 and f(1, 390624, 512) == 0            # 2e8 multiply-adds, exactly
    assert f(1 << 30, 1 << 30, 1 << 20) == 1                            # no integer overflow on the way


def test_callers_size_gate():
    from nwhead_amd import ops
    assert ops.KNN_FUSED_MIN_SCORE_BYTES == 1 << 30
    assert not ops.knn_fused_pays(256, 50000) and not ops.knn_fused_pays(256, (1 << 20) - 1)
    assert ops.knn_fused_pays(256, 1 << 20) and ops.knn_fused_pays(256, 2150000)
