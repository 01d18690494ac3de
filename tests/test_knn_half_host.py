"""The half-precision neighbour search's host-side surface (no GPU): the launch decision of the candidate form of the
256-query kernel (nw_debug_fwd_plan), nw_knn_f16_workspace_bytes, and the stand-alone sanitizer program of the two new
entries (tests/sanitize/abi_args_knn_f16.cpp: host-only AddressSanitizer + UndefinedBehaviorSanitizer build of the
library's own sources against a HIP runtime stand-in; nothing is loaded into python)."""
import os
import subprocess

NW_OK, NW_ERR_UNSUPPORTED = 0, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from nwhead_amd import _lib
    return _lib


def _plan(**kw):
    return _lib().fwd_plan(256, 50000, 512, 1, form="half", outputs="candidates", k=10, cus=256, **kw)


def test_plan_of_the_candidate_form():
    p = _plan()
    assert p.status == NW_OK
    assert p.persistent and p.variant == 3 and p.rs == 8 and p.n_stiles == 391 and not p.run_tables
    assert p.split_queries                      # the pack launch of the queries
    assert p.workgroups == 256
    assert _plan(persistent_wgs=250).workgroups == 248


def test_plan_still_refuses_what_the_half_form_does_not_cover():
    L = _lib()
    assert L.fwd_plan(256, 50000, 512, 1, form="half", outputs="scores", cus=256).status == NW_ERR_UNSUPPORTED
    assert L.fwd_plan(256, 50000, 100, 1, form="half", outputs="candidates", k=10, cus=256).status == NW_ERR_UNSUPPORTED
    assert L.fwd_plan(256, 50000, 512, 1, form="half", outputs="candidates", k=33, cus=256).status == NW_ERR_UNSUPPORTED
    assert L.fwd_plan(256, 50000, 512, 1, form="half", outputs="candidates", k=0, cus=256).status == NW_ERR_UNSUPPORTED


def _cand_slots(k, bs=128):
    return (min(k, bs) + 3) & ~3


def test_workspace_bytes():
    f = _lib().load().nw_knn_f16_workspace_bytes
    assert f(256, 50000, 100, 10) == 0 and f(256, 50000, 512, 33) == 0
    assert f(0, 50000, 512, 10) == 0 and f(256, 25, 512, 10) == 0 and f(256, 30, 512, 31) == 0
    # the grid of test_knn_fused_host.py
    Ns = [26, 27, 32, 33, 100, 400, 1000, 1001, 1999, 2000, 2100, 4100, 8000, 10000, 16000, 20000, 32000, 33000, 50000, 400000]
    Bs = [1, 37, 64, 65, 130, 200, 256, 257, 512, 1000, 4096]
    ks = [1, 4, 5, 10, 20, 32]
    for d in (192, 512):
        tab = {(B, N, k): f(B, N, d, k) for B in Bs for N in Ns for k in ks}
        assert all((v > 0) == (k <= N) for (B, N, k), v in tab.items())
        for (B, N, k), v in tab.items():
            if k > N:
                continue
            for B2 in Bs[Bs.index(B) + 1:][:1]:
                assert tab[(B2, N, k)] >= v, (B, B2, N, k, d)
            for N2 in Ns[Ns.index(N) + 1:][:1]:
                assert tab[(B, N2, k)] >= v, (B, N, N2, k, d)
            for k2 in [x for x in ks[ks.index(k) + 1:][:1] if x <= N]:
                assert tab[(B, N, k2)] >= v, (B, N, k, k2, d)
            # keys and rows of every (query, tile, slot) + the packed queries (fp16) with their scales and norms
            closed = 2 * 4 * B * -(-N // 128) * _cand_slots(k) + (2 * B * d + 2 * 4 * B)
            assert v >= closed, (B, N, k, d, v, closed)


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_knn_f16", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_knn_f16: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr
