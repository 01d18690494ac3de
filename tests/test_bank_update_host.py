"""The in-place row update of a prepared bank, host side (no GPU): the refusal rule as a pure function, the argument
checks of nw_bank_update_rows_f32 through ctypes in the order the header lists them (the library answers before any HIP
call), the stand-alone sanitizer program of the entry (tests/sanitize/abi_args_bank_update.cpp: host-only AddressSanitizer
+ UndefinedBehaviorSanitizer build of the library's own sources against a HIP runtime stand-in; nothing is loaded into
python), and the harness's new flags."""
import ctypes
import math
import os
import subprocess

import pytest

NW_OK, NW_ERR_INVALID_ARG, NW_ERR_UNSUPPORTED = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_is_in_the_table():
    from nwhead_amd import _lib
    res, args = _lib.SIGNATURES["nw_bank_update_rows_f32"]
    assert res is ctypes.c_int and len(args) == 16 and args[4] is ctypes.c_float


REFUSAL_CASES = [
    # split, packed, sorted_copy, shape, pad, width, R -> word of the reason (None: served)
    (dict(split=True, packed=False, sorted_copy=False, shape=(64, 96), pad=0, width=96, R=5), None),
    (dict(split=True, packed=False, sorted_copy=False, shape=(64, 128), pad=28, width=100, R=1), None),
    (dict(split=False, packed=True, sorted_copy=False, shape=(64, 192), pad=128, width=64, R=256), None),
    (dict(split=True, packed=False, sorted_copy=False, shape=(50000, 512), pad=0, width=512, R=16384), None),
    (dict(split=True, packed=False, sorted_copy=False, shape=(64, 96), pad=0, width=96, R=0), None),
    (dict(split=True, packed=False, sorted_copy=True, shape=(64, 96), pad=0, width=96, R=5), "class-sorted copy"),
    (dict(split=False, packed=True, sorted_copy=True, shape=(64, 192), pad=0, width=192, R=5), "class-sorted copy"),
    (dict(split=False, packed=False, sorted_copy=False, shape=(20, 64), pad=0, width=64, R=5), "norms-only"),
    (dict(split=False, packed=False, sorted_copy=False, shape=(64, 48), pad=0, width=48, R=5), "norms-only"),
    (dict(split=True, packed=False, sorted_copy=False, shape=(64, 96), pad=0, width=64, R=5), "width 64"),
    (dict(split=True, packed=False, sorted_copy=False, shape=(64, 128), pad=28, width=128, R=5), "width 128"),
    (dict(split=False, packed=True, sorted_copy=False, shape=(64, 192), pad=128, width=192, R=5), "width 192"),
    (dict(split=True, packed=False, sorted_copy=False, shape=(50000, 512), pad=0, width=512, R=16385), "16385 rows"),
    # the first reason in the documented order is the one given
    (dict(split=False, packed=False, sorted_copy=True, shape=(64, 96), pad=0, width=64, R=99999), "class-sorted copy"),
    (dict(split=False, packed=False, sorted_copy=False, shape=(64, 96), pad=0, width=64, R=99999), "norms-only"),
    (dict(split=True, packed=False, sorted_copy=False, shape=(64, 96), pad=0, width=64, R=99999), "width 64"),
]


@pytest.mark.parametrize("facts,word", REFUSAL_CASES)
def test_bank_update_refusal_table(facts, word):
    from nwhead_amd import ops
    why = ops.bank_update_refusal(**facts)
    if word is None:
        assert why is None
    else:
        assert why is not None and word in why


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_argument_checks_in_documented_order_without_a_device():
    from nwhead_amd import _lib
    lib = _lib.load()
    keep, F = _aligned(4096)
    keep2, H = _aligned(4096)
    rows = (ctypes.c_int64 * 64)()
    RW = ctypes.addressof(rows)
    f = lib.nw_bank_update_rows_f32

    def call(x=F, rw=RW, R=8, dx=64, m=0.0, s_rows=F, s_user=None, s_norm2=F, s_split=F, s_scale=F, s_f16=None, f16_scale=None,
             f16_norm2=None, N=64, d=64):
        return f(x, rw, R, dx, m, s_rows, s_user, s_norm2, s_split, s_scale, s_f16, f16_scale, f16_norm2, N, d, None)

    half = dict(s_split=None, s_scale=None, s_f16=H, f16_scale=F, f16_norm2=F, dx=192, d=192, N=8)
    # 1. a negative size -- whatever else is wrong with the call
    assert call(R=-1) == NW_ERR_INVALID_ARG
    assert call(N=-1) == NW_ERR_INVALID_ARG
    assert call(d=-64) == NW_ERR_INVALID_ARG
    assert call(R=-1, x=None, s_split=None, s_scale=None) == NW_ERR_INVALID_ARG
    # 2. dx outside [1, d] -- before "nothing to do"
    for dx in (0, -1, 65):
        assert call(dx=dx) == NW_ERR_INVALID_ARG
        assert call(dx=dx, R=0) == NW_ERR_INVALID_ARG
    assert call(dx=1, d=0) == NW_ERR_INVALID_ARG
    # 3. momentum not finite or outside [0, 1) -- before "nothing to do"
    for m in (-0.25, 1.0, 2.0, math.inf, -math.inf, math.nan):
        assert call(m=m) == NW_ERR_INVALID_ARG
        assert call(m=m, N=0) == NW_ERR_INVALID_ARG
    # 4. R == 0 or N == 0: NW_OK before any pointer is looked at
    assert call(R=0, x=None, rw=None, s_rows=None, s_norm2=None, s_split=None, s_scale=None) == NW_OK
    assert call(N=0, x=None, rw=None, s_rows=None, s_norm2=None, s_split=None, s_scale=None, m=0.5) == NW_OK
    assert call(R=0, s_rows=F + 4, s_scale=None, dx=20, d=20) == NW_OK
    # 5. null x, rows, s_rows, s_norm2 -- before the form groups are looked at
    for name in ("x", "rw", "s_rows", "s_norm2"):
        assert call(**{name: None}) == NW_ERR_INVALID_ARG
        assert call(**{name: None}, s_split=None, s_scale=None) == NW_ERR_INVALID_ARG
    # 6. a form group given in part -- before the alignment
    assert call(s_scale=None) == NW_ERR_INVALID_ARG
    assert call(s_split=None) == NW_ERR_INVALID_ARG
    assert call(s_scale=None, s_rows=F + 4) == NW_ERR_INVALID_ARG
    for name in ("s_f16", "f16_scale", "f16_norm2"):
        assert call(**{**half, name: None}) == NW_ERR_INVALID_ARG
        assert call(**{**half, name: None, "s_split": F, "s_scale": F}) == NW_ERR_INVALID_ARG
    # 7. s_rows, s_split or s_f16 not 16-byte aligned -- before the shape rules; x may have any alignment
    assert call(s_rows=F + 4) == NW_ERR_INVALID_ARG
    assert call(s_split=F + 8) == NW_ERR_INVALID_ARG
    assert call(**{**half, "s_f16": H + 2}) == NW_ERR_INVALID_ARG
    assert call(s_rows=F + 4, s_split=None, s_scale=None) == NW_ERR_INVALID_ARG
    assert call(s_split=F + 8, dx=48, d=48) == NW_ERR_INVALID_ARG
    # 8. neither form group: a norms-only bank
    assert call(s_split=None, s_scale=None) == NW_ERR_UNSUPPORTED
    assert call(s_split=None, s_scale=None, x=F + 4, dx=20, d=20, R=99999) == NW_ERR_UNSUPPORTED
    # 9. the split group with d % 32 != 0
    assert call(dx=48, d=48) == NW_ERR_UNSUPPORTED
    assert call(dx=20, d=100, s_user=F, R=99999) == NW_ERR_UNSUPPORTED
    # 10. the fp16 group with d % 64 != 0 or d < 192
    for d in (224, 128, 64):
        assert call(**{**half, "dx": d, "d": d}) == NW_ERR_UNSUPPORTED
    assert call(**{**half, "dx": 96, "d": 96, "s_split": F, "s_scale": F, "R": 99999}) == NW_ERR_UNSUPPORTED
    # 11. more items than a wave scans
    assert call(R=16385) == NW_ERR_UNSUPPORTED
    assert call(**{**half, "R": 16385, "m": 0.9}) == NW_ERR_UNSUPPORTED
    del keep, keep2


def test_sanitizer_program_builds_and_exits_0():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "nwhead_amd", "csrc"), "sanitize_bank_update", "-j4"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "abi_args_bank_update: all argument checks refused as documented" in r.stdout
    assert "runtime error" not in r.stdout + r.stderr and "AddressSanitizer" not in r.stdout + r.stderr


def test_harness_parser_has_the_bank_flags():
    from nwhead_amd.train import make_parser
    p = make_parser()
    a = p.parse_args([])
    assert a.train_type == "random" and a.bank_momentum == 0.5
    a = p.parse_args(["--train_type", "bank", "--bank_momentum", "0.9"])
    assert a.train_type == "bank" and a.bank_momentum == 0.9
    with pytest.raises(SystemExit):
        p.parse_args(["--train_type", "episodic"])
