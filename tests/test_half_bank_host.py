"""The half-precision bank's host-side surface (no GPU): the new C symbol is declared, exported and bound, and
nw_fwd_opts.operand_form sits in the slot older headers call `reserved`, with the struct's size and offsets unchanged."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "nwhead_hip.h")).read()


def test_header_declares_and_library_exports_pack_rows():
    from nwhead_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+nw_pack_rows_f16\s*\(\s*const\s+float\s*\*\s*x\s*,\s*uint16_t\s*\*\s*out_rows\s*,", code)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "nw_pack_rows_f16")
    res, args = _lib.SIGNATURES["nw_pack_rows_f16"]
    assert res is ctypes.c_int and len(args) == 7


def test_pack_rows_argument_checks_without_gpu():
    from nwhead_amd import _lib
    lib = _lib.load()
    assert lib.nw_pack_rows_f16(None, None, None, None, -1, 64, None) == -1      # negative size
    assert lib.nw_pack_rows_f16(None, None, None, None, 4, 96, None) == -2       # d % 64 != 0
    assert lib.nw_pack_rows_f16(None, None, None, None, 0, 64, None) == 0        # nothing to do
    assert lib.nw_pack_rows_f16(None, None, None, None, 4, 64, None) == -1       # null pointers


def test_operand_form_fills_the_reserved_slot():
    from nwhead_amd import _lib
    F = _lib.FwdOpts
    # the layout of ABI version 2: uint32 size, three int32, pointer, size_t, pointer, int64
    assert ctypes.sizeof(F) == 48
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [
        ("struct_size", 0), ("persistent_wgs", 4), ("force_split", 8), ("operand_form", 12), ("tables", 16),
        ("tables_bytes", 24), ("tables_sy", 32), ("tables_N", 40)]
    op = _lib.fwd_opts(operand_form=1)
    assert op.operand_form == 1 and op.struct_size == 48
    assert ctypes.cast(ctypes.addressof(op) + 12, ctypes.POINTER(ctypes.c_int32))[0] == 1
    assert _lib.fwd_opts().operand_form == 0
    # the C declaration: same field order, the fourth field renamed
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct nw_fwd_opts \{(.*?)\} nw_fwd_opts;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+);", body)
    assert names == ["struct_size", "persistent_wgs", "force_split", "operand_form", "tables", "tables_bytes", "tables_sy",
                     "tables_N"]
    assert "#define NW_ABI_VERSION 2" in code


def test_forward_refuses_unknown_operand_form_and_bad_half_shapes_before_any_launch():
    """Argument validation needs no device: null data pointers never get dereferenced on these paths."""
    from nwhead_amd import _lib
    lib = _lib.load()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)          # any non-null address: the calls below return before reading it

    def fwd(op, d, scores=None, sup_b=0):
        return lib.nw_fwd_f32(p, p, p, p, p, p, p, scores, None, None, None, 0, 4, 100, d, 5, 0, None, sup_b, 0,
                              ctypes.addressof(op), None)

    assert fwd(_lib.fwd_opts(operand_form=7), 256) == -1
    half = _lib.fwd_opts(operand_form=1)
    assert fwd(half, 128) == -2                  # fewer than three 64-k stages
    assert fwd(half, 224) == -2                  # d % 64 != 0
    assert fwd(half, 256, scores=p) == -2        # per-pair outputs
    assert fwd(half, 256, sup_b=1) == -2         # batched supports
    assert lib.nw_fwd_influence_f32(p, p, p, p, p, p, p, p, None, p, None, 0, 4, 100, 256, 5, 0, None,
                                    ctypes.addressof(half), None) == -2


def test_workspace_covers_the_half_forms_tile_layout():
    """Form 1 walks the bank in tiles of 128 supports at every size: m, den (tiles x B) and num (tiles x 128 x B) must fit."""
    from nwhead_amd import _lib
    lib = _lib.load()
    for B, N, d, C in ((1, 26, 192, 200), (257, 129, 256, 200), (300, 1100, 192, 200), (64, 640, 448, 200),
                       (256, 50000, 512, 200)):
        tiles = -(-N // 128)
        assert lib.nw_fwd_workspace_bytes(B, N, d, C) >= 4 * tiles * B * (2 + 128) + 2 * B * d
