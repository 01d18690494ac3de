"""Record what the row preparation entry points (nw_split_rows_f16x2, nw_pack_rows_f16, nw_row_norm2_f32) write, for
tests/test_bank_update_gpu.py::test_old_entry_points_keep_their_bits (needs the MI355X):

    python tests/golden/record_bank_forms.py <root of a checkout of the PARENT of the change under test, built> tests/golden/bank_forms.npz

nwhead_amd is imported from the checkout named.  bank_forms.npz was recorded from commit 996d875 (before the per-row
arithmetic moved into row_forms.h).  It must never be recorded from the tree it is used to test.

Shapes: 64 x 96 (in registers) and 8 x 2080 (streamed) for the split rows and the plain norms.  nw_pack_rows_f16 takes
widths that are multiples of 64 only, so its records are the nearest such shapes, 64 x 192 and 8 x 2112; its status at the
other two widths is recorded as well.  Rows 1..3 of every input are a row of zeros, a row whose largest magnitude is
subnormal and a row holding +inf: every branch of the scale rule."""
import os
import sys

os.environ.setdefault("NW_SPLIT_ALWAYS", "1")        # as tests/conftest.py pins it
sys.path.insert(0, os.path.abspath(sys.argv[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nwhead_amd import _lib  # noqa: E402

SHAPES = {"a": (64, 96), "b": (8, 2080), "pa": (64, 192), "pb": (8, 2112)}


def make_input(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, 1), generator=g).float())
    x[1] = 0.0
    x[2] = torch.randn(d, generator=g) * 1e-41
    x[3, d // 3] = float("inf")
    return x


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    rec = {}
    for seed, (name, (rows, d)) in enumerate(sorted(SHAPES.items())):
        x = make_input(rows, d, 100 + seed)
        xd = x.to(dev)
        rec[f"{name}_x"] = x.numpy()
        if name in ("a", "b"):
            split = torch.empty_like(xd)
            scale, norm2, plain = (torch.empty(rows, device=dev) for _ in range(3))
            _lib.check(lib.nw_split_rows_f16x2(xd.data_ptr(), split.data_ptr(), scale.data_ptr(), norm2.data_ptr(), rows, d, st),
                       "nw_split_rows_f16x2")
            _lib.check(lib.nw_row_norm2_f32(xd.data_ptr(), plain.data_ptr(), rows, d, st), "nw_row_norm2_f32")
            packed = torch.empty(rows, d, dtype=torch.float16, device=dev)
            rc = lib.nw_pack_rows_f16(xd.data_ptr(), packed.data_ptr(), scale.data_ptr(), norm2.data_ptr(), rows, d, st)
            torch.cuda.synchronize()
            rec[f"{name}_pack_status"] = np.int64(rc)
            # the fp32 words of the split rows hold fp16 pairs: kept as raw 32-bit patterns (a NaN pattern must survive)
            rec[f"{name}_split"] = split.cpu().numpy().view(np.uint32)
            rec[f"{name}_scale"], rec[f"{name}_norm2"] = scale.cpu().numpy(), norm2.cpu().numpy().view(np.uint32)
            rec[f"{name}_rownorm2"] = plain.cpu().numpy().view(np.uint32)
        else:
            packed = torch.empty(rows, d, dtype=torch.float16, device=dev)
            scale, norm2 = (torch.empty(rows, device=dev) for _ in range(2))
            _lib.check(lib.nw_pack_rows_f16(xd.data_ptr(), packed.data_ptr(), scale.data_ptr(), norm2.data_ptr(), rows, d, st),
                       "nw_pack_rows_f16")
            torch.cuda.synchronize()
            rec[f"{name}_packed"] = packed.cpu().numpy().view(np.uint16)
            rec[f"{name}_scale"], rec[f"{name}_norm2"] = scale.cpu().numpy(), norm2.cpu().numpy().view(np.uint32)
    print(f"{len(rec)} arrays, {sum(a.nbytes for a in rec.values())} bytes, library {_lib.LIB_PATH}")
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], **rec)


main()
