"""Runs ycx_conv2d_pair_pool on the kernel-side bounds-check library (YCX_LIB=libycx_hip_dbg.so)
at the three shapes of tests/test_gpu_conv_trio.py and prints one JSON line with the
store-violation count. Launched as a subprocess by that test."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "yolo-continuous_amd"),
                os.path.dirname(os.path.dirname(HERE))]

import torch  # noqa: E402

from trio_case import TrioCase  # noqa: E402
from ycx import _lib as L  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = (ctypes.c_uint32 * 2)()
    assert L.lib.ycx_debug_bounds(out, 1) == 0, "not the YCX_DEBUG_BOUNDS library"
    runs, equal = 0, True
    for shape, cin, cout_b, cout_c, store_a in (((1, 2, 32), 64, 128, 128, True), ((3, 6, 96), 128, 248, 120, False),
                                                ((2, 64, 160), 256, 128, 128, True)):
        case = TrioCase(dev, L.DT_BF16, shape, cin, cout_b, cout_c, (L.ACT_SILU_PS,) * 3)
        ref = case.unfused()
        got = case.fused(store_a)
        equal = equal and all(torch.equal(a, b) for a, b in list(zip(got, ref))[0 if store_a else 1:])
        runs += 1
    torch.cuda.synchronize()
    assert L.lib.ycx_debug_bounds(out, 0) == 0
    print(json.dumps({"runs": runs, "violations": int(out[0]), "first_line": int(out[1]), "equal": bool(equal)}))


if __name__ == "__main__":
    main()
