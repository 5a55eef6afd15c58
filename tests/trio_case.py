"""One ycx_conv2d_pair_pool problem (the 1x1 pair plus the MP branch's pooled 1x1) with its
unfused counterpart, shared by tests/test_gpu_conv_trio.py and tests/probes/bounds_trio.py.

The frame of the exact files (tests/helpers.py): x is the slice at channel 8 of a buffer 8 + cin + 8
wide with NaN around it, between NaN guards inside one allocation; each of the three outputs is the
interior slice of a sentinel-filled buffer (ya at 16 of 16 + 256 + 8, yb at 8 of 8 + cout_b + 8, yc at 16
of 16 + cout_c + 8); the padding rows cout .. cout_pad of w_b / w_c and of their biases are live (drawn
like the rows in front of them), so a stored padding channel is a value."""
import ctypes

import torch

from helpers import IN_TAIL, OUT_TAIL, SENTINEL, guard_elems, guarded
from ycx import _lib as L

X_OFF, YA_OFF, YB_OFF, YC_OFF = 8, 16, 8, 16
YA_STRIDE = YA_OFF + 256 + OUT_TAIL


def desc_1x1(n, h, w, cin, cout, cpad, in_off, in_stride, out_off, out_stride, act, dtype, in_pool=0):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = n, h, w, cin, in_off, in_stride
    d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = h, w, cout, cpad, out_off, out_stride
    d.kh = d.kw = 1
    d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout, d.in_pool = 1, 0, act, 0.1, dtype, L.OUT_NHWC, in_pool
    return d


class TrioCase:
    """device None: the operands and descriptors only (tests/test_conv_exact_plan.py)."""

    def __init__(self, device, dtype, shape, cin, cout_b, cout_c, acts, cpad_c=128):
        n, h, w = shape
        self.device, self.dtype, self.shape = device, dtype, shape
        self.tdt = tdt = torch.bfloat16 if dtype == L.DT_BF16 else torch.float16
        self.cin, self.cout_b, self.cout_c, self.acts = cin, cout_b, cout_c, acts
        self.cpad_b = cpad_b = 128 if cout_b <= 128 else 256
        g = torch.Generator().manual_seed(1000 * cin + 10 * cout_b + n + h)
        x = torch.full((n, h, w, X_OFF + cin + IN_TAIL), float('nan'), dtype=tdt)
        x[..., X_OFF:X_OFF + cin] = torch.randn(n, h, w, cin + X_OFF, generator=g)[..., X_OFF:].to(tdt)
        wa = (torch.randn(256, cin, generator=g) / cin ** 0.5).to(tdt)
        ba = torch.randn(256, generator=g) * 0.1
        wb = (torch.randn(cout_b, 256, generator=g) / 16.0).to(tdt)
        bb = torch.randn(cout_b, generator=g) * 0.1
        wc = (torch.randn(cout_c, 256, generator=g) / 16.0).to(tdt)
        bc = torch.randn(cout_c, generator=g) * 0.1

        def padded(wt, b, rows):  # live padding rows, drawn after everything else and like the rows before them
            extra = rows - wt.shape[0]
            if extra == 0:
                return wt, b
            wx, bx = (torch.randn(extra, 256, generator=g) / 16.0).to(tdt), torch.randn(extra, generator=g) * 0.1
            assert bool(wx.any(1).all()) and bool((bx != 0).all())
            return torch.cat([wt, wx]), torch.cat([b, bx])

        wb, bb = padded(wb, bb, cpad_b)
        wc, bc = padded(wc, bc, max(cpad_c, 128))
        self.host = dict(x=x, wa=wa, ba=ba, wb=wb, bb=bb, wc=wc, bc=bc)
        in_stride = X_OFF + cin + IN_TAIL
        self.x_guard = guard_elems(0, w, in_stride, 2)
        if device is not None:
            self.dev = {k: v.to(device) for k, v in self.host.items() if k != 'x'}
            self.dev['x'] = guarded(x, self.x_guard, device)
        self.da = desc_1x1(n, h, w, cin, 256, 256, X_OFF, in_stride, YA_OFF, YA_STRIDE, acts[0], dtype)
        self.db = desc_1x1(n, h, w, 256, cout_b, cpad_b, YA_OFF, YA_STRIDE, YB_OFF, YB_OFF + cout_b + OUT_TAIL, acts[1],
                           dtype)
        self.dc = desc_1x1(n, h // 2, w // 2, 256, cout_c, cpad_c, YA_OFF, YA_STRIDE, YC_OFF,
                           YC_OFF + cout_c + OUT_TAIL, acts[2], dtype, in_pool=1)

    def outputs(self):
        """The three output buffers, sentinel-filled."""
        n, h, w = self.shape
        z = dict(dtype=self.tdt, device=self.device)
        return (torch.full((n, h, w, YA_STRIDE), SENTINEL, **z),
                torch.full((n, h, w, YB_OFF + self.cout_b + OUT_TAIL), SENTINEL, **z),
                torch.full((n, h // 2, w // 2, YC_OFF + self.cout_c + OUT_TAIL), SENTINEL, **z))

    def fused_status(self, ya, yb, yc, store_a=True):
        t = self.dev
        return L.lib.ycx_conv2d_pair_pool(
            ctypes.byref(self.da), ctypes.byref(self.db), ctypes.byref(self.dc), t['x'].data_ptr(),
            t['wa'].data_ptr(), t['ba'].data_ptr(), ya.data_ptr() if store_a else None, t['wb'].data_ptr(),
            t['bb'].data_ptr(), yb.data_ptr(), t['wc'].data_ptr(), t['bc'].data_ptr(), yc.data_ptr(),
            L.stream_handle(self.device))

    def fused(self, store_a):
        ya, yb, yc = self.outputs()
        L.check(self.fused_status(ya, yb, yc, store_a))
        torch.cuda.synchronize()
        return ya, yb, yc

    def unfused(self):
        """ycx_conv2d_pair with the first map stored, then ycx_conv2d (in_pool = 1) on it."""
        ya, yb, yc = self.outputs()
        t, st = self.dev, L.stream_handle(self.device)
        L.check(L.lib.ycx_conv2d_pair(ctypes.byref(self.da), ctypes.byref(self.db), t['x'].data_ptr(),
                                      t['wa'].data_ptr(), t['ba'].data_ptr(), ya.data_ptr(), t['wb'].data_ptr(),
                                      t['bb'].data_ptr(), yb.data_ptr(), st))
        L.check(L.lib.ycx_conv2d(ctypes.byref(self.dc), ya.data_ptr(), t['wc'].data_ptr(), t['bc'].data_ptr(),
                                 yc.data_ptr(), None, st))
        torch.cuda.synchronize()
        return ya, yb, yc
