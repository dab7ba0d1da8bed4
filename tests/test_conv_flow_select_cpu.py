"""CPU: `tdvc_conv_desc::flow` and `tdvc_conv_flow_supported` are host arithmetic on the descriptor.  A descriptor whose flow is NULL
selects what the recorded dispatch (tests/golden/conv_dispatch.npz) says, the query answers without a device, and only the lean epilogue
of conv_mfma_v5 says yes."""
import ctypes as C
import os

import numpy as np

from tdvc_amd import _lib as L, ops

from tests import helpers_conv_dispatch as H

PFLOW = 0x90000000          # a dummy 16-byte aligned address, never dereferenced


def _select(lib, d):
    name = lib.tdvc_conv_select(C.byref(d))
    return H.REJECTED if name is None else name.decode()


def _flow(N, Ho, Wo, Cc=2, dtype=None):
    return H.fmap(L, PFLOW, N, Ho, Wo, Cc, dtype=L.F32 if dtype is None else dtype)


def test_descriptors_without_flow_select_what_they_selected():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", H.GOLDEN))
    names = [str(n) for n in g["names"]]
    descs, _ = H.sweep(L, ops._pick_ck)
    lib = L.lib()
    picks = [int(i) for i in np.linspace(0, len(descs) - 1, 10)]           # ten descriptors spread over the sweep's sections
    v5 = [i for i, k in enumerate(g["kernel"]) if names[k] == "conv_mfma_v5"][:3]
    for i in picks + v5:
        d = descs[i]
        assert d.flow.p is None                                            # the sweep sets none of the new fields
        assert _select(lib, d) == names[g["kernel"][i]], i
        assert lib.tdvc_conv_chan_sum_rows(C.byref(d)) == int(g["rows"][i]), i
    assert C.sizeof(L.ConvDesc) % 8 == 0 and L.ConvDesc.flow.offset + C.sizeof(L.FMapDesc) == C.sizeof(L.ConvDesc)      # the last field
    assert lib.tdvc_abi_version() >= 11


def test_flow_supported_answers_without_a_device():
    lib = L.lib()
    lr = dict(act=2, slope=0.1)
    ff = lambda H_, W_, **kw: H.desc(L, ops._pick_ck, 128, 64, H.WINDOWS[0], H_, W_, 1, **{**lr, **kw})
    d = ff(272, 480)                                                       # OffsetGen's level-1 fusion conv: 1x1 128 -> 64, LeakyReLU
    assert _select(lib, d) == "conv_mfma_v5" and lib.tdvc_conv_flow_supported(C.byref(d)) == 1
    d.flow = _flow(1, 272, 480)
    assert lib.tdvc_conv_flow_supported(C.byref(d)) == 1 and _select(lib, d) == "conv_mfma_v5"
    d.flow = _flow(1, 272, 480, Cc=4)                                      # a window of a wider flow map
    assert lib.tdvc_conv_flow_supported(C.byref(d)) == 1
    # 128 output channels: two blocks of 64, the same epilogue
    d2 = H.desc(L, ops._pick_ck, 128, 128, H.WINDOWS[0], 272, 480, 1, **lr)
    assert _select(lib, d2) == "conv_mfma_v5" and lib.tdvc_conv_flow_supported(C.byref(d2)) == 1
    # the map counts once it is given: wrong geometry, one channel, fp16
    for bad in (_flow(1, 272, 479), _flow(2, 272, 480), _flow(1, 272, 480, Cc=1), _flow(1, 272, 480, Cc=8, dtype=L.F16)):
        d.flow = bad
        assert lib.tdvc_conv_flow_supported(C.byref(d)) == 0
        assert lib.tdvc_conv_select(C.byref(d)) is None and b"flow" in lib.tdvc_last_error()
    # kernels that do not add it: the small-map kernel, a 3x3 layer, v5's other epilogues (fp32 output, no bias), the fp32 path
    others = [ff(32, 32), H.desc(L, ops._pick_ck, 64, 64, H.WINDOWS[1], 272, 480, 1, **lr), ff(272, 480, out="f32"), ff(272, 480, bias=False),
              H.desc(L, ops._pick_ck, 128, 64, H.WINDOWS[0], 272, 480, 1, x_f32=True, out="f32")]
    for o in others:
        before = _select(lib, o)
        assert before != H.REJECTED and lib.tdvc_conv_flow_supported(C.byref(o)) == 0, before
        o.flow = _flow(1, o.y.H, o.y.W)
        assert lib.tdvc_conv_flow_supported(C.byref(o)) == 0
        assert lib.tdvc_conv_select(C.byref(o)) is None, before
    assert _select(lib, others[0]) == H.REJECTED and _select(lib, ff(32, 32)) == "conv_mfma_v9"
    assert lib.tdvc_conv_flow_supported(None) < 0
    # the broadcast form is a v5 launch of its own: no flow there
    b = H.bcast_desc(L, 64, 272, 480, 1)
    assert _select(lib, b) == "conv_mfma_v5(bcast)" and lib.tdvc_conv_flow_supported(C.byref(b)) == 0
