"""SPyNet.run(f32=True) on a frame whose sides are no multiples of 32 (VideoCompressor only passes multiples of 64, so the model
tests never take this branch): the frame is resized up, and the flow resized back with a scale per flow channel.  In the fp32 mode
the flow map carries eight channels, two real ones and six of zeros, while there are two scales: the resize runs on the two real
channels, and ops.resize_bilinear refuses a scale vector shorter than its map's channel count before anything is launched.

Reference: the CPU oracle's SPyNet.forward in fp32.  Gate: relative L2 below 1e-4, the cap the whole-model test holds every stage in
front of the quantisers to (tests/test_model_fp32_gpu.py); the flow is one of them."""
import pytest
import torch

from tests import helpers_model_fp32 as M
from util import fm_to_cpu

pytestmark = pytest.mark.gpu

H, W = 40, 72                 # resized to 64 x 96 and back


def test_spynet_f32_on_a_frame_that_is_resized(report):
    from tdvc_amd import ops
    from tdvc_amd.model import VideoCompressor
    m = VideoCompressor()
    m.load_state_dict(M.oracle().state_dict(), strict=True)
    m = m.cuda().eval()
    gen = torch.Generator().manual_seed(72)
    cur = torch.rand(1, 3, H, W, generator=gen)
    ref = (cur.roll((1, 2), (2, 3)) + 0.05 * torch.rand(1, 3, H, W, generator=gen)).clamp(0, 1)
    with torch.no_grad():
        want = M.oracle().motion_est.spynet(cur, ref)
        flow = m.motion_est.spynet.run(ops.from_nchw(cur.cuda(), Cpad=4, dtype=torch.float32), ops.from_nchw(ref.cuda(), Cpad=4, dtype=torch.float32), f32=True)
    torch.cuda.synchronize()
    assert (flow.N, flow.H, flow.W, flow.C) == (1, H, W, 2) and flow.f32
    got = fm_to_cpu(flow)
    assert bool(torch.isfinite(got).all())
    err = float((got - want).norm() / want.norm())
    report(f"spynet f32, {H}x{W} resized: relative L2 against the oracle {err:.3e}, |flow| rms {float(want.pow(2).mean().sqrt()):.3f} px")
    assert float(want.norm()) > 0 and err < 1e-4, err


def test_resize_bilinear_refuses_a_short_scale_vector():
    from tdvc_amd import ops
    x = ops.FM(torch.zeros(1, 4, 4, 8, device="cuda"))
    with pytest.raises(ValueError):
        ops.resize_bilinear(x, 8, 8, torch.ones(2, device="cuda"))
    y = ops.resize_bilinear(x.ch(0, 2), 8, 8, torch.ones(2, device="cuda"))
    torch.cuda.synchronize()
    assert (y.H, y.W, y.C) == (8, 8, 2) and bool((y.t == 0).all())
