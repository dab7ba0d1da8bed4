"""The range encoder of lane-split y streams on the MI355X path (ar_encode_lanes_batch_kernel): its bytes against the host
encoder's (tdvc_rans_encode_lanes) and its host twin's, the bounded-write path with a scratch region that is too small,
compress(coder="device") against coder="host", and the VideoCompressor round trip.  Every comparison is an exact byte / bit
comparison."""
import numpy as np
import pytest
import torch

from test_rans_lanes_enc_cpu import CANARY, extremes_image, gathered, in_table_image, random_tables, symbols_for, wavefront
from util import randn, rnd16, to_fm

pytestmark = pytest.mark.gpu

M = 128


@pytest.fixture(scope="module")
def coders():
    from oracle.tdvc_ref.coder import MVCoder as RefCoder
    from tdvc_amd.model.coder import MVCoder
    from tdvc_amd.synth import fill_parameters
    ref = RefCoder(N=128).eval()
    h = torch.nn.Module(); h.add_module("mvCoder", ref); fill_parameters(h)
    m = MVCoder(N=128)
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.cuda().eval()
    m.update(force=True)
    return ref, m


@pytest.fixture(scope="module")
def tables():
    from tdvc_amd import ops
    t = random_tables()
    return ops.CdfTables(torch.from_numpy(t.cdf), torch.from_numpy(t.sizes), torch.from_numpy(t.offsets))


def kernel_strings(ops, sym, idx, pos, t, lanes, **kw):
    enc = ops.ar_encode_lanes_batch(torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(pos).cuda(), t, lanes, **kw)
    torch.cuda.synchronize()
    return enc, enc.out.cpu().numpy(), enc.info.cpu().numpy().view(np.uint32)


def check_against_host_and_twin(ops, sym, idx, pos, t, lanes):
    _, out, info = kernel_strings(ops, sym, idx, pos, t, lanes)
    got = ops.lanes_strings(out, info, "kernel")
    twin = ops.rans_encode_lanes_dev_ref(sym, idx, pos, t, lanes)
    for b in range(sym.shape[0]):
        assert got[b] == ops.rans_encode_lanes(gathered(sym[b], pos), gathered(idx[b], pos), t, lanes), f"image {b}: kernel bytes differ from tdvc_rans_encode_lanes"
        assert got[b] == twin[b], f"image {b}: kernel bytes differ from the host twin's"
    return got


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (5, 7)])
def test_kernel_bytes_random_tables(tables, grid, B, lanes):
    from tdvc_amd import ops
    H, W = grid
    idx, sym = symbols_for(tables, (B, H, W, M), 2000 * H + 10 * B + lanes)
    v = sym - tables.offsets[idx]
    if H > 1:
        assert (v < 0).any() and (v >= tables.sizes[idx] - 2).any()              # bypass symbols of both signs
    got = check_against_host_and_twin(ops, sym, idx, wavefront(H, W), tables, lanes)
    assert B == 1 or got[0] != got[1]


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (5, 7)])
def test_kernel_bytes_all_in_table_and_extremes(tables, grid, lanes):
    from tdvc_amd import ops
    H, W = grid
    i0, s0 = in_table_image(tables, H, W, 21)
    i1, s1 = extremes_image(tables, H, W, 22)
    i2, s2 = in_table_image(tables, H, W, 23)
    check_against_host_and_twin(ops, np.stack([s0, s1, s2]), np.stack([i0, i1, i2]), wavefront(H, W), tables, lanes)
    check_against_host_and_twin(ops, s1[None], i1[None], wavefront(H, W), tables, lanes)


@pytest.fixture(scope="module")
def real_case(coders):
    """a real coder's tables after update(force=True) and the symbols of its own context loop: 64 x 64 inputs (4 x 4 grids, B = 1
    and 3) and a 256 x 256 input (16 x 16 grid, B = 2); computed once"""
    from tdvc_amd import ops
    _, m = coders
    _, gct, _ = m._coder_tables()
    out = {}
    for name, (B, H, W) in {"64": (3, 64, 64), "256": (2, 256, 256)}.items():
        enc = m.compress(to_fm(rnd16(randn(B, 64, H, W, seed=51, scale=0.5)), ops), order="lanes")
        sym = np.stack([d["symbols"].cpu().numpy() for d in enc["_debug"]])
        idx = np.stack([d["indexes"].cpu().numpy() for d in enc["_debug"]])
        out[name] = (sym, idx, enc["strings"][0])
    return gct, out


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("case,B", [("64", 1), ("64", 3), ("256", 2)])
def test_kernel_bytes_real_tables_and_symbols(real_case, case, B, lanes):
    from tdvc_amd import ops
    gct, cases = real_case
    sym, idx, strings = cases[case]
    sym, idx = np.ascontiguousarray(sym[:B]), np.ascontiguousarray(idx[:B])
    got = check_against_host_and_twin(ops, sym, idx, wavefront(*sym.shape[1:3]), gct, lanes)
    if lanes == 64:
        assert got == list(strings[:B])                                          # what compress(order="lanes") wrote


def test_small_scratch_is_status_2_and_the_next_call_is_right(tables):
    """4 words per lane: every image ends with status 2 through the bounded-write path of the shared routine; the words after the
    scratch and after the output buffer are intact, nothing of a container is written, every region holds exactly the 4 words
    its own lane emits first, and a correct call right after gives the right bytes"""
    from tdvc_amd import ops
    lanes, B, H, W, words = 64, 3, 4, 4, 4
    pos = wavefront(H, W)
    idx, sym = symbols_for(tables, (B, H, W, M), 88)
    stride = (4 + 2 * lanes + 4 * lanes * words + 15) // 16 * 16
    sbuf = torch.full((B * lanes * words + 64,), CANARY - (1 << 32), dtype=torch.int32, device="cuda")
    obuf = torch.full((B * stride + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    enc, out, info = kernel_strings(ops, sym, idx, pos, tables, lanes, lane_words=words, scratch=sbuf[:B * lanes * words].view(B, lanes, words),
                                    out=obuf[:B * stride].view(B, stride))
    assert info.tolist() == [[0, 2]] * B
    s = sbuf.cpu().numpy().view(np.uint32)
    assert (s[B * lanes * words:] == CANARY).all() and bool((obuf == 0xEE).all())
    _, _, scr2 = ops.rans_encode_lanes_dev_ref(sym, idx, pos, tables, lanes, raw=True)
    assert np.array_equal(s[:B * lanes * words].reshape(B, lanes, words), scr2[:, :, -words:])
    with pytest.raises(RuntimeError, match="scratch"):
        ops.lanes_strings(out, info, "kernel")
    check_against_host_and_twin(ops, sym, idx, pos, tables, lanes)


@pytest.fixture(scope="module")
def host_case(coders):
    """per (H, W, f32, lanes, B): compress(order="lanes", coder="host"), computed once"""
    cache = {}

    def get(H, W, f32, lanes, B):
        from tdvc_amd import ops
        _, m = coders
        key = (H, W, f32, lanes, B)
        if key not in cache:
            xf = to_fm(rnd16(randn(B, 64, H, W, seed=37, scale=0.5)), ops)
            cache[key] = (xf, m.compress(xf, f32=f32, order="lanes", lanes=lanes, coder="host")["strings"])
        return cache[key]
    return get


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("H,W,B", [(64, 64, 1), (128, 192, 1), (64, 64, 2)])
@pytest.mark.parametrize("f32", [False, True])
def test_compress_device_equals_host(coders, host_case, H, W, B, f32, lanes, defer):
    _, m = coders
    xf, want = host_case(H, W, f32, lanes, B)
    enc = m.compress(xf, f32=f32, order="lanes", lanes=lanes, coder="device", defer=defer)
    strings = enc["strings"].result() if defer else enc["strings"]
    assert strings == want, "device-coded strings differ from the host coder's"
    assert len(strings[0]) == B and (B == 1 or strings[0][0] != strings[0][1])
    dec = m.decompress(strings, enc["shape"], synth=False, f32=f32, order="lanes")
    assert torch.equal(dec["y_hat"].t, torch.cat([d["y_hat"].t for d in enc["_debug"]], 0)), "decoder y_hat differs from the encoder's"


def test_device_coder_needs_the_lanes_order(coders, host_case):
    _, m = coders
    xf = host_case(64, 64, False, 64, 1)[0]
    for order in ("raster", "wavefront"):
        with pytest.raises(ValueError):
            m.compress(xf, order=order, coder="device")
    with pytest.raises(ValueError):
        m.compress(xf, order="lanes", coder="gpu")


def test_video_compressor_round_trip_device_coder():
    from tdvc_amd import synth
    from tdvc_amd.model import VideoCompressor
    net = VideoCompressor()
    synth.fill_parameters(net)
    net = net.cuda().eval()
    assert net.stream_coder == "host"
    gop = synth.make_gop(78, 3, 64, 64).cuda()
    refs = synth.ref_list([gop[0:1], gop[1:2]])
    net.stream_order = "lanes"
    enc_h = net.encode(gop[2:3], refs)
    net.stream_coder = "device"
    enc = net.encode(gop[2:3], refs)
    again = net.encode(gop[2:3], refs)                                           # right after: the deferred buffers are not reused early
    assert enc["strings"] == enc_h["strings"], "device-coded strings differ from the host coder's"
    assert again["strings"] == enc["strings"]
    assert torch.equal(enc["recon"], enc_h["recon"])
    dec = net.decode(enc["strings"], enc["shapes"], refs)
    assert torch.equal(dec, enc["recon"]), "decoder / encoder reconstruction mismatch"
    net.stream_order = "wavefront"
    with pytest.raises(ValueError):
        net.encode(gop[2:3], refs)
