"""Lane-split y streams (order="lanes") on the MI355X path: the on-device range decoder (ar_decode_lanes_batch_kernel) against the
host decoder that shares its decode routine, the coder and frame round trips against the "wavefront" order (same symbols,
same y_hat, bit for bit), and the error report of a damaged stream.  Every comparison is an exact integer / bit comparison."""
import io

import numpy as np
import pytest
import torch

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


def host_scale_index(scale, table):
    """GaussianConditional.build_indexes as ar_quantize_batch_kernel states it: ntable - 1 - #{j < ntable - 1: max(s, 0.11) <= table[j]}"""
    s = np.maximum(scale.astype(np.float32), np.float32(0.11))
    return (table.size - 1 - (s[..., None] <= table[None, None, :-1]).sum(-1)).astype(np.int32)


@pytest.fixture(scope="module")
def kernel_case(coders):
    """44 positions in three steps (1, 3, 40) of an 8 x 8 grid: scales over the whole table and beyond both ends, random means,
    symbols inside and outside their tables, at least one bypass symbol per channel (hence per lane)"""
    _, m = coders
    _, gct, table = m._coder_tables()
    tab = table.cpu().numpy()
    rng = np.random.default_rng(11)
    steps = [1, 3, 40]
    npos = sum(steps)
    scale = np.exp(rng.uniform(np.log(0.02), np.log(600.0), (npos, M))).astype(np.float32)
    scale[0, :4] = [0.05, 0.11, 256.0, 1e4]
    mean = (rng.standard_normal((npos, M)) * 3).astype(np.float32)
    idx = host_scale_index(scale, tab)
    assert idx.min() == 0 and idx.max() == tab.size - 1 and (scale < 0.11).any() and (scale > 256).any()
    size, off = gct.sizes[idx], gct.offsets[idx]
    sym = (off + rng.integers(0, size - 1)).astype(np.int32)                 # in the table (its last bin is the bypass bin)
    out = rng.random((npos, M)) < 0.04
    out[rng.integers(0, npos, M), np.arange(M)] = True                      # every channel gets one
    far = np.where(rng.random((npos, M)) < 0.5, off - rng.integers(1, 3000, (npos, M)), off + size - 2 + rng.integers(0, 3000, (npos, M)))
    sym = np.where(out, far, sym).astype(np.int32)
    v = sym - off
    bypass = (v < 0) | (v >= size - 2)
    perm = rng.permutation(64)[:npos]
    pos = np.stack([perm // 8, perm % 8], 1).astype(np.int32)
    return dict(steps=steps, scale=scale, mean=mean, idx=idx, sym=sym, bypass=bypass, pos=pos)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("lanes", [64, 128])
def test_decode_kernel_equals_host_decoder(coders, kernel_case, lanes, f32, report):
    from tdvc_amd import ops
    _, m = coders
    _, gct, table = m._coder_tables()
    k = kernel_case
    sym, idx, steps = k["sym"], k["idx"], k["steps"]
    npos = sym.shape[0]
    per_lane = k["bypass"].reshape(npos, M // lanes, lanes).any((0, 1))
    assert per_lane.all(), "a lane without a bypass symbol"
    data = ops.rans_encode_lanes(sym, idx, gct, lanes)
    assert np.array_equal(ops.rans_decode_lanes(data, idx, gct), sym)
    dev = "cuda"
    adt = torch.float32 if f32 else torch.float16
    stream_dev, _ = ops.ar_lanes_pack_batch([data], lanes, dev)                # one image: B = 1 of the entry points
    state = ops.ar_lanes_state_batch(lanes, 1, dev)
    ops.ar_lanes_init_batch(stream_dev, 1, lanes, state)
    pos = torch.from_numpy(k["pos"]).to(dev)
    gp = ops.FM.empty(1, 1, max(steps), 2 * M, dtype=torch.float32, device=dev)
    rows = torch.from_numpy(np.concatenate([k["scale"], k["mean"]], 1)).to(dev)
    y_hat, y_want = ops.FM.zeros(1, 8, 8, M, dtype=adt, device=dev), ops.FM.zeros(1, 8, 8, M, dtype=adt, device=dev)
    sym_d = torch.full((64, M), -12345, dtype=torch.int32, device=dev)           # compact rows of the image's H * W block
    idx_d = torch.full((64, M), -12345, dtype=torch.int32, device=dev)
    # what tdvc_ar_quantize_batch writes, given those symbols (raster arrays [1][H][W][M])
    sym_r = torch.zeros((1, 8, 8, M), dtype=torch.int32, device=dev)
    sym_r[0, pos[:, 0].long(), pos[:, 1].long()] = torch.from_numpy(sym).to(dev)
    sym_q, idx_q = torch.zeros_like(sym_r), torch.zeros_like(sym_r)
    o = 0
    for n in steps:                                                           # three launches on one state buffer
        gp.t.view(-1, 2 * M)[:n] = rows[o:o + n]
        ops.ar_decode_lanes_step_batch(gp, pos[o:], n, table, stream_dev, lanes, gct, state, y_hat, sym_d, idx_d, o)
        ops.ar_quantize_batch(None, gp, pos[o:], n, table, y_want, sym_q, idx_q, symbols_in=sym_r)
        o += n
    torch.cuda.synchronize()
    st = state[0].cpu().numpy().view(np.uint32)                               # image 0's lane states and error word
    report(f"lane decode kernel L={lanes} f32={f32}: {npos * M} symbols, {int(k['bypass'].sum())} bypass, {len(data)} B; bad word {st[-1]}; "
           f"words consumed {int((st[:-1].reshape(lanes, 4)[:, 2]).max())} of {(len(data) - 4 - 2 * lanes) // 4}")
    assert st[-1] == 0
    assert np.array_equal(sym_d[:npos].cpu().numpy(), sym), "symbols differ from the host decoder's"
    assert np.array_equal(idx_d[:npos].cpu().numpy(), idx), "CDF indexes differ from scale_index on the host"
    assert bool((sym_d[npos:] == -12345).all()) and bool((idx_d[npos:] == -12345).all())
    assert torch.equal(y_hat.t, y_want.t), "y_hat differs from tdvc_ar_quantize_batch's"
    assert bool((y_hat.t != 0).any())
    assert torch.equal(idx_q[0, pos[:, 0].long(), pos[:, 1].long()].cpu(), torch.from_numpy(idx))
    # every lane has read its sub-stream to the end, and no further
    assert np.array_equal(st[:-1].reshape(lanes, 4)[:, 2], st[:-1].reshape(lanes, 4)[:, 3])


@pytest.fixture(scope="module")
def coder_case(coders):
    """per (H, W, f32): the wavefront-order compress() every lane count is compared with, computed once"""
    cache = {}

    def get(H, W, f32):
        from tdvc_amd import ops
        _, m = coders
        if (H, W, f32) not in cache:
            xf = to_fm(rnd16(randn(1, 64, H, W, seed=37, scale=0.5)), ops)
            enc_w = m.compress(xf, f32=f32, order="wavefront")
            dec_w = m.decompress(enc_w["strings"], enc_w["shape"], synth=False, f32=f32, order="wavefront")
            cache[(H, W, f32)] = (xf, enc_w, dec_w["y_hat"].t.clone())
        return cache[(H, W, f32)]
    return get


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("H,W", [(64, 64), (128, 192)])
@pytest.mark.parametrize("f32", [False, True])
def test_lanes_stream_order(coders, coder_case, H, W, f32, lanes, report):
    from tdvc_amd import ops
    _, m = coders
    xf, enc_w, yh_w = coder_case(H, W, f32)
    _, gct, _ = m._coder_tables()
    enc = m.compress(xf, f32=f32, order="lanes", lanes=lanes)
    dl, dw = enc["_debug"][0], enc_w["_debug"][0]
    assert torch.equal(dl["symbols"], dw["symbols"]) and torch.equal(dl["indexes"], dw["indexes"])
    assert enc["strings"][1] == enc_w["strings"][1]                          # z stream: untouched
    ys, yw = enc["strings"][0][0], enc_w["strings"][0][0]
    assert ys[:4] == bytes([ord("L"), 1, lanes, 0])
    h, w = dl["symbols"].shape[:2]
    order = [p for st in m.wavefront_steps(h, w) for p in st]
    hs, ws = np.array([p[0] for p in order]), np.array([p[1] for p in order])
    sym, idx = dl["symbols"].cpu().numpy()[hs, ws], dl["indexes"].cpu().numpy()[hs, ws]
    assert np.array_equal(ops.rans_decode_lanes(ys, idx, gct), sym), "the y string does not decode to the wavefront-ordered symbols"
    report(f"lanes stream {H}x{W} f32={f32} L={lanes}: {len(ys)} B vs wavefront {len(yw)} B (+{len(ys) - len(yw)}, bound +{4 + 14 * lanes})")
    assert len(ys) <= len(yw) + 4 + 14 * lanes
    dec = m.decompress(enc["strings"], enc["shape"], synth=False, f32=f32, order="lanes")
    assert torch.equal(dec["y_hat"].t, dl["y_hat"].t), "decoder y_hat differs from the encoder's"
    assert torch.equal(dec["y_hat"].t, yh_w), "decoder y_hat differs from the wavefront decoder's"
    # deferred range coding gives the same strings
    assert m.compress(xf, f32=f32, order="lanes", lanes=lanes, defer=True)["strings"].result() == enc["strings"]


def test_lane_count_is_checked(coders, coder_case):
    _, m = coders
    xf = coder_case(64, 64, False)[0]
    for bad in (48, 32, 1, 256):
        with pytest.raises(ValueError):
            m.compress(xf, order="lanes", lanes=bad)


def test_batch_of_two_images(coders, report):
    from tdvc_amd import ops
    _, m = coders
    xf = to_fm(rnd16(randn(2, 64, 64, 64, seed=41, scale=0.5)), ops)
    enc = m.compress(xf, order="lanes")
    assert len(enc["strings"][0]) == 2 and enc["strings"][0][0] != enc["strings"][0][1]
    dec = m.decompress(enc["strings"], enc["shape"], synth=False, order="lanes")
    assert torch.equal(dec["y_hat"].t, torch.cat([d["y_hat"].t for d in enc["_debug"]], 0))


def test_frame_roundtrip_lanes_order(report):
    from tdvc_amd import bitstream, synth
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.tools.predict import STREAM_ORDER_FLAGS
    net = VideoCompressor()
    synth.fill_parameters(net)
    net = net.cuda().eval()
    gop = synth.make_gop(78, 3, 128, 64).cuda()
    refs = synth.ref_list([gop[0:1], gop[1:2]])
    enc_r = net.encode(gop[2:3], refs)
    net.stream_order = "wavefront"
    enc_w = net.encode(gop[2:3], refs)
    nb = lambda e: sum(len(s[0]) for s in e["strings"])
    net.stream_order = "lanes"
    for lanes in (64, 128):
        net.stream_lanes = lanes
        enc = net.encode(gop[2:3], refs)
        assert torch.equal(enc["recon"], enc_r["recon"])
        assert enc["strings"][0][0][2] == lanes and enc["strings"][2][0][2] == lanes
        flat = [s[0] for s in enc["strings"]]
        assert STREAM_ORDER_FLAGS["lanes"] == 2
        shp = [(2 if i % 2 == 0 else 0, 128, *enc["shapes"][i // 2]) for i in range(4)]
        buf = io.BytesIO()
        bitstream.write_records(buf, flat, shp)
        buf.seek(0)
        strings, shapes = bitstream.read_records(buf, 4)
        assert strings == flat and [tuple(s) for s in shapes] == shp and shapes[0][0] == 2 and shapes[2][0] == 2
        dec = net.decode([[s] for s in strings], [shapes[0][2:], shapes[2][2:]], refs)
        assert torch.equal(dec, enc["recon"]), "decoder / encoder reconstruction mismatch"
        report(f"frame round trip, lanes order L={lanes} 128x64: {nb(enc)} B vs wavefront {nb(enc_w)} B, raster {nb(enc_r)} B")
        assert 0 <= nb(enc) - nb(enc_w) <= 2 * (4 + 14 * lanes)


def test_damaged_stream_raises_and_the_process_goes_on(coders, coder_case):
    """the last lane cut by one word (length table adjusted, so the host's header check passes): the lane runs out of words on the
    device, reads 0 instead, and the sticky error word comes back as a RuntimeError; a valid decode right after it is exact"""
    _, m = coders
    xf = coder_case(64, 64, False)[0]
    lanes = 64
    enc = m.compress(xf, order="lanes", lanes=lanes)
    ys = enc["strings"][0][0]
    cut = bytearray(ys[:-4])
    e = 4 + 2 * (lanes - 1)
    cut[e:e + 2] = (int.from_bytes(ys[e:e + 2], "little") - 1).to_bytes(2, "little")
    with pytest.raises(RuntimeError, match="lane-split stream"):
        m.decompress([[bytes(cut)], enc["strings"][1]], enc["shape"], synth=False, order="lanes")
    dec = m.decompress(enc["strings"], enc["shape"], synth=False, order="lanes")
    assert torch.equal(dec["y_hat"].t, enc["_debug"][0]["y_hat"].t)
