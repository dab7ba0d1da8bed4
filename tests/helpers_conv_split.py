"""CPU restatement of conv_split's arithmetic (tdvc_amd/csrc/conv_split.hip): the exact three-way bf16 split of an fp32 value, the six-term
product sum the kernel accumulates, the three five-term sums a kernel that lost a second-order product would compute, and the packing of
tdvc_pack_conv_weights_indexed_bf16x3.  float64 throughout: every part is a bf16 value, every product of two parts exact in float64."""
import numpy as np
import torch

U = 2.0 ** -8                         # unit roundoff of bf16 (8 significand bits, round to nearest even)
DROPPED = 2 * U ** 3 + U ** 4         # |xm wl + xl wm + xl wl| <= DROPPED |x| |w|: the three terms the kernel does not compute
SIX = (("h", "h"), ("h", "m"), ("m", "h"), ("m", "m"), ("h", "l"), ("l", "h"))       # (x part, w part) of the six products
SECOND_ORDER = (("m", "m"), ("h", "l"), ("l", "h"))                                  # the 2^-16 products: a five-term sum drops one


def split3(v: torch.Tensor) -> dict:
    """fp32 tensor -> {"h", "m", "l"} as fp32 tensors holding bf16 values: h = bf16(v), m = bf16(v - h), l = bf16((v - h) - m), each
    conversion torch's round-to-nearest-even, both subtractions in fp32 (exact)"""
    assert v.dtype == torch.float32
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    h = bf(v)
    r1 = v - h
    m = bf(r1)
    return {"h": h, "m": m, "l": bf(r1 - m)}


def conv_terms(x: torch.Tensor, w: torch.Tensor, terms, **conv_kw) -> torch.Tensor:
    """float64 conv2d summed over the given (x part, w part) products of the split operands"""
    xs, ws = split3(x), split3(w)
    out = None
    for xp, wp in terms:
        t = torch.nn.functional.conv2d(xs[xp].double(), ws[wp].double(), **conv_kw)
        out = t if out is None else out + t
    return out


def five_term_sets():
    return [tuple(t for t in SIX if t != drop) for drop in SECOND_ORDER]


def rms(t: torch.Tensor) -> float:
    return float(t.double().pow(2).mean().sqrt())


def ref_pack_split(packed_f32: np.ndarray) -> np.ndarray:
    """the fp32 packing [tiles][nchunks][steps][64 lanes][8] (tests/test_lib_abi.ref_pack order) -> the split packing
    [tiles][k-step = chunk * steps + step][plane h, m, l][64 lanes][8] as fp32 arrays of bf16 values"""
    tiles, nchunks, steps = packed_f32.shape[:3]
    parts = split3(torch.from_numpy(np.ascontiguousarray(packed_f32, dtype=np.float32)))
    planes = [parts[k].numpy().reshape(tiles, nchunks * steps, 64, 8) for k in ("h", "m", "l")]
    return np.stack(planes, axis=2)


def ref_pack_f32(w: np.ndarray, cin_pad: int, taps, ck: int) -> np.ndarray:
    """the fragment order of the conv packings as floats, restated: [tile of 32 couts][chunk of ck channels][k-step][lane (r, h)][8]; lane
    (r, h) of step s holds cout 32 t + r and the 8 consecutive input channels c8 of tap `tap`, (tap, c8) = divmod(2 s + h, ck / 8)"""
    cout, cin = w.shape[:2]
    ck8 = ck // 8
    nchunks, steps = (cin_pad + ck - 1) // ck, (len(taps) * ck8 + 1) // 2
    tiles = 1 if cout <= 32 else 2 * ((cout + 63) // 64)
    out = np.zeros((tiles, nchunks, steps, 64, 8), dtype=np.float32)
    for t in range(tiles):
        for ch in range(nchunks):
            for s in range(steps):
                for lane in range(64):
                    r, h = lane & 31, lane >> 5
                    co, kc = t * 32 + r, 2 * s + h
                    if kc >= len(taps) * ck8 or co >= cout:
                        continue
                    tap, c8 = divmod(kc, ck8)
                    c0 = ch * ck + c8 * 8
                    n = max(0, min(8, cin - c0))
                    out[t, ch, s, lane, :n] = w[co, c0:c0 + n, taps[tap][0], taps[tap][1]]
    return out
