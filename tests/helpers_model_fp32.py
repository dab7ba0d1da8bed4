"""The pinned frame of the whole-model fp32 tests (tests/test_model_fp32_gpu.py compares `VideoCompressor.model_fp32 = True` with
the CPU oracle's default mode on it, tests/test_model_fp32_cases_cpu.py holds it to its margins without a GPU).

The margin of a coder is the smallest distance of any y - mu of the forward pass (mu: the means the entropy parameters give for
round(y)) from a rounding boundary, a half-integer.  The frame pinned here is the one of the seeds 1234 .. 1239 where it is largest
(64x64, synthetic filler, frame 1 of make_gop(seed, 2, 64, 64)): 5.25e-4 in the motion coder, 7.07e-4 in the residual coder (seed 1234:
1.43e-4).  The GPU test allows a quarter of the asserted margin as |d(y - mu)|.

What the symbols themselves rest on are two other distances, measured and asserted next to the margin: round(y) of the forward pass
(2.9e-4 / 4.1e-4 on this frame) and round(y - mu) of compress(), whose mu comes from the context loop's own y_hat (1.46e-4 / 1.11e-4):
both stay above the quarter-margin the GPU test allows."""
import functools

import torch

SEED, H, W = 1237, 64, 64
MARGIN = 4e-4                 # asserted on the oracle alone; the GPU test allows a quarter of it as |d(y - mu)|


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.tdvc_ref import VideoCompressor as Ref
    from tdvc_amd.synth import fill_parameters
    ref = Ref().eval()
    fill_parameters(ref)
    return ref


def frame(seed=SEED, h=H, w=W):
    """-> (x (1,3,h,w), refs (1,4,3,h,w)): frame 1 of the synthetic GOP, coded from its I-frame"""
    from tdvc_amd.synth import make_gop, ref_list
    g = make_gop(seed, 2, h, w)
    return g[1:2], ref_list([g[0:1]])


def y_minus_mu(y, dbg):
    """compress()'s debug record -> (y - mu, symbols) as (1, M, h, w): mu = y_hat - symbol at every position of the context loop"""
    q = torch.as_tensor(dbg["symbols"]).reshape(y.shape[2], y.shape[3], y.shape[1]).permute(2, 0, 1).unsqueeze(0).float()
    return y - (dbg["y_hat"] - q), q


def boundary_distance(d, q):
    """distance of y - mu from the nearest half-integer, given its rounding q"""
    return 0.5 - (d - q).abs()


@functools.lru_cache(maxsize=None)
def oracle_frame(seed=SEED, h=H, w=W):
    """the oracle's default mode (fp32 everywhere but the DCN's fp16 output) on the frame, with compress(): -> (outputs, trace)"""
    x, refs = frame(seed, h, w)
    tr = {}
    with torch.no_grad():
        out = oracle()(x, refs, False, is_compress=True, trace=tr)
    tr["ff_idx"] = oracle().loopfilter.last_match_index.clone()          # the module keeps the last call's only
    return out, tr


def margins(tr):
    """-> {coder: smallest distance of any y - mu of the forward pass from a rounding boundary}"""
    res = {}
    for c in ("mv", "res"):
        f = tr[c + "_dbg"]["y"] - tr[c + "_dbg"]["means"]
        res[c] = float(boundary_distance(f, f.round()).min())
    return res


def symbol_distances(tr):
    """-> {coder: (round(y) of the forward pass, round(y - mu) of compress())}: the smallest distances the coded symbols rest on"""
    res = {}
    for c in ("mv", "res"):
        y = tr[c + "_dbg"]["y"]
        d, q = y_minus_mu(y, tr["strings"][c]["_debug"][0])
        res[c] = (float(boundary_distance(y, y.round()).min()), float(boundary_distance(d, q).min()))
    return res
