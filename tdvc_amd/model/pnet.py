"""`VideoCompressor` — drop-in for `main/model/pnet.py:15-83` on MI355X.

Same constructor (no arguments), same `forward(input_image, refer_frames, enabled_amp,
is_compress=False)` signature and return tuple, same state-dict keys (`mvCoder, resCoder,
extra_fea, motion_est, mcnet, loopfilter, mcfilter`).  The whole forward runs in hand-written
gfx950 kernels (libtdvc_hip.so): fp16 NHWC activations with fp32 accumulation for every conv
(the reference under AMP computes its convs in fp16 too, and keeps the two coders in fp32 —
here they are fp16-in / fp32-accumulate as well), fp32 for flow, SE gates,
matching and rate terms.  There is no PyTorch/CPU fallback: tensors must live on a HIP device.
"""
from __future__ import annotations

import contextlib
import functools

import torch
import torch.nn as nn

from .. import ops
from ..ops import FM
from . import modules
from .coder import STREAM_CODERS, MVCoder, ResCoder
from .modules import FeaExtra, FeatureFix, LoopFilter, MCNet, OffsetGen


MV_SLOT, RES_SLOT = 0, 1      # the two coders' slots on the side stream (ops.rate_branch / ops.rate_join)


def _ref_views(refs8: FM, B: int):
    """(r-1, I) of every batch item as views of the converted reference stack (B*4, H, W, 8): items 4b + 3 and 4b"""
    return (FM(refs8.t, refs8.off + 3 * refs8.sn, B, refs8.C, 4 * refs8.sn), FM(refs8.t, refs8.off, B, refs8.C, 4 * refs8.sn))


def _under_f32_split(fn):
    """forward / encode / decode run their convs of fp32 maps as `VideoCompressor.f32_split` says (or an enclosing ops.f32_split block).
    The model's flag is an inference / coding switch: a .train() forward ignores it, with or without a recording tape"""
    @functools.wraps(fn)
    def run(self, *a, **kw):
        # `train_f32_split` is the training switch: a .train() forward that a tape records, and (through the tape) its backward sweep
        train_split = self.train_f32_split and self.training and ops.TAPE is not None
        if train_split:
            ops.TAPE.f32_split_train = True
        with ops.f32_split((self.f32_split and not self.training) or ops.F32_SPLIT), ops.f32_split_train(train_split or ops.F32_SPLIT_TRAIN):
            return fn(self, *a, **kw)
    return run


class VideoCompressor(nn.Module):
    fp32_islands_supported = True

    def __init__(self):
        super().__init__()
        # the reference keeps both coders outside autocast (pnet.py:33,57).  Default here: fp16-in / fp32-accumulate coders
        # (the 30 fps path); `enabled_amp=False` in forward(), or this flag for encode() / decode(), runs them as true fp32
        # islands (fp32 activations + weights on v_mfma_f32_32x32x2_f32): symbols and byte streams then equal the fp32 CPU
        # reference's on identical coder inputs (tests/test_entropy_coding_gpu.py).  NOTE for reference checkpoints: the reference's
        # `enable_amp: True` (cfg/predict.yaml) keeps fp32 coders; here that value selects the fp16-in coders, so the reference-faithful
        # setting is coder_fp32 = True (tools/predict: yaml key `coder_fp32: true` or --coder-fp32), independent of `enabled_amp`
        self.coder_fp32 = False
        # the convs of fp32 maps (wherever `enabled_amp=False`, `coder_fp32` or `model_fp32` make some) on conv_split instead of conv_f32:
        # every fp32 operand split exactly into three bf16 parts, six exact products per MAC on the bf16 matrix pipe (csrc/conv_split.hip,
        # DESIGN.md section 4c).  fp32-grade results, not bit-equal to conv_f32's: the strings are NOT promised byte-equal to the default
        # fp32 islands' or the oracle's beyond rounding ties, and, like `coder_fp32`, the ENCODER AND THE DECODER MUST AGREE on the flag.
        # Inference / coding only (under the tape nothing changes); the context loop's native chains stay on conv_f32.  No effect
        # without fp32 maps.  tools/predict: yaml key `f32_split: true` or --f32-split
        self.f32_split = False
        # training with fp32 coders (what the reference's tools/train.py optimises): a .train() forward keeps both coders in fp32 and the
        # tape differentiates them in fp32 (conv_f32 dgrad, conv_wgrad_f32).  Set by TrainStep(coder_fp32=True).  Unset, a .train()
        # forward runs the fp16-in / fp32-accumulate coders whatever `enabled_amp` / `coder_fp32` say (with a warning)
        self.train_coder_fp32 = False
        # the reference's `enable_amp: False`: an eval forward(), encode() and decode() run EVERY stage on fp32 maps with fp32 weights
        # (conv_f32, the fp32 deformable conv of csrc/dcn_f32.hip, the streaming kernels on fp32 maps), both coders as the fp32 islands;
        # only the deformable conv's output is rounded to fp16 and widened again, as in the reference (dcn_v2_amp.py:15,67-68).  No fused
        # inference form and no reuse cache takes fp32 maps: this mode runs the plain sequence of traced calls.  It is the mode that is
        # compared with the fp32 CPU oracle to fp32 accumulation error; it is bound by the fp32 matrix pipe and is no 30 fps path.
        # Inference only: with the flag set, .train() or a recording tape raises ValueError.  `enabled_amp` keeps its meaning while unset
        self.model_fp32 = False
        # the reference's `amp: False` in TRAINING (tools/train.py:152-159): with this flag a .train() forward, or any forward under
        # autograd.record(), runs every stage on fp32 maps exactly as the eval `model_fp32` forward does -- both coders fp32, the plain
        # sequence of traced calls, no fused inference form -- plus the training-mode differences (noise quantisation, scale-8 matching,
        # the 5-tuple return), and the tape differentiates all of it in fp32 (fp32 mirrors, conv_f32 dgrad, conv_wgrad_f32, the fp32
        # deformable-conv backward).  Set by TrainStep(model_fp32=True).  `model_fp32` alone keeps refusing .train() and the tape
        self.train_model_fp32 = False
        # the training form of `f32_split`: with this flag a .train() forward under a recording tape, and that tape's backward sweep, run
        # every conv of an fp32 map (forward, data gradient) on conv_split and every fp32 conv weight gradient on conv_wgrad_split_kernel
        # (six bf16 MFMA products per MAC) instead of conv_f32 / conv_wgrad_f32.  It needs fp32 maps to act on:
        # set by TrainStep(coder_fp32=True or model_fp32=True, f32_split=True).  `f32_split` alone keeps leaving training on conv_f32
        self.train_f32_split = False
        # symbol order of the y streams encode() writes and decode() expects: "raster" (compressai's, what the reference's
        # decoder reads), "wavefront" (an extension: the decoder takes an anti-diagonal per step instead of a position) or "lanes"
        # (a second extension: the wavefront sequence split over `stream_lanes` = 64 or 128 rANS sub-streams, which the decoder's
        # GPU kernel reads, one thread per lane, with no host round trip inside the loop; decode() reads the count from the stream)
        self.stream_order = "raster"
        self.stream_lanes = 64
        # where encode()'s range coder of the y streams runs: "host" (worker threads, the symbols copied off the device) or "device"
        # (stream_order "lanes" only: the encoder kernel on a side stream; only the finished strings leave the device).  The strings
        # are the same byte for byte
        self.stream_coder = "host"
        self.mvCoder = MVCoder(N=128)
        self.resCoder = ResCoder(N=128)
        self.extra_fea = FeaExtra(2)
        self.motion_est = OffsetGen()
        self.mcnet = MCNet(3)
        self.loopfilter = FeatureFix()      # reference-based in-loop filter (sic, pnet.py:23)
        self.mcfilter = LoopFilter()        # multi-frame feature fusion (sic, pnet.py:24)

    # packed-weight cache -------------------------------------------------------------------
    def clear_packed(self):
        for m in self.modules():
            m.__dict__.pop("_packed", None)
            m.__dict__.pop("_tables", None)         # host copies of the coder CDF tables (Cheng2020Anchor._coder_tables)
            m.__dict__.pop("_ar_cache", None)       # wavefront-loop descriptors point at the packed weights

    def load_state_dict(self, *a, **kw):
        r = super().load_state_dict(*a, **kw)
        self.clear_packed()
        return r

    def _apply(self, fn, *a, **kw):
        self.clear_packed()
        return super()._apply(fn, *a, **kw)

    # ----------------------------------------------------------------------------------------
    @_under_f32_split
    def forward(self, input_image, refer_frames, enabled_amp=True, is_compress=False, trace=None, noise=None):
        noise = noise or {}            # test hook: {"mv": {...}, "res": {...}} of fp32 FMs replaces the coders' training-mode draws
        mf32 = self._model_fp32_checked()
        if not (input_image.is_cuda and refer_frames.is_cuda):
            raise RuntimeError("tdvc_amd.VideoCompressor runs on a HIP device only (no CPU fallback)")
        adt = torch.float32 if mf32 else torch.float16           # activation dtype outside the coders
        f32 = (not enabled_amp) or self.coder_fp32 or mf32
        tm32 = mf32 and (self.training or ops.TAPE is not None)          # whole-model fp32 TRAINING (train_model_fp32): fp32 coders implied
        if self.training and (self.train_coder_fp32 or tm32):
            f32 = True
        elif f32 and self.training:
            if not self.__dict__.get("_warned_fp32_train"):
                import warnings
                warnings.warn("tdvc_amd: the fp32-island coders are an inference / coding mode; training runs the default "
                              "fp16-in / fp32-accumulate coders (enabled_amp=False ignored in .train())")
                self.__dict__["_warned_fp32_train"] = True
            f32 = False
        training = self.training       # noise quantisation, scale-8 matching, 5-tuple return (pnet.py:80-83); gradients
        # come from the tape of tdvc_amd/autograd.py (`with autograd.record(): model(...)`), not from torch.autograd
        B, _, H, W = input_image.shape
        if H % 64 or W % 64:
            raise RuntimeError(f"input must be padded to a multiple of 64 (got {H}x{W}); see tools/predict.py:51-53")
        dev = input_image.device
        # the coders' rate branches beside their synthesis transforms (modules.RATE_FORK): a plain inference forward only, under the
        # condition of the other inference forms (whole-model fp32 runs the plain sequence of traced calls)
        fork = modules.RATE_FORK and not is_compress and modules.glue_fusions_allowed(self, trace is not None or mf32)
        with torch.cuda.device(dev), torch.no_grad(), ops.train_model_fp32(tm32), self._rate_branches_joined():
            x = input_image.float()
            refs = refer_frames.float().reshape(B * 4, 3, H, W)
            cur32 = ops.from_nchw(x, Cpad=4, dtype=torch.float32)
            cur8 = ops.from_nchw(x, Cpad=8, dtype=adt)
            refs8 = ops.from_nchw(refs, Cpad=8, dtype=adt)               # (B*4,H,W,8): [I, r-3, r-2, r-1]
            last = refer_frames[:, 3].float()
            ref32 = ops.from_nchw(last, Cpad=4, dtype=torch.float32)
            ref8, iframe8 = _ref_views(refs8, B)                          # frames r-1 and I: strided batch views, not second conversions
            if ops.TAPE is not None:                                     # network inputs carry no gradient
                for t in (cur32, cur8, refs8, ref32, ref8, iframe8):
                    ops.TAPE.mark_input(t)

            feats = FM.empty(B, H, W, 192, dtype=adt, device=dev)        # [f_cur | f_ref | dcn_out]
            npx_ = float(B * H * W)
            f_cur = self.extra_fea.run(cur8, feats.ch(0, 64))
            self.extra_fea.run(ref8, feats.ch(64, 64))
            estmv = self.motion_est.run(feats, cur32, ref32, traced=trace is not None or mf32)

            tr_mv = {} if trace is not None else None
            mv_hat, mv_bits = self.mvCoder.run(estmv, training=training, trace=tr_mv, noise=noise.get("mv"), f32=f32, fork=MV_SLOT if fork else None)
            coded = {}
            if is_compress:                                      # pnet.py:45-49
                self.mvCoder.update(force=True)
                coded["mv"] = self.mvCoder.compress(estmv, f32=f32)

            xt = FM.empty(B, H, W, 256, dtype=adt, device=dev)           # 4 frames x 64 ch
            pred1 = self.mcnet.run(mv_hat, feats, xt.ch(192, 64))
            pred = FM.empty(B, H, W, 64, dtype=adt, device=dev)
            resid = FM.empty(B, H, W, 64, dtype=adt, device=dev)
            if modules.RESID_FUSED and modules.glue_fusions_allowed(self, trace is not None or mf32):
                self.mcfilter.run(xt, refs8, pred, then=(f_cur, -1.0, resid))       # resid = f_cur - pred from the pass that writes pred
            else:
                self.mcfilter.run(xt, refs8, pred)
                ops.scale_act_res(f_cur, resid, res=pred, res_sign=-1.0)

            tr_res = {} if trace is not None else None
            recon_f, res_bits = self.resCoder.run(resid, training=training, res=pred, trace=tr_res, noise=noise.get("res"), f32=f32,
                                                  fork=RES_SLOT if fork else None)
            if is_compress:                                      # pnet.py:69-73
                self.resCoder.update(force=True)
                coded["res"] = self.resCoder.compress(resid, f32=f32)
                # the reference computes these and drops them (pnet.py:49,73); kept for inspection
                self.last_strings = {k: v["strings"] for k, v in coded.items()}
                self.last_ac_bpp = {k: sum(len(s[0]) for s in v["strings"]) * 8.0 / npx_ for k, v in coded.items()}

            recon = self.loopfilter.run(recon_f, iframe8, training=training, trace=trace)

            npx = float(B * H * W)
            self._join_rate_branches()                # the bits are read from here on
            bpp_mv = (mv_bits.sum() / npx).float().view(-1)
            bpp_res = (res_bits.sum() / npx).float().view(-1)
            if trace is not None:
                trace.update(f_cur=f_cur, f_ref=feats.ch(64, 64), estmv=estmv, mv_x_hat=mv_hat, pred1=pred1, pred=pred,
                             resid=resid, recon_f=recon_f, mv=tr_mv, res=tr_res)
        if training:
            return recon, bpp_res, bpp_mv, self.mvCoder.aux_loss(), self.resCoder.aux_loss()
        return recon, bpp_res, bpp_mv

    def _join_rate_branches(self):
        """the launch stream waits for the rate branches the coders forked (coder.py `_fork_rate_branch`), and the buffers they touch are
        released to its allocator; nothing forked, or joined already: nothing happens"""
        for slot, coder in ((MV_SLOT, self.mvCoder), (RES_SLOT, self.resCoder)):
            if coder.rate_hold:
                try:
                    ops.rate_join(slot)
                finally:
                    coder.rate_hold.clear()

    @contextlib.contextmanager
    def _rate_branches_joined(self):
        """whatever ends the block -- forward's return or an exception between a fork and the join -- leaves no branch pending"""
        try:
            yield
        finally:
            self._join_rate_branches()

    # ---- real encode / decode (the reference only sketches it: tools/utils/encoder.py, decoder.py) ----
    def _model_fp32_checked(self) -> bool:
        """whether this call runs every stage on fp32 maps.  Inference: `model_fp32`.  .train() and the tape: `train_model_fp32`;
        `model_fp32` alone is refused there before the first launch (it is the inference / coding switch)"""
        if self.training or ops.TAPE is not None:
            if self.train_model_fp32:
                return True
            if self.model_fp32:
                raise ValueError("tdvc_amd: model_fp32 is an inference / coding mode: unset it for .train() and under autograd.record(), "
                                 "or set train_model_fp32 (TrainStep(model_fp32=True)) to train the whole model in fp32")
            return False
        return bool(self.model_fp32)

    def _adt(self):
        return torch.float32 if self.model_fp32 else torch.float16

    # ---- a call codes a batch of frames, a single frame as a batch of one: the networks run image by image, each coder's context loop
    # once for all images.  The forward conv dispatch counts pixels over the batch, so a layer can land on another kernel (other last
    # bits) in a batch than alone; run this way, frame b's strings and reconstruction are those of a call with frame b alone, whatever
    # the batch size (tools/predict --gop-batch writes the files of --gop-batch 1), and the loops -- launch-latency bound, the part a
    # batch speeds up -- are shared
    def _front(self, refer_frames, b, input_image=None):
        """image b in front of the motion coder, on N = 1 maps: the reference features and, with the frame given (the encoder), the
        frame's features and the motion features `estmv`"""
        _, _, _, H, W = refer_frames.shape
        if H % 64 or W % 64:
            raise RuntimeError(f"frames must be padded to a multiple of 64 (got {H}x{W})")
        dev, adt = refer_frames.device, self._adt()
        refs8 = ops.from_nchw(refer_frames[b:b + 1].float().reshape(4, 3, H, W), Cpad=8, dtype=adt)
        ref8, iframe8 = _ref_views(refs8, 1)
        feats = FM.empty(1, H, W, 192, dtype=adt, device=dev)
        self.extra_fea.run(ref8, feats.ch(64, 64))
        im = dict(H=H, W=W, dev=dev, refs8=refs8, iframe8=iframe8, feats=feats)
        if input_image is not None:
            x, last = input_image[b:b + 1].float(), refer_frames[b:b + 1, 3].float()
            im["f_cur"] = self.extra_fea.run(ops.from_nchw(x, Cpad=8, dtype=adt), feats.ch(0, 64))
            im["estmv"] = self.motion_est.run(feats, ops.from_nchw(x, Cpad=4, dtype=torch.float32), ops.from_nchw(last, Cpad=4, dtype=torch.float32))
        return im

    def _predict(self, im, mv_y_hat: FM) -> FM:
        """decoder-side prediction from the decoded motion latents"""
        adt = im["feats"].t.dtype
        mv_hat = self.mvCoder.run_g_s(mv_y_hat, out_dtype=adt)
        xt = FM.empty(1, im["H"], im["W"], 256, dtype=adt, device=im["dev"])
        self.mcnet.run(mv_hat, im["feats"], xt.ch(192, 64))
        pred = FM.empty(1, im["H"], im["W"], 64, dtype=adt, device=im["dev"])
        self.mcfilter.run(xt, im["refs8"], pred)
        return pred

    def _finish(self, im, res_y_hat: FM, pred: FM):
        return self.loopfilter.run(self.resCoder.run_g_s(res_y_hat, res=pred, out_dtype=pred.t.dtype), im["iframe8"], training=False)

    @staticmethod
    def _dense(fms) -> FM:
        """images given as FMs of N = 1 -> one dense batch FM (a single image that is dense already: itself, not a copy)"""
        f = fms[0]
        if len(fms) == 1 and f.off == 0 and f.C == f.t.shape[3] and f.N == f.t.shape[0] and f.t.is_contiguous():
            return f
        return FM(torch.cat([f.t[..., f.off:f.off + f.C] if (f.off or f.C != f.t.shape[3]) else f.t for f in fms], 0).contiguous())

    @_under_f32_split
    @torch.no_grad()
    def encode(self, input_image, refer_frames):
        """-> {"strings": [mv_y, mv_z, res_y, res_z] (lists over the batch), "shapes": z shapes, "recon": (B,3,H,W)}.
        The reconstruction is the DECODER's: it is built from the coded symbols (the residual is coded against the prediction the
        decoder will make), so a closed-loop encoder and the decoder stay bit-identical."""
        self._model_fp32_checked()
        assert not self.training
        if self.stream_coder not in STREAM_CODERS:
            raise ValueError(f"stream_coder must be one of {STREAM_CODERS}, got {self.stream_coder!r}")
        if self.stream_coder == "device" and self.stream_order != "lanes":
            raise ValueError(f"stream_coder=\"device\" needs stream_order=\"lanes\", got {self.stream_order!r}")
        ims = [self._front(refer_frames, b, input_image) for b in range(refer_frames.shape[0])]
        self.mvCoder.update()
        self.resCoder.update()
        # defer: range coding on worker threads, or on a side stream
        kw = dict(f32=self.coder_fp32 or self.model_fp32, order=self.stream_order, defer=True, lanes=self.stream_lanes, per_image=True, coder=self.stream_coder)
        mv = self.mvCoder.compress(self._dense([im["estmv"] for im in ims]), **kw)
        preds = [self._predict(im, d["y_hat"]) for im, d in zip(ims, mv["_debug"])]
        resid = [ops.scale_act_res(im["f_cur"], FM.empty(1, im["H"], im["W"], 64, dtype=p.t.dtype, device=im["dev"]), res=p, res_sign=-1.0) for im, p in zip(ims, preds)]
        rs = self.resCoder.compress(self._dense(resid), **kw)
        recon = [self._finish(im, d["y_hat"], p) for im, d, p in zip(ims, rs["_debug"], preds)]
        mvs, rss = mv["strings"].result(), rs["strings"].result()                     # join the range coders
        return {"strings": [mvs[0], mvs[1], rss[0], rss[1]], "shapes": [mv["shape"], rs["shape"]], "recon": recon[0] if len(recon) == 1 else torch.cat(recon, 0)}

    @_under_f32_split
    @torch.no_grad()
    def decode(self, strings, shapes, refer_frames):
        """inverse of encode(): strings [mv_y, mv_z, res_y, res_z] + z shapes + the reference list -> (B,3,H,W)"""
        self._model_fp32_checked()
        assert not self.training
        ims = [self._front(refer_frames, b) for b in range(refer_frames.shape[0])]
        self.mvCoder.update()
        self.resCoder.update()
        # synth=False: the coders hand out the latents only, `_predict` and `_finish` run the synthesis
        kw = dict(synth=False, f32=self.coder_fp32 or self.model_fp32, order=self.stream_order, per_image=True)
        mv = self.mvCoder.decompress([strings[0], strings[1]], shapes[0], **kw)["y_hat"]
        image = self.mvCoder._image
        preds = [self._predict(im, image(mv, b)) for b, im in enumerate(ims)]
        res = self.resCoder.decompress([strings[2], strings[3]], shapes[1], **kw)["y_hat"]
        recon = [self._finish(im, image(res, b), preds[b]) for b, im in enumerate(ims)]
        return recon[0] if len(recon) == 1 else torch.cat(recon, 0)
