"""MI355X-native blocks of TDVC's P-frame path.

Each class mirrors a reference module (same attribute names => same state-dict keys, so a
reference checkpoint loads with strict=True) but holds parameters only: the `nn.Conv2d`
objects are containers, their torch forward is never called.  Compute goes through
`tdvc_amd.ops` -> libtdvc_hip.so (hand-written gfx950 kernels).  Weights are packed once into
MFMA fragment order (fp16) and cached; `VideoCompressor.clear_packed()` drops the cache.

Activations are channel-innermost fp16 feature maps (`ops.FM`); concatenations are channel
slices of a shared buffer, never copies.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn

from .. import ops
from ..ops import ACT_LRELU, ACT_NONE, ACT_RELU, FM
from .ring import SlotRing


class PackCache:
    """mixin: lazily packed weights keyed by name, and the reuse states computed from them"""

    def _pk(self, key, fn):
        c = self.__dict__.setdefault("_packed", {})
        if key not in c:
            c[key] = fn()
        return c[key]

    def _state(self, name, key, make):
        """the `ReuseState` kept under `name`: the cached one while its key is `key`, else make(key) in its place"""
        c = self.__dict__.setdefault("_packed", {})
        st = c.get(name)
        if st is None or st.key != key:
            st = c[name] = make(key)
        return st

    @contextlib.contextmanager
    def _state_trusted(self, name):
        """around the launches that write the state's buffers: an exception may leave them half written, the state is never trusted again"""
        try:
            yield
        except BaseException:
            self.__dict__.get("_packed", {}).pop(name, None)
            raise


class ReuseState:
    """What a block keeps from one call to the next (FeatureFix: the I-frame's features; LoopFilter: the per-reference-frame maps), held
    in the packed-weight cache (`PackCache._state`), so that `clear_packed()` and `train.refresh_packed` drop it with the weights it was
    computed from.  `key`: what the buffers were made for.  `usable` is None until the first call has shown whether every launch of the
    chain carries the predicate; then True, or False for good: the buffers are dropped and every call computes in full, unpredicated.
    `log`: the last call's per-kernel answers (ops.predicate).  A subclass names its buffers in `BUFFERS`."""

    __slots__ = ("key", "usable", "log")
    BUFFERS = ()

    def __init__(self, key):
        self.key, self.usable, self.log = key, None, []
        self.drop()

    def drop(self):
        for name in self.BUFFERS:
            setattr(self, name, None)

    def refuse(self):
        """stop caching for this key"""
        self.drop()
        self.usable = False

    def took(self, log) -> bool:
        """the log of the call just enqueued -> usable.  An entry that is not true is a kernel outside the predicated set: it ran in
        full behind producers that may have skipped"""
        self.log = list(log)
        if all(self.log):
            self.usable = True
        else:
            self.refuse()
        return self.usable


def _dev(m: nn.Module):
    return next(m.parameters()).device


def pk_conv(owner: PackCache, name: str, conv: nn.Module, **kw) -> ops.PackedConv:
    """pack an nn.Conv2d / nn.Conv3d parameter holder for the MFMA conv kernel"""
    def build():
        w = conv.weight
        if w.dim() == 5:                       # Conv3d holders
            co, ci, kt, kh, kw_ = w.shape
            if kt == 1:                        # (1,3,3): a 2-D conv applied to every frame (a view of the parameter)
                return ops.pack_conv(w.view(co, ci, kh, kw_), conv.bias, stride=1, pad=conv.padding[-1], device=w.device,
                                     param_w=conv.weight, param_b=conv.bias, **kw)
            # (3,1,1) stride 3: 1x1 conv over T*C channels, t-major, gathered straight from the 5-D parameter
            return ops.pack_conv(w, conv.bias, stride=1, pad=0, device=w.device,
                                 layout=ops.convpack.WeightLayout.conv3d_temporal(co, ci, kt), param_w=conv.weight, param_b=conv.bias, **kw)
        return ops.pack_conv(w, conv.bias, stride=conv.stride[0], pad=conv.padding[0], device=w.device, **kw)
    return owner._pk(name, build)


# --------------------------------------------------------------------------------------
class ConvAct(nn.Module):
    """parameter twin of mmcv ConvModule (`conv` + optional `activate`)"""

    def __init__(self, cin, cout, k, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, padding, bias=True)


class SELayer(nn.Module, PackCache):
    """`main/model/inflate.py:159-208`"""

    def __init__(self, channels, ratio=16):
        super().__init__()
        self.channels = channels
        self.conv1 = ConvAct(channels, int(channels / ratio), 1)
        self.conv2 = ConvAct(int(channels / ratio), channels, 1)

    def params(self) -> ops.SEParams:
        def build():
            c, m = self.channels, self.conv1.conv.out_channels
            f = lambda t: t.detach().float().contiguous()
            return ops.SEParams(f(self.conv1.conv.weight.view(m, c)), f(self.conv1.conv.bias),
                                f(self.conv2.conv.weight.view(c, m)), f(self.conv2.conv.bias), c, m,
                                params=(self.conv1.conv.weight, self.conv1.conv.bias, self.conv2.conv.weight, self.conv2.conv.bias))
        return self._pk("se", build)

    def gate(self, x: FM, partial=None) -> torch.Tensor:
        return ops.se_gate(x, self.params(), partial=partial)

    def run(self, x: FM, out: FM | None = None, act=ACT_NONE, slope=0.0, res: FM | None = None, out2: FM | None = None, sums: list | None = None,
            then: tuple | None = None):
        """`sums`: what `ops.conv(..., chan_sum=sums)` left when it produced `x` (empty: no fused sums, one more pass over x);
        `then` = (b, sign, out3): a second result of the scaling pass, out3 = b + sign * out (`ops.scale_act_res3`)"""
        out = FM.empty(x.N, x.H, x.W, x.C, dtype=x.t.dtype, device=x.t.device) if out is None else out
        gate = self.gate(x, sums[0] if sums else None)
        if then is not None:
            assert out2 is None
            b, b_sign, out3 = then
            return ops.scale_act_res3(x, out, b, out3, b_sign, gate=gate, act=act, slope=slope, res=res)
        return ops.scale_act_res(x, out, gate=gate, act=act, slope=slope, res=res, out2=out2)


class Res_Block(nn.Module, PackCache):
    """`main/utils/utils.py:43-56`"""

    def __init__(self, channels=64):
        super().__init__()
        self.conv1 = nn.Conv2d(channels, channels, 3, 1, 1)
        self.conv2 = nn.Conv2d(channels, channels, 3, 1, 1)

    def run(self, x: FM, out: FM | None = None, res2: FM | None = None) -> FM:
        # inference: both convs in one launch, the intermediate map stays in LDS (tdvc_conv_pair); under the tape (training)
        # and for shapes the fused kernel does not take, two launches
        if self.conv1.in_channels == 64 and ops.conv_pair_supported(x, out, res2) and (out is None or out.desc().p != x.desc().p):
            pp = self._pk("pair", lambda: ops.pack_conv_pair(self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias))
            return ops.conv_pair(x, pp, out=out, act1=ACT_RELU, act2=ACT_NONE, add_input=True, res2=res2)
        t = ops.conv(x, pk_conv(self, "c1", self.conv1), act=ACT_RELU)
        return ops.conv(t, pk_conv(self, "c2", self.conv2), out=out, res=x, res2=res2)


def res_stack(n, ch=64):
    return nn.Sequential(*[Res_Block(ch) for _ in range(n)])


def run_stack(stack, x: FM, out: FM | None = None, res2: FM | None = None) -> FM:
    n = len(stack)
    for i, blk in enumerate(stack):
        last = i == n - 1
        x = blk.run(x, out=out if last else None, res2=res2 if last else None)
    return x


# --------------------------------------------------------------------------------------
# A/B switches of the glue fusions.  Each replaces launches by a fused form with the same bytes, in inference only: training, the tape,
# the per-kernel profile (a table of real work) and traced calls keep the separate launches
PYRAMID_FUSED = True            # SPyNet's two image pyramids in one launch (ops.avgpool2_pyramid) instead of ten avgpool2
FLOW_EPILOGUE = True            # OffsetGen: the flow added in the level-1 fusion conv's epilogue (ops.conv(..., flow=)) instead of add_flow
RESID_FUSED = True              # the residual f_cur - pred as a second result of LoopFilter's last pass (ops.scale_act_res3)
RGB_HEAD = True                 # FeatureFix.featdown on conv_head3 (a tile's loads in flight under the tile before) instead of conv_n16
RATE_FORK = True                # the coders' rate branches on a side stream beside their synthesis transforms (ops.rate_branch); not in coding calls


def glue_fusions_allowed(module: nn.Module, traced: bool = False) -> bool:
    return not module.training and ops.TAPE is None and ops.PROFILE is None and not traced


class SPyNetBasicModule(nn.Module):
    def __init__(self):
        super().__init__()
        ch = [8, 32, 64, 32, 16, 2]
        self.basic_module = nn.Sequential(*[ConvAct(ch[i], ch[i + 1], 7, 1, 3) for i in range(5)])


class SPyNet(nn.Module, PackCache):
    """`main/model/flownet.py:51-175`; one fused warp/upsample/concat kernel + five 7x7 MFMA
    convs per pyramid level, flow kept in fp32."""

    def __init__(self):
        super().__init__()
        self.basic_module = nn.ModuleList([SPyNetBasicModule() for _ in range(6)])
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def compute_flow(self, ref: FM, supp: FM, fused: bool = False, f32: bool = False) -> FM:
        """ref/supp: fp32 fmaps (C=4), H, W multiples of 32 -> flow fp32 fmap (C=2).  `fused` (inference): both image pyramids in
        one launch instead of ten (PYRAMID_FUSED); the level buffers stay separate maps, their bytes the same.  `f32` (the whole-model
        fp32 mode): the level input and the five convs on fp32 maps; the flow map then has 8 channels, 2..7 zero"""
        if fused and PYRAMID_FUSED and ops.avgpool2_pyramid_supported(ref, supp):
            lr_, ls_ = ops.avgpool2_pyramid(ref, supp)
            refs, supps = [ref] + lr_, [supp] + ls_
        else:
            refs, supps = [ref], [supp]
            for _ in range(5):
                refs.append(ops.avgpool2(refs[-1]))
                supps.append(ops.avgpool2(supps[-1]))
        refs, supps = refs[::-1], supps[::-1]
        dev = ref.t.device
        flow = None
        for lvl in range(6):
            r, s = refs[lvl], supps[lvl]
            up = FM.empty(r.N, r.H, r.W, 2, dtype=torch.float32, device=dev)
            x = FM.empty(r.N, r.H, r.W, 8, dtype=torch.float32 if f32 else torch.float16, device=dev)
            ops.spynet_level_input(r, s, flow, up, x)
            bm = self.basic_module[lvl].basic_module
            for i in range(4):
                x = ops.conv(x, pk_conv(self, f"l{lvl}c{i}", bm[i].conv), act=ACT_RELU)
            flow = ops.conv(x, pk_conv(self, f"l{lvl}c4", bm[4].conv), res=up, out_dtype=torch.float32)
        return flow

    def run(self, ref: FM, supp: FM, fused: bool = False, f32: bool = False) -> FM:
        H, W = ref.H, ref.W
        Hu = H if H % 32 == 0 else 32 * (H // 32 + 1)
        Wu = W if W % 32 == 0 else 32 * (W // 32 + 1)
        if (Hu, Wu) != (H, W):
            ref, supp = ops.resize_bilinear(ref, Hu, Wu), ops.resize_bilinear(supp, Hu, Wu)
        flow = self.compute_flow(ref, supp, fused, f32)
        if (Hu, Wu) != (H, W):
            sc = torch.tensor([float(W) / float(Wu), float(H) / float(Hu)], dtype=torch.float32, device=flow.t.device)
            # the fp32 mode's flow map carries six zero channels more; sc has a scale for the two real ones
            flow = ops.resize_bilinear(flow if flow.C == 2 else flow.ch(0, 2), H, W, sc)
        return flow


# --------------------------------------------------------------------------------------
class FeaExtra(nn.Module, PackCache):
    """`main/model/pnet.py:86-96`"""

    def __init__(self, num_block):
        super().__init__()
        self.conv_first = nn.Conv2d(3, 64, 3, 1, 1)
        self.residual_layer = res_stack(num_block)

    def run(self, img8: FM, out: FM) -> FM:
        x = ops.conv(img8, pk_conv(self, "first", self.conv_first), act=ACT_LRELU, slope=0.1)
        return run_stack(self.residual_layer, x, out=out)


class OffsetGen(nn.Module, PackCache):
    """`main/model/pnet.py:99-167`"""

    def __init__(self, nf=64):
        super().__init__()
        self.offset_conv11 = nn.ModuleDict()
        self.offset_conv11_1 = nn.ModuleDict()
        self.offset_conv12 = nn.ModuleDict()
        self.feat_fusion = nn.ModuleDict()
        for i in (3, 2, 1):
            lv = f"l{i}"
            self.offset_conv11[lv] = nn.Conv2d(nf * 2, nf, 3, 1, 1)
            self.offset_conv11_1[lv] = nn.Conv2d(nf, nf, 3, 1, 1)
            self.offset_conv12[lv] = nn.Conv2d(nf, nf, 3, 1, 1)
            if i < 3:
                self.feat_fusion[lv] = nn.Conv2d(nf * 2, nf, 1, 1, 0)
        self.upsample_conv = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv_l2_1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.conv_l2_2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv_l3_1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.conv_l3_2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.spynet = SPyNet()
        self.attn = SELayer(64)
        self.feat_fusion_ = nn.Conv2d(nf, nf, 3, 1, 1)

    def run(self, feats: FM, cur32: FM, ref32: FM, traced: bool = False) -> FM:
        """feats: (B,H,W,>=128) buffer with [f_cur | f_ref] in channels 0..127;
        cur32 / ref32: fp32 RGB fmaps.  Returns estmv (B,H,W,64) in the dtype of `feats` (fp32: the whole-model fp32 mode, every
        layer on fp32 maps in the plain sequence of traced calls)."""
        B, H, W = feats.N, feats.H, feats.W
        f32, adt = feats.f32, feats.t.dtype
        fuse = glue_fusions_allowed(self, traced) and not f32
        flow = None
        dev = feats.t.device
        lr = dict(act=ACT_LRELU, slope=0.1)
        cat1 = feats.ch(0, 128)
        cat2 = FM.empty(B, H // 2, W // 2, 128, dtype=adt, device=dev)
        cat3 = FM.empty(B, H // 4, W // 4, 128, dtype=adt, device=dev)
        for k in (0, 1):   # 0 = current frame features, 1 = reference
            t = ops.conv(cat1.ch(64 * k, 64), pk_conv(self, "l2_1", self.conv_l2_1), **lr)
            ops.conv(t, pk_conv(self, "l2_2", self.conv_l2_2), out=cat2.ch(64 * k, 64), **lr)
            t = ops.conv(cat2.ch(64 * k, 64), pk_conv(self, "l3_1", self.conv_l3_1), **lr)
            ops.conv(t, pk_conv(self, "l3_2", self.conv_l3_2), out=cat3.ch(64 * k, 64), **lr)
        cats = {1: cat1, 2: cat2, 3: cat3}
        up_o1 = None
        off = None
        for i in (3, 2, 1):
            lv = f"l{i}"
            c = cats[i]
            if i == 1 and fuse and FLOW_EPILOGUE:
                # the flow depends on the two frames only: computed ahead of the level whose fusion conv adds it in its epilogue
                flow = self.spynet.run(cur32, ref32, fused=fuse)
            o1 = ops.conv(c, pk_conv(self, "c11" + lv, self.offset_conv11[lv]), **lr)
            if i == 3:
                if ops.conv_pair_supported(o1):            # inference: offset_conv11_1 + offset_conv12 (both LeakyReLU) in one launch
                    c1_, c2_ = self.offset_conv11_1[lv], self.offset_conv12[lv]
                    pp = self._pk("pair_l3", lambda: ops.pack_conv_pair(c1_.weight, c1_.bias, c2_.weight, c2_.bias))
                    off = ops.conv_pair(o1, pp, act1=ACT_LRELU, slope1=0.1, act2=ACT_LRELU, slope2=0.1, add_input=False)
                else:
                    o1 = ops.conv(o1, pk_conv(self, "c11_1" + lv, self.offset_conv11_1[lv]), **lr)
                    off = ops.conv(o1, pk_conv(self, "c12" + lv, self.offset_conv12[lv]), **lr)
            else:
                ops.conv(o1, pk_conv(self, "c11_1" + lv, self.offset_conv11_1[lv]), out=up_o1.ch(64, 64), **lr)
                off = ops.conv(up_o1, pk_conv(self, "ff" + lv, self.feat_fusion[lv]), flow=flow if i == 1 else None, **lr)
            if i > 1:
                up = ops.upsample2x(off)
                up_o1 = FM.empty(B, up.H, up.W, 128, dtype=adt, device=dev)      # [upsampled_offset | offset1]
                ops.conv(up, pk_conv(self, "upc", self.upsample_conv), out=up_o1.ch(0, 64))
        if flow is None:
            flow = self.spynet.run(cur32, ref32, fused=fuse, f32=f32)
            if ops.TAPE is not None:
                off = ops.clone(off)      # keep the fusion conv's own output (LeakyReLU sign) for the backward pass
            ops.add_flow(off, flow)
        sums = []
        e = ops.conv(off, pk_conv(self, "ff_", self.feat_fusion_), chan_sum=sums)
        return self.attn.run(e, sums=sums)


class DCN(nn.Module, PackCache):
    """`main/utils/dcnv2/dcn_v2_amp.py:125-234`: parameters of DCNv2 + conv_offset_mask"""

    def __init__(self, cin, cout, k, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        assert k == 3 and stride == 1 and padding == 1 and dilation == 1
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout))
        self.conv_offset_mask = nn.Conv2d(cin, deformable_groups * 3 * k * k, k, stride, padding)

    def run(self, x: FM, y: FM, out: FM, act=ACT_NONE, slope=0.0) -> FM:
        om = ops.conv(y, pk_conv(self, "om", self.conv_offset_mask))
        pc = self._pk("w", lambda: ops.pack_conv(self.weight, self.bias, stride=1, pad=1, ck=8 * self.deformable_groups,
                                                 device=self.weight.device))
        # output rounded to fp16 BEFORE the activation (reference: `output.half()`, then lrelu on fp16)
        if x.f32:
            # whole-model fp32 mode: fp32 samples, offsets, mask and accumulation (csrc/dcn_f32.hip); the reference's output is an fp16
            # tensor in every mode (dcn_v2_amp.py:15,67-68) that the fp32 features around it widen again
            y16 = FM.empty(x.N, x.H, x.W, out.C, device=x.t.device)
            # Under the tape (train_model_fp32) the widening is a recorded cast: its adjoint rounds the incoming gradient to fp16, the only
            # fp16 value of the sweep -- what the reference's autograd does through `.half()`
            ops.dcn_fused(x, om, pc, y16, groups=self.deformable_groups, act=act, slope=slope, round16=True)
            ops.copy_cast(y16, out)
            ops._rec("cast", y16, out)
            return out
        return ops.dcn_fused(x, om, pc, out, groups=self.deformable_groups, act=act, slope=slope, round16=True)


class MCNet(nn.Module, PackCache):
    """`main/model/pnet.py:170-184`"""

    def __init__(self, num_block):
        super().__init__()
        self.dconv = DCN(64, 64, 3, stride=1, padding=1, deformable_groups=8)
        self.recon_layer = res_stack(num_block)
        self.feat_down = nn.Conv2d(64, 3, 3, 1, 1)
        self.conv = nn.Conv2d(128, 64, 3, 1, 1)

    def run(self, offset: FM, feats: FM, out: FM) -> FM:
        """feats: (B,H,W,192) buffer [f_cur | f_ref | dcn_out]; writes prediction1 into `out`."""
        ref = feats.ch(64, 64)
        dcn_out = feats.ch(128, 64)
        self.dconv.run(ref, offset, dcn_out, act=ACT_LRELU, slope=0.1)
        # reference: conv(cat([out, ref])); our buffer order is [ref | out] -> permute input channels
        perm = list(range(64, 128)) + list(range(0, 64))
        pc = self._pk("conv", lambda: ops.pack_conv(self.conv.weight, self.conv.bias, stride=1, pad=1, cin_perm=perm,
                                                    device=self.conv.weight.device))
        o2 = ops.conv(feats.ch(64, 128), pc, act=ACT_LRELU, slope=0.1)
        return run_stack(self.recon_layer, o2, out=out, res2=dcn_out)


class Bottleneck3D(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1))
        self.spatial_conv3d = nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1))
        self.temporal_conv3d = nn.Conv3d(64, 64, (3, 1, 1), stride=(3, 1, 1), bias=False)
        self.conv3 = nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1))


LOOPFILTER_PAIR = True          # A/B switch (tools/ab_infer.py): layer1.conv1 + spatial_conv3d as one tdvc_conv_pair launch
LOOPFILTER_BCAST = True         # A/B switch: temporal conv + broadcast add + LeakyReLU as one conv_mfma_v5 launch (bcast_T)
LOOPFILTER_REUSE = True         # A/B switch: the per-reference-frame maps of LoopFilter's head persist across P-frames (device-predicated per image)
LOOPFILTER_TAIL = True          # A/B switch: temporal conv + broadcast add + LeakyReLU + conv3 + residual as one tdvc_lf_tail launch (the map between them stays in LDS)
LOOPFILTER_RING = 9             # slots of per-frame maps; a call's window is four of them and slides by one per call (model/ring.py)


class LoopFilterReuse(ReuseState):
    """LoopFilter's state for one (device, stream, B, H, W, ring size): per batch item a ring of slots, each holding what the head of the
    block makes of ONE frame -- `A` (conv01 + conv02 + conv1) and `S` (layer1.conv1 + spatial_conv3d), 64 channels per slot -- and the
    frame it was made from (`F`).  `flags[b]` are the device flags of the last call (1 = slice computed; flags[b, 3], prediction1's,
    stays 1)."""

    __slots__ = ("ring", "A", "S", "F", "flags")
    BUFFERS = ("A", "S", "F", "flags")

    def __init__(self, key, slots):
        super().__init__(key)
        self.ring = SlotRing(slots)


class _LfPlace:
    """Where the per-frame maps of one LoopFilter call live.  `A4`, `S4`: the four slices of every batch item as (B,H,W,256) views --
    two dense buffers, or (`st` given) the window of four slots at position `p` of a LoopFilterReuse state's rings, whose launches run
    under the per-image flags (`force`: the ring's mask of slots that hold nothing comparable)."""

    __slots__ = ("A4", "S4", "st", "p", "force")

    def __init__(self, a: FM, s: FM, st: LoopFilterReuse | None = None, p: int = 0, force: int = 0):
        self.st, self.p, self.force = st, p, force
        self.A4, self.S4 = (a, s) if st is None else (a.ch(64 * p, 256), s.ch(64 * p, 256))

    @property
    def keep_S(self) -> bool:
        """the slots are the next call's inputs: the temporal stage, which rewrites all four slices, must run out of place"""
        return self.st is not None

    def A(self, b, j0=0, n=4) -> FM:
        """slices j0 .. j0 + n - 1 of batch item b as a batch of n 64-channel images: image stride 64 channels, pixel stride the
        buffer's (256 channels, or the whole ring's)"""
        return self.A4.as_slices(b, 4, 64).batch(j0, n)

    def S(self, b, j0=0, n=4) -> FM:
        return self.S4.as_slices(b, 4, 64).batch(j0, n)

    def flags(self, b, n):
        """`with place.flags(b, n) as log:` -- the launches inside run under the flags of the first n slices of batch item b"""
        return contextlib.nullcontext([]) if self.st is None else ops.predicate_images(self.st.flags[b, :n])


class LoopFilter(nn.Module, PackCache):
    """`main/model/pnet.py:266-317`: multi-frame feature fusion.  The (B,64,T=4,H,W) tensor of the
    reference is one (B,H,W,256) buffer whose four 64-channel slices are the frames, so the
    Conv3d(1,3,3) layers are 2-D convs over slices and the final flatten is free."""

    def __init__(self):
        super().__init__()
        self.conv01 = nn.Conv2d(3, 64, 3, 1, 1)
        self.conv02 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv1 = nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1))
        self.layer1 = Bottleneck3D()
        self.attn = SELayer(64)
        self.feat_fusion = nn.Conv2d(256, 64, 1, 1)

    def _slices(self, name, conv, src: FM, dst: FM, **kw):
        pc = pk_conv(self, name, conv)
        for b in range(src.N):
            ops.conv(src.as_slices(b, 4, 64), pc, out=dst.as_slices(b, 4, 64), **kw)

    def run(self, xt: FM, refs8: FM, out: FM, then: tuple | None = None) -> FM:
        """xt: (B,H,W,256) with prediction1 already in slice 3; refs8: (B*4,H,W,8) fp16 frames
        [I, r-3, r-2, r-1] per batch item; writes the fused prediction into `out`.  `then` = (b, sign, out3), inference only: the last
        pass also writes out3 = b + sign * out (the residual `f_cur - pred`, RESID_FUSED) instead of a launch that reads `out` back."""
        B, H, W = xt.N, xt.H, xt.W
        dev, adt = xt.t.device, xt.t.dtype
        # conv01, conv02 + conv1 and layer1.conv1 + spatial_conv3d do not mix frames, and by the reference-list rule (synth.ref_list) this
        # call's r-3 and r-2 are the previous call's r-2 and r-1: their maps are kept in ring slots (`_ring_place`).  Training, the tape, the
        # per-kernel profile (a table of real work), fp32 inputs and shapes the fused kernels do not take compute everything afresh
        if (LOOPFILTER_REUSE and LOOPFILTER_PAIR and LOOPFILTER_BCAST and glue_fusions_allowed(self) and not xt.f32 and not refs8.f32
                and H * W >= 8192 and ops.conv_pair_supported(xt.as_slices(0, 4, 64))):
            key = (dev.index, ops._stream().value, B, H, W, LOOPFILTER_RING)
            st = self._state("lf_reuse", key, lambda key: LoopFilterReuse(key, LOOPFILTER_RING))
            if st.usable is not False:                    # False: some launch of the head does not test the flags at this shape
                with self._state_trusted("lf_reuse"):
                    place = self._ring_place(st, refs8)
                    if place is not None and st.took(self._head(place, xt, refs8)):
                        st.ring.commit()
                        return self._finish(self._tail(place), xt, out, then)
            # the skipping cannot be relied on: the state's buffers are gone, and the plain form below computes everything
        place = _LfPlace(FM.empty(B, H, W, 256, dtype=adt, device=dev), FM.empty(B, H, W, 256, dtype=adt, device=dev))
        if LOOPFILTER_PAIR and ops.conv_pair_supported(place.A(0), place.S(0)):
            self._head(place, xt, refs8)
            bf = None
        else:
            bf = self._head_unfused(place, xt, refs8)
        return self._finish(self._tail(place, bf), xt, out, then)

    def reuse_state(self) -> LoopFilterReuse | None:
        return self.__dict__.get("_packed", {}).get("lf_reuse")

    def _ring_place(self, st: LoopFilterReuse, refs8: FM) -> _LfPlace | None:
        """The window of this call on the persistent per-frame slots of `st`.  Per batch item `ops.frames_changed` compares the three
        reference frames with the frames the window's slots were computed from (exact, on the device; slots that hold nothing comparable
        are forced) and the head's launches run under the per-image flags: conv_c8 and conv_pair compute the images whose flag is set,
        their workgroups sharing that work, and leave the other slots as they are.  No host wait, no dependence on tensor identity,
        bit-identical results.  -> None when the launcher does not take the windows (nothing has been launched then)."""
        first = st.A is None
        if first:
            _, _, B, H, W, R = st.key
            dev = refs8.t.device
            st.A, st.S = FM.empty(B, H, W, 64 * R, device=dev), FM.empty(B, H, W, 64 * R, device=dev)
            st.F = FM.empty(B * R, H, W, refs8.C, device=dev)
            st.flags = torch.ones((B, 4), dtype=torch.int32, device=dev)
        p, force = st.ring.begin()                        # first call and first call behind a wrap: every slot forced
        place = _LfPlace(st.A, st.S, st, p, force)
        # the launcher must take the views the head really runs on: slot windows of pixel stride 64 R (not the dense slices that `run`
        # asked about); A(0, 0, 3) as the first pair's output (geometry query)
        if first and not (ops.conv_pair_supported(place.A(0, 0, 3)) and ops.conv_pair_supported(place.A(0), place.S(0))):
            st.refuse()
            return None
        return place

    def _head(self, place: _LfPlace, xt: FM, refs8: FM) -> list:
        """The fused head (inference), batch item by batch item: conv01, then conv02 (no activation) + conv1 (LeakyReLU) of the three
        reference slices in one launch -- nothing else reads conv02's output; slice 3 (prediction1, already in xt) takes conv1 alone;
        then layer1.conv1 (LeakyReLU) + layer1.spatial_conv3d of the four slices in one launch, their intermediate map stays in LDS.
        -> the launches' answers under the per-image flags: three per batch item on ring slots, none on dense buffers"""
        lr = dict(act=ACT_LRELU, slope=0.1)
        l1, st = self.layer1, place.st
        p01, pc1 = pk_conv(self, "c01", self.conv01), pk_conv(self, "c1", self.conv1)
        pp_a = self._pk("pair_c02_c1", lambda: ops.pack_conv_pair(self.conv02.weight, self.conv02.bias,
                                                                   self.conv1.weight.view(64, 64, 3, 3), self.conv1.bias))
        pp_b = self._pk("pair_b1_bs", lambda: ops.pack_conv_pair(l1.conv1.weight.view(64, 64, 3, 3), l1.conv1.bias,
                                                                  l1.spatial_conv3d.weight.view(64, 64, 3, 3), l1.spatial_conv3d.bias))
        log = []
        for b in range(xt.N):
            frames = refs8.batch(4 * b + 1, 3)
            if st is not None:
                ops.frames_changed(frames, st.F.batch(b * st.ring.slots + place.p, 3), st.flags[b, :3], place.force)
            with place.flags(b, 3) as lg:
                t = ops.conv(frames, p01, **lr)           # a skipped image's slice of `t` is never written, and never read
                ops.conv_pair(t, pp_a, out=place.A(b, 0, 3), act1=ACT_NONE, act2=ACT_LRELU, slope2=0.1, add_input=False)
            log += lg
            ops.conv(xt.as_slices(b, 4, 64).batch(3, 1), pc1, out=place.A(b, 3, 1), **lr)
            with place.flags(b, 4) as lg:
                ops.conv_pair(place.A(b), pp_b, out=place.S(b), act1=ACT_LRELU, slope1=0.1, act2=ACT_NONE, add_input=False)
            log += lg
        return log

    def _head_unfused(self, place: _LfPlace, xt: FM, refs8: FM) -> FM:
        """The head layer by layer over the whole batch, on dense buffers: under the tape (this is the order training records), on fp32
        maps, with LOOPFILTER_PAIR off and at shapes conv_pair does not take.  -> `bf`, layer1.conv1's output: the backward pass of
        spatial_conv3d needs it; in inference it is free again"""
        lr = dict(act=ACT_LRELU, slope=0.1)
        p01, p02 = pk_conv(self, "c01", self.conv01), pk_conv(self, "c02", self.conv02)
        for b in range(xt.N):
            t = ops.conv(refs8.batch(4 * b + 1, 3), p01, **lr)                 # (3,H,W,64)
            ops.conv(t, p02, out=xt.as_slices(b, 4, 64).batch(0, 3))
        self._slices("c1", self.conv1, xt, place.A4, **lr)
        bf = FM.empty(xt.N, xt.H, xt.W, 256, dtype=xt.t.dtype, device=xt.t.device)
        self._slices("b1", self.layer1.conv1, place.A4, bf, **lr)
        self._slices("bs", self.layer1.spatial_conv3d, bf, place.S4)
        return bf

    def _tail(self, place: _LfPlace, bf: FM | None = None) -> FM:
        """The temporal (3,1,1) conv over slices 0-2, `S + temporal` + LeakyReLU over the four slices (pnet.py:304-314), conv3 and the
        residual A -> the block's output `o` (B,H,W,256).  `bf`: the unfused head's spare buffer, which inference re-uses for `o`; under
        the tape the backward pass of spatial_conv3d still needs it"""
        l1 = self.layer1
        A4, S4 = place.A4, place.S4
        fresh = lambda: FM.empty(A4.N, A4.H, A4.W, 256, dtype=A4.t.dtype, device=A4.t.device)
        pct, pc3 = pk_conv(self, "bt", l1.temporal_conv3d), pk_conv(self, "b3", l1.conv3)
        o = bf if bf is not None and ops.TAPE is None else fresh()
        if (LOOPFILTER_TAIL and LOOPFILTER_BCAST and glue_fusions_allowed(self) and l1.temporal_conv3d.bias is None
                and ops.lf_tail_supported(S4, A4, o)):
            # all of it as one launch, the map between the temporal stage and conv3 never reaches memory
            return ops.lf_tail(S4, A4, pct, pc3, out=o, slope=0.1)
        if ops.TAPE is None and LOOPFILTER_BCAST and A4.H * A4.W >= 8192 and not S4.f32:      # per IMAGE: conv_v5_eligible (csrc/conv_mfma_v5.hip) counts one map
            # the temporal stage as ONE pass: a wave computes the 64 temporal channels of its pixels and rewrites their four slices, in
            # place on dense buffers; ring slots keep what the next call reuses, so from them the pass writes a buffer of its own
            s = fresh() if place.keep_S else S4
            ops.conv(S4.ch(0, 192), pct, out=s.ch(0, 64), bcast_T=4, bcast_slope=0.1, res=S4.ch(0, 64) if place.keep_S else None)
        else:
            assert not place.keep_S, "the reuse form is entered only where the one-pass temporal stage runs"
            tm = ops.conv(S4.ch(0, 192), pct)
            s = ops.clone(S4) if ops.TAPE is not None else S4          # S is the temporal conv's input: kept for the backward pass
            ops.bcast_add_act(s, tm, 4, 0.1)
        for b in range(A4.N):
            ops.conv(s.as_slices(b, 4, 64), pc3, out=o.as_slices(b, 4, 64), res=place.A(b))
        return o

    def _finish(self, o: FM, xt: FM, out: FM, then: tuple | None) -> FM:
        sums = []
        f = ops.conv(o, pk_conv(self, "ff", self.feat_fusion), chan_sum=sums, act=ACT_LRELU, slope=0.1)
        return self.attn.run(f, out=out, res=xt.ch(192, 64), sums=sums, then=then)


class FeatureExtract(nn.Module, PackCache):
    """`main/model/pnet.py:320-332` (F.leaky_relu default slope 0.01)"""

    def __init__(self, cin, mid, nblocks):
        super().__init__()
        self.conv_first = nn.Conv2d(cin, mid, 3, 1, 1)
        self.body = res_stack(nblocks, mid)
        self.conv_last = nn.Conv2d(mid, mid, 3, 1, 1)

    def run(self, x: FM, out: FM | None = None) -> FM:
        x1 = ops.conv(x, pk_conv(self, "first", self.conv_first), act=ACT_LRELU, slope=0.01)
        t = run_stack(self.body, x1)
        return ops.conv(t, pk_conv(self, "last", self.conv_last), out=out, res=x1)


FEATUREFIX_REUSE = True         # A/B switch: FeatureFix keeps the I-frame's feature maps across the P-frames of a GOP (device-predicated)


class IFrameReuse(ReuseState):
    """FeatureFix's state for one (device, stream, B, H, W, scale): what `FeatureExtract_ref` + `avgpool_k` make of the I-frame (`y`,
    `pref`), the frame they were made from (`iframe`) and the device flag of the last call (`flag`: 1 = the frame had changed)."""

    __slots__ = ("y", "iframe", "pref", "flag")
    BUFFERS = __slots__


class FeatureFix(nn.Module, PackCache):
    """`main/model/pnet.py:187-263`: reference-based in-loop filter"""

    def __init__(self):
        super().__init__()
        self.FeatureExtract_input = FeatureExtract(64, 64, 2)
        self.FeatureExtract_ref = FeatureExtract(3, 64, 2)
        self.recon_layer = res_stack(2)
        self.conv_10 = nn.Conv2d(64, 64, 3, 2, 1)
        self.conv_11 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_12 = nn.Conv2d(64, 64, 3, 2, 1)
        self.conv_13 = nn.Conv2d(64, 64, 3, 1, 1)
        self.featfusion = nn.Conv2d(128, 64, 3, 1, 1)
        self.featfusion2 = nn.Conv2d(128, 64, 3, 1, 1)
        self.featdown = nn.Conv2d(64, 3, 3, 1, 1)
        self.attn = SELayer(64)

    def run(self, x: FM, iframe8: FM, training: bool, trace=None) -> torch.Tensor:
        """x: reconstructed features (B,H,W,64); iframe8: I-frame (B,H,W,8) fp16 (both fp32 in the whole-model fp32 mode).
        Returns the clamped RGB reconstruction as NCHW fp32."""
        B, H, W = x.N, x.H, x.W
        dev = x.t.device
        lr = dict(act=ACT_LRELU, slope=0.1)
        fin = self.FeatureExtract_input.run(x)
        scale = 8 if training else int(H / 8)
        # fref and its pooled map depend on the I-frame and the weights only: slot 0 of the reference list is the GOP's I-frame for every
        # P-frame of the GOP (tools/predict.py).  Training, the tape, the per-kernel profile (a table of real work) and traced calls (they
        # hand out `fref`) compute them afresh
        if FEATUREFIX_REUSE and not training and ops.TAPE is None and ops.PROFILE is None and trace is None and not iframe8.f32:
            y, pref = self._iframe_features(iframe8, scale)
            fref = y.ch(64, 64)
        else:
            y = FM.empty(B, H, W, 128, dtype=x.t.dtype, device=dev)            # [o | fref]
            fref = self.FeatureExtract_ref.run(iframe8, out=y.ch(64, 64))
            pref = ops.avgpool_k(fref, scale)
        pin = ops.avgpool_k(fin, scale)
        idx = ops.patch_match(pin, pref)
        cat = FM.empty(B, H, W, 128, dtype=x.t.dtype, device=dev)          # [fin*cor | out*cor]
        ops.match_gather(fin, fref, idx, scale, cat)
        ops.conv(cat, pk_conv(self, "ff", self.featfusion), out=y.ch(0, 64), **lr)
        sums = []
        o2 = ops.conv(y, pk_conv(self, "ff2", self.featfusion2), chan_sum=sums)
        o2 = self.attn.run(o2, sums=sums, **lr)
        o = run_stack(self.recon_layer, o2, res2=x)
        rgb = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        with ops.rgb_head_kernel(RGB_HEAD and glue_fusions_allowed(self, trace is not None)):
            ops.conv(o, pk_conv(self, "down", self.featdown), act=ops.ACT_CLAMP01, nchw_out=rgb)
        if trace is not None:
            trace.update(ff_idx=idx, ff_fin=fin, ff_fref=fref)
        return rgb

    def reuse_state(self) -> IFrameReuse | None:
        return self.__dict__.get("_packed", {}).get("iframe_reuse")

    def _iframe_features(self, iframe8: FM, scale: int):
        """-> (y, pref): the (B,H,W,128) buffer whose upper half is FeatureExtract_ref(I-frame), and its pooled map.  Both persist
        in the state; from the second call on a device-side compare of the I-frame with the cached one (`ops.frame_changed`) sets a flag
        and the chain's six kernels are launched under it: they return at once when the frame is the cached one.  No host wait, no
        dependence on tensor identity, and bit-identical results (the compare is exact).  The state lives in the packed-weight
        cache: `clear_packed()` (load_state_dict, .to()) and `train.refresh_packed` drop it with the weights it was computed from."""
        B, H, W = iframe8.N, iframe8.H, iframe8.W
        dev = iframe8.t.device
        st = self._state("iframe_reuse", (dev.index, ops._stream().value, B, H, W, scale), IFrameReuse)

        def chain(y, pref):
            fref = self.FeatureExtract_ref.run(iframe8, out=y.ch(64, 64))
            ops.avgpool_k(fref, scale, out=pref)

        def fresh():
            return (FM.empty(B, H, W, 128, device=dev),
                    torch.empty((B, H // scale, W // scale, 64), dtype=torch.float32, device=dev))

        if st.usable is False:                            # some kernel of the chain does not test the flag at this shape
            y, pref = fresh()
            chain(y, pref)
            return y, pref
        with self._state_trusted("iframe_reuse"):
            first = st.usable is None
            if first:                                     # fill the cache, computing under a flag of 1 to learn who tests it
                st.y, st.pref = fresh()
                st.iframe = FM.empty(B, H, W, iframe8.C, device=dev)
                st.flag = torch.ones(1, dtype=torch.int32, device=dev)
                ops.copy_cast(iframe8, st.iframe)
            else:
                ops.frame_changed(iframe8, st.iframe, st.flag)
            with ops.predicate(st.flag) as log:
                chain(st.y, st.pref)
            y, pref = st.y, st.pref
            if not st.took(log) and not first:
                chain(y, pref)                            # producers may have skipped in front of a kernel that ran: again, without the flag
        return y, pref
