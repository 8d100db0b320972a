"""ResNet trunk with the reference's interface (models/resnet.py:11-45: `ResNet(n_layers)`, `model(x)` -> the `res5`
activation of chainer's ResNetLayers): conv1 7x7/2 + BN + ReLU, max-pool 3x3/2, res2..res5 of Caffe-style bottlenecks
(stride on the first 1x1 of a stage, projection shortcut in block `a`), BatchNormalization in TEST mode.

Wiring chosen for Faster R-CNN (the reference never instantiates FasterRCNN with it): the literal one --
`res5` (1,2048,H/32,W/32), so `FasterRCNN(trunk_class=ResNet101, rpn_in_ch=2048, feat_stride=32)`.

Every convolution runs on the fp32 MFMA kernel (csrc/conv.hip): 3x3 as is, 1x1 as the KS=1 instantiation, the 7x7 stem
as an explicit im2col + 1x1, a stride-2 1x1 as subsample + 1x1; BN is folded into weights and bias at load
(W' = W * gamma/sqrt(var+eps), b' = beta - mean * gamma/sqrt(var+eps), eps = 2e-5: chainer's default); the bottleneck
tail relu(conv3 + shortcut) is fused into conv3's epilogue.  Parameters keep chainer's link paths
(`conv1/W`, `bn1/gamma|beta|avg_mean|avg_var`, `res3/a/conv1/W`, `res3/b1/bn2/gamma`, ...).
Train-mode BatchNormalization (batch statistics) is not implemented: the trunk is inference-only.

conv_dtype="bf16" runs the trunk on the 16-bit chain (channel-blocked [C/16][H][W][16] maps, operands rounded to nearest even, fp32
accumulation): the stem as frcnn_im2col7x7s2_bf16 + the 1x1 kernel (Kp = 160), frcnn_maxpool3x3s2_bf16, every 1x1 (stride 2 folded into
the load, the tail relu(conv3 + shortcut) fused) on frcnn_conv1x1_bf16 (csrc/resnet_bf16.hip), every 3x3 on frcnn_conv_bf16_ws.  On a
with_half("f16") runtime the same calls run the fp16 twins (FasterRCNN(conv_dtype="f16") hands the trunk such a runtime).
"""
import numpy as np

from ..chainer_compat import unwrap
from ..runtime import default_runtime

BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
STAGES = [("res2", 64, 64, 256, 1), ("res3", 256, 128, 512, 2), ("res4", 512, 256, 1024, 2), ("res5", 1024, 512, 2048, 2)]
BN_EPS = 2e-5


def block_names(n):
    return ["a"] + ["b%d" % i for i in range(1, n)]


def conv_specs(blocks):
    """[(link path of the conv, link path of its BN, cin, cout, ksize)] in execution order."""
    out = [("conv1", "bn1", 3, 64, 7)]
    for (stage, cin, mid, cout, _), n in zip(STAGES, blocks):
        for b in block_names(n):
            i = cin if b == "a" else cout
            p = "%s/%s/" % (stage, b)
            out += [(p + "conv1", p + "bn1", i, mid, 1), (p + "conv2", p + "bn2", mid, mid, 3), (p + "conv3", p + "bn3", mid, cout, 1)]
            if b == "a":
                out.append((p + "conv4", p + "bn4", i, cout, 1))
    return out


class _FoldedConv(object):
    def __init__(self, rt, W, bn, ksize, conv_bias=None, half=False):
        """W (co,ci,k,k) [+ an optional convolution bias: chainer's ResNetLayers creates conv1 WITH one] + its BN statistics ->
        packed (ci*k*k [padded], co) weights and a (co,) bias on device:  bn(conv(x) + b) = s*conv(x) + beta + (b - mean)*s."""
        gamma, beta, mean, var = [np.asarray(v, dtype=np.float64) for v in bn]
        s = gamma / np.sqrt(var + BN_EPS)
        if conv_bias is not None:
            mean = mean - np.asarray(conv_bias, dtype=np.float64)
        Wf = (np.asarray(W, dtype=np.float64) * s[:, None, None, None]).astype(np.float32)
        co = Wf.shape[0]
        packed = np.ascontiguousarray(Wf.reshape(co, -1).T)                 # (ci*k*k, co): the kernels' layout
        if ksize == 7:                                                      # im2col rows padded to a multiple of 8
            kp = (packed.shape[0] + 7) // 8 * 8
            packed = np.concatenate([packed, np.zeros((kp - packed.shape[0], co), np.float32)], 0)
        self.Wp = rt.mem.from_numpy(packed)
        self.b = rt.mem.from_numpy((beta - mean * s).astype(np.float32))
        self.ksize = ksize
        self.cin, self.cout = Wf.shape[1] * ksize * ksize if ksize == 7 else Wf.shape[1], co
        self.Wh = None
        if half:
            # the same folded weights packed once for the 16-bit kernels ([CinP/16][tap][CoutP][16]): the stem's (co, ci*49) matrix as a 1x1 layer
            # whose input is the im2col of csrc/resnet_bf16.hip (rows padded to 160 by the packing)
            w = Wf.reshape(co, -1, 1, 1) if ksize == 7 else Wf
            self.Wh = rt.bf16_pack_conv_w(rt.mem.from_numpy(np.ascontiguousarray(w)), ksize=1 if ksize == 7 else ksize)
            if ksize == 7:
                self.cin = rt.bf16_pad(self.cin)


class ResNet(object):
    def __init__(self, n_layers=101, runtime=None, blocks=None, conv_dtype="f32"):
        if conv_dtype == "f32s":
            raise ValueError("ResNet: conv_dtype 'f32s' (split-product fp32) is not implemented for the ResNet trunk; use 'f32' or 'bf16'")
        if conv_dtype not in ("f32", "bf16"):
            raise ValueError("ResNet: conv_dtype must be 'f32' or 'bf16' (fp16: a with_half('f16') runtime), not %r" % (conv_dtype,))
        self.rt = runtime or default_runtime()
        self.blocks = tuple(blocks) if blocks is not None else BLOCKS[n_layers]
        self.conv_dtype = conv_dtype
        self.train = False
        self.convs = {}
        self.skip_nchw = False
        self.feat_bf16 = self.feat_shape = None

    def load_params(self, params, prefix="trunk/"):
        for conv, bn, ci, co, k in conv_specs(self.blocks):
            W = params[prefix + conv + "/W"]
            assert tuple(W.shape) == (co, ci, k, k), (conv, tuple(W.shape))
            stats = [params[prefix + bn + "/" + n] for n in ("gamma", "beta", "avg_mean", "avg_var")]
            self.convs[conv] = _FoldedConv(self.rt, W, stats, k, conv_bias=params.get(prefix + conv + "/b"), half=self.conv_dtype == "bf16")

    def _conv(self, name, x, act=1, residual=None):
        c = self.convs[name]
        return self.rt.conv_ex(x, c.Wp, c.b, 1 if c.ksize == 7 else c.ksize, act=act, mask=residual)

    def __call__(self, x, timer=None, collect=None):
        if self.train:
            raise NotImplementedError("train-mode BatchNormalization (batch statistics) is not part of this path")
        rt = self.rt
        h = rt.asarray(unwrap(x), "f32")
        assert h.ndim == 4 and int(h.shape[0]) == 1, "batch size 1 (models/faster_rcnn.py:77)"
        if self.conv_dtype == "bf16":
            return self._call_bf16(h, timer, collect)
        if collect is not None:
            raise ValueError("ResNet: per-layer collection is a feature of the 16-bit trunk (conv_dtype='bf16')")
        h = self._conv("conv1", rt.im2col7x7s2(h, int(self.convs["conv1"].Wp.shape[0])))      # conv1 + bn1 + relu
        h = rt.maxpool3x3s2(h)
        for (stage, _, _, _, stride), n in zip(STAGES, self.blocks):
            for b in block_names(n):
                p = "%s/%s/" % (stage, b)
                xin = rt.subsample2(h) if (b == "a" and stride == 2) else h                # stride sits on the first 1x1 (and the shortcut)
                shortcut = self._conv(p + "conv4", xin, act=0) if b == "a" else h
                t = self._conv(p + "conv1", xin)
                t = self._conv(p + "conv2", t)
                h = self._conv(p + "conv3", t, act=3, residual=shortcut)                   # relu(bn3(conv3) + shortcut)
            if timer:
                timer.mark(stage)
        return h

    def _h1x1(self, name, x, stride=1, act=1, residual=None):
        c = self.convs[name]
        return self.rt.conv1x1_bf16(x, c.Wh, c.b, c.cin, c.cout, stride=stride, act=act, residual=residual)

    def _call_bf16(self, x, timer, collect=None):
        """16-bit chain: fp32 NCHW image -> stem columns (blocked) -> conv1 -> pool1 -> res2..res5 -> res5 as fp32 NCHW (or None when
        skip_nchw: FasterRCNN.forward_device pools from feat_bf16 itself).  `collect` (optional dict) receives every layer's blocked map
        as (array, channels) under its link path (`conv1`, `pool1`, `res3/a/conv4`, ...)."""
        rt = self.rt

        def keep(name, h, c):
            if collect is not None:
                collect[name] = (h, c)

        stem = self.convs["conv1"]
        h = self._h1x1("conv1", rt.im2col7x7s2_bf16(x, stem.cin))                         # conv1 + bn1 + relu
        keep("conv1", h, 64)
        h = rt.maxpool3x3s2_bf16(h)
        keep("pool1", h, 64)
        cout = 64
        for (stage, _, mid, cout, stride), n in zip(STAGES, self.blocks):
            for b in block_names(n):
                p = "%s/%s/" % (stage, b)
                s = stride if b == "a" else 1                                             # stride sits on the first 1x1 (and the shortcut)
                shortcut = self._h1x1(p + "conv4", h, stride=s, act=0) if b == "a" else h
                if b == "a":
                    keep(p + "conv4", shortcut, cout)
                t = self._h1x1(p + "conv1", h, stride=s)
                keep(p + "conv1", t, mid)
                c2 = self.convs[p + "conv2"]
                t = rt.conv_bf16(t, c2.Wh, c2.b, mid, mid, ksize=3, relu=True)
                keep(p + "conv2", t, mid)
                h = self._h1x1(p + "conv3", t, act=3, residual=shortcut)                  # relu(bn3(conv3) + shortcut)
                keep(p + "conv3", h, cout)
            if timer:
                timer.mark(stage)
        self.feat_bf16 = h
        self.feat_shape = (1, cout, int(h.shape[1]), int(h.shape[2]))
        if self.skip_nchw:
            return None
        feat = rt.bf16_to_nchw(h, cout)
        if timer:
            timer.mark("to_nchw")
        return feat


def ResNet50(runtime=None, **kw):
    return ResNet(50, runtime=runtime, **kw)


def ResNet101(runtime=None, **kw):
    return ResNet(101, runtime=runtime, **kw)


def ResNet152(runtime=None, **kw):
    return ResNet(152, runtime=runtime, **kw)
