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

Training (fp32): with `train = True` (the reference's default, models/resnet.py:41-45: `test = not self.train`) every BatchNormalization
runs on the statistics of the map it is given (csrc/bn_train.hip): each convolution runs unfolded with act = 0, frcnn_bn_train_fwd_f32
normalises its output with the ReLU -- and in a bottleneck tail the shortcut sum -- fused, and updates the running statistics.  The call
keeps a tape (conv inputs, pre-BN maps z, outputs y, saved mean and 1/std); `backward(g, grads)` walks it in reverse and fills the gradient
of every W (packed layout), gamma, beta and `conv1/b`.  `mark_params_updated()` re-folds the inference weights from the current parameters
and running statistics.  The 16-bit trunks (conv_dtype) are inference-only.

Training on bf16 operands: train_dtype="bf16" (with conv_dtype="f32"; parameters stay the fp32 master copies in `tp`).  The trunk owns its tape and its
backward pass, so it owns the arithmetic of its train-mode pass, as it owns conv_dtype for inference; a trainer's conv_math / precision stay the
arithmetic of the trainer's own links.  In the train-mode pass every convolution PRODUCT then runs on bf16 operands with fp32 accumulation -- the forward
pass of every layer, the input gradient of every layer but the stem, the weight gradient of every layer -- each operand the round-to-nearest-even image
of the fp32 tensor the tape holds (x, the master W, dz).  1x1 layers and the stem (over its fp32 im2col columns) run csrc/conv1x1_train_bf16.hip, which
rounds while it stages: no per-step weight re-pack, the input gradient reads the forward pass's packed weights.  The 3x3 conv2 layers run
frcnn_bf16_from_nchw_f32 + frcnn_conv3x3_bf16_train (forward, and the input gradient on input-gradient weights) and frcnn_conv_wgrad_bf16; their 16-bit
weights are re-packed once after an update, sixteen layers per launch (frcnn_bf16_pack_many).  Everything else is the fp32 step's: im2col, conv1/b and
the bias gradient, BatchNorm forward and backward on the fp32 pre-BN maps, ReLU masks, pooling, subsampling, shortcut adds, the tape, the running
statistics, the re-fold.  The test-mode pass and the fp32 train-mode pass are untouched.

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
BN_DECAY = 0.9          # L.BatchNormalization's default: running = decay * running + (1 - decay) * batch statistic


def block_names(n):
    return ["a"] + ["b%d" % i for i in range(1, n)]


def stages(base_width=64):
    """STAGES with every width scaled by base_width / 64 (64: the published network)"""
    return [(s, ci * base_width // 64, mid * base_width // 64, co * base_width // 64, st) for s, ci, mid, co, st in STAGES]


def conv_specs(blocks, base_width=64):
    """[(link path of the conv, link path of its BN, cin, cout, ksize)] in execution order."""
    out = [("conv1", "bn1", 3, base_width, 7)]
    for (stage, cin, mid, cout, _), n in zip(stages(base_width), blocks):
        for b in block_names(n):
            i = cin if b == "a" else cout
            p = "%s/%s/" % (stage, b)
            out += [(p + "conv1", p + "bn1", i, mid, 1), (p + "conv2", p + "bn2", mid, mid, 3), (p + "conv3", p + "bn3", mid, cout, 1)]
            if b == "a":
                out.append((p + "conv4", p + "bn4", i, cout, 1))
    return out


def pack_w(W, ksize):
    """(co,ci,k,k) -> the convolution kernels' (ci*k*k [the 7x7 stem's im2col rows padded to a multiple of 8], co) fp32"""
    W = np.asarray(W, dtype=np.float32)
    co = W.shape[0]
    packed = np.ascontiguousarray(W.reshape(co, -1).T)
    if ksize == 7:
        kp = (packed.shape[0] + 7) // 8 * 8
        packed = np.concatenate([packed, np.zeros((kp - packed.shape[0], co), np.float32)], 0)
    return packed


def unpack_w(packed, co, ci, ksize):
    """pack_w's inverse (the stem's padding rows dropped)"""
    return np.ascontiguousarray(np.asarray(packed)[:ci * ksize * ksize].T).reshape(co, ci, ksize, ksize)


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
    def __init__(self, n_layers=101, runtime=None, blocks=None, conv_dtype="f32", base_width=64, train_dtype="f32"):
        if conv_dtype == "f32s":
            raise ValueError("ResNet: conv_dtype 'f32s' (split-product fp32) is not implemented for the ResNet trunk; use 'f32' or 'bf16'")
        if conv_dtype not in ("f32", "bf16"):
            raise ValueError("ResNet: conv_dtype must be 'f32' or 'bf16' (fp16: a with_half('f16') runtime), not %r" % (conv_dtype,))
        if train_dtype not in ("f32", "bf16"):
            raise ValueError("ResNet: train_dtype must be 'f32' or 'bf16' (fp16 training needs a loss scale: not built), not %r" % (train_dtype,))
        if train_dtype == "bf16" and conv_dtype != "f32":
            raise ValueError("ResNet: train_dtype='bf16' needs conv_dtype='f32' (the train-mode pass rounds the fp32 master parameters; the 16-bit "
                             "inference trunks hold none), not conv_dtype=%r" % (conv_dtype,))
        self.rt = runtime or default_runtime()
        self.train_dtype = train_dtype
        self.blocks = tuple(blocks) if blocks is not None else BLOCKS[n_layers]
        self.conv_dtype = conv_dtype
        if int(base_width) < 64 or int(base_width) % 64:
            raise ValueError("ResNet: base_width must be a multiple of 64 (the fp32 convolution kernels take Cout %% 64 == 0, and every width is "
                             "some layer's Cout, forward or in its input-gradient convolution), not %r" % (base_width,))
        self.base_width = int(base_width)
        self.stages = stages(self.base_width)
        self.train = False
        self.convs = {}
        self.tp = {}                                           # train-mode parameters on the device, by link path below the prefix
        self.tape = None
        self._wd, self._wd_stale = {}, True                    # input-gradient packings of tp's weights, re-packed after an update
        self._w16, self._w16_stale = {}, True                  # train_dtype "bf16": 16-bit forward / input-gradient weights of the 3x3 layers
        self._zero_bias = {}
        self._fold_stale = False
        self.skip_nchw = False
        self.feat_bf16 = self.feat_shape = None

    def load_params(self, params, prefix="trunk/"):
        m = self.rt.mem
        for conv, bn, ci, co, k in conv_specs(self.blocks, self.base_width):
            W = params[prefix + conv + "/W"]
            assert tuple(W.shape) == (co, ci, k, k), (conv, tuple(W.shape))
            stats = [params[prefix + bn + "/" + n] for n in ("gamma", "beta", "avg_mean", "avg_var")]
            self.convs[conv] = _FoldedConv(self.rt, W, stats, k, conv_bias=params.get(prefix + conv + "/b"), half=self.conv_dtype == "bf16")
            if self.conv_dtype == "f32":                       # the unfolded parameters, for the train-mode pass
                self.tp[conv + "/W"] = m.from_numpy(pack_w(W, k))
                for n, v in zip(("gamma", "beta", "avg_mean", "avg_var"), stats):
                    self.tp[bn + "/" + n] = m.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
                if (prefix + conv + "/b") in params:
                    self.tp[conv + "/b"] = m.from_numpy(np.ascontiguousarray(params[prefix + conv + "/b"], dtype=np.float32))
        self._wd, self._wd_stale = {}, True
        self._w16, self._w16_stale = {}, True
        self._fold_stale = False

    # ---- the trainable form ---------------------------------------------------------------------------------------------------------------
    def param_specs(self):
        """[(key below the prefix, Chainer-layout shape, kind)] of everything an optimizer moves, in execution order; kind 'W' (stored packed,
        see pack_w / unpack_w), 'v' (a vector stored as it is)."""
        out = []
        for conv, bn, ci, co, k in conv_specs(self.blocks, self.base_width):
            out.append((conv + "/W", (co, ci, k, k), "W"))
            if (conv + "/b") in self.tp:
                out.append((conv + "/b", (co,), "v"))
            out += [(bn + "/gamma", (co,), "v"), (bn + "/beta", (co,), "v")]
        return out

    def persistent_keys(self):
        """the running statistics: saved with a snapshot, moved by the forward pass, not by the optimizer"""
        return [bn + "/" + n for _, bn, _, _, _ in conv_specs(self.blocks, self.base_width) for n in ("avg_mean", "avg_var")]

    def mark_params_updated(self):
        """the parameters (or running statistics) changed on the device: the input-gradient packings are rebuilt at the next backward pass and the
        folded inference weights at the next test-mode call"""
        self._wd_stale = True
        self._w16_stale = True
        self._fold_stale = True

    def params_host(self, prefix="trunk/"):
        """the current parameters and running statistics in Chainer's layout, keyed like load_params' input"""
        m = self.rt.mem
        out = {}
        for conv, bn, ci, co, k in conv_specs(self.blocks, self.base_width):
            out[prefix + conv + "/W"] = unpack_w(m.to_numpy(self.tp[conv + "/W"]), co, ci, k)
            if (conv + "/b") in self.tp:
                out[prefix + conv + "/b"] = m.to_numpy(self.tp[conv + "/b"])
            for n in ("gamma", "beta", "avg_mean", "avg_var"):
                out[prefix + bn + "/" + n] = m.to_numpy(self.tp[bn + "/" + n])
        return out

    def _refold(self):
        p = self.params_host("")
        for conv, bn, ci, co, k in conv_specs(self.blocks, self.base_width):
            self.convs[conv] = _FoldedConv(self.rt, p[conv + "/W"], [p[bn + "/" + n] for n in ("gamma", "beta", "avg_mean", "avg_var")], k,
                                           conv_bias=p.get(conv + "/b"), half=False)
        self._fold_stale = False

    def _zeros(self, n):
        if n not in self._zero_bias:
            self._zero_bias[n] = self.rt.mem.zeros((n,), "f32")
        return self._zero_bias[n]

    def _conv_bn(self, conv, bn, x, ksize, relu, residual=None):
        """one convolution (unfolded, act 0) + BatchNormalization on the map's own statistics [+ residual] [+ ReLU]; taped"""
        rt, tp = self.rt, self.tp
        W = tp[conv + "/W"]
        co = int(W.shape[1])
        if self.train_dtype == "bf16":
            z = self._conv16(conv, x, W, ksize)
        else:
            z = rt.conv_ex(x, W, tp.get(conv + "/b", self._zeros(co)), ksize, act=0)
        y, mean, rstd = rt.bn_train_fwd(z, tp[bn + "/gamma"], tp[bn + "/beta"], residual=residual, relu=relu, eps=BN_EPS, decay=BN_DECAY,
                                        running_mean=tp[bn + "/avg_mean"], running_var=tp[bn + "/avg_var"])
        self.tape[conv] = dict(x=x, z=z, y=y, mean=mean, rstd=rstd, relu=relu, bn=bn, ksize=ksize)
        return y

    def _w16_of(self, conv):
        """(forward, input-gradient) 16-bit weights of a 3x3 layer from the current master weights; after an update ALL 3x3 layers are re-packed at the
        first request, sixteen per launch (frcnn_bf16_pack_many), into buffers that are kept -- _dgrad_w's scheme"""
        if self._w16_stale:
            rt, todo = self.rt.with_half("bf16"), []
            pad = rt.bf16_pad
            for c, _, ci, co, k in conv_specs(self.blocks, self.base_width):
                if k != 3:
                    continue
                if c not in self._w16:
                    self._w16[c] = (rt.mem.empty((pad(ci) // 16, 9, pad(co), 16), "i16"), rt.mem.empty((pad(co) // 16, 9, pad(ci), 16), "i16"))
                todo.append((self.tp[c + "/W"], self._w16[c][0], self._w16[c][1], ci, co))
            for i in range(0, len(todo), 16):
                rt.bf16_pack_many(todo[i:i + 16])
            self._w16_stale = False
        return self._w16[conv]

    def _conv16(self, conv, x, W, ksize):
        """the pre-BN map of one layer on bf16 products: z = conv(RNE(x), RNE(W)) (+ conv1/b), fp32 accumulation"""
        rt = self.rt.with_half("bf16")
        if ksize == 1:
            return rt.conv1x1_bf16_train(x, W, self.tp.get(conv + "/b"))
        ci, co = int(x.shape[1]), int(W.shape[1])
        return rt.conv3x3_bf16_train(rt.bf16_from_nchw(x), self._w16_of(conv)[0], self._zeros(co), ci, co, relu=False, want_bf16=False)[1]

    def _call_train(self, h, timer=None, collect=None):
        rt = self.rt
        if not self.tp:
            raise ValueError("ResNet: load_params first")
        self.tape = {}
        h = self._conv_bn("conv1", "bn1", rt.im2col7x7s2(h, int(self.tp["conv1/W"].shape[0])), 1, True)
        h = rt.maxpool3x3s2(h)
        for (stage, _, _, _, stride), n in zip(self.stages, self.blocks):
            for b in block_names(n):
                p = "%s/%s/" % (stage, b)
                xin = rt.subsample2(h) if (b == "a" and stride == 2) else h
                self.tape[p] = dict(hw=(int(h.shape[2]), int(h.shape[3])), strided=xin is not h)
                shortcut = self._conv_bn(p + "conv4", p + "bn4", xin, 1, False) if b == "a" else h
                t = self._conv_bn(p + "conv1", p + "bn1", xin, 1, True)
                t = self._conv_bn(p + "conv2", p + "bn2", t, 3, True)
                h = self._conv_bn(p + "conv3", p + "bn3", t, 1, True, residual=shortcut)
            if timer:
                timer.mark(stage)
        if collect is not None:                                # the tape's maps by link path: (pre-BN z, output y)
            for name, t in self.tape.items():
                if "z" in t:
                    collect[name] = (t["z"], t["y"])
        self._fold_stale = True                                # the running statistics moved
        return h

    def _dgrad_w(self, conv, ksize):
        """the input-gradient packing of a layer's current weights; after an update ALL layers are re-packed at the first request, sixteen per
        launch (frcnn_pack_conv_dgrad_w_many), into buffers that are kept"""
        if self._wd_stale:
            rt, todo = self.rt, []
            for c, _, ci, co, k in conv_specs(self.blocks, self.base_width)[1:]:          # (the stem needs no input gradient)
                if c not in self._wd:
                    self._wd[c] = rt.mem.empty((co * k * k, ci), "f32")
                todo.append((self.tp[c + "/W"], self._wd[c], k))
            for i in range(0, len(todo), 16):
                rt.pack_conv_dgrad_w_many(todo[i:i + 16])
            self._wd_stale = False
        return self._wd[conv]

    def _conv_bn_bwd(self, conv, dy, grads, want_dres=False, want_dx=True, ready=None, collect=None):
        """backward of _conv_bn: fills grads[conv/W], grads[bn/gamma], grads[bn/beta] -> (dL/dx or None, dres or None)"""
        rt, t = self.rt, self.tape[conv]
        bn, ks = t["bn"], t["ksize"]
        dz, dg, db, dres = rt.bn_train_bwd(dy, t["y"] if t["relu"] else None, t["z"], self.tp[bn + "/gamma"], t["mean"], t["rstd"], want_dres=want_dres,
                                           dgamma=grads.get(bn + "/gamma"), dbeta=grads.get(bn + "/beta"))
        grads[bn + "/gamma"], grads[bn + "/beta"] = dg, db
        bf16 = self.train_dtype == "bf16"
        if bf16:
            rt16 = rt.with_half("bf16")
            wgrad = rt16.conv1x1_wgrad_bf16 if ks == 1 else rt16.conv_wgrad_bf16
            grads[conv + "/W"] = wgrad(t["x"], dz, out=grads.get(conv + "/W"))
        else:
            grads[conv + "/W"] = rt.conv_wgrad(t["x"], dz, ks, out=grads.get(conv + "/W"))
        if (conv + "/b") in self.tp:
            grads[conv + "/b"] = rt.bias_grad(dz, out=grads.get(conv + "/b"))
        if ready is not None:
            ready(conv)                                        # a data-parallel trainer: this layer's gradients are enqueued
        dx = None
        if want_dx:
            ci = int(t["x"].shape[1])
            if bf16 and ks == 1:
                dx = rt16.conv1x1_dgrad_bf16(dz, self.tp[conv + "/W"])
            elif bf16:
                dx = rt16.conv3x3_bf16_train(rt16.bf16_from_nchw(dz), self._w16_of(conv)[1], self._zeros(ci), int(dz.shape[1]), ci, relu=False,
                                             want_bf16=False)[1]
            else:
                dx = rt.conv_ex(dz, self._dgrad_w(conv, ks), self._zeros(ci), ks, act=0)
        if collect is not None:
            collect[conv] = (dy, dz, dx)
        return dx, dres

    def backward(self, g, grads=None, ready=None, collect=None):
        """g = dL/d res5 of the last train-mode call -> grads: {key below the prefix: device array}, the gradient of every W (in the packed
        layout of tp), gamma, beta and conv1/b.  Arrays already present in `grads` are written in place (a trainer's arena views); `ready(conv)`
        is called once a layer's gradients are enqueued, in reverse execution order (conv3, conv2, conv1, conv4 within a block `a`).  `collect`
        (optional dict, tests) receives per convolution (dy into its BN, dz = the pre-BN map's gradient, dx or None for the stem) and per block
        `res3/a/` (the shortcut's gradient, dL/d(block input))."""
        rt = self.rt
        if self.tape is None:
            raise ValueError("ResNet.backward: no train-mode forward pass to differentiate")
        grads = {} if grads is None else grads
        g = rt.asarray(unwrap(g), "f32")
        for (stage, _, _, _, stride), n in reversed(list(zip(self.stages, self.blocks))):
            for b in reversed(block_names(n)):
                p = "%s/%s/" % (stage, b)
                # g = dL/d(block output); its ReLU mask is applied by bn3's backward, which also hands back dres = the shortcut's gradient
                d, dres = self._conv_bn_bwd(p + "conv3", g, grads, want_dres=True, ready=ready, collect=collect)
                d, _ = self._conv_bn_bwd(p + "conv2", d, grads, ready=ready, collect=collect)
                d, _ = self._conv_bn_bwd(p + "conv1", d, grads, ready=ready, collect=collect)
                if b == "a":
                    d4, _ = self._conv_bn_bwd(p + "conv4", dres, grads, ready=ready, collect=collect)
                    other = d4
                    d = rt.add(d, d4, out=None if collect is not None else d)      # (collected: the layers' own dx stay as they were written)
                    if self.tape[p]["strided"]:
                        d = rt.subsample2_bwd(d, *self.tape[p]["hw"])
                else:
                    other = dres
                    d = rt.add(d, dres, out=None if collect is not None else d)    # the identity shortcut
                if collect is not None:
                    collect[p] = (other, d)                    # the shortcut's gradient and dL/d(block input)
                g = d
        g = rt.maxpool3x3s2_bwd(self.tape["conv1"]["y"], g)
        self._conv_bn_bwd("conv1", g, grads, want_dx=False, ready=ready, collect=collect)     # the image needs no gradient
        return grads

    def _conv(self, name, x, act=1, residual=None):
        c = self.convs[name]
        return self.rt.conv_ex(x, c.Wp, c.b, 1 if c.ksize == 7 else c.ksize, act=act, mask=residual)

    def __call__(self, x, timer=None, collect=None):
        rt = self.rt
        h = rt.asarray(unwrap(x), "f32")
        assert h.ndim == 4 and int(h.shape[0]) == 1, "batch size 1 (models/faster_rcnn.py:77)"
        if self.train:
            if self.conv_dtype != "f32":
                raise ValueError("ResNet: train-mode BatchNormalization runs on the fp32 trunk only (conv_dtype='f32'); the 16-bit trunks are inference-only "
                                 "(bf16 training: conv_dtype='f32' with train_dtype='bf16')")
            return self._call_train(h, timer, collect)
        if self.conv_dtype == "bf16":
            return self._call_bf16(h, timer, collect)
        if collect is not None:
            raise ValueError("ResNet: per-layer collection is a feature of the 16-bit trunk (conv_dtype='bf16') and of the train-mode pass")
        if self._fold_stale:
            self._refold()
        h = self._conv("conv1", rt.im2col7x7s2(h, int(self.convs["conv1"].Wp.shape[0])))      # conv1 + bn1 + relu
        h = rt.maxpool3x3s2(h)
        for (stage, _, _, _, stride), n in zip(self.stages, self.blocks):
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
        keep("conv1", h, self.base_width)
        h = rt.maxpool3x3s2_bf16(h)
        keep("pool1", h, self.base_width)
        cout = self.base_width
        for (stage, _, mid, cout, stride), n in zip(self.stages, self.blocks):
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
