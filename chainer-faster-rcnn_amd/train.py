"""The RPN training step of train_rpn.py (train_rpn.py:140-182 + chainer's StandardUpdater / ParallelUpdater and
MomentumSGD(lr=0.001) + WeightDecay(0.0005)) as one object over the HIP kernels.

    trainer = RPNTrainer(model)                       # model: models.FasterRCNN with parameters loaded
    out = trainer.step(x, img_info, gt_boxes)         # forward, AnchorTargetLayer, losses, backward, all-reduce, update

What runs where:
  forward         trunk + rpn_conv_3x3 + heads on the MFMA conv kernel (csrc/conv.hip), activations kept in HBM
  targets         AnchorTargetLayer (device: csrc/train.hip; host: the NumPy-RNG subsample, as in the reference)
  losses          frcnn_rpn_loss: softmax-CE + Huber and their gradients w.r.t. the two head outputs
  backward        per conv: weight gradient (MFMA, pixels as the reduction axis), bias gradient, input gradient = the forward
                  kernel on 180-degree-rotated weights with the ReLU mask fused into the epilogue; max-pool: gather
  data parallel   all_reduce(SUM) of the flat fp32 gradient buffer (RCCL over xGMI; gloo on CPU), launched per bucket (three
                  contiguous tail ranges) while the backward pass is still running -- see RPNTrainer._plan_buckets; i.e. the
                  gradients are summed over replicas exactly as ParallelUpdater's addgrads does, then every rank applies
                  the identical update (replaces gather-to-main + copyparams broadcast)
  update          one fused MomentumSGD + WeightDecay launch over the flat parameter / gradient / velocity buffers

Trained parameters are the trunk and the RPN (in rpn_train mode FasterRCNN.__call__ returns before the head:
models/faster_rcnn.py:115-116).  Convolution weights live in the kernels' packed layout (Cin*9, Cout) while training;
`sync_params()` writes them back to Chainer's (Cout, Cin, 3, 3) arrays for snapshots.
ProposalLayer runs inside the training step exactly where the reference runs it (train-mode top-N 12000 / 2000,
region_proposal_network.py:123-126) and its result is discarded, as there; `run_proposal_layer=False` skips it (same gradients).
"""

import contextlib
import functools

import numpy as np

from . import tuning as _tuning
from .chainer_compat import unwrap
from .models.anchor_target_layer import AnchorTargetLayer


class _PoolArg(object):
    """What the backward pass of a pool FUSED into its convolution needs: the arg-max byte of every window and the pre-pool size."""

    def __init__(self, idx, H, W):
        self.idx, self.H, self.W = idx, int(H), int(W)


def trunk_forward(model, x, fuse_pools=True):
    """Trunk forward keeping every layer's input (the backward pass needs them) -> (feat, inputs).  A convolution that is followed by a
    pool runs conv + ReLU + pool as ONE launch (csrc/conv.hip, act 5) and keeps a byte per window instead of the pre-pool map: the
    pool's entry in `inputs` is then a _PoolArg (fuse_pools=False / FRCNN_TRAIN_FUSE_POOL=0: two launches, the pre-pool map kept --
    the tests that impose the device's decisions on a float64 pass read it)."""
    rt = model.rt
    layers = model.trunk.layers
    fuse = fuse_pools and _tuning.get("FRCNN_TRAIN_FUSE_POOL") != "0"
    inputs, h, skip = [], x, None
    for idx, l in enumerate(layers):
        if l == "pool":
            if skip is not None:                                      # applied inside the previous convolution
                inputs.append(skip)
                skip = None
                continue
            inputs.append(h)
            h = rt.maxpool2x2(h)
            continue
        inputs.append(h)
        link = model.trunk.links[l[0]]
        if fuse and idx + 1 < len(layers) and layers[idx + 1] == "pool" and int(link.cin) > 3 and int(link.cout) % 64 == 0:
            H, W = int(h.shape[2]), int(h.shape[3])
            h, arg = rt.conv_relu_pool_train(h, link.Wp, link.b)
            skip = _PoolArg(arg, H, W)
        else:
            h = link(h, relu=True)
    return h, inputs


def _grad_stream(rt, *arrays):
    if _tuning.get("FRCNN_TRAIN_STREAMS") == "1":
        return contextlib.nullcontext()
    return rt.mem.aux_stream("grad", *arrays)


def trunk_backward(trainer, layer_inputs, g):
    """Backward through [(layer, input)] in reverse, starting from g = dL/d(output of the last layer) ALREADY masked by that
    layer's ReLU.  Writes weight / bias gradients into trainer.grad and re-packs the input-gradient weights."""
    rt = trainer.rt
    first = trainer.convs[0][0]
    links = dict(trainer.convs)
    unpool = _tuning.get("FRCNN_TRAIN_FUSE_POOL") != "0"
    skip_pool = False
    for pos in range(len(layer_inputs) - 1, -1, -1):
        l, xin = layer_inputs[pos]
        if l == "pool":
            if skip_pool:                                             # done in the epilogue of the input-gradient convolution above
                skip_pool = False
                continue
            if isinstance(xin, _PoolArg):                             # the pool ran inside its convolution: route by the kept bytes
                g = rt.maxpool2x2_bwd_idx(xin.idx, g, xin.H, xin.W)
                continue
            trainer._tap_pool(xin)
            g = rt.maxpool2x2_bwd(xin, g)
            continue
        name = l[0]
        trainer._tap(name, xin, g)
        trainer._param_grads(name, xin, g, rt.conv_wgrad)
        if name != first:                                         # the image needs no gradient
            if not trainer._dgrad_packed:                             # (the trainers re-pack every layer in one launch per step)
                rt.pack_conv_dgrad_w(links[name].Wp, 3, out=trainer.wd[name])
            below = layer_inputs[pos - 1] if pos > 0 else None
            if unpool and below is not None and below[0] == "pool" and isinstance(below[1], _PoolArg):
                # the layer below ran conv + ReLU + pool as one launch: its ReLU mask (pooled > 0) and the pool's routing both sit in
                # its arg-max bytes, and this convolution writes dL/d(pre-pool map) directly (csrc/conv.hip, act 6)
                pa = below[1]
                g = rt.conv_dgrad_unpool(g, trainer.wd[name], trainer.zero_bias, pa.idx, pa.H, pa.W)
                skip_pool = True
            else:
                g = rt.conv_ex(g, trainer.wd[name], trainer.zero_bias, 3, act=2, mask=xin)
    rt.mem.join_aux_stream("grad")
    return g


class _OperandMath(object):
    """One arithmetic of the operand-form trunk walkers below (trainer.arith; None for the fp32 MFMA step, which has walkers of its own).  In these
    arithmetics a 3x3 convolution reads an OPERAND tensor -- the 3-way split or the 16-bit image of the fp32 NCHW map -- and weights re-packed into
    the same form once per step.  A subclass holds exactly what differs: the runtime it runs on, the operand conversion, the convolution and its
    `want_*` keyword, the first-layer form and the predicate that selects it, the weight-gradient entry, the re-pack entry and the buffer shape.
    links: [(name, link)] whose forward weights are re-packed (w_fwd); dgrad: those whose input-gradient weights are (w_dgrad).  The trainer
    passes the convolutions it runs forward / takes an input gradient of; _SplitMath narrows both to the layers it has split weights for."""

    def __init__(self, rt, links, dgrad):
        self.rt, self.links = rt, links
        self.w_fwd = {n: rt.mem.empty(self.w_shape(l.cin, l.cout), "i16") for n, l in links}
        self.w_dgrad = {n: rt.mem.empty(self.w_shape(l.cout, l.cin), "i16") for n, l in dgrad}

    def repack(self):
        """Operand-form weights of every forward / input-gradient convolution from the current (packed fp32) weights: one launch."""
        if self.links:
            self.pack_many([(l.Wp, self.w_fwd[n], self.w_dgrad.get(n), l.cin, l.cout) for n, l in self.links])


class _SplitMath(_OperandMath):
    """conv_math="split": six bf16 MFMA products of 3-way split fp32 operands (csrc/conv_f32s.hip; weight gradients: csrc/train.hip
    conv_wgrad_f32s_kernel, fp32 NCHW in, the split happens in the kernel).  The 3-channel layers stay outside: they have no split weights, run
    the fp32 link (or, for conv1_1 in front of a convolution, the first-layer kernel) and get no input gradient."""

    def __init__(self, rt, links, dgrad):
        big = [(n, l) for n, l in links if int(l.cin) > 3]
        _OperandMath.__init__(self, rt, big, big)                     # both forms for every cin > 3 layer, not `dgrad`: one launch packs them in pairs
        self.operand, self.wgrad, self.pack_many = rt.f32s_from_nchw, rt.conv_wgrad_f32s, rt.f32s_pack_many

    def w_shape(self, ci, co):
        pad = self.rt.bf16_pad
        return (3, pad(ci) // 16, 9, pad(co), 16)

    def conv(self, x, w, bias, cin, cout, relu, want, **mask):
        return self.rt.conv3x3_f32s_train(x, w, bias, cin, cout, relu=relu, want_split=want, **mask)

    def first_layer(self, link, idx, layers):
        return int(link.cin) <= 3 and idx == 0 and int(link.cout) <= 64 and idx + 1 < len(layers) and layers[idx + 1] != "pool"

    def conv1(self, x, link):
        return self.rt.conv1_f32s_train(x, link.Wp, link.b, link.cout, relu=True)


class _HalfMath(_OperandMath):
    """conv_math / precision "bf16" or "f16": every product on RNE-rounded 16-bit operands with fp32 accumulation (csrc/conv_f32s.hip's one-part
    form, csrc/train.hip conv_wgrad_f32s_kernel<1>).  rt is the trainer's runtime seen through its operand format (rt.with_half(half)): the fp16
    twins of every 16-bit entry when half == "f16".  Every layer is re-packed; the first one has no input-gradient weights."""

    def __init__(self, rt, links, dgrad):
        _OperandMath.__init__(self, rt, links, dgrad)
        self.operand, self.wgrad, self.pack_many = rt.bf16_from_nchw, rt.conv_wgrad_bf16, rt.bf16_pack_many

    def w_shape(self, ci, co):
        pad = self.rt.bf16_pad
        return (pad(ci) // 16, 9, pad(co), 16)

    def conv(self, x, w, bias, cin, cout, relu, want, **mask):
        return self.rt.conv3x3_bf16_train(x, w, bias, cin, cout, relu=relu, want_bf16=want, **mask)

    def first_layer(self, link, idx, layers):
        return int(link.cin) <= 3 and int(link.cout) <= 64

    def conv1(self, x, link):                                         # fp32 image and weights rounded in registers
        return self.rt.conv1_bf16_train(x, link.Wp, link.b, link.cout, relu=True)


def trunk_forward_operand(trainer, x):
    """trunk_forward in an operand-form arithmetic (trainer.arith).  Every convolution leaves its result as fp32 NCHW (what the weight-gradient
    kernel, pooling and the ReLU masks read) and, when a convolution follows, as the operand tensor that one reads.  Pools run on fp32 and
    leave no operand.  A layer the arithmetic has no weights for runs its fp32 link.  -> (feat, inputs, feat as operand)."""
    arith = trainer.arith
    rt, trunk = arith.rt, trainer.model.trunk
    layers = trunk.layers
    inputs, h, hop = [], x, None
    for idx, l in enumerate(layers):
        inputs.append(h)
        if l == "pool":
            h, hop = rt.maxpool2x2(h), None
            continue
        name, link = l[0], trunk.links[l[0]]
        if arith.first_layer(link, idx, layers):                      # conv1_1: the first-layer kernel, fp32 NCHW image in
            hop, h = arith.conv1(h, link)
        elif name not in arith.w_fwd:
            h, hop = link(h, relu=True), None
        else:
            if hop is None:
                hop = arith.operand(h)
            conv_next = idx + 1 == len(layers) or layers[idx + 1] != "pool"        # the last map feeds rpn_conv_3x3
            hop, h = arith.conv(hop, arith.w_fwd[name], link.b, link.cin, link.cout, relu=True, want=conv_next)
    if hop is None:
        hop = arith.operand(h)                                        # (trunks that end in a pool or in the first layer)
    return h, inputs, hop


def trunk_backward_operand(trainer, layer_inputs, g):
    """trunk_backward in an operand-form arithmetic: the input-gradient convolutions on the operand form of the upstream gradient and of the
    rotated weights with the ReLU mask fused, weight gradients by the arithmetic's own entry (fp32 NCHW in), bias gradients and pools in fp32.
    A layer has an input gradient when it is not the trunk's first and the arithmetic keeps input-gradient weights for it."""
    arith = trainer.arith
    rt = arith.rt
    first = trainer.convs[0][0]
    links = dict(trainer.convs)
    names = [l if l == "pool" else l[0] for l, _ in layer_inputs]
    dgrad = set(arith.w_dgrad) - {first}                              # the layers with an input gradient
    gop = None
    for pos in range(len(layer_inputs) - 1, -1, -1):
        l, xin = layer_inputs[pos]
        if l == "pool":
            trainer._tap_pool(xin)
            g, gop = rt.maxpool2x2_bwd(xin, g), None
            continue
        name = l[0]
        trainer._tap(name, xin, g)
        trainer._param_grads(name, xin, g, arith.wgrad)                # next to the input-gradient convolution below (see trunk_backward)
        if name not in dgrad:
            continue                                                  # the image needs no gradient
        if gop is None:
            gop = arith.operand(g)
        cin, cout = int(links[name].cin), int(links[name].cout)
        below_conv = pos > 0 and names[pos - 1] in dgrad               # who consumes dL/d(input): a convolution with an input gradient of its own?
        gop, g = arith.conv(gop, arith.w_dgrad[name], trainer.zero_bias, cout, cin, relu=False, want=below_conv, mask=xin)
    rt.mem.join_aux_stream("grad")
    return g


def _is_resnet(model):
    from .models.resnet import ResNet
    return isinstance(getattr(model, "trunk", None), ResNet)


class _ResNetTrunk(object):
    """What a trainer needs from a ResNet trunk (models/resnet.py), so that one trainer drives both trunk families: the arena segments of its
    parameters, their adoption into the arena, forward-with-tape and backward, and the layout conversions of a flat buffer.  Segment keys are
    the link paths below `trunk/` (`conv1/W`, `bn1/gamma`, `res3/a/conv4/W`, ...); a W segment holds the convolution kernels' packed layout.
    The buffer is laid out in EXECUTION order -- a block's projection shortcut conv4 before its conv1 -- so the backward pass fills it from
    the end and the all-reduce's tail buckets close as they do for VGG."""

    def __init__(self, trunk, who="RPNTrainer"):
        from .models.resnet import conv_specs
        self.trunk = trunk
        if trunk.conv_dtype != "f32":
            raise ValueError("%s: ResNet training runs on the fp32 trunk (conv_dtype='f32'); mixed-precision ResNet training is not built" % who)
        if not trunk.tp:
            raise ValueError("%s: load the ResNet model's parameters first" % who)
        specs = conv_specs(trunk.blocks, trunk.base_width)
        order, i = [], 0
        while i < len(specs):                                        # (conv1, conv2, conv3, conv4) of a block `a` -> (conv4, conv1, conv2, conv3)
            if specs[i][0].endswith("/a/conv1"):
                order += [specs[i + 3]] + specs[i:i + 3]
                i += 4
            else:
                order.append(specs[i])
                i += 1
        self.specs = order
        self.names = [c[0] for c in order]

    def segments(self):
        """[(key, shape)] in buffer order"""
        tp, out = self.trunk.tp, []
        for conv, bn, ci, co, k in self.specs:
            out.append((conv + "/W", tuple(int(v) for v in tp[conv + "/W"].shape)))
            if (conv + "/b") in tp:
                out.append((conv + "/b", (co,)))
            out += [(bn + "/gamma", (co,)), (bn + "/beta", (co,))]
        return out

    def adopt(self, arena):
        tp = self.trunk.tp
        for key, _ in self.segments():
            tp[key] = arena._adopt(key, tp[key])

    def feat_hw(self, H, W):
        f = lambda v: (v - 1) // 2 + 1                               # noqa: E731
        H, W = (f(H) - 2) // 2 + 1, (f(W) - 2) // 2 + 1              # the stem's stride, pool1 (cover_all)
        for _, _, _, _, stride in self.trunk.stages:
            if stride == 2:
                H, W = f(H), f(W)
        return H, W

    def to_chainer(self, seg, out):
        from .models.resnet import unpack_w
        for conv, bn, ci, co, k in self.specs:
            out["trunk/" + conv + "/W"] = unpack_w(seg(conv + "/W"), co, ci, k)
            if (conv + "/b") in self.trunk.tp:
                out["trunk/" + conv + "/b"] = seg(conv + "/b").copy()
            for n in ("gamma", "beta"):
                out["trunk/%s/%s" % (bn, n)] = seg(bn + "/" + n).copy()

    def from_chainer(self, arrays, put):
        from .models.resnet import pack_w
        for conv, bn, ci, co, k in self.specs:
            if "trunk/" + conv + "/W" in arrays:
                put(conv + "/W", pack_w(arrays["trunk/" + conv + "/W"], k))
            for key in (conv + "/b", bn + "/gamma", bn + "/beta"):
                if "trunk/" + key in arrays and key in self.trunk.tp:
                    put(key, arrays["trunk/" + key])


class _Seg(object):
    def __init__(self, name, shape, offset):
        self.name, self.shape, self.offset = name, tuple(shape), offset
        self.size = int(np.prod(shape))


# Chainer's defaults (optimizers.Adam / AdaGrad / RMSprop); MomentumSGD's lr and momentum are the trainers' own arguments
OPT_DEFAULTS = {"MomentumSGD": {}, "Adam": dict(alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), "AdaGrad": dict(lr=1e-3, eps=1e-8),
                "RMSprop": dict(lr=1e-2, alpha=0.99, eps=1e-8)}
# the per-parameter state of each rule under Chainer's names (serializers.py: updater/optimizer:main/<link path>/<name>)
OPT_STATE_KEYS = {"MomentumSGD": ("v",), "Adam": ("m", "v"), "AdaGrad": ("h",), "RMSprop": ("ms",)}


class AdamState(object):
    """Adam's step count on the device (csrc/optimizer.hip): t = the number of APPLIED steps, the running double products beta1^t and
    beta2^t, and lr_t.  The update launches read and write them; nothing here synchronises except state()."""

    WORDS = 8

    def __init__(self, rt):
        self.rt = rt
        self.buf = rt.mem.zeros((self.WORDS,), "i32")
        rt.opt_state_init(self.buf)

    def state(self):
        """Host copy of the device state (SYNCHRONISES: snapshots, logs and tests only)."""
        w = np.ascontiguousarray(self.rt.mem.to_numpy(self.buf)).astype(np.int32)
        d = w.view(np.float64)
        return dict(t=int(w[0]), lr_t=float(w.view(np.float32)[1]), beta1_pow_t=float(d[1]), beta2_pow_t=float(d[2]))

    def load(self, t, beta1_pow_t, beta2_pow_t):
        """Resume: the step count and the two running products from a snapshot."""
        self.rt.opt_state_init(self.buf, t, beta1_pow_t, beta2_pow_t)

    @staticmethod
    def running_power(beta, t):
        """beta^t as the device forms it: t multiplications in double, starting from 1.0."""
        p = 1.0
        for _ in range(int(t)):
            p = p * float(beta)
        return p


def _is_pow2(v):
    try:
        m, _ = np.frexp(float(v))
    except (TypeError, ValueError):
        return False
    return bool(np.isfinite(v)) and float(v) > 0 and m == 0.5


class LossScaler(object):
    """The loss scale of the fp16 step, resident on the device (csrc/loss_scale.hip): scale, overflow flag, skip decision and growth /
    back-off are words of `self.buf` that the kernels read and write; nothing here synchronises except state().
    loss_scale: "dynamic" (init_scale, doubled after growth_interval clean steps, halved by every step whose gradients hold an Inf / NaN,
    clamped to [min_scale, max_scale]) or a power of two (static: an overflowing step is still skipped, the scale never moves).
    Every constant must be a power of two (scaling is then exact): ValueError otherwise."""

    WORDS = 8
    DEFAULTS = dict(init_scale=2.0 ** 16, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24)

    def __init__(self, rt, loss_scale="dynamic", **constants):
        unknown = set(constants) - set(self.DEFAULTS)
        if unknown:
            raise ValueError("LossScaler: unknown constants %s" % sorted(unknown))
        c = dict(self.DEFAULTS, **constants)
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError("loss_scale must be 'dynamic' or a power of two, not %r" % (loss_scale,))
            self.dynamic = True
        else:
            if not _is_pow2(loss_scale):
                raise ValueError("a static loss_scale must be a power of two, not %r" % (loss_scale,))
            self.dynamic = False
            s = float(loss_scale)
            c.update(init_scale=s, growth=1.0, backoff=1.0, min_scale=s, max_scale=s)
        for k in ("init_scale", "growth", "backoff", "min_scale", "max_scale"):
            if not _is_pow2(c[k]):
                raise ValueError("LossScaler: %s must be a power of two, not %r" % (k, c[k]))
        if c["growth"] < 1 or c["backoff"] > 1 or not c["min_scale"] <= c["init_scale"] <= c["max_scale"] or int(c["growth_interval"]) < 1:
            raise ValueError("LossScaler: need growth >= 1, backoff <= 1, min_scale <= init_scale <= max_scale, growth_interval >= 1")
        self.rt, self.c = rt, c
        self.buf = rt.mem.zeros((self.WORDS,), "i32")
        rt.loss_scaler_init(self.buf, c["init_scale"])

    def scale(self, x):
        """x *= S (the gradient of the loss with respect to the heads' outputs)."""
        self.rt.scale_by_loss_scale(x, self.buf)

    def check(self, g):
        self.rt.grad_check_finite(g, self.buf)

    def update(self):
        c = self.c
        self.rt.loss_scaler_update(self.buf, c["growth"], c["backoff"], c["growth_interval"], c["min_scale"], c["max_scale"])

    def _words(self):
        w = np.ascontiguousarray(self.rt.mem.to_numpy(self.buf)).astype(np.int32)
        return w, w.view(np.float32)

    def state(self):
        """Host copy of the device state (SYNCHRONISES: logs and tests only)."""
        w, f = self._words()
        return dict(scale=float(f[0]), good_steps=int(w[2]), found_nonfinite=int(w[3]), skipped_steps=int(w[4]), overflow_steps=int(w[5]),
                    step_scale=float(f[6]))

    def load(self, scale, good_steps=0, skipped_steps=0):
        """Resume: scale and counters from a snapshot."""
        if not _is_pow2(scale):
            raise ValueError("LossScaler.load: scale must be a power of two, not %r" % (scale,))
        w = np.zeros((self.WORDS,), np.int32)
        f = w.view(np.float32)
        f[0], f[1], f[6] = float(scale), 1.0 / float(scale), float(scale)
        w[2], w[4] = int(good_steps), int(skipped_steps)
        self.buf[...] = self.rt.mem.from_numpy(w)


def _packed_to_chainer(wp, link):
    """A 3x3 convolution's weights, the kernels' packed layout (Cin*9, Cout) -> Chainer's (Cout, Cin, 3, 3) (host arrays)."""
    return np.ascontiguousarray(wp.T).reshape(link.cout, link.cin, 3, 3)


def _chainer_to_packed(w, link):
    return np.asarray(w, dtype=np.float32).reshape(link.cout, -1).T


class _Trainer(object):
    """What RPNTrainer and RCNNTrainer share: the parameter arena, the bucketed gradient all-reduce, the buffers of the step's arithmetic, the
    update, and the trunk-convolution half of the layout conversions.  A subclass sets model, rt, comm, layers and convs ([(name, link)] of the
    3x3 convolutions it trains, forward order), lays out its arena (_build_arena), picks its arithmetic (_init_arithmetic) and plans its buckets.

    The arena: a trainer keeps its parameters in ONE flat buffer (self.W) and re-points the links' arrays at windows of it, so a single
    fused launch updates everything.  Two trainers on one model (the reference's rpn -> rcnn -> rpn alternation, train.py; the
    hidden RCNNTrainer of FasterRCNN.__call__) would orphan each other's windows: before every step a trainer therefore checks
    that each link still points INTO its buffer and re-adopts the link's current values if not (velocities are kept).

    Data parallel: the gradient all-reduce as a few contiguous TAIL buckets of the flat buffer, each launched asynchronously
    the moment the layer that completes it has its gradient kernels enqueued (the buffer is laid out in forward order and the
    backward pass fills it from the end), so the exchange runs under the rest of the backward pass.  Same element-wise sums over
    ranks as one all-reduce.  Few large buckets, not many small ones: xGMI is point-to-point, a ring collective is per-link bound,
    and every extra collective adds its latency.
    comm: None (one replica) or a TorchComm-like object: all_reduce_sum, all_reduce_sum_async, wait, and the attribute `active` -- False is
    the one way a communicator says "skip the exchange" (TorchComm: a single rank that was not forced)."""

    keep_dy = None              # tests: a set of layer names -> the step records what _tap() sees into kept_dy (and runs its pools unfused)
    kept_dy = None
    _dgrad_packed = False       # True between the step's one-launch re-pack of the input-gradient weights and the end of its backward pass
    arith = None                # the operand-form arithmetic (_OperandMath); None: fp32 MFMA convolutions

    def _build_arena(self, segments):
        """segments: [(key, shape)] in buffer order -> seg, n_flat, one flat buffer each for parameters (W), gradients (G) and the rule's state
        (moments), the links adopted into W, and grad: a view of G per segment.  Every segment is 256-byte aligned."""
        rt = self.rt
        self.seg, off = {}, 0
        for key, shape in segments:
            self.seg[key] = _Seg(key, shape, off)
            off += (self.seg[key].size + 63) // 64 * 64
        self.n_flat = off
        self.W = rt.mem.zeros((off,), "f32")
        self.G = rt.mem.zeros((off,), "f32")
        self._alloc_optimizer_state()
        self._ensure_adopted()
        self.grad = {k: rt.mem.view(self.G, s.offset, s.shape) for k, s in self.seg.items()}

    def _conv_segments(self):
        return [(name + sfx, arr.shape) for name, link in self.convs for sfx, arr in (("/W", link.Wp), ("/b", link.b))]

    def _adopt(self, key, current):
        seg = self.seg[key]
        v = self.rt.mem.view(self.W, seg.offset, seg.shape)
        if not self.rt.mem.within(current, self.W):
            v[...] = current
        return v

    def _adopt_convs(self):
        for name, link in self.convs:
            link.Wp = self._adopt(name + "/W", link.Wp)
            link.b = self._adopt(name + "/b", link.b)
            link._adopted = True

    def _ensure_adopted(self):
        raise NotImplementedError

    def _init_arithmetic(self, arithmetic, loss_scale, fwd, dgrad):
        """The buffers of the step's arithmetic ("mfma", "split", "bf16" or "f16").  fwd / dgrad: [(name, link)] of the 3x3 convolutions whose
        forward pass / input gradient the trainer runs.  Always: wd, the weights of the fp32 input-gradient convolutions (re-packed from the
        current weights every step).  split / 16-bit: self.arith and its re-packed weights (ws_* / wb_*: only a trainer that uses them has the
        attribute).  f16: the device-side loss scale from `loss_scale` -- None = "dynamic", a power of two, or a dict of LossScaler's arguments."""
        rt = self.rt
        self.wd = {name: rt.mem.empty((int(link.Wp.shape[1]) * 9, int(link.Wp.shape[0]) // 9), "f32") for name, link in dgrad}
        self.half = "f16" if arithmetic == "f16" else "bf16"          # the 16-bit operand format of the mixed-precision step
        if arithmetic == "split":
            self.arith = _SplitMath(rt, fwd, dgrad)
            self.ws_fwd, self.ws_dgrad = self.arith.w_fwd, self.arith.w_dgrad
        elif arithmetic in ("bf16", "f16"):
            # one view for the trainer's life: with_half copies the runtime's attributes as they are NOW, so one re-bound on self.rt later is not seen
            self.arith = _HalfMath(rt.with_half(self.half), fwd, dgrad)
            self.wb_fwd, self.wb_dgrad = self.arith.w_fwd, self.arith.w_dgrad
        self.loss_scaler = None
        if arithmetic == "f16":
            kw = dict(loss_scale) if isinstance(loss_scale, dict) else {"loss_scale": "dynamic" if loss_scale is None else loss_scale}
            self.loss_scaler = LossScaler(rt, **kw)
            self._g_scale_word = 0                                    # which state word holds the scale self.G is multiplied by

    # ------------------------------------------------------------------ backward-pass helpers of every trunk walker and of the trainers' own layers
    def _tap(self, name, xin, g):
        """tests (keep_dy set): the (input, upstream gradient) pair a layer's weight gradient is computed from"""
        if self.keep_dy is not None and name in self.keep_dy:
            self.kept_dy[name] = (xin, g.clone() if hasattr(g, "clone") else g.copy())      # hasattr: a torch tensor or the emulator's NumPy array

    def _tap_pool(self, xin):
        """tests (keep_dy set): the pre-pool maps (near-tie windows = where two fp32 passes may route differently)"""
        if self.keep_dy is not None:
            self.kept_dy.setdefault("pool_inputs", []).append(xin)

    def _param_grads(self, name, xin, g, wgrad, ready=True):
        """A convolution's weight / bias gradient from (input, upstream gradient), on the gradient stream: they need (xin, g) only, so they run
        NEXT TO the input-gradient convolution the caller launches next (FRCNN_TRAIN_STREAMS=1: one stream, A/B hook).  wgrad: the
        arithmetic's weight-gradient entry, (xin, g, out=...) of a 3x3 convolution.
        ready: data parallel -- a bucket that `name` closes starts its all-reduce now."""
        rt = self.rt
        with _grad_stream(rt, xin, g):
            wgrad(xin, g, out=self.grad[name + "/W"])
            rt.bias_grad(g, out=self.grad[name + "/b"])
            if ready:
                self._grads_ready(name)

    # ------------------------------------------------------------------ the update rule (utils/prepare_train.py:146-167 get_optimizer)
    def _init_optimizer(self, who, opt, opt_args, weight_decay):
        """Validate `opt` / `opt_args` and set the rule's hyper-parameters as plain attributes (read at every update(), like self.lr)."""
        if opt not in OPT_DEFAULTS:
            raise ValueError("%s: opt must be one of %s, not %r" % (who, sorted(OPT_DEFAULTS), opt))
        args = dict(opt_args or {})
        unknown = set(args) - set(OPT_DEFAULTS[opt])
        if unknown:
            raise ValueError("%s: opt=%r has no hyper-parameter %s (it takes %s)" % (who, opt, sorted(unknown), sorted(OPT_DEFAULTS[opt])))
        for k, v in dict(OPT_DEFAULTS[opt], **args).items():
            setattr(self, k, v)
        if opt != "MomentumSGD" and not float(self.eps) > 0:
            raise ValueError("%s: eps must be positive (the zero padding of the parameter buffer would compute 0 / 0), not %r" % (who, self.eps))
        self.opt = opt
        # train_rpn.py:167 hooks WeightDecay(0.0005) onto MomentumSGD only; an explicit value is honoured by every rule
        self.weight_decay = (0.0005 if opt == "MomentumSGD" else 0.0) if weight_decay is None else weight_decay

    def _alloc_optimizer_state(self):
        """The rule's state: one or two zero-initialised arenas in self.W's layout (self.moments: Chainer's state name -> buffer) and, for
        Adam, the device-resident step count / bias correction (self.opt_state)."""
        rt = self.rt
        self.moments = {k: rt.mem.zeros((self.n_flat,), "f32") for k in OPT_STATE_KEYS[self.opt]}
        self.V = self.moments["v"] if self.opt == "MomentumSGD" else None      # MomentumSGD's velocities
        self.opt_state = AdamState(rt) if self.opt == "Adam" else None

    def _optimizer_step(self, scaler_state=None):
        """Adam / AdaGrad / RMSprop over the flat buffers (csrc/optimizer.hip); with a loss scaler's state on G / S, or nothing when its flag is set."""
        rt, mo = self.rt, self.moments
        if self.opt == "Adam":
            rt.opt_step("Adam", self.W, self.G, mo["m"], mo["v"], lr=self.alpha, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                        weight_decay=self.weight_decay, opt_state=self.opt_state.buf, scaler_state=scaler_state)
        elif self.opt == "AdaGrad":
            rt.opt_step("AdaGrad", self.W, self.G, mo["h"], lr=self.lr, eps=self.eps, weight_decay=self.weight_decay, scaler_state=scaler_state)
        else:
            rt.opt_step("RMSprop", self.W, self.G, mo["ms"], lr=self.lr, beta1=self.alpha, eps=self.eps, weight_decay=self.weight_decay,
                        scaler_state=scaler_state)

    def update(self):
        self._ensure_adopted()
        if self.loss_scaler is not None:
            # finite check of the (all-reduced) sums -> the update on G / S, or nothing -> back-off / growth: three launches, the host reads nothing
            self.loss_scaler.check(self.G)
            if self.opt == "MomentumSGD":
                self.rt.sgd_momentum_wd_scaled(self.W, self.G, self.V, self.lr, self.momentum, self.weight_decay, self.loss_scaler.buf)
            else:                                                     # (Adam: one more one-lane launch, which counts the step unless it is skipped)
                self._optimizer_step(self.loss_scaler.buf)
            self.loss_scaler.update()
            self._g_scale_word = 6                                    # self.G is still multiplied by the scale this step used
        elif self.opt == "MomentumSGD":
            self.rt.sgd_momentum_wd(self.W, self.G, self.V, self.lr, self.momentum, self.weight_decay)
        else:
            self._optimizer_step()
        self.model.mark_params_updated(self)
        self.iteration += 1

    # ------------------------------------------------------------------ data parallel
    def _comm_active(self):
        return self.comm is not None and self.comm.active

    def _plan_buckets(self, names, n_buckets=3):
        """names: parameter groups in FORWARD (= buffer) order; every group's gradients precede, in time, those of the groups
        before it.  Buckets are (closing group, start, end) in backward order and tile [0, n_flat)."""
        total, end = self.n_flat, self.n_flat
        target = total / float(n_buckets)
        self.buckets = []
        for i in range(len(names) - 1, -1, -1):
            start = self.seg[names[i] + "/W"].offset
            if end - start >= target or i == 0:
                self.buckets.append((names[i], start if i else 0, end))
                end = start
        self._closing = {b[0]: k for k, b in enumerate(self.buckets)}
        self._works = []

    def _grads_ready(self, name):
        k = self._closing.get(name)
        if k is None or not self._comm_active():
            return
        _, start, end = self.buckets[k]
        self._works.append(self.comm.all_reduce_sum_async(self.G[start:end]))

    def _drain(self):
        for w in self._works:
            self.comm.wait(w)
        self._works = []

    def all_reduce(self):
        """Sum the gradient buffer over the replicas (ParallelUpdater: grads are added, not averaged).  The buckets were launched
        during the backward pass (_grads_ready); this waits for them -- the update must see every sum."""
        if not self._comm_active():
            return
        complete = len(self._works) == len(self.buckets)
        self._drain()
        if not complete:                                          # forward_backward was not the producer (e.g. a hand-filled G)
            self.comm.all_reduce_sum(self.G)

    # ------------------------------------------------------------------ layouts: the trunk-convolution half; the subclasses add what else they train
    def sync_params(self):
        """Packed training weights -> Chainer-layout arrays on the links (for snapshots / inference objects)."""
        for name, link in self.convs:
            link.W = self.rt.transpose(link.Wp).reshape(link.cout, link.cin, 3, 3)

    def _segment_reader(self, flat):
        """seg(key): the host copy of one segment of a flat buffer in this trainer's layout, in the segment's shape"""
        host = self.rt.mem.to_numpy(flat)

        def seg(key):
            sg = self.seg[key]
            return host[sg.offset:sg.offset + sg.size].reshape(sg.shape)
        return seg

    @contextlib.contextmanager
    def _segment_writer(self, flat):
        """put(key, value) into a host copy of `flat`, which goes back to the device on exit"""
        host = self.rt.mem.to_numpy(flat).copy()

        def put(key, val):
            sg = self.seg[key]
            host[sg.offset:sg.offset + sg.size] = np.asarray(val, dtype=np.float32).reshape(-1)
        yield put
        flat[...] = self.rt.mem.from_numpy(host)

    @staticmethod
    def _conv_path(name):
        return ("RPN/" if name == "rpn_conv_3x3" else "trunk/") + name

    def _convs_to_chainer(self, seg, out):
        for name, link in self.convs:
            out[self._conv_path(name) + "/W"] = _packed_to_chainer(seg(name + "/W"), link)
            out[self._conv_path(name) + "/b"] = seg(name + "/b").copy()

    def _convs_from_chainer(self, arrays, put):
        for name, link in self.convs:
            path = self._conv_path(name)
            if path + "/W" in arrays:
                put(name + "/W", _chainer_to_packed(arrays[path + "/W"], link))
            if path + "/b" in arrays:
                put(name + "/b", arrays[path + "/b"])

    def grads_chainer_layout(self):
        """{link path: gradient in Chainer's layout} (host arrays) -- for tests and inspection.  An fp16 trainer returns UNSCALED gradients:
        the raw buffer self.G holds S times the gradient (S = the loss scale of the step that filled it); the division is exact."""
        out = self.flat_to_chainer_layout(self.G)
        if self.loss_scaler is not None:
            s = np.float32(self.loss_scaler._words()[1][self._g_scale_word])
            out = {k: v / s for k, v in out.items()}
        return out


class RPNTrainer(_Trainer):
    def __init__(self, model, lr=0.001, momentum=0.9, weight_decay=None, comm=None, run_proposal_layer=True, conv_math="mfma", loss_scale=None,
                 opt="MomentumSGD", opt_args=None):
        """conv_math: "mfma" = forward and input-gradient convolutions on the fp32 MFMA kernel; "split" = the same fp32 convolutions as
        six bf16 MFMA products of 3-way split operands (csrc/conv_f32s.hip), the 3x3 weight gradients likewise (csrc/train.hip
        conv_wgrad_f32s_kernel); "bf16" = mixed precision: every product of the 3x3 convolutions' forward, input gradient and weight
        gradient on bf16 operands (RNE of the fp32 activations, gradients and master weights) with fp32 accumulation -- everything
        else (bias, ReLU, pools, the RPN heads and losses, the update, the fp32 master weights) as in the fp32 step; "f16" = the same
        contract with fp16 operands (three more mantissa bits, |v| <= 65504) plus a loss scale S that lives on the device (LossScaler):
        the gradient of the loss with respect to the heads' outputs is multiplied by S, so self.G holds S times the gradient until
        update(), which skips the step when the all-reduced buffer holds an Inf / NaN and otherwise applies G / S.
        loss_scale (conv_math="f16" only): "dynamic" (the default), a power of two (static), or a dict(loss_scale=..., init_scale=...,
        growth=..., backoff=..., growth_interval=..., min_scale=..., max_scale=...) of LossScaler's constants.
        opt: the update rule under the reference's spellings (utils/prepare_train.py:146-167): "MomentumSGD" (lr, momentum: the arguments
        above), "Adam", "AdaGrad" or "RMSprop", whose hyper-parameters come from opt_args -- dict(alpha, beta1, beta2, eps), dict(lr, eps),
        dict(lr, alpha, eps); Chainer's defaults otherwise -- and become attributes read at every update() (trainer.alpha *= gamma).
        weight_decay: None = 0.0005 for MomentumSGD (the reference hooks WeightDecay onto that rule only) and 0 for the others."""
        if conv_math not in ("mfma", "split", "bf16", "f16"):
            raise ValueError("RPNTrainer: conv_math must be 'mfma', 'split', 'bf16' or 'f16', not %r" % (conv_math,))
        if loss_scale is not None and conv_math != "f16":
            raise ValueError("RPNTrainer: loss_scale belongs to conv_math='f16', not %r" % (conv_math,))
        if _is_resnet(model) and conv_math != "mfma":
            raise ValueError("RPNTrainer: a ResNet model trains with conv_math='mfma' (fp32) only, not %r: split-product and mixed-precision "
                             "ResNet training are not built" % (conv_math,))
        self.resnet = _ResNetTrunk(model.trunk, "RPNTrainer") if _is_resnet(model) else None
        self.model, self.rt = model, model.rt
        self.lr, self.momentum = lr, momentum
        self._init_optimizer("RPNTrainer", opt, opt_args, weight_decay)      # (AdaGrad / RMSprop: self.lr is the rule's own)
        self.comm = comm
        self.conv_math = conv_math
        self.run_proposal_layer = run_proposal_layer
        self.proposals = None
        rt = self.rt
        rpn = model.RPN
        self.atl = AnchorTargetLayer(rpn.proposal_layer._feat_stride, runtime=rt)
        self.atl._anchors = rpn.proposal_layer._anchors
        self.atl._num_anchors = rpn.proposal_layer._num_anchors
        # (a ResNet trunk's parameters are not `links`: self.resnet lays them out, and rpn_conv_3x3 is the only conv link of this list)
        self.layers = model.trunk.layers if self.resnet is None else []
        self.convs = [(l[0], model.trunk.links[l[0]]) for l in self.layers if l != "pool"] + [("rpn_conv_3x3", rpn.rpn_conv_3x3)]
        # ---- one flat buffer each for parameters, gradients, velocities: the ResNet trunk, the 3x3 convolutions, the stacked heads
        wp, bp, self.A = rpn._heads_packed
        self._build_arena((self.resnet.segments() if self.resnet is not None else []) + self._conv_segments()
                          + [("heads/W", wp.shape), ("heads/b", bp.shape)])
        # (VGG's first layer needs no input gradient)
        self._init_arithmetic(conv_math, loss_scale, fwd=self.convs, dgrad=self.convs[1:] if self.resnet is None else self.convs)
        self.wd_heads = rt.mem.empty((int(wp.shape[1]), int(wp.shape[0])), "f32")
        self.zero_bias = rt.mem.zeros((512 if self.resnet is None else max(512, int(rpn.rpn_conv_3x3.cin)),), "f32")
        self._draw = None
        self.iteration = 0
        self._plan_buckets((self.resnet.names if self.resnet is not None else []) + [n for n, _ in self.convs])       # heads follow rpn_conv_3x3 in the buffer and precede it in time

    def _ensure_adopted(self):
        rpn = self.model.RPN
        if self.resnet is not None:
            self.resnet.adopt(self)
        self._adopt_convs()
        wp, bp, A = rpn._heads_packed
        rpn._heads_packed = (self._adopt("heads/W", wp), self._adopt("heads/b", bp), A)
        rpn._heads_adopted = True

    # ------------------------------------------------------------------
    def forward_backward(self, x, img_info, gt_boxes):
        """Fills self.G with this replica's gradients; returns dict(loss, loss_cls, loss_bbox, accuracy) (device scalars)."""
        rt, model, rpn = self.rt, self.model, self.model.RPN
        self._drain()                                              # a previous backward whose sums were never consumed
        self._ensure_adopted()
        x = rt.asarray(unwrap(x), "f32")
        im_h, im_w = rpn.proposal_layer._img_hw(img_info)
        # ---- targets first, on their own stream: AnchorTargetLayer depends on the ground truth and the map size only, and its fg / bg
        #      subsample runs on the HOST (NumPy's global RNG, the reference's call sequence) -- a device round trip.  Python runs a whole
        #      step ahead of the GPU, so here the round trip overlaps the previous step's backward pass; after the forward pass (where
        #      the reference has it) it drained the stream and left the GPU idle while the host sampled (0.4 ms per step).  One draw
        #      per step either way: the RNG sequence is the reference's.
        H, W = int(x.shape[2]), int(x.shape[3])
        for l in self.layers:
            if l == "pool":
                H, W = (H + 1) // 2, (W + 1) // 2
        if self.resnet is not None:
            H, W = self.resnet.feat_hw(H, W)
        with rt.mem.early_stream(unwrap(gt_boxes)):                   # its own stream: it must not wait for the previous step's backward
            labels, targets, inds, n_in, _ = self.atl.forward_device(H, W, gt_boxes, im_h, im_w)      # (host ground truth; a DEVICE array is waited for)
        rt.mem.join_early_stream(labels, targets, inds)
        if self.arith is not None:
            self.arith.repack()
            feat, inputs, feat_op = trunk_forward_operand(self, x)
            link = rpn.rpn_conv_3x3
            _, mid = self.arith.conv(feat_op, self.arith.w_fwd["rpn_conv_3x3"], link.b, link.cin, link.cout, relu=True, want=False)
        elif self.resnet is not None:
            # train-mode BatchNormalization trunk: the forward pass keeps its own tape; its input-gradient packings are rebuilt after an update
            rt.pack_conv_dgrad_w_many([(rpn.rpn_conv_3x3.Wp, self.wd["rpn_conv_3x3"], 3), (rpn._heads_packed[0], self.wd_heads, 1)])
            self._dgrad_packed = True
            model.trunk.train = True
            feat, inputs = model.trunk(x), []
            mid = rpn.rpn_conv_3x3(feat, relu=True)
        else:
            # weights of every input-gradient convolution (rotated / transposed copies of the current packed weights): one launch
            if _tuning.get("FRCNN_DGRAD_PACK") != "each":          # (=each: A/B hook, one launch per layer inside the backward pass)
                with _grad_stream(rt):                                # on the gradient stream: under the forward pass, joined before the backward pass
                    rt.pack_conv_dgrad_w_many([(l.Wp, self.wd[n], 3) for n, l in self.convs[1:]] + [(rpn._heads_packed[0], self.wd_heads, 1)])
                self._dgrad_packed = True
            feat, inputs = trunk_forward(model, x, fuse_pools=self.keep_dy is None)     # keeps every layer's input
            mid = rpn.rpn_conv_3x3(feat, relu=True)
        score, prob, bbox = rt.rpn_heads(mid, rpn._heads_packed)
        if self.keep_dy is not None:                                 # tests: every activation map a ReLU / max-pool decision was taken on
            self.kept_dy["rpn_mid"] = mid
            self.kept_dy["layer_inputs"] = list(inputs) + [feat]
        if self.run_proposal_layer:
            # region_proposal_network.py:123-126: `proposals, probs = self.proposal_layer(...)` in train mode (12000 -> NMS -> 2000);
            # nothing downstream consumes it in rpn_train mode (faster_rcnn.py:115-116 returns the loss) -- kept for inspection.
            # Its sequential NMS pass keeps one wave busy for ~0.5 ms: it runs on a second stream, under the backward pass.
            with rt.mem.side_stream(prob, bbox):
                self.proposals = rpn.proposal_layer.forward_device(prob, bbox, im_h, im_w)
        A = self.A
        assert (H, W) == (int(feat.shape[2]), int(feat.shape[3]))
        NP = int(rpn._heads_packed[0].shape[1])
        # ---- losses
        if self._draw is None or tuple(self._draw.shape) != (NP, H, W):
            self._draw = rt.mem.zeros((NP, H, W), "f32")             # rows >= 6A (channel padding) stay zero
        draw = self._draw
        losses, _, _ = rt.rpn_loss(score[0], bbox[0], labels, targets, inds, n_in, A, H, W, rpn._delta, rpn._loss_lambda,
                                   d_score=draw[:2 * A], d_bbox=draw[2 * A:6 * A])
        if self.loss_scaler is not None:                             # fp16 step: everything below computes S * gradient (the losses are not scaled)
            self.loss_scaler.scale(draw)
            self._g_scale_word = 0
        # ---- backward: heads (one 1x1 convolution over the stacked cls|bbox matrix)
        rt.mem.join_aux_stream("grad")                               # the re-packed input-gradient weights are ready
        self._param_grads("heads", mid, draw, functools.partial(rt.conv_wgrad, ksize=1), ready=False)      # (the heads lie in the bucket that rpn_conv_3x3 or a layer below it closes)
        if not self._dgrad_packed:
            rt.pack_conv_dgrad_w(rpn._heads_packed[0], 1, out=self.wd_heads)
        g = rt.conv_ex(draw.reshape(1, NP, H, W), self.wd_heads, self.zero_bias, 1, act=2, mask=mid)
        if self.resnet is not None:
            # ---- rpn_conv_3x3 (g is already under its ReLU mask), then the trunk's own backward pass: res5's ReLU mask is bn3's to apply
            self._param_grads("rpn_conv_3x3", feat, g, rt.conv_wgrad)
            g = rt.conv_ex(g, self.wd["rpn_conv_3x3"], self.zero_bias, 3, act=0)
            rt.mem.join_aux_stream("grad")
            model.trunk.backward(g, self.grad, ready=self._grads_ready)
            self._dgrad_packed = False
            if self.run_proposal_layer:
                rt.mem.join_side_stream()
            return dict(losses=losses)
        # ---- rpn_conv_3x3, then the trunk in reverse
        backward = trunk_backward if self.arith is None else trunk_backward_operand
        backward(self, list(zip(self.layers, inputs)) + [(("rpn_conv_3x3", 0, 0), feat)], g)
        self._dgrad_packed = False
        if self.run_proposal_layer:
            rt.mem.join_side_stream()
        return dict(losses=losses)

    def step(self, x, img_info, gt_boxes):
        out = self.forward_backward(x, img_info, gt_boxes)
        self.all_reduce()
        self.update()
        return out

    def losses_host(self, out):
        l = self.rt.mem.to_numpy(out["losses"])
        return dict(rpn_loss_cls=float(l[0]), rpn_loss_bbox=float(l[1]), rpn_cls_accuracy=float(l[2]),
                    rpn_loss=float(l[0] + self.model.RPN._loss_lambda * l[1]))

    # ------------------------------------------------------------------
    def sync_params(self):
        _Trainer.sync_params(self)
        wp, bp, A = self.model.RPN._heads_packed
        wt = self.rt.transpose(wp)                                   # (NP, Cmid)
        rpn = self.model.RPN
        rpn.rpn_cls_score["W"], rpn.rpn_cls_score["b"] = wt[:2 * A], bp[:2 * A]
        rpn.rpn_bbox_pred["W"], rpn.rpn_bbox_pred["b"] = wt[2 * A:6 * A], bp[2 * A:6 * A]

    def flat_to_chainer_layout(self, flat):
        """A flat buffer in this trainer's segment layout (gradients, velocities, parameters) -> {link path: host array in
        Chainer's layout}: packed (Cin*9, Cout) -> (Cout, Cin, 3, 3); the stacked heads -> rpn_cls_score / rpn_bbox_pred."""
        seg, out = self._segment_reader(flat), {}
        if self.resnet is not None:
            self.resnet.to_chainer(seg, out)
        self._convs_to_chainer(seg, out)
        A = self.A
        gw, gb = seg("heads/W").T, seg("heads/b")
        out["RPN/rpn_cls_score/W"], out["RPN/rpn_cls_score/b"] = np.ascontiguousarray(gw[:2 * A]).reshape(2 * A, -1, 1, 1), gb[:2 * A].copy()
        out["RPN/rpn_bbox_pred/W"], out["RPN/rpn_bbox_pred/b"] = np.ascontiguousarray(gw[2 * A:6 * A]).reshape(4 * A, -1, 1, 1), gb[2 * A:6 * A].copy()
        return out

    def chainer_layout_to_flat(self, arrays, flat):
        """Inverse of flat_to_chainer_layout: write {link path: array} into `flat` (missing keys leave their segment untouched)."""
        with self._segment_writer(flat) as put:
            if self.resnet is not None:
                self.resnet.from_chainer(arrays, put)
            self._convs_from_chainer(arrays, put)
            A = self.A
            sw, sb = self.seg["heads/W"], self.seg["heads/b"]
            if "RPN/rpn_cls_score/W" in arrays and "RPN/rpn_bbox_pred/W" in arrays:
                w = np.zeros((sw.shape[1], sw.shape[0]), np.float32)                       # (NP, Cmid): rows past 6A are channel padding
                w[:2 * A] = np.asarray(arrays["RPN/rpn_cls_score/W"], dtype=np.float32).reshape(2 * A, -1)
                w[2 * A:6 * A] = np.asarray(arrays["RPN/rpn_bbox_pred/W"], dtype=np.float32).reshape(4 * A, -1)
                put("heads/W", w.T)
                b = np.zeros((sb.shape[0],), np.float32)
                b[:2 * A], b[2 * A:6 * A] = arrays["RPN/rpn_cls_score/b"], arrays["RPN/rpn_bbox_pred/b"]
                put("heads/b", b)


class RCNNTrainer(_Trainer):
    """Stage-2 step of train_rcnn.py (train_rcnn.py:35-78; models/faster_rcnn.py:110-173 with rcnn_train = True): trunk -> RPN
    proposals (test-mode ProposalLayer, no gradient) -> RoI pooling -> fc6/fc7 with dropout -> cls_score / bbox_pred ->
    ProposalTargetLayer sampling -> softmax-CE + Huber(1) on the sampled rows -> backward through the head (the four L.Linear
    as GEMMs on transposed operands), RoI pooling (arg-max scatter), the trunk -> MomentumSGD + WeightDecay over trunk + head.

    Dropout masks are drawn on the host from NumPy's global RNG in the order chainer's CPU path draws them (fc6's mask, fc7's
    mask, then ProposalTargetLayer's two np.random.choice calls), so a seeded run follows the reference's random stream.
    """

    HEAD = ("fc6", "fc7", "cls_score", "bbox_pred")
    stage_hook = None           # bench.py --mode train-rcnn: called with a stage's name at every stage boundary of forward_backward
    trunk_collect = None        # tests, ResNet model: a dict -> the step's train-mode trunk call fills it (ResNet.__call__(x, collect=...): the taped maps)
    _dropout_iter = None        # dropout_rng="device": the iteration whose forward passes _dropout_fwd counts

    def __init__(self, model, lr=0.001, momentum=0.9, weight_decay=None, dropout_ratio=0.5, comm=None, conv_math="mfma", dropout_rng="numpy",
                 dropout_seed=0, precision=None, loss_scale=None, opt="MomentumSGD", opt_args=None, roi_bwd=None):
        """dropout_rng: "numpy" (default) draws both masks on the host from NumPy's global stream exactly as chainer's CPU F.dropout does (two
        np.random.rand calls of n_rois x 4096 values per step: ~7 ms of host time at 300 RoIs, bench.py --mode train-rcnn); "device" draws them
        in the dropout kernel from a counter-based hash of (dropout_seed, step, layer) -- the throughput form, no host work, no H2D.
        conv_math: as in RPNTrainer -- "mfma" = the trunk's forward / input-gradient / weight-gradient convolutions on the fp32 MFMA
        kernels, "split" = the same fp32 convolutions as six bf16 MFMA products of 3-way split operands (csrc/conv_f32s.hip).
        precision: None (default: every path above, untouched), "bf16" = mixed precision: EVERY matrix product of the step -- forward, input gradient
        and weight gradient of the trunk's convolutions, rpn_conv_3x3's forward, forward / dx / dW of the four L.Linear layers -- on RNE-bf16
        images of the fp32 activations, gradients and master weights, with fp32 accumulation (csrc/conv_f32s.hip, train.hip,
        linear_train_bf16.hip); everything else (bias, ReLU, pools, the RPN 1x1 heads, proposals, RoI pooling, dropout, losses, the
        all-reduce, the update on the fp32 master weights) as in the fp32 step; "f16" = the same contract with fp16 operands plus the
        device-side loss scale of RPNTrainer(conv_math="f16") (LossScaler): rcnn_loss's two gradient outputs are multiplied by S, self.G holds
        S times the gradient until update(), which skips the step when the all-reduced buffer holds an Inf / NaN.
        loss_scale (precision="f16" only): "dynamic" (the default), a power of two (static), or a dict of LossScaler's constants.
        opt, opt_args, weight_decay=None: the update rule and its hyper-parameters, as in RPNTrainer.
        roi_bwd: the RoI-pooling scatter, "planes" (csrc/roi_pool.hip: LDS planes, float adds in the order the waves arrive -- two runs agree to rounding) or
        "ordered" (csrc/roi_bwd_ordered.hip: the reference loop's order of additions, the same bits every run -- what a bit-for-bit resume needs); None = "planes"
        for the fp32 step, "ordered" for precision="bf16" / "f16" (which always was).
        A ResNet model (FasterRCNN(trunk_class=ResNet101, rpn_in_ch=2048, feat_stride=32)) trains in fp32 only: conv_math="mfma", precision=None; its trunk runs
        BatchNormalization on batch statistics (models/resnet.py) and keeps its own tape, the RPN runs in test mode, the head is the code VGG runs."""
        from .models.proposal_target_layer import ProposalTargetLayer
        if conv_math not in ("mfma", "split"):
            raise ValueError("RCNNTrainer: conv_math is the arithmetic of the trunk's fp32 convolutions, 'mfma' or 'split', not %r "
                             "(16-bit operands: precision='bf16' / 'f16')" % (conv_math,))
        if precision not in (None, "bf16", "f16"):
            raise ValueError("RCNNTrainer: precision must be None, 'bf16' or 'f16', not %r" % (precision,))
        if precision is not None and conv_math == "split":
            raise ValueError("RCNNTrainer: precision=%r replaces the fp32 convolutions; it does not combine with conv_math='split'" % (precision,))
        if loss_scale is not None and precision != "f16":
            raise ValueError("RCNNTrainer: loss_scale belongs to precision='f16', not %r" % (precision,))
        if roi_bwd not in (None, "planes", "ordered"):
            raise ValueError("RCNNTrainer: roi_bwd must be None, 'planes' or 'ordered', not %r" % (roi_bwd,))
        if _is_resnet(model):
            if conv_math != "mfma" or precision is not None:
                raise ValueError("RCNNTrainer: a ResNet model trains with conv_math='mfma' and precision=None (fp32) only, not conv_math=%r, precision=%r: "
                                 "split-product and mixed-precision ResNet training are not built" % (conv_math, precision))
            if any(getattr(model, n).W is None or getattr(model, n).b is None for n in self.HEAD):        # (before anything is allocated)
                raise ValueError("RCNNTrainer: this ResNet model's head (fc6, fc7, cls_score, bbox_pred) holds no parameters; load them first")
        self.resnet = _ResNetTrunk(model.trunk, "RCNNTrainer") if _is_resnet(model) else None
        self.conv_math, self.precision = conv_math, precision
        self.roi_bwd = roi_bwd or ("ordered" if precision is not None else "planes")
        self.model, self.rt = model, model.rt
        self.lr, self.momentum, self.dropout_ratio, self.comm = lr, momentum, dropout_ratio, comm
        self._init_optimizer("RCNNTrainer", opt, opt_args, weight_decay)
        assert dropout_rng in ("numpy", "device")
        self.dropout_rng, self.dropout_seed = dropout_rng, int(dropout_seed)
        rt = self.rt
        self.ptl = ProposalTargetLayer(model._feat_stride, num_classes=model._num_classes, runtime=rt)
        # (a ResNet trunk's parameters are not `links`: self.resnet lays them out, in execution order, and the trunk re-packs its own input-gradient weights)
        self.layers = model.trunk.layers if self.resnet is None else []
        self.convs = [(l[0], model.trunk.links[l[0]]) for l in self.layers if l != "pool"]
        head = [getattr(model, n) for n in self.HEAD]
        self._build_arena((self.resnet.segments() if self.resnet is not None else []) + self._conv_segments()
                          + [(n + sfx, a.shape) for n, lin in zip(self.HEAD, head) for sfx, a in (("/W", lin.W), ("/b", lin.b))])
        rpn3 = [("rpn_conv_3x3", model.RPN.rpn_conv_3x3)] if precision is not None else []      # 16-bit forward only: stage 2 gives the RPN no gradient
        self._init_arithmetic(precision or conv_math, loss_scale, fwd=self.convs + rpn3, dgrad=self.convs[1:])
        self.zero_bias = rt.mem.zeros((max(512, max(int(lin.W.shape[1]) for lin in head)),), "f32")
        self.iteration = 0
        # the head (fc6: 411 MB of gradients) is complete before the trunk's backward starts: its bucket rides under all of it
        self._plan_buckets((self.resnet.names if self.resnet is not None else []) + [n for n, _ in self.convs] + list(self.HEAD))

    def _ensure_adopted(self):
        if self.resnet is not None:
            self.resnet.adopt(self)
        self._adopt_convs()
        for n in self.HEAD:
            lin = getattr(self.model, n)
            lin.W = self._adopt(n + "/W", lin.W)
            lin.b = self._adopt(n + "/b", lin.b)
            lin._adopted = True

    # ------------------------------------------------------------------ one L.Linear backward: GEMMs on transposed operands
    def _linear_backward(self, name, x, dy, need_dx=True):
        """x (M,K) the layer's input, dy (M,N): fills grad[name/W] (N,K), grad[name/b]; returns dx (M,K) or None."""
        rt = self.rt
        lin = getattr(self.model, name)
        M, K = int(x.shape[0]), int(np.prod(x.shape[1:]))
        N = int(dy.shape[1])
        self._tap(name, x.reshape(M, K), dy)
        if self.precision is not None:
            # 16-bit operands: dW = RNE(dy)^T RNE(x) and dx = RNE(dy) RNE(W) with W read as stored -- fp32 arrays in, rounded inside the kernels
            # (csrc/linear_train_bf16.hip): no transposed or padded copies of x, W or dW
            rth = self.arith.rt
            rth.linear_wgrad_bf16(dy, x.reshape(M, K), out=self.grad[name + "/W"])
            rt.bias_grad(rt.transpose(dy).reshape(1, N, 1, M), out=self.grad[name + "/b"])      # db = column sums of dy, as in the fp32 step
            return rth.linear_dgrad_bf16(dy, lin.W) if need_dx else None
        Mp = (M + 3) // 4 * 4                                        # the GEMM contracts over M here: pad it to a multiple of 4
        if Mp == M:                                                  # (the 128 kept rows of a full sample: nothing to pad, four launches fewer)
            xpad, dpad = x.reshape(M, K), dy
        else:
            xpad, dpad = rt.mem.zeros((Mp, K), "f32"), rt.mem.zeros((Mp, N), "f32")
            xpad[:M] = x.reshape(M, K)
            dpad[:M] = dy
        dyT, xT = rt.transpose(dpad), rt.transpose(xpad)             # (N, Mp), (K, Mp)
        rt.linear(dyT, xT, None, out=self.grad[name + "/W"])                        # dW = dy^T x (no bias term: a single K slab goes straight into the gradient)
        rt.bias_grad(dyT.reshape(1, N, 1, Mp), out=self.grad[name + "/b"])          # db = column sums of dy
        if not need_dx:
            return None
        if N % 64 == 0 and K % 64 == 0 and M <= 4096 and _tuning.get("FRCNN_LINEAR_DX", "conv") == "conv":
            # dx = dy W with W (N, K) READ AS STORED: a 1x1 convolution whose "image" is W itself -- N channels of K "pixels" -- and whose
            # packed weights (Cin, Cout) are dy^T padded to 64 output channels: y[m][k] = sum_n dy[m][n] W[n][k].  No transposed copy of W
            # (fc6: 411 MB read + written every step), and W is streamed exactly once.
            Mc = (M + 63) // 64 * 64
            wh = 1
            for c in (256, 224, 128, 64):                          # a map shape for the kernel's 2-D tiles; any factorisation of K is the same sum
                if K % c == 0:
                    wh = c
                    break
            if Mc == Mp:
                dycT = dyT                                           # already (N, Mc)
            else:
                dyc = rt.mem.zeros((Mc, N), "f32")
                dyc[:M] = dy
                dycT = rt.transpose(dyc)
            dx = rt.conv_ex(lin.W.reshape(1, N, K // wh, wh), dycT, self.zero_bias[:Mc], ksize=1, act=0)
            return dx.reshape(Mc, K)[:M]
        Np = (N + 3) // 4 * 4                                        # dx = dy W contracts over N: pad it to a multiple of 4 as well
        if Np != N:
            dyn, wn = rt.mem.zeros((M, Np), "f32"), rt.mem.zeros((Np, K), "f32")
            dyn[:, :N] = dy
            wn[:N] = lin.W
        else:
            dyn, wn = dy, lin.W
        return rt.linear(dyn, rt.transpose(wn), None)                               # W^T is (K, Np)

    def forward_backward(self, x, img_info, gt_boxes, masks=None):
        """Fills self.G; returns dict(losses (3,) device [loss_cls, loss_bbox, cls_accuracy], n_rois, keep_inds)."""
        rt, model = self.rt, self.model
        stage = self.stage_hook or (lambda name: None)               # bench.py --mode train-rcnn: a HIP event per stage boundary
        self._drain()                                              # a previous backward whose sums were never consumed
        self._ensure_adopted()
        x = rt.asarray(unwrap(x), "f32")
        im_h, im_w = model.RPN.proposal_layer._img_hw(img_info)
        # the gt boxes go up FIRST and without blocking the host: everything up to the one host read behind the ProposalLayer is then enqueued while
        # the trunk still runs (a pageable copy issued where the boxes are needed stalled the host -- and, behind it, the GPU -- in the middle of the step)
        gt_host = unwrap(gt_boxes)
        gt_host = np.ascontiguousarray(rt.mem.to_numpy(gt_host) if rt.mem.is_array(gt_host) else np.asarray(gt_host), dtype=np.float32)
        gt_dev64 = rt.mem.from_numpy_async(np.ascontiguousarray(gt_host[0][:, :4], dtype=np.float64))
        stage("start")
        if self.arith is not None:                                    # (16-bit: rpn_conv_3x3's forward weights are re-packed with the trunk's)
            self.arith.repack()
            feat, inputs, feat_op = trunk_forward_operand(self, x)
        elif self.resnet is not None:
            # train-mode BatchNormalization trunk: the forward pass keeps its own tape (and moves the running statistics); its input-gradient packings are its own
            model.trunk.train = True
            feat, inputs = (model.trunk(x, collect=self.trunk_collect) if self.trunk_collect is not None else model.trunk(x)), []
        else:
            # weights of every input-gradient convolution (rotated / transposed copies of the current packed weights): ONE launch on the gradient
            # stream, under the forward pass -- as in RPNTrainer (one launch per layer inside the backward pass was 12 x 17 us on its critical path)
            if _tuning.get("FRCNN_DGRAD_PACK") != "each":
                with _grad_stream(rt):
                    rt.pack_conv_dgrad_w_many([(l.Wp, self.wd[n], 3) for n, l in self.convs[1:]])
                self._dgrad_packed = True
            feat, inputs = trunk_forward(model, x, fuse_pools=self.keep_dy is None)
        C, H, W = [int(v) for v in feat.shape[1:]]
        stage("trunk_fwd")
        if self.precision is not None:                                # rpn_conv_3x3 on the blocked 16-bit map, the 1x1 heads in fp32 (as RPNTrainer)
            rpn3 = model.RPN.rpn_conv_3x3
            _, mid = self.arith.conv(feat_op, self.arith.w_fwd["rpn_conv_3x3"], rpn3.b, rpn3.cin, rpn3.cout, relu=True, want=False)
            _, prob, bbox = rt.rpn_heads(mid, model.RPN._heads_packed)
        else:
            _, _, prob, bbox = model.RPN.heads(feat, want_score=False, wino=False)      # the training step keeps the direct convolution
        rois, _, n_out = model.RPN.proposal_layer.forward_device(prob, bbox, im_h, im_w)      # RPN.train is False in rcnn_train mode
        # ProposalTargetLayer needs the RoIs and the gt boxes only: its float64 IoU matrix is enqueued here and comes back with the RoI count (the
        # one host read the step needs anyway), so the host-side sampling further down overlaps the head's forward pass instead of waiting for it
        if self.ptl.type_check_enable:
            self.ptl._check_data_type_forward(rois, gt_boxes)
        ov_dev = self.ptl.overlaps_device(rois, gt_dev64)
        fetch = rt.mem.to_numpy_many_async([ov_dev, rois, n_out])                            # one device -> host copy, one host round trip
        scale = 1.0 / (1.0 - self.dropout_ratio)
        on_device = masks is None and self.dropout_rng == "device"

        def collect():
            ov_host, rois_host, n_host = fetch()
            n = int(n_host[0])
            assert n > 0, "the ProposalLayer returned no RoI (proposal_target_layer.py:52 asserts the same)"
            return n, rois_host[:n], ov_host[:n]

        def head_forward(rois, n):
            """RoI pooling -> fc6 -> dropout -> fc7 -> dropout -> cls_score / bbox_pred on n rows."""
            pool5, argmax = rt.roi_pool_fwd_chw(feat, rois, 7, 7, model._spatial_scale, want_argmax=True)
            stage("roi_pool_fwd")
            pool5 = pool5.reshape(n, -1)
            if self.precision is not None:                           # the four L.Linear on RNE(x), RNE(W), fp32 accumulation, bias and ReLU
                rth = self.arith.rt
                fc = lambda lin, xin, relu=False: rth.linear_bf16_train(xin, lin.W, lin.b, relu=relu)
            else:
                fc = lambda lin, xin, relu=False: lin(xin, relu=relu)
            a6 = fc(model.fc6, pool5, relu=True)
            if on_device:                                            # one launch: mask drawn, stored and applied
                # one counter per FORWARD (two draws each) -- not per update: forward_backward twice without update() must not reuse its masks -- and
                # the data-parallel rank folded in: every rank draws its own masks from one dropout_seed
                # the stream is a function of (dropout_seed, rank, iteration, forward-within-iteration) -- a trainer rebuilt mid-run (resume: `iteration`
                # comes back from the snapshot) continues the mask sequence instead of replaying step 0's; the within-iteration index resets when update() advances
                # `iteration`
                if self._dropout_iter != self.iteration:
                    self._dropout_iter, self._dropout_fwd = self.iteration, 0
                fwd = self._dropout_fwd
                self._dropout_fwd += 1
                rank = int(getattr(self.comm, "rank", 0) or 0)      # getattr: comm may be None, and a communicator owes the trainers no `rank`
                base = (self.dropout_seed * 0x100000001b3 + rank * 0x9E3779B97F4A7C15 + (int(self.iteration) << 20) + 2 * fwd) & 0xFFFFFFFFFFFFFFFF
                d6, m6 = rt.dropout(a6, self.dropout_ratio, base)
            else:
                if masks is None:                                    # F.dropout [chainer-ext]: mask = (rand >= ratio) * 1/(1-ratio)
                    m6 = ((np.random.rand(*a6.shape) >= self.dropout_ratio) * scale).astype(np.float32)
                else:
                    m6 = masks[0]
                m6 = rt.asarray(m6, "f32")
                d6 = rt.mul(a6, m6)
            a7 = fc(model.fc7, d6, relu=True)
            if on_device:
                d7, m7 = rt.dropout(a7, self.dropout_ratio, (base + 1) & 0xFFFFFFFFFFFFFFFF)
            else:
                m7 = ((np.random.rand(*a7.shape) >= self.dropout_ratio) * scale).astype(np.float32) if masks is None else masks[1]
                m7 = rt.asarray(m7, "f32")
                d7 = rt.mul(a7, m7)
            cls_score, bbox_pred = fc(model.cls_score, d7), fc(model.bbox_pred, d7)
            stage("head_fwd")
            return pool5, argmax, a6, d6, m6, a7, d7, m7, cls_score, bbox_pred

        if on_device and _tuning.get("FRCNN_RCNN_HEAD_FWD", "early") == "early":
            # Device-drawn masks: nothing on the host has to know the RoI count before the head's forward pass, so it is enqueued at the
            # ProposalLayer's CAPACITY (rows past the count are zero boxes -- detect.hip defines them -- and a row's results, its mask included,
            # do not depend on the row count) BEFORE the host waits for its copy: the round trip, the sampling and the enqueueing of the losses
            # and the head's backward pass all run under 0.65 ms of GPU work instead of in front of it.  (The NumPy-stream masks are
            # (n, 4096) draws in the reference's order: that form reads the count first.)
            stage("rpn_proposals")
            cap = int(rois.shape[0])
            fw = head_forward(rois, cap)
            n, rois_host, ov_host = collect()
            if n < cap:
                fw = tuple(t[:n] for t in fw)
            rois = rois[:n]
        else:
            n, rois_host, ov_host = collect()
            rois = rois[:n]
            stage("rpn_proposals")
            fw = head_forward(rois, n)
        pool5, argmax, a6, d6, m6, a7, d7, m7, cls_score, bbox_pred = fw
        # host work under the head's forward pass: np.random.choice in the reference's call order (after the two dropout draws)
        use_gt, ext, keep = self.ptl.sample(np.ascontiguousarray(rois_host, dtype=np.float32), gt_host[0], overlaps=ov_host)
        k = int(keep.shape[0])
        blob = np.empty((k * (2 + ext.shape[1]),), dtype=np.float32)                         # keep | labels | targets: ONE host -> device copy
        blob[:k] = np.ascontiguousarray(keep, dtype=np.int32).view(np.float32)
        blob[k:2 * k] = use_gt[:, -1].astype(np.int32).view(np.float32)                      # faster_rcnn.py:153
        blob[2 * k:] = ext.reshape(-1)
        blob = rt.mem.from_numpy_async(blob)                                                 # the host keeps running ahead of the head's forward pass
        keep, labels = rt.mem.bitcast(blob[:k], "i32"), rt.mem.bitcast(blob[k:2 * k], "i32")
        ext = blob[2 * k:].reshape(k, -1)
        losses, dcs, dbp = rt.rcnn_loss(rt.gather_rows(cls_score, keep), rt.gather_rows(bbox_pred, keep), labels, ext, model._rcnn_delta)
        if self.loss_scaler is not None:                             # fp16 step: everything below computes S * gradient (the losses are not scaled)
            self.loss_scaler.scale(dcs)
            self.loss_scaler.scale(dbp)
            self._g_scale_word = 0
        stage("targets_loss")
        # ---- backward: head.  Only the sampled rows carry a gradient (faster_rcnn.py:155-160: the losses see cls_score[keep_inds] and
        # bbox_pred[keep_inds]; get_item's adjoint leaves every other row of the 300 EXACTLY zero), so the four L.Linear backward passes, the
        # dropout / ReLU adjoints and the RoI-pooling scatter run on the k <= 128 kept rows: the same sums without their zero terms
        # (fc6's two 61.7-GFLOP GEMMs become two of 26.3).  FRCNN_RCNN_BWD_ROWS=all runs them over all n rows (A/B; the zero-padded form).
        if 0 < k < n and _tuning.get("FRCNN_RCNN_BWD_ROWS", "kept") != "all":
            rows = k
            dcls, dbb = dcs, dbp
            d7b, m7b = rt.gather_rows(d7, keep), rt.gather_rows(m7, keep)
            d6b, m6b = rt.gather_rows(d6, keep), rt.gather_rows(m6, keep)
            pool5b, argmaxb = rt.gather_rows(pool5, keep), rt.gather_rows(argmax.reshape(n, -1), keep)
        else:
            rows = n
            dcls, dbb = rt.scatter_rows(dcs, keep, n), rt.scatter_rows(dbp, keep, n)
            d7b, m7b, d6b, m6b, pool5b, argmaxb = d7, m7, d6, m6, pool5, argmax
        # dropout then ReLU, backwards: g * mask where relu(.) > 0.  d = relu(.) * mask is positive exactly where both are, and where the mask is zero
        # the product already is (for finite g): the ReLU test reads d (no third row set to gather)
        g7 = rt.add(self._linear_backward("cls_score", d7b, dcls), self._linear_backward("bbox_pred", d7b, dbb))
        g7 = rt.relu_bwd_(rt.mul(g7, m7b, out=g7), d7b)
        g6 = self._linear_backward("fc7", d6b, g7)
        g6 = rt.relu_bwd_(rt.mul(g6, m6b, out=g6), d6b)
        stage("head_bwd_small")
        gp = self._linear_backward("fc6", pool5b, g6)
        stage("fc6_bwd")
        for n_ in reversed(self.HEAD):                             # every head gradient is enqueued: a bucket closed by a head layer starts now
            self._grads_ready(n_)
        # ---- RoI pooling (arg-max scatter) and the trunk; feat = relu(conv5_3): mask before entering conv5_3's backward
        # (16-bit step: this map is rounded for conv5_3's backward products, where the last bit of a cell can decide a rounding -- the scatter with a fixed order
        # of additions keeps two steps from one state bit-identical; the fp32 step keeps its plane kernel, whose float atomics stay at rounding level)
        roi_bwd = rt.roi_pool_bwd_ordered if self.roi_bwd == "ordered" else rt.roi_pool_bwd
        gfeat = roi_bwd(gp.reshape(rows, C, 7, 7), argmaxb.reshape(rows, C, 7, 7), C, H, W)
        if self.resnet is not None:
            # dL/d res5 goes in UNMASKED: res5 = relu(bn3(conv3) + shortcut), and bn3's backward applies that ReLU's mask (models/resnet.py ResNet.backward)
            stage("roi_pool_bwd")
            model.trunk.backward(gfeat, self.grad, ready=self._grads_ready)
        else:
            gfeat = rt.relu_bwd_(gfeat, feat)
            stage("roi_pool_bwd")
            rt.mem.join_aux_stream("grad")                           # the re-packed input-gradient weights are ready
            backward = trunk_backward if self.arith is None else trunk_backward_operand
            backward(self, list(zip(self.layers, inputs)), gfeat)
            self._dgrad_packed = False
        stage("trunk_bwd")
        # rois: the (n, 4) proposals THIS step pooled -- a parity test must hand the oracle these, not the proposals of a second, inference-form forward: the
        # fused conv + ReLU + pool launches of the training forward (act 5) and of the inference forward (act 4) may run different decompositions (round 6:
        # pick_conv_config), i.e. conv5_3 agrees to the last bits but one, and near-tied proposals can then differ
        # head_acts: relu(fc6), relu(fc7) before dropout (the parity tests read the device's ReLU decisions off them)
        # layer_inputs / roi_argmax: every discrete decision of this step's forward pass (a fused pool's entry is its _PoolArg: the winning cell and the ReLU bit of
        # every window; an unfused layer's successor input is its post-ReLU map; the arg-max cell of every RoI bin) -- the float64 arbiter of the parity tests imposes them
        # (a ResNet model: layer_inputs is [] -- the trunk's tape is the record of its decisions, self.trunk_collect receives its maps)
        layer_inputs = (list(inputs) + [feat]) if self.resnet is None else []
        return dict(losses=losses, n_rois=n, keep_inds=keep, masks=(m6, m7), rois=rois, head_acts=(a6, a7), layer_inputs=layer_inputs, roi_argmax=argmax)

    def step(self, x, img_info, gt_boxes, masks=None):
        out = self.forward_backward(x, img_info, gt_boxes, masks)
        self.all_reduce()
        self.update()
        return out

    def losses_host(self, out):
        l = self.rt.mem.to_numpy(out["losses"])
        return dict(loss_cls=float(l[0]), loss_bbox=float(l[1]), cls_accuracy=float(l[2]), loss_rcnn=float(l[0] + l[1]))

    def flat_to_chainer_layout(self, flat):
        seg, out = self._segment_reader(flat), {}
        if self.resnet is not None:
            self.resnet.to_chainer(seg, out)
        self._convs_to_chainer(seg, out)
        for n in self.HEAD:
            out[n + "/W"], out[n + "/b"] = seg(n + "/W").copy(), seg(n + "/b").copy()
        return out

    def chainer_layout_to_flat(self, arrays, flat):
        with self._segment_writer(flat) as put:
            if self.resnet is not None:
                self.resnet.from_chainer(arrays, put)
            self._convs_from_chainer(arrays, put)
            for n in self.HEAD:
                for sfx in ("/W", "/b"):
                    if n + sfx in arrays:
                        put(n + sfx, arrays[n + sfx])


class TorchComm(object):
    """torch.distributed as the collective layer: backend "nccl" is RCCL on ROCm (xGMI), "gloo" on CPU.

    gloo with DEVICE tensors (ranks sharing one GPU: the functional smoke of the N > 1 path on a 1-GPU box) is staged by hand
    through pinned host memory: the device -> host copy of a bucket rides on a copy stream behind the kernels that fill it, the
    reduction itself runs on host tensors when the trainer waits, the sum goes back with one async copy.  (Handing gloo the device
    tensor makes every call synchronise the whole device and poll: 2 s per step for three buckets, profiles/r02_bench_2rank_gloo_train.json.)
    FRCNN_COMM_TRACE=1 collects host milliseconds per call kind in `self.trace`."""

    def __init__(self, force_single_rank=False):
        import os
        import time
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self._time = torch, dist, time
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        # `active` is what the trainers ask (every communicator has it; False = skip the exchange): one rank normally skips it;
        # force_single_rank runs it anyway (bench.py --dist-world1, the RCCL smoke test)
        self.active = dist.is_initialized() and (self.world_size > 1 or force_single_rank)
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.backend = dist.get_backend() if dist.is_initialized() else None
        self._pinned, self._copy_stream = None, None
        self.trace = {} if _tuning.get("FRCNN_COMM_TRACE") == "1" else None

    def _note(self, kind, t0):
        if self.trace is not None:
            e = self.trace.setdefault(kind, [0, 0.0])
            e[0] += 1
            e[1] += (self._time.perf_counter() - t0) * 1e3

    def _staged(self, t):
        return self.backend == "gloo" and t.is_cuda

    def _stage_out(self, t):
        """Device slice -> pinned host slice on the copy stream, ordered behind everything already enqueued on the current stream."""
        torch = self.torch
        n = t.numel()
        if self._pinned is None:
            self._pinned = {}
        key = (t.data_ptr(), n)                                    # a trainer's buckets are fixed slices of its gradient buffer
        host = self._pinned.get(key)
        if host is None:
            host = self._pinned[key] = torch.empty(n, dtype=t.dtype).pin_memory()
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=t.device)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(t.device))
        done = torch.cuda.Event()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(ready)
            host.copy_(t.reshape(-1), non_blocking=True)
            done.record(self._copy_stream)
        return ("staged", t, host, done)

    def all_reduce_sum(self, buf):
        t0 = self._time.perf_counter()
        t = buf if isinstance(buf, self.torch.Tensor) else self.torch.from_numpy(buf)      # NumPy buffers are reduced in place
        if self._staged(t):
            self.wait(self._stage_out(t))
        else:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        self._note("all_reduce_sum", t0)

    def all_reduce_sum_async(self, buf):
        """Launch the all-reduce of a (contiguous) slice now and return a handle: with RCCL it is enqueued behind the kernels
        already on the current stream and runs on the collective's stream, under whatever the caller launches next."""
        t0 = self._time.perf_counter()
        t = buf if isinstance(buf, self.torch.Tensor) else self.torch.from_numpy(buf)
        w = self._stage_out(t) if self._staged(t) else self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, async_op=True)
        self._note("launch", t0)
        return w

    def wait(self, work):
        t0 = self._time.perf_counter()
        if isinstance(work, tuple) and work[0] == "staged":
            _, t, host, done = work
            done.synchronize()                                     # the bucket is on the host
            self.dist.all_reduce(host, op=self.dist.ReduceOp.SUM)  # gloo, host tensors: blocks this thread only
            t.reshape(-1).copy_(host, non_blocking=True)           # back on the current stream: later kernels see the sum
        else:
            work.wait()                                # RCCL: the current stream waits for the collective (no host block); gloo: blocks
        self._note("wait", t0)
