"""Checks of the trainable ResNet trunk (csrc/bn_train.hip, models/resnet.py train mode, RPNTrainer on a ResNet model), written once and run on
the host emulator (tests/test_resnet_train_emulated.py) and on the MI355X (tests/test_gpu_resnet_train.py).

Kernel level: train-mode BatchNormalization forward / backward against a float64 restatement on the same fp32 inputs, with the bound taken
from what torch-CPU fp32 does on those inputs (4 x its error + 2^-23: the factor allows for another summation order); the two glue adjoints
bit for bit against torch autograd.  Trunk level: a torch restatement of the train-mode trunk (fp32 and float64; oracle/ holds the test-mode
one, O.resnet_forward, which this follows) with the DEVICE's ReLU masks imposed, under conditions that keep the imposition honest."""
import numpy as np

from parity_cases import dev, host

BN_EPS, BN_DECAY = 2e-5, 0.9
NARROW = 64          # the smallest base_width the fp32 conv kernels take (Cout % 64 == 0, and every stage width is some layer's Cout): the published widths

# (C, HW) of the issue; the last one has parts > 1 on the emulator too (C small, HW > 2048), (64, 37500) is the GPU's
BN_SHAPES = [(1, 1), (3, 6), (64, 255), (64, 256), (65, 257), (5, 1023), (7, 4097), (2048, 608)]
BN_SHAPE_PARTS_GPU = (64, 37500)
BN_SHAPE_PARTS_EMU = (3, 6151)
# (relu, residual, running buffers, dres): every flag on and off, alone and together
BN_FLAGS = [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)]
POOL_SHAPES = [(5, 13, 18), (1, 2, 2), (3, 7, 8), (64, 75, 125)]


def _maxabs(a):
    return float(np.abs(a).max())


def _nerr(got, want):
    """max-abs error normalised by the reference's max-abs"""
    return _maxabs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / max(_maxabs(want), 1e-30)


def bn_reference(z, gamma, beta, res, mask, dy, dtype):
    """torch-CPU functional BatchNormalization on batch statistics, forward and autograd, in `dtype`:
    pre = bn(z) [+ res]; y = relu(pre) when a mask is given; gradients of sum(pre * mask * dy) -- the ReLU's backward with the mask IMPOSED (it is
    one of the backward kernel's inputs: the forward output it is handed)."""
    import torch
    F = torch.nn.functional
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)        # noqa: E731
    zt, gt, bt = t(z).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    if z.shape[2] * z.shape[3] > 1:
        pre = F.batch_norm(zt, None, None, gt, bt, training=True, eps=BN_EPS)
    else:                                   # one value per channel: torch's functional refuses; the same formula spelled out
        mean = zt.mean((0, 2, 3), keepdim=True)
        var = ((zt - mean) ** 2).mean((0, 2, 3), keepdim=True)
        pre = (zt - mean) / torch.sqrt(var + BN_EPS) * gt.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
    if res is not None:
        pre = pre + t(res)
    y = torch.relu(pre) if mask is not None else pre
    g = t(dy) * (t(mask.astype(np.float32)) if mask is not None else 1.0)
    (pre * g).sum().backward()
    return {"y": y.detach().numpy(), "dz": zt.grad.numpy(), "dgamma": gt.grad.numpy(), "dbeta": bt.grad.numpy()}


def bn_inputs(C, HW, seed, mean_scale=1.0, std_lo=0.5, std_hi=2.0):
    rs = np.random.RandomState(seed)
    z = (rs.randn(1, C, 1, HW) * rs.uniform(std_lo, std_hi, (1, C, 1, 1)) + rs.randn(1, C, 1, 1) * mean_scale).astype(np.float32)
    return dict(z=z, gamma=rs.uniform(0.5, 1.5, C).astype(np.float32), beta=(rs.randn(C) * 0.1).astype(np.float32),
                res=rs.randn(1, C, 1, HW).astype(np.float32), dy=rs.randn(1, C, 1, HW).astype(np.float32),
                rm=(rs.randn(C) * 0.1).astype(np.float32), rv=rs.uniform(0.5, 1.5, C).astype(np.float32))


def _ulps(got, want64):
    want32 = want64.astype(np.float32)
    return float((np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)).max())


def check_bn(rt, C, HW, relu, residual, running, dres, seed=0):
    """One shape and flag combination, forward and backward, each launched twice (bit-identical).  -> the largest err / bound seen."""
    I = bn_inputs(C, HW, seed)
    z, gamma, beta, dy = I["z"], I["gamma"], I["beta"], I["dy"]
    res = I["res"] if residual else None
    zd, gd, bd, rd, dyd = dev(rt, z), dev(rt, gamma), dev(rt, beta), dev(rt, res) if residual else None, dev(rt, dy)
    outs = []
    for _ in range(2):
        rm, rv = (dev(rt, I["rm"]), dev(rt, I["rv"])) if running else (None, None)
        y, mean, rstd = rt.bn_train_fwd(zd, gd, bd, residual=rd, relu=relu, eps=BN_EPS, decay=BN_DECAY, running_mean=rm, running_var=rv)
        dz, dgamma, dbeta, dr = rt.bn_train_bwd(dyd, y if relu else None, zd, gd, mean, rstd, want_dres=dres)
        outs.append([host(rt, a) for a in (y, mean, rstd, dz, dgamma, dbeta)] + [host(rt, a) for a in (rm, rv, dr) if a is not None])
    for a, b in zip(*outs):
        assert np.array_equal(a, b), "two launches on the same inputs differ"
    y, mean, rstd, dz, dgamma, dbeta = outs[0][:6]
    mask = (y > 0) if relu else None
    import torch
    r64 = bn_reference(z, gamma, beta, res, mask, dy, torch.float64)
    r32 = bn_reference(z, gamma, beta, res, mask, dy, torch.float32)
    worst = 0.0
    for name, got in (("y", y), ("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta)):
        e_ref, e_dev = _nerr(r32[name], r64[name]), _nerr(got.reshape(r64[name].shape), r64[name])
        bound = 4 * e_ref + 2.0 ** -23
        print("bn (%d,%d) flags %d%d%d%d %-6s device %.3e  torch-fp32 %.3e  ratio to bound %.3f" % (C, HW, relu, residual, running, dres, name, e_dev, e_ref, e_dev / bound))
        assert e_dev <= bound, (name, e_dev, e_ref)
        worst = max(worst, e_dev / bound)
    # the saved statistics and the running update against float64
    z64 = z.astype(np.float64)[0, :, 0, :]
    m64, v64 = z64.mean(1), z64.var(1)
    assert np.all(np.abs(mean - m64) <= 1e-5 * np.maximum(np.abs(m64), np.sqrt(v64 + BN_EPS)))
    assert np.all(np.abs(rstd * np.sqrt(v64 + BN_EPS) - 1.0) <= 1e-5)
    if running:
        rm, rv = outs[0][6], outs[0][7]
        adjust = HW / max(HW - 1.0, 1.0)
        assert _ulps(rm, BN_DECAY * I["rm"].astype(np.float64) + (1 - BN_DECAY) * m64) <= 4
        assert _ulps(rv, BN_DECAY * I["rv"].astype(np.float64) + (1 - BN_DECAY) * adjust * (v64 + BN_EPS)) <= 4
    if dres:
        assert np.array_equal(outs[0][-1], dy * mask if relu else dy)
    if (C, HW) == (1, 1):
        assert rstd[0] == np.float32(1.0 / np.sqrt(BN_EPS))                # var = 0
    return worst


def check_bn_cancellation(rt):
    """A channel with mean 100 and std 0.01 over 4096 pixels: a single fp32 pass over sum x^2 loses the variance entirely."""
    rs = np.random.RandomState(5)
    z = (100.0 + 0.01 * rs.randn(1, 2, 64, 64)).astype(np.float32)
    z[0, 1] = rs.randn(64, 64)
    one = dev(rt, np.ones(2, np.float32))
    _, mean, rstd = rt.bn_train_fwd(dev(rt, z), one, dev(rt, np.zeros(2, np.float32)), eps=BN_EPS)
    z64 = z.astype(np.float64).reshape(2, -1)
    m64, r64 = z64.mean(1), 1.0 / np.sqrt(z64.var(1) + BN_EPS)
    em, er = np.abs(host(rt, mean) / m64 - 1.0), np.abs(host(rt, rstd) / r64 - 1.0)
    print("cancellation: save_mean rel %.2e, save_rstd rel %.2e (channel 0)" % (em[0], er[0]))
    assert em[0] <= 1e-5 and er[0] <= 1e-5 and er[1] <= 1e-5, (em, er)


def pool_maps(C, H, W, seed):
    rs = np.random.RandomState(seed)
    return {"randn": rs.randn(1, C, H, W).astype(np.float32),
            "ties": rs.randint(0, 4, (1, C, H, W)).astype(np.float32),                               # exact ties inside windows
            "relu": np.maximum(rs.randn(1, C, H, W) - 0.5, 0).astype(np.float32)}                    # runs of zeros


def check_glue_bwd(rt, C, H, W, seed=0):
    import torch
    F = torch.nn.functional
    rs = np.random.RandomState(seed + 100)
    for kind, x in pool_maps(C, H, W, seed).items():
        xt = torch.from_numpy(x).requires_grad_(True)
        yt = F.max_pool2d(xt, 3, 2, ceil_mode=True)
        dy = rs.randn(*yt.shape).astype(np.float32)
        yt.backward(torch.from_numpy(dy))
        want = xt.grad.numpy()
        for _ in range(2):
            got = host(rt, rt.maxpool3x3s2_bwd(dev(rt, x), dev(rt, dy)))
            assert got.shape == want.shape and np.array_equal(got, want), ("maxpool3x3s2_bwd", kind, (C, H, W))
    dy = rs.randn(1, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1).astype(np.float32)
    want = np.zeros((1, C, H, W), np.float32)
    want[:, :, ::2, ::2] = dy                                                                        # the strided slice's adjoint
    for _ in range(2):
        got = host(rt, rt.subsample2_bwd(dev(rt, dy), H, W))
        assert np.array_equal(got, want), ("subsample2_bwd", (C, H, W))


def check_refusals(rt):
    """a NULL required pointer, C or HW <= 0, a too small workspace: FRCNN_ERR_INVALID, and nothing written"""
    L, m = rt.lib, rt.mem
    C, HW = 4, 10
    a = lambda *s: dev(rt, np.full(s, 7.0, np.float32))                                              # noqa: E731
    z, y, dz, dy, ga, be, mean, rstd, dg, db = a(C, HW), a(C, HW), a(C, HW), a(C, HW), a(C), a(C), a(C), a(C), a(C), a(C)
    nbytes = L.frcnn_bn_workspace_bytes(C, HW)
    assert nbytes >= C * 16 and L.frcnn_bn_workspace_bytes(0, HW) == 0 and L.frcnn_bn_workspace_bytes(C, 0) == 0
    ws = m.zeros((nbytes,), "u8")
    P, S = m.ptr, m.stream()

    def fwd(z_=z, ga_=ga, be_=be, y_=y, mean_=mean, rstd_=rstd, C_=C, HW_=HW, ws_=ws, n=nbytes):
        return L.frcnn_bn_train_fwd_f32(P(z_), P(ga_), P(be_), None, 1, C_, HW_, BN_EPS, BN_DECAY, P(y_), P(mean_), P(rstd_), None, None, P(ws_), n, S)

    def bwd(dy_=dy, z_=z, ga_=ga, mean_=mean, rstd_=rstd, dz_=dz, dg_=dg, db_=db, C_=C, HW_=HW, ws_=ws, n=nbytes):
        return L.frcnn_bn_train_bwd_f32(P(dy_), None, P(z_), P(ga_), P(mean_), P(rstd_), C_, HW_, P(dz_), P(dg_), P(db_), None, P(ws_), n, S)
    bad = [fwd(z_=None), fwd(ga_=None), fwd(be_=None), fwd(y_=None), fwd(mean_=None), fwd(rstd_=None), fwd(C_=0), fwd(HW_=0), fwd(C_=-1), fwd(ws_=None),
           fwd(n=C * 16 - 1), bwd(dy_=None), bwd(z_=None), bwd(ga_=None), bwd(mean_=None), bwd(rstd_=None), bwd(dz_=None), bwd(dg_=None),
           bwd(db_=None), bwd(C_=0), bwd(HW_=-3), bwd(ws_=None), bwd(n=C * 16 - 1),
           L.frcnn_maxpool3x3s2_bwd_f32(None, P(dy), P(dz), 1, 5, 8, S), L.frcnn_maxpool3x3s2_bwd_f32(P(z), None, P(dz), 1, 5, 8, S),
           L.frcnn_maxpool3x3s2_bwd_f32(P(z), P(dy), None, 1, 5, 8, S), L.frcnn_maxpool3x3s2_bwd_f32(P(z), P(dy), P(dz), 0, 5, 8, S),
           L.frcnn_maxpool3x3s2_bwd_f32(P(z), P(dy), P(dz), 1, 0, 8, S), L.frcnn_subsample2_bwd_f32(None, P(dz), 1, 5, 8, S),
           L.frcnn_subsample2_bwd_f32(P(dy), None, 1, 5, 8, S), L.frcnn_subsample2_bwd_f32(P(dy), P(dz), 1, 5, 0, S)]
    assert all(v == -1 for v in bad), bad
    m.synchronize()
    for t in (y, dz, mean, rstd, dg, db):
        assert (host(rt, t) == 7.0).all()                                                            # nothing was launched
    assert fwd() == 0 and bwd() == 0


# ------------------------------------------------------------------------------------------------------------------ trunk level
def trunk_reference(params, x, blocks, dtype, cot=None, masks=None, prefix="trunk/"):
    """The train-mode trunk (models/resnet.py:41-45 -> ResNetLayers with test=False) restated with torch-CPU in `dtype`, after O.resnet_forward:
    BatchNormalization on batch statistics everywhere.  masks: {conv link path: bool map} IMPOSED in place of every ReLU's own (y = pre * mask,
    so forward and backward both follow the given mask); None: free-running ReLUs.  -> dict(res5, conv1 (the pool's input), masks (this pass's
    own pre > 0), grads {key below the prefix: Chainer-layout array} of sum(res5 * cot) when a cotangent is given)."""
    import torch
    F = torch.nn.functional
    leaves, own = {}, {}

    def P(key):
        if key not in leaves:
            leaves[key] = torch.from_numpy(np.ascontiguousarray(params[prefix + key])).to(dtype).requires_grad_(True)
        return leaves[key]

    def act(pre, name):
        own[name] = (pre.detach() > 0).numpy()
        return torch.relu(pre) if masks is None else pre * torch.from_numpy(np.ascontiguousarray(masks[name])).to(dtype)

    def conv_bn(h, conv, bn, stride=1, pad=0):
        z = F.conv2d(h, P(conv + "/W"), P(conv + "/b") if (prefix + conv + "/b") in params else None, stride=stride, padding=pad)
        return F.batch_norm(z, None, None, P(bn + "/gamma"), P(bn + "/beta"), training=True, eps=BN_EPS)

    h = act(conv_bn(torch.from_numpy(x).to(dtype), "conv1", "bn1", 2, 3), "conv1")
    conv1 = h
    h = F.max_pool2d(h, 3, 2, ceil_mode=True)
    for (stage, stride), n in zip([("res2", 1), ("res3", 2), ("res4", 2), ("res5", 2)], blocks):
        for i in range(n):
            q = "%s/%s/" % (stage, "a" if i == 0 else "b%d" % i)
            s = stride if i == 0 else 1
            sc = conv_bn(h, q + "conv4", q + "bn4", s) if i == 0 else h
            t = act(conv_bn(h, q + "conv1", q + "bn1", s), q + "conv1")
            t = act(conv_bn(t, q + "conv2", q + "bn2", 1, 1), q + "conv2")
            h = act(conv_bn(t, q + "conv3", q + "bn3") + sc, q + "conv3")
    out = dict(res5=h.detach().numpy(), conv1=conv1.detach().numpy(), masks=own)
    if cot is not None:
        (h * torch.from_numpy(cot).to(dtype)).sum().backward()
        out["grads"] = {k: v.grad.numpy() for k, v in leaves.items()}
    return out


def pool_windows_separated(conv1, rel=1e-4):
    """no 3x3/2 (cover_all) window of the map has its two largest DISTINCT positive values within `rel` of each other: the pool's routing cannot
    hinge on a rounding"""
    import torch
    F = torch.nn.functional
    t = torch.from_numpy(np.ascontiguousarray(conv1, dtype=np.float64))
    H, W = t.shape[2:]
    OH, OW = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    t = F.pad(t, (0, 2 * OW + 1 - W, 0, 2 * OH + 1 - H), value=0.0)                      # post-ReLU map: a 0 never is a positive runner-up
    w = F.unfold(t.transpose(0, 1), 3, stride=2).transpose(1, 2).reshape(-1, 9).numpy()   # (C * windows, 9)
    v1 = w.max(1)
    v2 = np.where(w < v1[:, None], w, -np.inf).max(1)
    both = v2 > 0
    return bool(np.all((v1[both] - v2[both]) > rel * v1[both]))


def trunk_case(rt, blocks, im_h, im_w, seed=2, base_width=NARROW):
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import ResNet
    params = synthetic.resnet_params(seed=seed, blocks=blocks, base_width=base_width)
    rs = np.random.RandomState(seed + 50)
    params["trunk/conv1/b"] = (rs.randn(base_width) * 0.1).astype(np.float32)           # chainer's ResNetLayers creates conv1 WITH a bias
    x = synthetic.image(seed=6, h=im_h, w=im_w) / 64.0
    model = ResNet(runtime=rt, blocks=blocks, base_width=base_width)
    model.load_params(params)
    model.train = True
    return params, x, model


MASK_FLIP_CAP = 8
# (blocks, image height, width, parameter seed).  res5 is 3 x 4 in the first case (m = 12 in the last BatchNormalizations); the second has odd
# maps, a `b` block and ragged pool edges.  The seeds are the first ones (of synthetic.resnet_params, image seed 6) at which the float64 conv1
# map has no pool window whose two largest distinct positive values lie within 1e-4 of each other -- with ~40 000 windows per case about one
# seed in a thousand (96 x 128) / in a hundred (75 x 110) -- so that the pool's routing cannot hinge on a rounding (check_trunk asserts it).
TRUNK_CASES = [((1, 1, 1, 1), 96, 128, 2744), ((2, 1, 2, 1), 75, 110, 170)]


def check_trunk(rt, blocks, im_h, im_w, seed=2, base_width=NARROW):
    """Forward and backward of the train-mode trunk against the float64 restatement with the device's ReLU masks imposed.
    -> (device res5 error, worst device gradient error, the torch-fp32 restatement's worst error): all max-abs normalised."""
    import torch
    from chainer_faster_rcnn_amd.models.resnet import conv_specs, unpack_w
    params, x, model = trunk_case(rt, blocks, im_h, im_w, seed, base_width)
    col = {}
    res5 = host(rt, model(dev(rt, x), collect=col))
    cot = np.random.RandomState(seed + 7).randn(*res5.shape).astype(np.float32)
    g = model.backward(dev(rt, cot))
    specs = conv_specs(blocks, base_width)
    got = {}
    for conv, bn, ci, co, k in specs:
        got[conv + "/W"] = unpack_w(host(rt, g[conv + "/W"]), co, ci, k)
        got[bn + "/gamma"], got[bn + "/beta"] = host(rt, g[bn + "/gamma"]), host(rt, g[bn + "/beta"])
    got["conv1/b"] = host(rt, g["conv1/b"])
    masks = {name: host(rt, y) > 0 for name, (z, y) in col.items() if not name.endswith("conv4")}
    free64 = trunk_reference(params, x, blocks, torch.float64)
    free32 = trunk_reference(params, x, blocks, torch.float32)
    flips_dev = sum(int((masks[n] != free64["masks"][n]).sum()) for n in masks)
    flips_32 = sum(int((free32["masks"][n] != free64["masks"][n]).sum()) for n in masks)
    print("trunk %s %dx%d: ReLU mask elements differing from the free float64 pass: device %d, torch-fp32 %d" % (blocks, im_h, im_w, flips_dev, flips_32))
    assert flips_dev <= MASK_FLIP_CAP and flips_32 <= MASK_FLIP_CAP, (flips_dev, flips_32)
    arb = trunk_reference(params, x, blocks, torch.float64, cot, masks)
    r32 = trunk_reference(params, x, blocks, torch.float32, cot, masks)
    assert pool_windows_separated(arb["conv1"])
    assert set(got) == set(arb["grads"]), set(got) ^ set(arb["grads"])
    e32 = max([_nerr(r32["res5"], arb["res5"])] + [_nerr(r32["grads"][k], arb["grads"][k]) for k in got if k != "conv1/b"])
    e_fwd = _nerr(res5, arb["res5"])
    e_grad = {k: _nerr(got[k], arb["grads"][k]) for k in got if k != "conv1/b"}
    worst = max(e_grad, key=e_grad.get)
    print("trunk %s %dx%d: device res5 %.3e, worst gradient %.3e (%s); torch-fp32 worst %.3e (res5 %.3e); device / (4 x fp32) = %.3f"
          % (blocks, im_h, im_w, e_fwd, e_grad[worst], worst, e32, _nerr(r32["res5"], arb["res5"]), max(e_fwd, e_grad[worst]) / (4 * e32)))
    assert e_fwd <= 4 * e32, (e_fwd, e32)
    for k, e in e_grad.items():
        assert e <= 4 * e32, (k, e, e32)
    # non-vacuity: every gradient is there; conv1/b sits in front of a BatchNormalization, its gradient is analytically 0
    for k in e_grad:
        assert _maxabs(arb["grads"][k]) > 1e-3 and _maxabs(got[k]) > 1e-3, k
    assert _maxabs(got["conv1/b"]) <= 1e-3 * _maxabs(got["conv1/W"]) and _maxabs(arb["grads"]["conv1/b"]) <= 1e-3 * _maxabs(arb["grads"]["conv1/W"])
    return e_fwd, e_grad[worst], e32


# ------------------------------------------------------------------------------------------------------------------ trainer level
TRAINER_BLOCKS, TRAINER_HW = (1, 1, 1, 1), (128, 160)          # res5 and the RPN maps are 4 x 5


def trainer_params(seed=2, blocks=TRAINER_BLOCKS, mid=64, n_anchors=9):
    """synthetic.resnet_params (no conv1/b: O.resnet_forward, the arbiter of the inference check, has none) + an RPN on res5's 2048 channels"""
    from chainer_faster_rcnn_amd import synthetic
    p = synthetic.resnet_params(seed=seed, blocks=blocks, base_width=NARROW)
    rs = np.random.RandomState(seed + 1)
    cin = 32 * NARROW
    p["RPN/rpn_conv_3x3/W"] = (rs.randn(mid, cin, 3, 3) * np.sqrt(2.0 / (cin * 9))).astype(np.float32)
    p["RPN/rpn_conv_3x3/b"] = (rs.randn(mid) * 0.01).astype(np.float32)
    for name, n in (("rpn_cls_score", 2 * n_anchors), ("rpn_bbox_pred", 4 * n_anchors)):
        p["RPN/%s/W" % name] = (rs.randn(n, mid, 1, 1) * 0.05).astype(np.float32)
        p["RPN/%s/b" % name] = (rs.randn(n) * 0.01).astype(np.float32)
    return p


def build_model(rt, params, blocks=TRAINER_BLOCKS, **kw):
    import functools
    from chainer_faster_rcnn_amd.models import FasterRCNN, ResNet
    model = FasterRCNN(trunk_class=functools.partial(ResNet, blocks=blocks, base_width=NARROW), rpn_in_ch=32 * NARROW, rpn_mid_ch=64, feat_stride=32,
                       anchor_scales=(1, 2, 3), runtime=rt, **kw)
    model.trunk.load_params(params, "trunk/")
    model.RPN.load_params(params, "RPN/")
    model.rpn_train = True
    return model


def trainer_inputs(seed=0):
    import optimizer_cases as OC
    return OC.rpn_inputs(seed, *TRAINER_HW)


def make_trainer(rt, params=None, **kw):
    from chainer_faster_rcnn_amd.train import RPNTrainer
    return RPNTrainer(build_model(rt, params if params is not None else trainer_params()), **kw)


def fill_grads(tr, inputs, seed):
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    x, gt, info = inputs
    np.random.seed(seed)
    out = tr.forward_backward(Variable(x), Variable(info), Variable(gt))
    tr.all_reduce()
    return out


def expected_keys(blocks=TRAINER_BLOCKS, conv1_bias=False):
    """Chainer's link paths and shapes of everything the optimizer moves"""
    from chainer_faster_rcnn_amd.models.resnet import conv_specs
    want = {}
    for conv, bn, ci, co, k in conv_specs(blocks, NARROW):
        want["trunk/%s/W" % conv] = (co, ci, k, k)
        want["trunk/%s/gamma" % bn] = want["trunk/%s/beta" % bn] = (co,)
    if conv1_bias:
        want["trunk/conv1/b"] = (NARROW,)
    want.update({"RPN/rpn_conv_3x3/W": (64, 32 * NARROW, 3, 3), "RPN/rpn_conv_3x3/b": (64,), "RPN/rpn_cls_score/W": (18, 64, 1, 1),
                 "RPN/rpn_cls_score/b": (18,), "RPN/rpn_bbox_pred/W": (36, 64, 1, 1), "RPN/rpn_bbox_pred/b": (36,)})
    return want


def check_trainer_rule(rt, rule, steps=2):
    """Each step: the device's own G copied out, the NumPy restatement of the rule applied (optimizer_cases.Witness; MomentumSGD + WeightDecay:
    O.momentum_sgd_wd), and W and the state arenas equal it bit for bit.  Also: the loss is finite, every gradient segment is filled, the
    trunk's arrays are windows of the arena, and grads_chainer_layout() speaks Chainer's paths."""
    import optimizer_cases as OC
    from oracle import frcnn_oracle as O
    tr = make_trainer(rt, **({} if rule == "MomentumSGD" else {"opt": rule}))
    assert tr.opt == rule and tr.weight_decay == (0.0005 if rule == "MomentumSGD" else 0.0)
    inputs = trainer_inputs()
    if rule == "MomentumSGD":
        w, v = host(rt, tr.W).copy(), np.zeros(tr.n_flat, np.float32)
    else:
        wit = OC.Witness(rule, host(rt, tr.W), wd=tr.weight_decay, **OC.trainer_hyper(tr))
    for it in range(steps):
        out = fill_grads(tr, inputs, 11 + it)
        loss = tr.losses_host(out)
        assert np.isfinite(loss["rpn_loss"]) and loss["rpn_loss"] > 0, loss
        g = host(rt, tr.G).copy()
        if it == 0:
            got = tr.grads_chainer_layout()
            want = expected_keys()
            assert set(got) == set(want), set(got) ^ set(want)
            for k in want:
                assert got[k].shape == want[k] and np.isfinite(got[k]).all() and np.abs(got[k]).max() > 0, k
        tr.update()
        if rule == "MomentumSGD":
            w, v = O.momentum_sgd_wd(w, g, v)
            OC.assert_same_bits(host(rt, tr.W), w, "MomentumSGD W step %d" % it)
            OC.assert_same_bits(host(rt, tr.V), v, "MomentumSGD v step %d" % it)
        else:
            wit.step(g)
            OC.compare_trainer(rt, tr, wit, "resnet %s step %d" % (rule, it))
    assert tr.iteration == steps
    seg = tr.seg["res3/a/conv4/W"]
    assert np.array_equal(host(rt, tr.model.trunk.tp["res3/a/conv4/W"]).reshape(-1), host(rt, tr.W)[seg.offset:seg.offset + seg.size])
    return tr


def check_snapshot_resume(rt, tmp_path, n=3, k=2):
    """k steps + save + load into a fresh trainer built on OTHER parameters + one step == n uninterrupted steps, bit for bit: W, the velocities
    and the running statistics (saved as the BatchNormalization links' persistents, not as parameters: no optimizer state goes with them)."""
    from chainer_faster_rcnn_amd.serializers import load_trainer_npz, save_trainer_npz
    inputs = trainer_inputs()

    def run(tr, first, last):
        for it in range(first, last):
            fill_grads(tr, inputs, 40 + it)
            tr.update()
    a = make_trainer(rt)
    run(a, 0, n)
    b = make_trainer(rt)
    run(b, 0, k)
    path = str(tmp_path / "resnet_snapshot")
    save_trainer_npz(path, b)
    with np.load(path) as f:
        keys = set(f.files)
    M, Opt = "updater/model:main/", "updater/optimizer:main/"
    assert {M + q for q in expected_keys()} <= keys and {Opt + q + "/v" for q in expected_keys()} <= keys
    assert {M + "trunk/bn1/avg_mean", M + "trunk/res5/a/bn4/avg_var"} <= keys
    assert not any(q.startswith(Opt) and "/avg_" in q for q in keys)
    c = load_trainer_npz(path, make_trainer(rt, params=trainer_params(seed=3)))
    assert c.iteration == k
    run(c, k, n)
    assert np.array_equal(host(rt, a.W).view(np.uint32), host(rt, c.W).view(np.uint32))
    assert np.array_equal(host(rt, a.V).view(np.uint32), host(rt, c.V).view(np.uint32))
    ta, tc = a.model.trunk, c.model.trunk
    for q in ta.persistent_keys():
        assert np.array_equal(host(rt, ta.tp[q]).view(np.uint32), host(rt, tc.tp[q]).view(np.uint32)), q
    return a


def check_inference_after_training(rt, tr):
    """model.rpn_train = False after training: the test-mode forward (BN folded from the trained parameters and the moved running statistics)
    equals O.resnet_forward on the synced parameters within check_resnet's 1e-3."""
    from oracle import frcnn_oracle as O
    from chainer_faster_rcnn_amd import synthetic
    model = tr.model
    before = trainer_params()
    model.rpn_train = False
    assert model.trunk.train is False
    params = model.trunk.params_host("trunk/")
    assert not np.array_equal(params["trunk/bn1/avg_mean"], before["trunk/bn1/avg_mean"]) and not np.array_equal(params["trunk/conv1/W"], before["trunk/conv1/W"])
    x = synthetic.image(seed=6, h=TRAINER_HW[0], w=TRAINER_HW[1]) / 64.0
    want = O.resnet_forward(params, x, blocks=TRAINER_BLOCKS)
    got = host(rt, model.trunk(dev(rt, x)))
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)
    print("inference after training: res5 rel err %.2e" % err)
    assert got.shape == want.shape and err < 1e-3 and np.abs(want).max() > 1e-3, err
    stale = O.resnet_forward(before, x, blocks=TRAINER_BLOCKS)
    assert np.abs(stale - want).max() / np.abs(want).max() > 10 * 1e-3                              # the re-fold is what made it pass
    model.rpn_train = True


def check_call_returns_loss(rt):
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    model = build_model(rt, trainer_params())
    x, gt, info = trainer_inputs()
    np.random.seed(5)
    loss = model(Variable(x), Variable(info), Variable(gt))
    val = float(np.asarray(rt.mem.to_numpy(loss.data) if rt.mem.is_array(loss.data) else loss.data))
    assert np.isfinite(val) and val > 0, val


def check_trainer_refusals(rt):
    import pytest
    from chainer_faster_rcnn_amd.models import ResNet
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    params = trainer_params()
    for math in ("split", "bf16", "f16"):
        with pytest.raises(ValueError, match="ResNet"):
            RPNTrainer(build_model(rt, params), conv_math=math)
    with pytest.raises(ValueError, match="ResNet"):
        RCNNTrainer(build_model(rt, params))
    with pytest.raises(ValueError, match="base_width"):
        ResNet(runtime=rt, base_width=16)
    trunk16 = ResNet(runtime=rt, blocks=TRAINER_BLOCKS, conv_dtype="bf16")
    trunk16.train = True
    with pytest.raises(ValueError, match="fp32"):
        trunk16(dev(rt, np.zeros((1, 3, 32, 32), np.float32)))


def check_vgg_trainer_unaffected(rt):
    """A default VGG RPNTrainer: no adapter, the arena is exactly its conv links + the heads in forward order, its gradients are the oracle's
    (train_cases.check_small_step) and three default steps are MomentumSGD + WeightDecay on the device's own gradients, bit for bit."""
    import optimizer_cases as OC
    import train_cases as TC
    from oracle import frcnn_oracle as O
    TC.check_small_step(rt)
    tr = OC.make_trainer(rt, "rpn")
    assert tr.resnet is None and [n for n, _ in tr.convs] == ["conv1_1", "conv2_1", "conv2_2", "rpn_conv_3x3"]
    keys, off = [], 0
    for name, link in tr.convs:
        keys += [(name + "/W", tuple(link.Wp.shape)), (name + "/b", tuple(link.b.shape))]
    wp, bp, _ = tr.model.RPN._heads_packed
    keys += [("heads/W", tuple(wp.shape)), ("heads/b", tuple(bp.shape))]
    assert list(tr.seg) == [q for q, _ in keys]
    for q, shape in keys:
        assert (tr.seg[q].offset, tr.seg[q].shape) == (off, tuple(int(s) for s in shape)), q
        off += (int(np.prod(shape)) + 63) // 64 * 64
    assert tr.n_flat == off and tuple(tr.zero_bias.shape) == (512,) and sorted(tr.wd) == ["conv2_1", "conv2_2", "rpn_conv_3x3"]
    inputs = OC.trainer_inputs(rt, "rpn")
    w, v = host(rt, tr.W).copy(), np.zeros(tr.n_flat, np.float32)
    for it in range(3):
        OC.forward_backward(tr, "rpn", inputs, 30 + it)
        g = host(rt, tr.G).copy()
        tr.update()
        w, v = O.momentum_sgd_wd(w, g, v)
        OC.assert_same_bits(host(rt, tr.W), w, "VGG W step %d" % it)
        OC.assert_same_bits(host(rt, tr.V), v, "VGG v step %d" % it)
