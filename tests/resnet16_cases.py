"""Parity checks of the ResNet trunk's 16-bit pieces (csrc/resnet_bf16.hip / resnet_f16.hip), written once and run on the host emulator
(tests/test_resnet16_emulated.py) and on the MI355X (tests/test_gpu_resnet16.py).  Every check feeds the oracle the kernel's exact operands
(inputs, weights and residuals rounded to the current 16-bit format) and allows one rounding of the stored output; pooling and im2col are
bit-exact."""
import numpy as np

from oracle import frcnn_oracle as O
from chainer_faster_rcnn_amd import tuning
from parity_cases import _HALF, blocked_to_hwc, dev, from_bf16_bits, host, to_bf16


def rounding_unit():
    """relative size of one rounding to nearest in the current 16-bit format"""
    return 2.0 ** -11 if _HALF[-1] == "f16" else 2.0 ** -8


def blocked(rt, a):
    """(1, C, H, W) fp32 -> the runtime's blocked 16-bit map (one rounding: the operands the kernels see)"""
    return rt.bf16_from_nchw(dev(rt, np.ascontiguousarray(a, dtype=np.float32)))


def widened(rt, a_blk, C):
    """blocked 16-bit map -> (1, C, H, W) fp32 on the host, exact"""
    return from_bf16_bits(blocked_to_hwc(host(rt, a_blk)))[:, :, :C].transpose(2, 0, 1)[None].copy()


def conv1x1_want(xw, w, b, stride, act, rw=None):
    """the oracle on the kernel's operands: xw (1,Cin,H,W) and w (Cout,Cin,1,1) already rounded, rw the widened residual"""
    want = O.conv2d(np.ascontiguousarray(xw[:, :, ::stride, ::stride]), w, b, 0)
    if act == 3:
        want = want + rw
    return O.relu(want) if act in (1, 3) else want


def assert_one_rounding(got, want, what=""):
    scale = max(float(np.abs(want).max()), 1e-6)
    err = np.abs(got - want)
    bound = np.abs(want) * rounding_unit() + 2e-5 * scale
    assert np.all(err <= bound), (what, float((err / scale).max()))
    return float((err / scale).max())


def check_conv1x1(rt, Cin, Cout, H, W, stride=1, act=1, seed=0, split=None, expect_split=None):
    """frcnn_conv1x1_bf16 against O.conv2d on its exact operands: the stored value within one rounding of the fp32-accumulated value
    (+ 2e-5 of the scale for the summation order), padding channels zero.  `split` forces the K split through the tuning registry."""
    rs = np.random.RandomState(seed)
    x = np.abs(rs.randn(1, Cin, H, W)).astype(np.float32)
    w = (rs.randn(Cout, Cin, 1, 1) * np.sqrt(2.0 / Cin)).astype(np.float32)
    b = (rs.randn(Cout) * 0.1).astype(np.float32)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    r = rs.randn(1, Cout, Ho, Wo).astype(np.float32)
    xd, rd = blocked(rt, x), blocked(rt, r)
    wpk = rt.bf16_pack_conv_w(dev(rt, w), 1)
    ctx = tuning.override(FRCNN_C1_SPLIT=str(split)) if split else _nothing()
    with ctx:
        if expect_split is not None:
            assert rt.conv1x1_bf16_splits(Cin, Cout, H, W, stride) == expect_split
        y = host(rt, rt.conv1x1_bf16(xd, wpk, dev(rt, b), Cin, Cout, stride=stride, act=act, residual=rd if act == 3 else None))
    assert y.shape == (rt.bf16_pad(Cout) // 16, Ho, Wo, 16), y.shape
    got = from_bf16_bits(blocked_to_hwc(y))
    assert not got[:, :, Cout:].any()
    want = conv1x1_want(widened(rt, xd, Cin), to_bf16(w)[0], b, stride, act, widened(rt, rd, Cout) if act == 3 else None)
    return assert_one_rounding(got[:, :, :Cout], want[0].transpose(1, 2, 0), "conv1x1 %d->%d %dx%d s%d act%d" % (Cin, Cout, H, W, stride, act))


class _nothing(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def check_conv1x1_split_deterministic(rt, Cin, Cout, H, W, stride=1, split=4, seed=1):
    """a forced K split gives the same words on two launches (partials summed in split order) and stays within one rounding of the
    unsplit launch's value"""
    rs = np.random.RandomState(seed)
    x = np.abs(rs.randn(1, Cin, H, W)).astype(np.float32)
    w = (rs.randn(Cout, Cin, 1, 1) * np.sqrt(2.0 / Cin)).astype(np.float32)
    b = dev(rt, (rs.randn(Cout) * 0.1).astype(np.float32))
    xd, wpk = blocked(rt, x), rt.bf16_pack_conv_w(dev(rt, w), 1)
    with tuning.override(FRCNN_C1_SPLIT=str(split)):
        assert rt.conv1x1_bf16_splits(Cin, Cout, H, W, stride) == split
        a = host(rt, rt.conv1x1_bf16(xd, wpk, b, Cin, Cout, stride=stride, act=0))
        c = host(rt, rt.conv1x1_bf16(xd, wpk, b, Cin, Cout, stride=stride, act=0))
    with tuning.override(FRCNN_C1_SPLIT="1"):
        one = host(rt, rt.conv1x1_bf16(xd, wpk, b, Cin, Cout, stride=stride, act=0))
    assert np.array_equal(a, c)
    ga, g1 = from_bf16_bits(blocked_to_hwc(a)), from_bf16_bits(blocked_to_hwc(one))
    assert np.all(np.abs(ga - g1) <= np.abs(g1) * 2 * rounding_unit() + 2e-5 * np.abs(g1).max())


def check_maxpool3x3s2_16(rt, C, H, W, seed=0):
    """bit-exact against torch max_pool2d(3, 2, ceil_mode=True) of the widened map (a maximum of 16-bit values is one of them)"""
    import torch
    rs = np.random.RandomState(seed)
    xd = blocked(rt, rs.randn(1, C, H, W).astype(np.float32))
    y = host(rt, rt.maxpool3x3s2_bf16(xd))
    want = torch.nn.functional.max_pool2d(torch.from_numpy(widened(rt, xd, C)), 3, 2, ceil_mode=True).numpy()
    got = from_bf16_bits(blocked_to_hwc(y))
    assert got.shape[:2] == want.shape[2:], (got.shape, want.shape)
    assert np.array_equal(got[:, :, :C], want[0].transpose(1, 2, 0)) and not got[:, :, C:].any()
    # and what the fp32 kernel gives on the widened map
    assert np.array_equal(got[:, :, :C], host(rt, rt.maxpool3x3s2(dev(rt, widened(rt, xd, C))))[0].transpose(1, 2, 0))


def check_im2col7x7s2_16(rt, H, W, Kp=160, seed=0):
    """bit-exact against unfold of the rounded image, zero rows past 147"""
    import torch
    rs = np.random.RandomState(seed)
    x = (rs.uniform(0, 255, (1, 3, H, W)) - 120).astype(np.float32)
    cols = host(rt, rt.im2col7x7s2_bf16(dev(rt, x), Kp))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert cols.shape == (Kp // 16, Ho, Wo, 16), cols.shape
    want = torch.nn.functional.unfold(torch.from_numpy(to_bf16(x)[0]), 7, padding=3, stride=2).numpy().reshape(147, Ho, Wo)
    got = from_bf16_bits(blocked_to_hwc(cols))
    assert np.array_equal(got[:, :, :147], want.transpose(1, 2, 0)) and not got[:, :, 147:].any()


def resnet_case(rt, blocks, im_h, im_w, n_layers=101, seed=2):
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import ResNet
    params = synthetic.resnet_params(n_layers, seed=seed, blocks=blocks)
    x = synthetic.image(seed=6, h=im_h, w=im_w) / 64.0
    model = ResNet(n_layers, runtime=rt, blocks=blocks, conv_dtype="bf16")
    model.load_params(params)
    return params, x, model


def folded(params, conv, bn, prefix="trunk/", eps=2e-5):
    """the BN-folded fp32 (W, b) of one convolution, as models/resnet.py folds them"""
    gamma, beta, mean, var = [np.asarray(params[prefix + bn + "/" + n], np.float64) for n in ("gamma", "beta", "avg_mean", "avg_var")]
    s = gamma / np.sqrt(var + eps)
    if (prefix + conv + "/b") in params:
        mean = mean - np.asarray(params[prefix + conv + "/b"], np.float64)
    return (np.asarray(params[prefix + conv + "/W"], np.float64) * s[:, None, None, None]).astype(np.float32), (beta - mean * s).astype(np.float32)


def check_resnet16_layers(rt, blocks, im_h, im_w, n_layers=101, seed=2, tol_res5=None):
    """A 16-bit trunk checked LAYER BY LAYER: each layer's device output against the oracle applied to the device's own input of that layer
    (one rounding), then the end-to-end res5 against O.resnet_forward (fp32) within `tol_res5` of the feature scale.  Returns that error."""
    import torch
    from chainer_faster_rcnn_amd.models.resnet import STAGES, block_names
    params, x, model = resnet_case(rt, blocks, im_h, im_w, n_layers, seed)
    col = {}
    feat = host(rt, model(dev(rt, x), collect=col))
    W = lambda name: widened(rt, *col[name])                                  # noqa: E731
    # stem: conv1 on the rounded image (7x7/2 pad 3), bn folded, relu
    w1, b1 = folded(params, "conv1", "bn1")
    want = O.relu(torch.nn.functional.conv2d(torch.from_numpy(to_bf16(x)[0]), torch.from_numpy(to_bf16(w1)[0]), torch.from_numpy(b1),
                                             stride=2, padding=3).numpy())
    errs = {"conv1": assert_one_rounding(W("conv1"), want, "conv1")}
    want = torch.nn.functional.max_pool2d(torch.from_numpy(W("conv1")), 3, 2, ceil_mode=True).numpy()
    assert np.array_equal(W("pool1"), want)
    h = "pool1"
    for (stage, _, _, _, stride), n in zip(STAGES, blocks):
        for b in block_names(n):
            p = "%s/%s/" % (stage, b)
            s = stride if b == "a" else 1
            xin = W(h)
            if b == "a":
                w4, b4 = folded(params, p + "conv4", p + "bn4")
                errs[p + "conv4"] = assert_one_rounding(W(p + "conv4"), conv1x1_want(xin, to_bf16(w4)[0], b4, s, 0), p + "conv4")
            wc, bc = folded(params, p + "conv1", p + "bn1")
            errs[p + "conv1"] = assert_one_rounding(W(p + "conv1"), conv1x1_want(xin, to_bf16(wc)[0], bc, s, 1), p + "conv1")
            wc, bc = folded(params, p + "conv2", p + "bn2")
            want = O.relu(O.conv2d(W(p + "conv1"), to_bf16(wc)[0], bc, 1))
            errs[p + "conv2"] = assert_one_rounding(W(p + "conv2"), want, p + "conv2")
            wc, bc = folded(params, p + "conv3", p + "bn3")
            short = W(p + "conv4") if b == "a" else xin
            errs[p + "conv3"] = assert_one_rounding(W(p + "conv3"), conv1x1_want(W(p + "conv2"), to_bf16(wc)[0], bc, 1, 3, short), p + "conv3")
            h = p + "conv3"
    assert np.array_equal(feat, W(h))                                          # res5 as fp32 NCHW: the widened blocked map, exactly
    want = O.resnet_forward(params, x, blocks=blocks)
    assert feat.shape == want.shape, (feat.shape, want.shape)
    err = float(np.abs(feat - want).max() / max(np.abs(want).max(), 1e-6))
    assert np.abs(want).max() > 1e-3 and np.isfinite(feat).all()
    if tol_res5 is not None:
        assert err < tol_res5, err
    return err, errs


def resnet101_layer_shapes(im_h=600, im_w=1000):
    """every distinct (Cin, Cout, H, W, stride, act) of the 1x1 layers of ResNet-101 (and its stem as a 1x1 on 160 columns) at im_h x im_w"""
    from chainer_faster_rcnn_amd.models.resnet import STAGES
    h, w = (im_h - 1) // 2 + 1, (im_w - 1) // 2 + 1
    out = [(160, 64, h, w, 1, 1)]
    h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    for stage, cin, mid, cout, stride in STAGES:
        out.append((cin, cout, h, w, stride, 0))                               # conv4 (block a)
        out.append((cin, mid, h, w, stride, 1))                                # conv1 (block a)
        if stride == 2:
            h, w = (h + 1) // 2, (w + 1) // 2
        out.append((mid, cout, h, w, 1, 3))                                    # conv3
        out.append((cout, mid, h, w, 1, 1))                                    # conv1 (blocks b*)
    return sorted(set(out), key=out.index)
