"""bf16 mixed-precision RPN training (RPNTrainer(conv_math="bf16")) on the MI355X: the new kernels at every VGG-16 layer shape of the
600 x 1000 step, the VGG-16 step at 160 x 224 and 600 x 1000 under the CPU suite's bars, determinism of the full-size step, and a
50-step run against the fp32 step from the same initialisation."""
import numpy as np
import pytest

import bf16_train_cases as B
import parity_cases as P
import train_cases as T

pytestmark = pytest.mark.gpu

# (cin, cout, H, W) of every 3x3 convolution of the 600 x 1000 step (forward shapes; the input-gradient launches swap cin / cout)
VGG_SHAPES = [(64, 64, 600, 1000), (64, 128, 300, 500), (128, 128, 300, 500), (128, 256, 150, 250), (256, 256, 150, 250),
              (256, 512, 75, 125), (512, 512, 75, 125), (512, 512, 38, 63), (128, 64, 600, 1000), (512, 256, 75, 125)]


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("cin,cout,h,w", VGG_SHAPES)
def test_conv3x3_bf16_train_vgg_shapes(rt, cin, cout, h, w):
    B.check_conv3x3_bf16_train(rt, cin, cout, h, w, seed=cin + cout, sample=(6, 5))


@pytest.mark.parametrize("cin,cout,h,w", [(3, 64, 600, 1000)] + [s for s in VGG_SHAPES if s[0] <= s[1]])
def test_conv_wgrad_bf16_vgg_shapes(rt, cin, cout, h, w):
    B.check_conv_wgrad_bf16(rt, cin, cout, h, w, seed=cin)


def test_conv1_bf16_train_full_size(rt):
    B.check_conv1_bf16_train(rt, 3, 64, 600, 1000)


def test_bf16_pack_many_vgg(rt):
    B.check_bf16_pack_many(rt, dims=((64, 64), (256, 512), (512, 512), (3, 64)))


def _vgg(seed=0, im_h=160, im_w=224):
    from chainer_faster_rcnn_amd import synthetic
    rs = np.random.RandomState(seed)
    params = synthetic.params(seed=1)
    for k in list(params):
        if k.endswith("/b") and (k.startswith("trunk/") or k.startswith("RPN/")):
            params[k] = (rs.randn(*params[k].shape) * 0.01).astype(np.float32)
    x = synthetic.image(seed=4, h=im_h, w=im_w)
    gt = P.gt_case(rs, 4, im_h, im_w)
    info = np.array([[im_h, im_w]], dtype=np.int32)
    return params, x, gt, info


def _build(rt, params):
    from chainer_faster_rcnn_amd.models import FasterRCNN
    model = FasterRCNN(runtime=rt)
    model.load_params(params)
    model.rpn_train = True
    return model


@pytest.mark.parametrize("im_h,im_w", [(160, 224), (600, 1000)])
def test_vgg_rpn_step_bf16(rt, im_h, im_w):
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    params, x, gt, info = _vgg(im_h=im_h, im_w=im_w)
    # given_tol 3e-2 (the narrow trunk: 1e-2): the float64 pass under the device's decisions still carries exact activations, while the
    # device's carry one bf16 operand rounding (2^-9) per layer through 14 layers -- measured 1.4e-2 on the heads at 160 x 224
    loss, worst, table, flips = B.check_step_bf16(rt, params, _build, LAYERS, x, gt, info, 16, (8, 16, 32), seed=11, given_tol=3e-2)
    print("vgg bf16 step %dx%d: loss %.6g worst vs fp32 %.3g, flips %s" % (im_h, im_w, loss, worst, flips))


def test_vgg_rpn_step_bf16_deterministic_full_size(rt):
    params, x, gt, info = _vgg(im_h=600, im_w=1000)
    B.check_step_deterministic(rt, params, _build, x, gt, info)


def test_vgg_rpn_bf16_training_curve(rt):
    """50 steps at 160 x 224 from one initialisation, bf16 against fp32 with the same seeds: both losses fall, and every bf16 loss stays
    within 5 % (+ 0.01) of the fp32 loss of the same step."""
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.train import RPNTrainer
    params, x, gt, info = _vgg()
    curves = {}
    for cm in ("mfma", "bf16"):
        tr = RPNTrainer(_build(rt, params), conv_math=cm)
        ls = []
        for it in range(50):
            np.random.seed(100 + it)
            out = tr.step(Variable(x), Variable(info), Variable(gt))
            ls.append(tr.losses_host(out)["rpn_loss"])
        curves[cm] = np.array(ls)
    f, b = curves["mfma"], curves["bf16"]
    print("\nBF16_CURVE %s" % T.json_dumps({"fp32": [float("%.5g" % v) for v in f], "bf16": [float("%.5g" % v) for v in b]}))
    for c in (f, b):
        assert np.all(np.isfinite(c)) and c[-5:].mean() < c[:5].mean()
    assert np.all(np.abs(b - f) <= 0.05 * np.abs(f) + 0.01), np.abs(b - f).max()
