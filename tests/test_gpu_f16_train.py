"""fp16 mixed-precision RPN training (RPNTrainer(conv_math="f16")) and its device-side loss scaler on the MI355X: the fp16 twins of the
training kernels at every VGG-16 layer shape of the 600 x 1000 step, fp16's range behaviour, why the scale exists, the scaler's entries
at the real gradient-buffer size, the narrow-trunk and VGG-16 steps under the bf16 step's bars, fewer flipped decisions than the bf16
step at every size, overflow handling, resume, and 50-step runs against the fp32 step (static scale) and with the dynamic default."""
import numpy as np
import pytest

import f16_train_cases as F
import parity_cases as P
import train_cases as T
from test_gpu_bf16_train import VGG_SHAPES, _build, _vgg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("cin,cout,h,w", VGG_SHAPES)
def test_conv3x3_f16_train_vgg_shapes(rt, cin, cout, h, w):
    F.check_conv3x3_train(rt, cin, cout, h, w, seed=cin + cout, sample=(6, 5))


@pytest.mark.parametrize("cin,cout,h,w", [(3, 64, 600, 1000)] + [s for s in VGG_SHAPES if s[0] <= s[1]])
def test_conv_wgrad_f16_vgg_shapes(rt, cin, cout, h, w):
    F.check_conv_wgrad(rt, cin, cout, h, w, seed=cin)


def test_conv1_f16_train_full_size(rt):
    F.check_conv1_train(rt, 3, 64, 600, 1000)


def test_f16_pack_many_vgg(rt):
    F.check_pack_many(rt, dims=((64, 64), (256, 512), (512, 512), (3, 64)))


def test_conv3x3_f16_train_split_k(rt):
    F.check_conv3x3_train_split_k(rt, 512, 512, 38, 63, splits=("2", "3", "4"))


def test_f16_range_behaviour(rt):
    F.check_range_behaviour(rt)


def test_why_the_scale_exists(rt):
    F.check_why_the_scale_exists(rt)


def test_kernel_scale_invariance(rt):
    F.check_kernel_scale_invariance(rt)
    F.check_kernel_scale_invariance(rt, cin=128, cout=256, h=75, w=125, seed=5)


def test_loss_scaler_entries(rt):
    """The issue's sizes and the gradient buffer of VGG-16 + RPN (about 17.1 M floats)."""
    from chainer_faster_rcnn_amd.train import RPNTrainer
    params, x, gt, info = _vgg()
    n_flat = RPNTrainer(_build(rt, params), conv_math="f16").n_flat
    assert n_flat > 17_000_000
    F.check_loss_scaler_entries(rt, sizes=(1, 63, 64, 65, (1 << 20) + 3, n_flat))


def test_small_rpn_step_f16(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_step(rt, params, T.build_small, T.SMALL_LAYERS, x, gt, info, 4, (2, 4, 8))
    F.check_step_scale_invariance(rt, params, T.build_small, x, gt, info)
    F.check_step_deterministic(rt, params, T.build_small, x, gt, info)


def test_small_rpn_step_f16_flips_fewer_decisions_than_bf16(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_fewer_flips_than_bf16(rt, params, T.build_small, T.SMALL_LAYERS, x, gt, info, 4, (2, 4, 8))


@pytest.mark.parametrize("im_h,im_w", [(160, 224), (600, 1000)])
def test_vgg_rpn_step_f16(rt, im_h, im_w):
    """The bf16 step's bars on the fp16 step (check_step inside the comparison: kernel 1e-4, loss 1e-2, given_tol 3e-2 for the 14-layer
    trunk, the update bit for bit) and, from the same state and seed, fewer flipped ReLU signs / pool winners than the bf16 step."""
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    params, x, gt, info = _vgg(im_h=im_h, im_w=im_w)
    F.check_fewer_flips_than_bf16(rt, params, _build, LAYERS, x, gt, info, 16, (8, 16, 32), seed=11, given_tol=3e-2)


def test_vgg_rpn_step_f16_scale_invariance_and_determinism(rt):
    params, x, gt, info = _vgg()
    F.check_step_scale_invariance(rt, params, _build, x, gt, info, seed=11)
    F.check_step_deterministic(rt, params, _build, x, gt, info)


def test_small_rpn_step_f16_overflow_handling(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_overflow_handling(rt, params, T.build_small, x, gt, info)


def test_small_rpn_step_f16_resume(rt, tmp_path):
    params, x, gt, info = F.small_case(rt)
    F.check_resume(rt, params, T.build_small, T.small_params(seed=5), x, gt, info, tmp_path)


def test_vgg_rpn_f16_training_curve(rt):
    """50 steps at 160 x 224 from one initialisation: fp32 beside fp16 with a STATIC scale of 2^10 (draw is at most 1 / 256 per element, so
    the scaled head gradient is at most 4: no step may be skipped, so that step k of one run is step k of the other) -- both losses fall,
    every fp16 loss within 5 % (+ 0.01) of the fp32 loss of that step.  Beside it the dynamic default: the scale trajectory and the
    skipped steps are printed; the last loss is finite and below the first, and applied updates + skipped steps == 50."""
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.train import RPNTrainer
    params, x, gt, info = _vgg()
    curves, traj, states, updates = {}, [], {}, {}
    for tag, kw in (("fp32", dict(conv_math="mfma")), ("f16_static", dict(conv_math="f16", loss_scale=2.0 ** 10)), ("f16_dynamic", dict(conv_math="f16"))):
        tr = RPNTrainer(_build(rt, params), **kw)
        ls, applied = [], 0
        for it in range(50):
            np.random.seed(100 + it)
            w_before = tr.W.clone()
            out = tr.step(Variable(x), Variable(info), Variable(gt))
            ls.append(tr.losses_host(out)["rpn_loss"])
            applied += int(not bool((w_before == tr.W).all()))      # an applied update moves the weights, a skipped one leaves every bit
            if tag == "f16_dynamic":
                traj.append(tr.loss_scaler.state()["scale"])
        updates[tag] = applied
        curves[tag] = np.array(ls)
        if tr.loss_scaler is not None:
            states[tag] = tr.loss_scaler.state()
    f, s, d = curves["fp32"], curves["f16_static"], curves["f16_dynamic"]
    print("\nF16_CURVE %s" % T.json_dumps({k: [float("%.5g" % v) for v in c] for k, c in curves.items()}))
    print("F16_CURVE dynamic scale trajectory %s state %s; static state %s" % (T.json_dumps(traj), T.json_dumps(states["f16_dynamic"]),
                                                                            T.json_dumps(states["f16_static"])))
    assert states["f16_static"]["skipped_steps"] == 0 and states["f16_static"]["scale"] == 2.0 ** 10
    for c in (f, s):
        assert np.all(np.isfinite(c)) and c[-5:].mean() < c[:5].mean()
    assert np.all(np.abs(s - f) <= 0.05 * np.abs(f) + 0.01), np.abs(s - f).max()
    assert np.isfinite(d[-1]) and d[-1] < d[0]
    st = states["f16_dynamic"]
    assert updates["fp32"] == 50 and updates["f16_static"] == 50
    assert updates["f16_dynamic"] + st["skipped_steps"] == 50 and st["found_nonfinite"] == 0, (updates, st)
