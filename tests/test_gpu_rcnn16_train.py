"""bf16 / fp16 mixed-precision stage-2 training (RCNNTrainer(precision="bf16" / "f16")) on the MI355X: the three L.Linear training kernels and
their fp16 twins at the five full-size shapes of the VGG-16 head (forward at the ProposalLayer's 300 rows, both backward products at 128 and at
300 rows) against float64 with the rounding imposed; the narrow-trunk and VGG-16 steps (160 x 224 and 600 x 1000) under the RPN step's bars;
determinism at full size; the fp16 loss scale; and 30-step runs of the three precisions."""
import numpy as np
import pytest

import rcnn16_train_cases as R
import train_cases as T

pytestmark = pytest.mark.gpu

HALVES = ("bf16", "f16")
FWD = [(300, 4096, 25088), (300, 4096, 4096), (300, 21, 4096), (300, 84, 4096)]                  # fc6, fc7, cls_score, bbox_pred
BWD = [(m, n, k) for m in (128, 300) for (_, n, k) in FWD]


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("M,N,K", FWD)
def test_linear_train_forward_full_size(rt, M, N, K, half):
    R.check_linear_forward(rt, M, N, K, half=half, relu=(N >= 4096), seed=N, sample=(40, 48))


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("M,N,K", BWD)
def test_linear_dgrad_full_size(rt, M, N, K, half):
    R.check_linear_dgrad(rt, M, N, K, half=half, seed=M + N, sample=(40, 64))


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("M,N,K", BWD)
def test_linear_wgrad_full_size(rt, M, N, K, half):
    R.check_linear_wgrad(rt, M, N, K, half=half, seed=M + N, sample=(48, 64))


def test_f16_closer_to_float64_than_bf16(rt):
    R.check_f16_closer_than_bf16(rt, M=128, N=84, K=4096)


@pytest.mark.parametrize("half", HALVES)
def test_linear_split_k_is_bit_identical(rt, half):
    R.check_linear_split_k(rt, 300, 84, 4096, half=half, splits=("2", "3", "8"))


@pytest.mark.parametrize("n_rois,C,H,W", [(37, 6, 9, 13), (1, 1, 1, 1), (128, 512, 38, 63), (300, 512, 38, 63), (64, 16, 100, 120)])
def test_roi_pool_bwd_ordered(rt, n_rois, C, H, W):
    R.check_roi_pool_bwd_ordered(rt, R=n_rois, C=C, H=H, W=W, seed=n_rois + C)


@pytest.mark.parametrize("precision", HALVES)
def test_small_rcnn_step(rt, precision):
    params, x, gt, info = R.small_case(rt)
    R.check_step(rt, params, R.build_small, T.SMALL_LAYERS, x, gt, info, 4, precision, given_tol=1e-2)


@pytest.mark.parametrize("precision", HALVES)
@pytest.mark.parametrize("im_h,im_w", [(160, 224), (600, 1000)])
def test_vgg_rcnn_step(rt, im_h, im_w, precision):
    """VGG-16: the loss within 1e-2 of the oracle's, every weight gradient (13 conv, 4 linear) within 1e-4 of float64 on its own kept pair with
    the rounding imposed, every gradient within 3e-2 (the RPN step's bar for the 13-layer trunk) of the float64 pass under all of the device's
    decisions, the update bit for bit."""
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    params, x, gt, info = R.vgg_case(im_h, im_w)
    R.check_step(rt, params, R.build_vgg, LAYERS, x, gt, info, 16, precision, given_tol=3e-2)


@pytest.mark.parametrize("precision", HALVES)
def test_vgg_rcnn_step_deterministic_full_size(rt, precision):
    params, x, gt, info = R.vgg_case(600, 1000)
    R.check_step_deterministic(rt, params, R.build_vgg, x, gt, info, precision=precision)


def test_rcnn_step_f16_scale_invariance(rt):
    params, x, gt, info = R.vgg_case()
    R.check_scale_invariance(rt, params, R.build_vgg, x, gt, info)


def test_rcnn_step_f16_overflow_handling(rt):
    params, x, gt, info = R.small_case(rt)
    R.check_overflow_handling(rt, params, R.build_small, x, gt, info)
    params, x, gt, info = R.vgg_case()
    R.check_overflow_handling(rt, params, R.build_vgg, x, gt, info)


def test_construction_and_refusals(rt):
    params, _, _, _ = R.small_case(rt)
    R.check_construction(rt, params, R.build_small)


def test_rcnn_step_f16_resume(rt, tmp_path):
    params, x, gt, info = R.small_case(rt)
    other = dict(T.small_params(seed=5))
    other.update(T.small_head_params(np.random.RandomState(9)))
    R.check_resume(rt, params, R.build_small, other, x, gt, info, tmp_path)


def test_vgg_rcnn_training_curves(rt):
    """30 steps at 160 x 224 with device-drawn dropout, fp32 / bf16 / f16 from one initialisation: finite and falling (last-5 mean below first-5 mean)."""
    params, x, gt, info = R.vgg_case()
    R.check_curves(rt, params, R.build_vgg, x, gt, info, steps=30)
