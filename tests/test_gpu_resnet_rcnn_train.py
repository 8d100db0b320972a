"""Stage-2 training of a ResNet model on the MI355X: RoI pooling and the fc6-shaped L.Linear backward at the shapes the wiring brings (a 2048-channel
stride-32 map up to 19 x 32, K = 100 352), the whole step against the float64 arbiter of tests/resnet_rcnn_train_cases.py, every update rule,
snapshots and resume, inference after training, the rpn -> rcnn -> rpn alternation, the model call and the refusals."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_rcnn_train_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("R_", R.ROI_COUNTS)
@pytest.mark.parametrize("hw", R.ROI_MAPS, ids=lambda s: "%dx%d" % s)
def test_roi_pool_c2048_stride32(rt, hw, R_):
    R.check_roi_shapes(rt, hw[0], hw[1], R_)


@pytest.mark.parametrize("shape", R.FC6_SHAPES + R.FC6_SHAPES_SMALL, ids=lambda s: "M%d_N%d_K%d" % s)
def test_fc6_backward(rt, shape):
    R.check_fc6_backward(rt, *shape)


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: "%s_%dx%d" % ("".join(str(b) for b in c[0]), c[1], c[2]))
def test_step_against_float64(rt, case):
    R.check_step(rt, case)


@pytest.mark.parametrize("rule", ["MomentumSGD", "Adam", "AdaGrad", "RMSprop"])
def test_trainer_rule(rt, rule):
    R.check_trainer_rule(rt, rule)


def test_snapshot_resume_and_inference(rt, tmp_path):
    tr = R.check_snapshot_resume(rt, tmp_path)              # three steps on the uninterrupted trainer
    R.check_inference_after_training(rt, tr)


@pytest.mark.parametrize("rule", ["Adam", "AdaGrad", "RMSprop"])
def test_snapshot_resume_rule(rt, tmp_path, rule):
    R.check_snapshot_resume(rt, tmp_path, rule)


def test_alternation_rpn_rcnn_rpn(rt):
    R.check_alternation(rt)


def test_call_returns_rcnn_loss(rt):
    R.check_model_call(rt)


def test_refusals(rt):
    R.check_refusals(rt)
