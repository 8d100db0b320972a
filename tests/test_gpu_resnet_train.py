"""The trainable ResNet trunk on the MI355X: train-mode BatchNormalization and the glue adjoints (csrc/bn_train.hip) at every shape of
tests/resnet_train_cases.py, the train-mode trunk's forward and backward against the float64 restatement, and RPNTrainer on a ResNet model
(every update rule, snapshots, inference after training, the refusals)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_train_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("flags", T.BN_FLAGS, ids=lambda f: "relu%d_res%d_run%d_dres%d" % f)
@pytest.mark.parametrize("shape", T.BN_SHAPES + [T.BN_SHAPE_PARTS_EMU, T.BN_SHAPE_PARTS_GPU], ids=lambda s: "%dx%d" % s)
def test_bn_train(rt, shape, flags):
    print("BN_RATIO %s %s %.3f" % (shape, flags, T.check_bn(rt, shape[0], shape[1], *flags)))


def test_bn_train_cancellation(rt):
    T.check_bn_cancellation(rt)


@pytest.mark.parametrize("shape", T.POOL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_glue_bwd(rt, shape):
    T.check_glue_bwd(rt, *shape)


def test_refusals(rt):
    T.check_refusals(rt)


@pytest.mark.parametrize("case", T.TRUNK_CASES, ids=lambda c: "%s_%dx%d" % ("".join(str(b) for b in c[0]), c[1], c[2]))
def test_trunk_forward_backward(rt, case):
    print("TRUNK_ERR %s fwd %.3e grad %.3e torch-fp32 %.3e" % ((case,) + T.check_trunk(rt, *case)))


@pytest.mark.parametrize("rule", ["MomentumSGD", "Adam", "AdaGrad", "RMSprop"])
def test_trainer_rule(rt, rule):
    T.check_trainer_rule(rt, rule)


def test_trainer_snapshot_resume_and_inference(rt, tmp_path):
    tr = T.check_snapshot_resume(rt, tmp_path)              # three steps on the uninterrupted trainer
    T.check_inference_after_training(rt, tr)


def test_call_returns_rpn_loss(rt):
    T.check_call_returns_loss(rt)


def test_trainer_refusals(rt):
    T.check_trainer_refusals(rt)


def test_vgg_trainer_unaffected(rt):
    T.check_vgg_trainer_unaffected(rt)
