"""The ResNet trunk's bf16 train-mode pass on the MI355X: the three 1x1 training entries of csrc/conv1x1_train_bf16.hip at the emulator's shapes and at
one shape per layer class of the real network, a narrow train_dtype="bf16" trunk checked layer by layer, both trainers on such a model, and 50 RPN
steps against the fp32 trunk's (tests/resnet16_train_cases.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet16_train_cases as C  # noqa: E402
import resnet_train_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

_ID = lambda s: "x".join(str(v) for v in s)  # noqa: E731


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("shape", C.EMU_SHAPES + C.REAL_SHAPES, ids=_ID)
def test_entries_against_float64(rt, shape):
    C.check_float64(rt, *shape)


@pytest.mark.parametrize("shape", C.EMU_SHAPES + C.REAL_SHAPES, ids=_ID)
def test_entries_exact_at_every_split(rt, shape):
    C.check_exact(rt, *shape)


def test_entry_refusals(rt):
    C.check_refusals(rt)


@pytest.mark.parametrize("case", T.TRUNK_CASES, ids=lambda c: "%s_%dx%d" % ("".join(str(b) for b in c[0]), c[1], c[2]))
def test_trunk_layer_by_layer(rt, case):
    C.check_trunk(rt, *case)


def test_train_dtype_f32_is_the_unchanged_pass(rt):
    C.check_f32_unchanged(rt, *T.TRUNK_CASES[0])


def test_constructor_refusals(rt):
    C.check_constructor_refusals(rt)


def test_rpn_trainer_one_step(rt):
    C.check_rpn_step(rt)


def test_rcnn_trainer_one_step(rt):
    C.check_rcnn_step(rt)


def test_resume_and_inference_after_training(rt, tmp_path):
    C.check_resume_and_inference(rt, tmp_path)


def test_pinned_trainer_refusals(rt):
    C.check_pinned_refusals(rt)


def test_fifty_rpn_steps_against_the_fp32_trunk(rt):
    C.check_loss_curves(rt)
