"""Adam / AdaGrad / RMSprop (csrc/optimizer.hip, RPNTrainer / RCNNTrainer(opt=...)) on the MI355X, through the C ABI: the kernels against the
NumPy restatement of optimizer_cases.py BIT FOR BIT (so this is also the measurement of the device's `/`, sqrtf and double sqrt being
correctly rounded under the product's flags, and of subnormals being kept) -- every size / alignment / value edge, a second trip of the
real launch, the loss scaler's skip, the refusals -- then both trainers on the narrow model under every rule, the fp16 step's skipped
update, snapshots and the API."""
import os

import numpy as np
import pytest

import optimizer_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F16 = dict(conv_math="f16", loss_scale=dict(init_scale=2.0 ** 10))


@pytest.fixture(scope="module")
def rt():
    import chainer_faster_rcnn_amd as pkg
    return pkg.runtime.default_runtime()


@pytest.mark.parametrize("wd", [0.0, 0.0005])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_sizes_and_alignments(rt, rule, scaled, wd):
    C.check_sizes_and_alignments(rt, rule, scaled, wd)


@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_second_trip_and_tail(rt, rule):
    """One full trip of the launch on 256 CUs is 2048 workgroups: 8.4 M floats on the 16-byte path."""
    C.check_second_trip(rt, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_zero_gradient_keeps_w(rt, rule):
    C.check_zero_gradient_keeps_w(rt, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_overflowing_square(rt, rule):
    C.check_overflowing_square(rt, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_skip_keeps_every_bit(rt, rule):
    C.check_skip(rt, rule)


@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_scaled_equals_unscaled(rt, rule):
    C.check_scaled_equals_unscaled(rt, rule)


def test_refusals(rt):
    C.check_refusals(rt)


@pytest.mark.parametrize("rule", C.RULES)
@pytest.mark.parametrize("kind", ["rpn", "rcnn"])
def test_trainer_rule(rt, kind, rule):
    C.check_trainer_rule(rt, kind, rule)


def test_trainer_schedule_and_weight_decay(rt):
    C.check_trainer_schedule_and_weight_decay(rt)


@pytest.mark.parametrize("kind", ["rpn", "rcnn"])
def test_trainer_f16_adam_skips_and_resumes_at_t1(rt, kind):
    C.check_trainer_f16_skip(rt, kind)


# (RCNNTrainer's fp32 step scatters RoI gradients with float atomics: two runs of it are compared under the 16-bit steps, whose scatter is ordered)
@pytest.mark.parametrize("kind,kw", [("rpn", {}), ("rpn", F16), ("rcnn", dict(conv_math="bf16")), ("rcnn", F16)], ids=["rpn-fp32", "rpn-f16", "rcnn-bf16", "rcnn-f16"])
def test_adam_snapshot_resume(rt, tmp_path, kind, kw):
    C.check_snapshot_resume(rt, kind, tmp_path, **kw)


def test_snapshot_of_another_rule_is_refused(rt, tmp_path):
    C.check_snapshot_rule_mismatch(rt, tmp_path)


def test_chainer_snapshot_fixture_loads_into_a_default_trainer_only(rt):
    from chainer_faster_rcnn_amd.serializers import load_trainer_npz
    src = os.path.join(HERE, "golden", "chainer_trainer_snapshot_small.npz")
    with np.load(src) as f:
        want = {k: f[k] for k in f.files}
    tr = load_trainer_npz(src, C.make_trainer(rt, "rpn"))
    assert tr.iteration == 37 and tr.opt == "MomentumSGD"
    w, v = tr.flat_to_chainer_layout(tr.W), tr.flat_to_chainer_layout(tr.V)
    for k in w:
        assert np.array_equal(w[k], want["updater/model:main/" + k]), k
        assert np.array_equal(v[k], want["updater/optimizer:main/" + k + "/v"]), k
    with pytest.raises(ValueError):
        load_trainer_npz(src, C.make_trainer(rt, "rpn", opt="Adam"))


def test_api(rt):
    C.check_api(rt)


@pytest.mark.parametrize("kind", ["rpn", "rcnn"])
def test_default_trainer_is_momentum_sgd_with_weight_decay(rt, kind):
    C.check_default_is_momentum_sgd(rt, kind, **(dict(conv_math="bf16") if kind == "rcnn" else {}))


def test_readoption_keeps_the_moments(rt):
    C.check_readoption_keeps_moments(rt)
