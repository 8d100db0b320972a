"""Stage-2 training of a ResNet model on the host emulator (tests/hipemu): RoI pooling with arg-max and its backward on the 2048-channel stride-32 maps
of the two test trunks, the L.Linear backward's four paths, and on the (1, 1, 1, 1) trunk the step against the float64 arbiter, the update rule,
snapshot and resume, inference after training, the alternation, the model call and the refusals of tests/resnet_rcnn_train_cases.py; two gloo
ranks.  The emulator runs a step of this model in about half a minute, so the GPU suite keeps what only costs time here: the 19 x 32 map, two of the
four K = 100 352 shapes, the second trunk, the resume of the three other rules and the model call's comparison with an independent trainer."""
import os
import socket
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import resnet_rcnn_train_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


@pytest.mark.parametrize("R_", R.ROI_COUNTS)
@pytest.mark.parametrize("hw", R.ROI_MAPS[:2], ids=lambda s: "%dx%d" % s)
def test_roi_pool_c2048_stride32(rt, hw, R_):
    R.check_roi_shapes(rt, hw[0], hw[1], R_)


@pytest.mark.parametrize("shape", R.FC6_SHAPES_SMALL + [R.FC6_SHAPES[0], R.FC6_SHAPES[3]], ids=lambda s: "M%d_N%d_K%d" % s)
def test_linear_backward_paths(rt, shape):
    R.check_fc6_backward(rt, *shape)


def test_step_against_float64(rt):
    R.check_step(rt, R.STEP_CASES[0])


@pytest.mark.parametrize("rule", ["MomentumSGD", "Adam", "AdaGrad", "RMSprop"])
def test_trainer_rule(rt, rule):
    R.check_trainer_rule(rt, rule)


def test_snapshot_resume_and_inference(rt, tmp_path):
    tr = R.check_snapshot_resume(rt, tmp_path)              # two steps + save + load + one step against three; inference after those three
    R.check_inference_after_training(rt, tr)


def test_alternation_rpn_rcnn_rpn(rt):
    R.check_alternation(rt)


def test_call_returns_rcnn_loss(rt):
    R.check_model_call(rt, independent=False)


def test_refusals(rt):
    R.check_refusals(rt)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import optimizer_cases as OC
        import resnet_train_cases as T
        from emu_runtime import emu_runtime
        from chainer_faster_rcnn_amd.train import TorchComm
        rt = emu_runtime()
        tr = R.make_trainer(rt, comm=TorchComm())
        assert len(tr.buckets) > 1 and tr.buckets[0][0] == "fc6"      # the head's bucket, then tail buckets launched from inside the trunk's backward pass

        class Quiet(object):                                          # no exchange (`active` False), but this rank's dropout stream: the masks fold the rank in
            active = False
        Quiet.rank = rank
        own = R.make_trainer(rt, comm=Quiet())                        # the same replica: this rank's own gradient
        inputs = OC.rpn_inputs(R.STEP_CASES[0][4] + 13 * rank, *T.TRAINER_HW)      # every rank its own image
        R.fill_grads(own, inputs, 7 + rank)
        R.fill_grads(tr, inputs, 7 + rank)
        g_own, g_sum = rt.mem.to_numpy(own.G).copy(), rt.mem.to_numpy(tr.G).copy()
        tr.update()
        stats = rt.mem.to_numpy(tr.model.trunk.tp["bn1/avg_mean"]).copy()
        q.put((rank, g_own, g_sum, rt.mem.to_numpy(tr.W).copy(), stats))
    finally:
        dist.destroy_process_group()


def test_data_parallel_gloo_world2():
    """Two ranks over gloo, one step, each on its own image: the all-reduced gradient buffer is the same on both ranks and is the sum of the two
    ranks' own gradients (every bucket -- the head's, and those ResNet.backward's `ready` callbacks close -- was launched after its last
    gradient), the updated parameters are equal, the running statistics are each rank's own (they are not all-reduced)."""
    import numpy as np
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:                                   # a port the system hands out: no scheme shared with the other world-2 tests
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    (_, own0, sum0, w0, s0), (_, own1, sum1, w1, s1) = res
    assert np.array_equal(sum0.view(np.uint32), sum1.view(np.uint32)) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    assert np.array_equal(sum0, own0 + own1) and np.abs(own0 - own1).max() > 0
    assert not np.array_equal(s0, s1)
