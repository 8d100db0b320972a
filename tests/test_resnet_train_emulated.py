"""The trainable ResNet trunk on the host emulator (tests/hipemu): train-mode BatchNormalization forward / backward and the adjoints of the two
glue kernels (csrc/bn_train.hip) at the shapes where their paths change, and a narrow trunk's forward and backward against the float64
restatement of tests/resnet_train_cases.py."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import resnet_train_cases as T  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


# res5's real shape runs two flag combinations here (each flag on and off); all four on the GPU
BN_CASES = [(s, f) for s in T.BN_SHAPES + [T.BN_SHAPE_PARTS_EMU] for f in T.BN_FLAGS if s != (2048, 608) or f in (T.BN_FLAGS[1], T.BN_FLAGS[3])]


@pytest.mark.parametrize("shape,flags", BN_CASES, ids=lambda v: "x".join(str(i) for i in v))
def test_bn_train(rt, shape, flags):
    T.check_bn(rt, shape[0], shape[1], *flags)


def test_bn_train_cancellation(rt):
    T.check_bn_cancellation(rt)


@pytest.mark.parametrize("shape", T.POOL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_glue_bwd(rt, shape):
    T.check_glue_bwd(rt, *shape)


def test_refusals(rt):
    T.check_refusals(rt)


@pytest.mark.parametrize("case", T.TRUNK_CASES, ids=lambda c: "%s_%dx%d" % ("".join(str(b) for b in c[0]), c[1], c[2]))
def test_trunk_forward_backward(rt, case):
    T.check_trunk(rt, *case)


def test_trainer_refusals(rt):
    T.check_trainer_refusals(rt)


def test_trainer_one_step_momentum_sgd(rt):
    T.check_trainer_rule(rt, "MomentumSGD", steps=1)


def test_vgg_trainer_unaffected(rt):
    T.check_vgg_trainer_unaffected(rt)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import numpy as np
        from emu_runtime import emu_runtime
        from chainer_faster_rcnn_amd.train import TorchComm
        rt = emu_runtime()
        tr = T.make_trainer(rt, comm=TorchComm())
        assert len(tr.buckets) > 1                                    # the tail buckets are launched from inside the trunk's backward pass
        own = T.make_trainer(rt)                                      # the same replica without a communicator: this rank's own gradient
        inputs = T.trainer_inputs(seed=rank)                          # every rank its own image
        T.fill_grads(own, inputs, 7 + rank)
        T.fill_grads(tr, inputs, 7 + rank)
        g_own, g_sum = rt.mem.to_numpy(own.G).copy(), rt.mem.to_numpy(tr.G).copy()
        tr.update()
        stats = rt.mem.to_numpy(tr.model.trunk.tp["bn1/avg_mean"]).copy()
        q.put((rank, g_own, g_sum, rt.mem.to_numpy(tr.W).copy(), stats))
    finally:
        dist.destroy_process_group()


def test_data_parallel_gloo_world2():
    """Two ranks over gloo, one step, each on its own image: the all-reduced gradient buffer is the same on both ranks and is the sum of the two
    ranks' own gradients (every bucket was launched after its last gradient), the updated parameters are equal, the running statistics are
    each rank's own."""
    import numpy as np
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
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


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc (cross-compiles without a GPU)")
def test_bn_train_kernel_listings(tmp_path):
    """bn_train.hip for gfx950 with the product's flags: no private segment (no spills), LDS only for the two reduction arrays of the statistics
    kernels, at most 128 registers (four or more waves per SIMD), and the maps move as 16-byte vectors."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "chainer-faster-rcnn_amd", "csrc")
    asm = str(tmp_path / "bn_train.s")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(root, "include"),
                    "-I", csrc, os.path.join(csrc, "bn_train.hip"), "-o", asm], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(kernels) == 13, [k for k, _ in kernels]               # 1 + 4 forward, 2 + 4 backward, the two glue adjoints
    for name, body in kernels:
        field = lambda n: int(re.search(r"\.%s\s+(\d+)" % n, body).group(1))     # noqa: E731
        assert field("amdhsa_private_segment_fixed_size") == 0, name
        assert field("amdhsa_group_segment_fixed_size") == (4096 if "stats" in name else 0), name
        assert field("amdhsa_next_free_vgpr") <= 128, name
    assert "scratch_" not in text
    assert text.count("global_load_dwordx4") >= 13 and text.count("global_store_dwordx4") >= 8
