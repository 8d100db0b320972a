"""Adam / AdaGrad / RMSprop (csrc/optimizer.hip, RPNTrainer / RCNNTrainer(opt=...)) on the host-emulated kernels (CPU): the unmodified
kernel source against the NumPy restatement of optimizer_cases.py bit for bit -- sizes around every vector / tail / grid-stride edge,
three pointer alignments, edge values, the loss scaler's skip, the refusals -- then both trainers under every rule, the fp16 step's
skipped update, snapshots, the API, data parallel over gloo, and the gfx950 listing of the new code object."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import optimizer_cases as C  # noqa: E402
import train_cases as T  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "chainer-faster-rcnn_amd", "csrc")


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


def test_lr_t_rule_within_one_ulp_of_chainer():
    C.check_lr_t_rule_against_chainer()


@pytest.mark.parametrize("wd", [0.0, 0.0005])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_sizes_and_alignments(rt, rule, scaled, wd):
    C.check_sizes_and_alignments(rt, rule, scaled, wd)


@pytest.mark.parametrize("rule", C.RULES)
def test_kernel_second_trip_and_tail(rt, rule):
    """The emulated chip has 3 CUs: one full trip is 24 workgroups, 98 304 floats on the 16-byte path."""
    assert C.cu_count(rt) <= 8
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


@pytest.mark.parametrize("kind,kw", [("rpn", {}), ("rpn", dict(conv_math="f16", loss_scale=dict(init_scale=2.0 ** 10)))], ids=["rpn-fp32", "rpn-f16"])
def test_adam_snapshot_resume(rt, tmp_path, kind, kw):
    C.check_snapshot_resume(rt, kind, tmp_path, **kw)


def test_snapshot_of_another_rule_is_refused(rt, tmp_path):
    C.check_snapshot_rule_mismatch(rt, tmp_path)


def test_chainer_snapshot_fixture_loads_into_a_default_trainer_only(rt):
    """tests/golden/chainer_trainer_snapshot_small.npz (MomentumSGD velocities) loads into a default trainer exactly as before, and an Adam
    trainer refuses it."""
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


def test_default_trainer_is_momentum_sgd_with_weight_decay(rt):
    """(RCNNTrainer: the GPU suite, where three steps of it take no time.)"""
    C.check_default_is_momentum_sgd(rt, "rpn")


def test_readoption_keeps_the_moments(rt):
    C.check_readoption_keeps_moments(rt)


def _dp_adam_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, os.path.join(HERE, "hipemu")); sys.path.insert(0, HERE)
        from emu_runtime import emu_runtime
        from chainer_faster_rcnn_amd.chainer_compat import Variable
        from chainer_faster_rcnn_amd.train import RPNTrainer, TorchComm
        import parity_cases as P
        rt = emu_runtime()
        params = T.small_params()
        info = np.array([[40, 56]], dtype=np.int32)

        def sample(i):
            rs = np.random.RandomState(100 + i)
            gt = P.gt_case(rs, 2, 40, 56)
            gt[0, :, 2] = np.minimum(gt[0, :, 0] + 20, 55); gt[0, :, 3] = np.minimum(gt[0, :, 1] + 20, 39)
            return rs.randn(1, 3, 40, 56).astype(np.float32), gt
        tr = RPNTrainer(T.build_small(rt, params), comm=TorchComm(), opt="Adam")
        wit = C.Witness("Adam", rt.mem.to_numpy(tr.W))
        ok = True
        for it in range(2):                                           # rank r takes image 2 * it + r; the all-reduce precedes the update
            x, gt = sample(2 * it + rank)
            np.random.seed(5 + 2 * it + rank)
            tr.forward_backward(Variable(x), Variable(info), Variable(gt))
            tr.all_reduce()
            g = rt.mem.to_numpy(tr.G).copy()                          # the summed gradient: the same on both ranks
            tr.update()
            wit.step(g)
            ok = ok and np.array_equal(rt.mem.to_numpy(tr.W).view(np.uint32), wit.w.view(np.uint32))
        sums = [float(np.abs(rt.mem.to_numpy(a)).astype(np.float64).sum()) for a in (tr.W, tr.moments["m"], tr.moments["v"])]
        q.put((rank, bool(ok), sums, tr.opt_state.state()["t"]))
    finally:
        dist.destroy_process_group()


def test_data_parallel_adam_gloo_world2():
    """Two ranks over gloo, two Adam steps: every rank applies the same rule to the same sums -- parameters and both moments are equal
    across ranks (and equal the restatement applied to the summed gradient)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_adam_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _, _ in res), res
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3] == 2
    assert all(s > 0 for s in res[0][2])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_optimizer_kernel_listings(tmp_path):
    """optimizer.hip for gfx950 with the product's flags: every kernel's metadata shows no private segment, no spills and no LDS; the
    16-byte path of each rule is there, and it moves 16-byte vectors."""
    asm = str(tmp_path / "optimizer.s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(CSRC, "optimizer.hip"), "-o", asm], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)
    names = [k for k, _ in kernels]
    assert sum("opt_update_kernel" in k for k in names) == 6 and any("opt_state_advance_kernel" in k for k in names) \
        and any("opt_state_init_kernel" in k for k in names), names
    for k, meta in kernels:
        field = lambda n: int(re.search(r"\.amdhsa_%s\s+(\d+)" % n, meta).group(1))     # noqa: E731
        assert field("private_segment_fixed_size") == 0, k + ": scratch in use"
        assert field("group_segment_fixed_size") == 0, k + ": LDS in use"
    # the per-kernel metadata records (YAML at the end of the listing): one spill pair per kernel, all zero
    sg = [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)]
    vg = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    assert len(sg) == len(vg) == len(kernels) and not any(sg) and not any(vg), (sg, vg)
    assert "scratch_" not in text
    for rule in (1, 2, 3):
        m = re.search(r"^(_ZN\S*opt_update_kernelILi%dEDv4_f\S*):.*?\n(.*?)^\.Lfunc_end" % rule, text, re.S | re.M)
        assert m, rule
        body = m.group(2)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, rule
