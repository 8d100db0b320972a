"""fp16 mixed-precision RPN training (RPNTrainer(conv_math="f16")) and its device-side loss scaler on the host-emulated kernels (CPU): the
fp16 twins of the one-part training kernels against float64 with RNE-fp16 imposed on their operands, fp16's range behaviour, why the scale
exists, the scaler's entries against a plain-Python state machine, the narrow-trunk step (40 x 56), overflow handling, resume, data
parallel over gloo, the refusals, and the gfx950 listings of the new code objects."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import f16_train_cases as F  # noqa: E402
import parity_cases as P  # noqa: E402
import train_cases as T  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "chainer-faster-rcnn_amd", "csrc")


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


@pytest.mark.parametrize("cin,cout,h,w,relu", [(16, 64, 9, 37, True), (48, 80, 5, 30, False), (17, 33, 3, 65, True), (64, 64, 1, 1, True)])
def test_conv3x3_f16_train(rt, cin, cout, h, w, relu):
    F.check_conv3x3_train(rt, cin, cout, h, w, relu=relu, seed=cin)


def test_conv3x3_f16_train_split_k(rt):
    F.check_conv3x3_train_split_k(rt, 192, 64, 5, 33)


@pytest.mark.parametrize("cin,cout,h,w", [(3, 64, 11, 40), (64, 64, 7, 33), (20, 70, 4, 65), (130, 16, 5, 9)])
def test_conv_wgrad_f16(rt, cin, cout, h, w):
    F.check_conv_wgrad(rt, cin, cout, h, w, seed=cin)


@pytest.mark.parametrize("cin,cout,h,w", [(3, 64, 11, 70), (3, 21, 5, 9), (1, 64, 4, 64)])
def test_conv1_f16_train(rt, cin, cout, h, w):
    F.check_conv1_train(rt, cin, cout, h, w, seed=cout)


def test_f16_pack_many(rt):
    F.check_pack_many(rt)


def test_f16_differs_from_bf16(rt):
    """The fp16 entries really compute in fp16: same inputs, different bits from the bf16 twins, and closer to the unrounded float64."""
    rs = np.random.RandomState(1)
    x = np.maximum(rs.randn(1, 32, 6, 33), 0).astype(np.float32)
    dy = (rs.randn(1, 32, 6, 33) * 1e-2).astype(np.float32)
    want = F.wgrad64(x, dy, 32, 32)
    e = {h: F.rel(P.host(rt, rt.with_half(h).conv_wgrad_bf16(P.dev(rt, x), P.dev(rt, dy))), want) for h in ("bf16", "f16")}
    assert e["f16"] < e["bf16"] / 2, e


def test_f16_range_behaviour(rt):
    F.check_range_behaviour(rt)


def test_why_the_scale_exists(rt):
    F.check_why_the_scale_exists(rt)


def test_kernel_scale_invariance(rt):
    F.check_kernel_scale_invariance(rt)


def test_loss_scaler_entries(rt):
    F.check_loss_scaler_entries(rt)


def test_small_rpn_step_f16(rt):
    """The narrow-trunk step under the bf16 step's bars: weight gradients within 1e-4 of float64 on their kept pairs with fp16 rounding
    imposed, the loss within 1e-2 of the fp32 oracle's, every unscaled gradient within 1e-2 of the float64 pass under the device's own
    decisions, the update bit for bit momentum_sgd_wd(W, G / S, V)."""
    params, x, gt, info = F.small_case(rt)
    F.check_step(rt, params, T.build_small, T.SMALL_LAYERS, x, gt, info, 4, (2, 4, 8))


def test_small_rpn_step_f16_flips_fewer_decisions_than_bf16(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_fewer_flips_than_bf16(rt, params, T.build_small, T.SMALL_LAYERS, x, gt, info, 4, (2, 4, 8))


def test_small_rpn_step_f16_scale_invariance(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_step_scale_invariance(rt, params, T.build_small, x, gt, info)


def test_small_rpn_step_f16_deterministic(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_step_deterministic(rt, params, T.build_small, x, gt, info)


def test_small_rpn_step_f16_overflow_handling(rt):
    params, x, gt, info = F.small_case(rt)
    F.check_overflow_handling(rt, params, T.build_small, x, gt, info)


def test_small_rpn_step_f16_resume(rt, tmp_path):
    params, x, gt, info = F.small_case(rt)
    F.check_resume(rt, params, T.build_small, T.small_params(seed=5), x, gt, info, tmp_path)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from emu_runtime import emu_runtime
        from chainer_faster_rcnn_amd.chainer_compat import Variable
        from chainer_faster_rcnn_amd.train import RPNTrainer, TorchComm
        rt = emu_runtime()
        params, x, gt, info = F.small_case(rt, seed=rank)
        tr = RPNTrainer(T.build_small(rt, T.small_params()), comm=TorchComm(), conv_math="f16", loss_scale=dict(init_scale=2.0 ** 10))
        w0 = rt.mem.to_numpy(tr.W)
        np.random.seed(5 + rank)
        tr.forward_backward(Variable(x), Variable(info), Variable(gt))
        tr.all_reduce()                                            # drain the buckets launched during the backward pass, then poison ONE rank
        if rank == 1:
            g = rt.mem.to_numpy(tr.G)
            g[11] = np.inf
            tr.G[...] = rt.mem.from_numpy(g)
        tr.comm.all_reduce_sum(tr.G)                               # the exchange the update decides on: Inf + finite = Inf on both ranks
        tr.update()
        st = tr.loss_scaler.state()
        skipped = bool(np.array_equal(rt.mem.to_numpy(tr.W), w0))
        np.random.seed(9 + rank)
        tr.step(Variable(x), Variable(info), Variable(gt))         # a clean step: both ranks update identically
        import hashlib
        q.put((rank, skipped, st["scale"], st["skipped_steps"], hashlib.sha1(rt.mem.to_numpy(tr.W).tobytes()).hexdigest(),
               bool(not np.array_equal(rt.mem.to_numpy(tr.W), w0)), tr.loss_scaler.state()["scale"]))
    finally:
        dist.destroy_process_group()


def test_data_parallel_overflow_on_one_rank_skips_on_both():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for rank, skipped, scale, nskip, _, moved, scale2 in res:
        assert skipped and scale == 2.0 ** 9 and nskip == 1 and moved and scale2 == 2.0 ** 9, res
    assert res[0][4] == res[1][4], res                             # parameters stay equal across ranks


def test_api_refusals(rt):
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    params = T.small_params()
    for cm in ("mfma", "split", "bf16"):
        with pytest.raises(ValueError):
            RPNTrainer(T.build_small(rt, params), conv_math=cm, loss_scale="dynamic")
    for bad in (3.0, 0.0, -4.0, "static", float("inf")):
        with pytest.raises(ValueError):
            RPNTrainer(T.build_small(rt, params), conv_math="f16", loss_scale=bad)
    with pytest.raises(ValueError):
        RPNTrainer(T.build_small(rt, params), conv_math="f16", loss_scale=dict(growth=3.0))
    with pytest.raises(ValueError):
        RPNTrainer(T.build_small(rt, params), conv_math="f16x")
    with pytest.raises((ValueError, AssertionError)):
        RCNNTrainer(T.build_small(rt, params), conv_math="f16")
    tr = RPNTrainer(T.build_small(rt, params), conv_math="f16")
    st = tr.loss_scaler.state()
    assert tr.loss_scaler.dynamic and (st["scale"], st["good_steps"], st["skipped_steps"], st["overflow_steps"], st["found_nonfinite"]) == (2.0 ** 16, 0, 0, 0, 0)
    assert not RPNTrainer(T.build_small(rt, params), conv_math="f16", loss_scale=256.0).loss_scaler.dynamic


# ---- gfx950 listings of the new code objects (hipcc -S cross-compiles without a GPU): the bf16 twins' budgets, nothing in scratch
NEW_KERNELS = {
    "conv_f32s_f16": [("conv_f32s_kernelILi4ELi0ELi1ELi1E", 26 * 1024 + 4, 128), ("conv1_f32s_kernelILi2ELb0ELb1ELb0E", None, None),
                      ("conv1_f32s_kernelILi1ELb0ELb1ELb0E", None, None), ("pack_w_f32s_many_kernelILi1E", 0, None),
                      ("conv1_f32s_kernelILi2ELb0ELb0ELb0E", None, None), ("conv1_f32s_kernelILi1ELb0ELb0ELb0E", None, None)],   # (y_nchw == NULL)
    "train_f16": [("conv_wgrad_f32s_kernelILi1E", 64 * (5 * 96 + 16) + 64 * (3 * 64 + 16), 336), ("wgrad_reduce_kernel", 0, None)],
    "loss_scale": [("grad_check_finite_kernel", 4, None), ("sgd_momentum_wd_scaled_kernel", 0, None), ("loss_scaler_update_kernel", 0, None),
                   ("scale_by_loss_scale_kernel", 0, None), ("loss_scaler_init_kernel", 0, None)],
}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("src", sorted(NEW_KERNELS))
def test_new_kernel_listings(src, tmp_path):
    from test_bf16_train_emulated import _kernel_meta

    def listing(name):
        asm = str(tmp_path / (name + ".s"))
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, os.path.join(CSRC, name + ".hip"), "-o", asm], check=True, stderr=subprocess.DEVNULL)
        return asm
    asm = listing(src)
    meta = _kernel_meta(asm)
    if src.endswith("_f16"):                                        # every fp16 twin within its bf16 twin's register and LDS budget
        twin = _kernel_meta(listing(src[:-4]))
        for k, d in meta.items():
            assert k in twin, k
            assert int(d["vgpr_count"]) <= int(twin[k]["vgpr_count"]) and int(d["group_segment_fixed_size"]) == int(twin[k]["group_segment_fixed_size"]), (
                k, d["vgpr_count"], twin[k]["vgpr_count"])
    txt = open(asm).read()
    wanted = [f for f, _, _ in NEW_KERNELS[src]]
    extra = [k for k in meta if not any(f in k for f in wanted)]
    assert not extra, "kernels that are not fp16 twins were compiled into %s: %s" % (src, extra)
    if src != "loss_scale":
        assert "v_mfma_f32_32x32x16_f16" in txt and "v_mfma_f32_32x32x16_bf16" not in txt and "v_cvt_pk_bf16_f32" not in txt
    for frag, lds, vgprs in NEW_KERNELS[src]:
        hits = [k for k in meta if frag in k]
        assert hits, "%s not in %s.hip" % (frag, src)
        for k in hits:
            d = meta[k]
            assert int(d["private_segment_fixed_size"]) == 0 and int(d.get("vgpr_spill_count", 0)) == 0, (k, d)
            if lds is not None:
                assert int(d["group_segment_fixed_size"]) == lds, (k, d["group_segment_fixed_size"])
            if vgprs is not None:
                assert int(d["vgpr_count"]) <= vgprs, (k, d["vgpr_count"])
