"""bf16 / fp16 mixed-precision stage-2 training (RCNNTrainer(precision="bf16" / "f16")) on the host-emulated kernels (CPU): the three L.Linear
training kernels of csrc/linear_train_bf16.hip and their fp16 twins against float64 with the rounding imposed, on small ragged shapes; the
narrow-trunk step at 48 x 64 under the RPN step's bars; determinism; the fp16 loss scale (scaling, overflow, construction, resume, two ranks
over gloo); the keyword's refusals; and the gfx950 listings of the two new translation units."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
sys.path.insert(0, HERE)
import rcnn16_train_cases as R  # noqa: E402
import train_cases as T  # noqa: E402

ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "chainer-faster-rcnn_amd", "csrc")
HALVES = ("bf16", "f16")
# small and ragged: M in {1, 7, 128, 300}, N in {21, 84, 130}, K in {64, 200 * 16}; one K = 25088 case with M, N <= 32
SHAPES = [(1, 21, 64), (7, 84, 64), (128, 130, 64), (300, 21, 64), (7, 130, 3200), (128, 21, 3200), (300, 84, 3200), (20, 30, 25088)]


@pytest.fixture(scope="module")
def rt():
    from emu_runtime import emu_runtime
    return emu_runtime()


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_train_forward(rt, M, N, K, half):
    R.check_linear_forward(rt, M, N, K, half=half, relu=(M % 2 == 1), seed=M + N)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_dgrad(rt, M, N, K, half):
    R.check_linear_dgrad(rt, M, N, K, half=half, seed=M + N)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_wgrad(rt, M, N, K, half):
    R.check_linear_wgrad(rt, M, N, K, half=half, seed=M + N)


def test_f16_closer_to_float64_than_bf16(rt):
    R.check_f16_closer_than_bf16(rt)


@pytest.mark.parametrize("half", HALVES)
def test_linear_split_k_is_bit_identical(rt, half):
    R.check_linear_split_k(rt, 37, 130, 640, half=half, splits=("2", "3", "5"))


def test_linear_train_refuses_unaligned_k(rt):
    x, w, dy = np.zeros((4, 30), np.float32), np.zeros((8, 30), np.float32), np.zeros((4, 8), np.float32)
    for call in (lambda: rt.linear_bf16_train(x, w, None), lambda: rt.linear_dgrad_bf16(dy, w), lambda: rt.linear_wgrad_bf16(dy, x)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("n_rois,C,H,W", [(37, 6, 9, 13), (1, 1, 1, 1), (130, 5, 38, 63), (9, 2, 50, 60)])
def test_roi_pool_bwd_ordered(rt, n_rois, C, H, W):
    R.check_roi_pool_bwd_ordered(rt, R=n_rois, C=C, H=H, W=W, seed=n_rois + C)


@pytest.mark.parametrize("precision", HALVES)
def test_small_rcnn_step(rt, precision):
    """The narrow trunk at 48 x 64: loss within 1e-2 of the oracle's, every weight gradient within 1e-4 of float64 on its kept pair with the
    rounding imposed, every gradient within 1e-2 of the float64 pass under all of the device's decisions, the update bit for bit."""
    params, x, gt, info = R.small_case(rt)
    R.check_step(rt, params, R.build_small, T.SMALL_LAYERS, x, gt, info, 4, precision, given_tol=1e-2)


@pytest.mark.parametrize("precision", HALVES)
def test_small_rcnn_step_deterministic(rt, precision):
    params, x, gt, info = R.small_case(rt)
    R.check_step_deterministic(rt, params, R.build_small, x, gt, info, precision=precision)


def test_small_rcnn_step_f16_scale_invariance(rt):
    params, x, gt, info = R.small_case(rt)
    R.check_scale_invariance(rt, params, R.build_small, x, gt, info)


def test_small_rcnn_step_f16_overflow_handling(rt):
    params, x, gt, info = R.small_case(rt)
    R.check_overflow_handling(rt, params, R.build_small, x, gt, info)


def test_construction_and_refusals(rt):
    params, _, _, _ = R.small_case(rt)
    R.check_construction(rt, params, R.build_small)


def test_small_rcnn_step_f16_resume(rt, tmp_path):
    params, x, gt, info = R.small_case(rt)
    other = dict(T.small_params(seed=5))
    other.update(T.small_head_params(np.random.RandomState(9)))
    R.check_resume(rt, params, R.build_small, other, x, gt, info, tmp_path)


def test_precision_none_is_the_fp32_step(rt):
    """precision=None leaves the existing step alone: same gradient bits as a trainer built without the keyword."""
    from chainer_faster_rcnn_amd.train import RCNNTrainer
    params, x, gt, info = R.small_case(rt)
    gs = []
    for kw in ({}, dict(precision=None)):
        tr = RCNNTrainer(R.build_small(rt, params), **kw)
        R.run_step(tr, x, gt, info, 0)
        gs.append(rt.mem.to_numpy(tr.G))
    assert np.array_equal(gs[0], gs[1])


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import hashlib
        from emu_runtime import emu_runtime
        from chainer_faster_rcnn_amd.chainer_compat import Variable
        from chainer_faster_rcnn_amd.train import RCNNTrainer, TorchComm
        rt = emu_runtime()
        params, x, gt, info = R.small_case(rt, seed=rank)
        tr = RCNNTrainer(R.build_small(rt, R.small_case(rt)[0]), comm=TorchComm(), precision="f16", loss_scale=dict(init_scale=2.0 ** 10))
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
        q.put((rank, skipped, st["scale"], st["skipped_steps"], hashlib.sha1(rt.mem.to_numpy(tr.W).tobytes()).hexdigest(),
               bool(not np.array_equal(rt.mem.to_numpy(tr.W), w0)), tr.loss_scaler.state()["scale"]))
    finally:
        dist.destroy_process_group()


def test_data_parallel_overflow_on_one_rank_skips_on_both():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for rank, skipped, scale, nskip, _, moved, scale2 in res:
        assert skipped and scale == 2.0 ** 9 and nskip == 1 and moved and scale2 == 2.0 ** 9, res
    assert res[0][4] == res[1][4], res                             # parameters stay equal across ranks


# ---- gfx950 listings of the two new translation units (hipcc -S cross-compiles without a GPU).  DESIGN 3.15: LDS = 2 stages x (32 MT + 128) rows x 128 B;
# a full vmcnt(0) drain once in the prologue and once per chunk where the staged values are deposited (<= 4 in the listing); the forms whose A operand has
# a leading dimension that is no multiple of 4 (cls_score / bbox_pred: 4-byte loads) <= 12.
LDS = {10: 2 * (320 + 128) * 128, 4: 2 * (128 + 128) * 128, 1: 2 * (32 + 128) * 128}
FORMS = [(mt, at, bt) for mt in (10, 4, 1) for at, bt in ((0, 0), (0, 1))] + [(4, 1, 1), (1, 1, 1)]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
@pytest.mark.parametrize("src", ["linear_train_bf16", "linear_train_f16"])
def test_new_kernel_listings(src, tmp_path):
    from test_bf16_train_emulated import _kernel_meta
    from test_isa_waits import full_waits
    asm = str(tmp_path / (src + ".s"))
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, os.path.join(CSRC, src + ".hip"), "-o", asm], check=True, stderr=subprocess.DEVNULL)
    meta, waits, txt = _kernel_meta(asm), full_waits(asm), open(asm).read()
    if src.endswith("_f16"):
        assert "v_mfma_f32_32x32x16_f16" in txt and "v_mfma_f32_32x32x16_bf16" not in txt and "v_cvt_pk_bf16_f32" not in txt
    else:
        assert "v_mfma_f32_32x32x16_bf16" in txt and "v_cvt_pk_bf16_f32" in txt and "v_mfma_f32_32x32x16_f16" not in txt
    assert "scratch_" not in txt and "ds_read_b128" in txt
    seen = 0
    for mt, at, bt in FORMS:
        for al in (1, 0):
            frag = "linear_train_kernelILi%dELb%dELb%dELb%dE" % (mt, at, bt, al)
            hits = [k for k in meta if frag in k]
            assert len(hits) == 1, frag
            d = meta[hits[0]]
            assert int(d["private_segment_fixed_size"]) == 0 and int(d.get("vgpr_spill_count", 0)) == 0, (frag, d)      # nothing in scratch
            assert int(d["group_segment_fixed_size"]) == LDS[mt] <= 160 * 1024, (frag, d["group_segment_fixed_size"])
            assert int(d["vgpr_count"]) <= 512, (frag, d["vgpr_count"])
            assert waits.get(hits[0], 0) <= (4 if al else 12), (frag, waits.get(hits[0]))
            seen += 1
    red = [k for k in meta if "linear_train_reduce_kernel" in k]
    assert len(red) == 1 and int(meta[red[0]]["private_segment_fixed_size"]) == 0 and int(meta[red[0]]["group_segment_fixed_size"]) == 0
    assert waits.get(red[0], 0) <= 5
    assert len(meta) == seen + 1, sorted(meta)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_isa_wait_scan_is_clean_on_the_new_units():
    """scripts/isa_wait_scan.py at its default threshold on the two new translation units: no kernel waits for its loads one at a time.  The 16-byte forms
    stay below the threshold and are not listed; a listed kernel (the 4-byte-load forms: 7 - 10 full waits) issues at least four loads per full wait -- batches, not load - wait - use chains
    (a serialised kernel has about one)."""
    import re
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_wait_scan.py"), "6", "linear_train_"], check=True, capture_output=True, text=True).stdout
    for ln in out.splitlines():
        m = re.search(r"loads\s+(\d+)\s+vmcnt\(0\)\s+(\d+)\s+stores\s+\d+\s+(.*)", ln)
        assert m, ln
        loads, waits, name = int(m.group(1)), int(m.group(2)), m.group(3)
        assert "true>" not in name.replace(" ", ""), ln              # <..., AAL = true>: the 16-byte forms are below the threshold
        assert loads >= 4 * waits, ln
