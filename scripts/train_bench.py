"""The 600 x 1000 VGG-16 RPN training step (BASELINE.json configs[4]: synthetic parameters and image, bench.py's ground truth) for
RPNTrainer(conv_math="mfma" / "split" / "bf16" / "f16"), interleaved in ONE process over several rounds, one JSON line:
ms/step (median of the rounds), the fwd_bwd / all_reduce / update event times, the fraction of the matching dense peak (fp32 matrix
157 TF for mfma; split products run on the bf16 pipe at 6 MFMAs per product, so their fp32-equivalent rate is also held against
2.5 PF / 6; bf16 against the bf16 dense 2.5 PF) -- and the bf16 step's loss and worst gradient distance from the fp32 step on the same
image and RNG seed.

    python scripts/train_bench.py [--rounds 5] [--steps 10] [--warmup 3]

--stage rcnn: the stage-2 step of the same schedule (RCNNTrainer, train_rcnn.py's step) instead, with dropout_rng="device": "mfma" and "split"
(conv_math), "bf16" and "f16" (precision=...), interleaved the same way; per mode ms/step, the rounds, the round-to-round spread, the event
times; the bf16 / split ratio; --out writes the JSON line to a file as well (profiles/rcnn16_train_bench.json).

    python scripts/train_bench.py --stage rcnn [--rounds 5] [--steps 10] [--warmup 3] [--out profiles/rcnn16_train_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IM_H, IM_W = 600, 1000
# 2 x the multiply-adds of the 13 trunk convolutions + rpn_conv_3x3 at 600 x 1000, times three (forward, input gradient, weight gradient;
# conv1_1 has no input gradient -- counted anyway, it is 0.1 % of the total)
PEAK = {"mfma": (157.3e12, "fp32 dense (v_mfma_f32_32x32x2_f32)"), "split": (2.5e15 / 6, "bf16 dense 2.5 PF / 6 products"),
        "bf16": (2.5e15, "bf16 dense 2.5 PF"), "f16": (2.5e15, "fp16 dense 2.5 PF")}


def conv_flops():
    from chainer_faster_rcnn_amd.models.vgg16 import LAYERS
    h, w, total, c = IM_H, IM_W, 0.0, 3
    for l in LAYERS:
        if l == "pool":
            h, w = (h + 1) // 2, (w + 1) // 2
            continue
        _, ci, co = l
        total += 2.0 * ci * co * 9 * h * w
        c = co
    total += 2.0 * c * 512 * 9 * h * w                           # rpn_conv_3x3
    return 3 * total


RCNN_KW = {"mfma": dict(conv_math="mfma"), "split": dict(conv_math="split"), "bf16": dict(precision="bf16"), "f16": dict(precision="f16")}


def bench_inputs(rt):
    from chainer_faster_rcnn_amd import synthetic
    x_host = synthetic.image(seed=0, h=IM_H, w=IM_W)
    rs = np.random.RandomState(0)                                # bench.py's ground truth for rank 0
    G = 4
    w, h = rs.uniform(32, 400, G), rs.uniform(32, 400, G)
    x1, y1 = rs.uniform(0, IM_W - 1 - w), rs.uniform(0, IM_H - 1 - h)
    gt = np.stack([x1, y1, x1 + w, y1 + h, rs.randint(1, 21, G)], axis=1).astype(np.float32)[None]
    info = np.array([[IM_H, IM_W]], dtype=np.int32)
    return rt.mem.from_numpy(x_host), gt, rt.mem.from_numpy(gt), info


def main_rcnn(args):
    """Stage 2: RCNNTrainer with device-drawn dropout, the trainers interleaved over the rounds in one process."""
    import torch
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.models import FasterRCNN
    from chainer_faster_rcnn_amd.train import RCNNTrainer
    rt = pkg.runtime.default_runtime()
    params = synthetic.params(seed=1)
    x, gt, _, info = bench_inputs(rt)
    x, gt, info = Variable(x), Variable(gt), Variable(info)     # (the ground truth stays on the host: ProposalTargetLayer samples there)
    modes = args.modes.split(",")
    trainers = {}
    for m in modes:
        model = FasterRCNN(runtime=rt)
        model.load_params(params)
        model.rcnn_train = True
        trainers[m] = RCNNTrainer(model, dropout_rng="device", dropout_seed=1, **RCNN_KW[m])
    first = {}
    for m in modes:                                               # the first step's losses, from the identical initial state
        np.random.seed(0)
        out = trainers[m].forward_backward(x, info, gt)
        torch.cuda.synchronize()
        first[m] = dict(trainers[m].losses_host(out), n_rois=int(out["n_rois"]))
    ms = {m: [] for m in modes}
    ev_ms = {m: {"fwd_bwd": [], "all_reduce": [], "update": []} for m in modes}
    np.random.seed(0)
    for r in range(args.rounds):
        for m in modes:
            tr = trainers[m]
            for _ in range(args.warmup):
                tr.step(x, info, gt)
            torch.cuda.synchronize()
            evs = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                tr.forward_backward(x, info, gt)
                e[1].record()
                tr.all_reduce()
                e[2].record()
                tr.update()
                e[3].record()
                evs.append(e)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / args.steps * 1e3)
            for e in evs:
                for i, k in enumerate(("fwd_bwd", "all_reduce", "update")):
                    ev_ms[m][k].append(e[i].elapsed_time(e[i + 1]))
    res = {"bench": "rcnn_train_step_600x1000", "rounds": args.rounds, "steps_per_round": args.steps, "warmup_per_round": args.warmup,
           "dropout_rng": "device", "modes": {}}
    for m in modes:
        res["modes"][m] = {"ms_per_step": round(float(np.median(ms[m])), 4), "ms_per_round": [round(v, 4) for v in ms[m]],
                           "round_spread_ms": round(float(max(ms[m]) - min(ms[m])), 4),
                           "event_ms_median": {k: round(float(np.median(v)), 4) for k, v in ev_ms[m].items()}, "first_step": first[m]}
    if "f16" in ms:
        res["modes"]["f16"]["loss_scaler"] = trainers["f16"].loss_scaler.state()
    for a, b in (("bf16", "split"), ("f16", "split"), ("bf16", "mfma"), ("f16", "bf16")):
        if a in ms and b in ms:
            res["%s_over_%s" % (a, b)] = round(res["modes"][a]["ms_per_step"] / res["modes"][b]["ms_per_step"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="mfma,split,bf16,f16")
    ap.add_argument("--stage", default="rpn", choices=("rpn", "rcnn"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stage == "rcnn":
        return main_rcnn(args)
    import torch
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.models import FasterRCNN
    from chainer_faster_rcnn_amd.train import RPNTrainer
    rt = pkg.runtime.default_runtime()
    params = synthetic.params(seed=1)
    x_host = synthetic.image(seed=0, h=IM_H, w=IM_W)
    rs = np.random.RandomState(0)                                # bench.py's ground truth for rank 0
    G = 4
    w, h = rs.uniform(32, 400, G), rs.uniform(32, 400, G)
    x1, y1 = rs.uniform(0, IM_W - 1 - w), rs.uniform(0, IM_H - 1 - h)
    gt = np.stack([x1, y1, x1 + w, y1 + h, rs.randint(1, 21, G)], axis=1).astype(np.float32)[None]
    info = np.array([[IM_H, IM_W]], dtype=np.int32)
    x, gt_dev = rt.mem.from_numpy(x_host), rt.mem.from_numpy(gt)
    modes = args.modes.split(",")
    trainers = {}
    for m in modes:
        model = FasterRCNN(runtime=rt)
        model.load_params(params)
        model.rpn_train = True
        trainers[m] = RPNTrainer(model, conv_math=m)
    # accuracy first, from the identical initial state: one forward_backward each with the same NumPy seed
    grads, losses = {}, {}
    for m in modes:
        np.random.seed(0)
        out = trainers[m].forward_backward(Variable(x), Variable(info), Variable(gt))
        torch.cuda.synchronize()
        losses[m] = trainers[m].losses_host(out)["rpn_loss"]
        grads[m] = trainers[m].grads_chainer_layout()
    acc = {}
    for m in modes:
        if m == "mfma" or "mfma" not in modes:
            continue
        worst = max(float(np.abs(grads[m][k] - grads["mfma"][k]).max() / max(np.abs(grads["mfma"][k]).max(), 1e-12)) for k in grads["mfma"])
        acc[m] = {"loss": losses[m], "loss_rel_to_fp32": abs(losses[m] - losses["mfma"]) / abs(losses["mfma"]), "worst_grad_rel_to_fp32": worst}
    ms = {m: [] for m in modes}
    ev_ms = {m: {"fwd_bwd": [], "all_reduce": [], "update": []} for m in modes}
    np.random.seed(0)
    for r in range(args.rounds):
        for m in modes:
            tr = trainers[m]
            for _ in range(args.warmup):
                tr.step(x, info, gt_dev)
            torch.cuda.synchronize()
            evs = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                tr.forward_backward(x, info, gt_dev)
                e[1].record()
                tr.all_reduce()
                e[2].record()
                tr.update()
                e[3].record()
                evs.append(e)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / args.steps * 1e3)
            for e in evs:
                for i, k in enumerate(("fwd_bwd", "all_reduce", "update")):
                    ev_ms[m][k].append(e[i].elapsed_time(e[i + 1]))
    flops = conv_flops()
    res = {"bench": "rpn_train_step_600x1000", "rounds": args.rounds, "steps_per_round": args.steps, "conv_flops_per_step": flops, "modes": {}}
    for m in modes:
        med = float(np.median(ms[m]))
        res["modes"][m] = {"ms_per_step": round(med, 4), "ms_per_round": [round(v, 4) for v in ms[m]],
                           "event_ms_median": {k: round(float(np.median(v)), 4) for k, v in ev_ms[m].items()},
                           "conv_fraction_of_peak": round(flops / (med * 1e-3) / PEAK[m][0], 4), "peak": PEAK[m][1]}
        if m in acc:
            res["modes"][m]["accuracy_vs_fp32_step"] = {k: float("%.4g" % v) for k, v in acc[m].items()}
    if "f16" in ms:                                               # the device-side loss scaler after the timed steps (one synchronising read, here only)
        res["modes"]["f16"]["loss_scaler"] = trainers["f16"].loss_scaler.state()
        if "bf16" in ms:
            res["f16_over_bf16"] = round(res["modes"]["f16"]["ms_per_step"] / res["modes"]["bf16"]["ms_per_step"], 4)
    if "bf16" in ms and "split" in ms:
        res["bf16_over_split"] = round(res["modes"]["bf16"]["ms_per_step"] / res["modes"]["split"]["ms_per_step"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
