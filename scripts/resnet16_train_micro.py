"""The ResNet trunk's bf16 train-mode pass (ResNet(train_dtype="bf16"), csrc/conv1x1_train_bf16.hip) next to the fp32 pass it replaces.  GPU only.

    python scripts/resnet16_train_micro.py [--rounds 5] [--calls 50] [--steps 5] [--out profiles/resnet16_train_micro.txt]

(a) kernels: each of the three 1x1 training entries against the fp32 call that computes the same product today (conv_ex with ksize 1, conv_ex on
    pack_conv_dgrad_w weights, conv_wgrad(ksize=1)) at one shape per layer class of ResNet-101 at 600 x 1000: `rounds` interleaved rounds of `calls`
    back-to-back calls between two device events, the median over the rounds; FLOP/s against the dense bf16 peak, the bytes the product has to move
    (operands once, result once) against HBM, and which of the two bounds it.
(b) steps: ResNet-101 RPNTrainer.step() and RCNNTrainer.step() at 600 x 1000 with train_dtype f32 against bf16, in one process, interleaved, `rounds`
    rounds of `steps` steps; the stage split of the stage-2 step through RCNNTrainer.stage_hook; and, on one seeded step from equal parameters,
    the bf16 step's losses and its worst gradient distance from the fp32 step's.

Each part is a child process under its own time limit (`timeout -k 10 <seconds>`); the second starts only if the first ended with status 0."""
import argparse
import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(152, 64, 150000), (64, 256, 37500), (256, 64, 37500), (512, 128, 9375), (1024, 256, 2394), (256, 1024, 2394), (2048, 512, 608), (512, 2048, 608)]
HW = {150000: (300, 500), 37500: (150, 250), 9375: (75, 125), 2394: (38, 63), 608: (19, 32)}
PEAK_BF16, PEAK_HBM = 2.5e15, 8.0e12
STAGES = ("trunk_fwd", "rpn_proposals", "roi_pool_fwd", "head_fwd", "targets_loss", "head_bwd_small", "fc6_bwd", "roi_pool_bwd", "trunk_bwd", "update")


def part_kernels(args):
    import torch
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import tuning
    rt = pkg.runtime.default_runtime()
    m = rt.mem
    rs = np.random.RandomState(0)
    print("resnet16_train_micro (a): %s, %d interleaved rounds x %d calls (us per call: median over the rounds); share of peak = max(FLOPs / %.1f PF, bytes / %.1f TB/s) / time"
          % (torch.cuda.get_device_name(0), args.rounds, args.calls, PEAK_BF16 / 1e15, PEAK_HBM / 1e12))
    print("  (bf16/128: the same entry with the 128-row tile forced, FRCNN_C1T_MT=4)")
    print("  %-18s %-15s %10s %10s %7s %9s %9s  %-18s %s" % ("Cin, Cout, HW", "product", "fp32 us", "bf16 us", "ratio", "TFLOP/s", "TB/s", "bound, share of it", "bf16/128 us"))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls

    for ci, co, hw in SHAPES:
        h, w = HW[hw]
        x = m.from_numpy(np.maximum(rs.randn(1, ci, h, w), 0).astype(np.float32))
        dz = m.from_numpy((rs.randn(1, co, h, w) * 1e-2).astype(np.float32))
        wp = m.from_numpy((rs.randn(ci, co) * np.sqrt(2.0 / ci)).astype(np.float32))
        wd = rt.pack_conv_dgrad_w(wp, 1)
        zb_o, zb_i = m.zeros((co,), "f32"), m.zeros((ci,), "f32")
        pairs = [("forward", lambda: rt.conv_ex(x, wp, zb_o, 1, act=0), lambda: rt.conv1x1_bf16_train(x, wp), (ci + co) * hw + ci * co),
                 ("input gradient", lambda: rt.conv_ex(dz, wd, zb_i, 1, act=0), lambda: rt.conv1x1_dgrad_bf16(dz, wp), (ci + co) * hw + ci * co),
                 ("weight gradient", lambda: rt.conv_wgrad(x, dz, 1), lambda: rt.conv1x1_wgrad_bf16(x, dz), (ci + co) * hw + ci * co)]
        if ci == 152:
            pairs.pop(1)                                              # the stem takes no input gradient
        for name, f32, b16, floats in pairs:
            f32(), b16()
            t = {"f32": [], "bf16": [], "bf16/128": []}
            for _ in range(args.rounds):
                t["f32"].append(timed(f32))
                t["bf16"].append(timed(b16))
                with tuning.override(FRCNN_C1T_MT="4"):
                    b16()
                    t["bf16/128"].append(timed(b16))
            a, b = float(np.median(t["f32"])), float(np.median(t["bf16"]))
            flops, nbytes = 2.0 * ci * co * hw, 4.0 * floats
            t_flop, t_mem = flops / PEAK_BF16, nbytes / PEAK_HBM
            print("  %-18s %-15s %10.1f %10.1f %7.2f %9.1f %9.2f  %-18s %10.1f" % ("%d, %d, %d" % (ci, co, hw), name, a, b, a / b, flops / (b * 1e-6) / 1e12,
                                                                                    nbytes / (b * 1e-6) / 1e12, "%s, %.0f %%" % ("HBM" if t_mem >= t_flop else "MFMA",
                                                                                                                              100 * max(t_flop, t_mem) / (b * 1e-6)),
                                                                                    float(np.median(t["bf16/128"]))))


def resnet_model(rt, train_dtype):
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import FasterRCNN, ResNet101
    params = synthetic.resnet_params(101, seed=2)
    rs = np.random.RandomState(3)
    head = synthetic.params(seed=1, rpn_ch=512, roi_feat=2048 * 49)
    params["RPN/rpn_conv_3x3/W"] = (rs.randn(512, 2048, 3, 3) * 0.01).astype(np.float32)
    params["RPN/rpn_conv_3x3/b"] = np.zeros(512, np.float32)
    for k in ("rpn_cls_score", "rpn_bbox_pred"):
        params["RPN/%s/W" % k], params["RPN/%s/b" % k] = head["RPN/%s/W" % k], head["RPN/%s/b" % k]
    model = FasterRCNN(trunk_class=functools.partial(ResNet101, train_dtype=train_dtype), rpn_in_ch=2048, rpn_mid_ch=512, feat_stride=32, runtime=rt)
    model.trunk.load_params(params, "trunk/")
    model.RPN.load_params(params, "RPN/")
    for n in ("fc6", "fc7", "cls_score", "bbox_pred"):
        getattr(model, n).set(head[n + "/W"], head[n + "/b"])
    return model


def part_steps(args):
    import torch
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    rt = pkg.runtime.default_runtime()
    h, w = 600, 1000
    info = Variable(np.array([[h, w]], dtype=np.int32))
    gt = Variable(np.array([[[100, 80, 420, 380, 3], [500, 200, 900, 560, 7], [300, 300, 460, 520, 12]]], dtype=np.float32))
    x = Variable(rt.mem.from_numpy(synthetic.image(seed=6, h=h, w=w) / 64.0))
    variants = [(kind, dt) for kind in ("rpn", "rcnn") for dt in ("f32", "bf16")]
    models = {dt: resnet_model(rt, dt) for dt in ("f32", "bf16")}
    tr = {}
    for kind, dt in variants:
        models[dt].rcnn_train = True
        tr[kind, dt] = RPNTrainer(models[dt]) if kind == "rpn" else RCNNTrainer(models[dt], dropout_rng="device")
    events = {v: [] for v in variants}

    def run(v, steps, staged=False):
        kind, dt = v
        t, model = tr[v], models[dt]
        if kind == "rpn":
            model.rpn_train = True
            return [t.step(x, info, gt) for _ in range(steps)][-1]
        model.rcnn_train = True
        out = None
        for _ in range(steps):
            if staged:
                events[v].append([])

                def hook(name, ev=events[v][-1]):
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    ev.append((name, e))
                t.stage_hook = hook
            out = t.forward_backward(x, info, gt)
            t.stage_hook = None
            t.all_reduce()
            t.update()
            if staged:
                hook("update")
        return out

    # ---- one seeded step from equal parameters: losses and gradient distance (before anything is updated differently)
    print("resnet16_train_micro (b): %s, ResNet-101 at %d x %d, %d rounds x %d steps per variant, interleaved" % (torch.cuda.get_device_name(0), h, w, args.rounds, args.steps))
    for kind in ("rpn", "rcnn"):
        outs = {}
        for dt in ("f32", "bf16"):
            t, model = tr[kind, dt], models[dt]
            setattr(model, "rpn_train" if kind == "rpn" else "rcnn_train", True)
            np.random.seed(7)
            out = t.forward_backward(x, info, gt)
            t.all_reduce()
            outs[dt] = (t.losses_host(out), t.grads_chainer_layout())
        worst, where = 0.0, None
        for k, g32 in outs["f32"][1].items():
            scale = float(np.abs(g32).max())
            if scale > 0:
                d = float(np.abs(outs["bf16"][1][k] - g32).max()) / scale
                if d > worst:
                    worst, where = d, k
        key = "rpn_loss" if kind == "rpn" else "loss_rcnn"
        keys = sorted(outs["f32"][1])
        g32 = np.concatenate([outs["f32"][1][k].ravel() for k in keys]).astype(np.float64)
        g16 = np.concatenate([outs["bf16"][1][k].ravel() for k in keys]).astype(np.float64)
        print("  one seeded %s step from equal parameters: fp32 %s %.6f, bf16 %.6f; worst gradient distance (max-abs over the fp32 gradient's max-abs) %.3e at %s; "
              "all gradients as one vector: |bf16 - fp32| / |fp32| = %.3e, cosine %.6f"
              % (kind, key, outs["f32"][0][key], outs["bf16"][0][key], worst, where, np.linalg.norm(g16 - g32) / np.linalg.norm(g32),
                 float(g16 @ g32) / (np.linalg.norm(g16) * np.linalg.norm(g32))))
    np.random.seed(0)
    ms = {v: [] for v in variants}
    for v in variants:
        run(v, 2)
    for _ in range(args.rounds):
        for v in variants:
            run(v, 1)                                                 # untimed: the hand-over of the shared trunk
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(v, args.steps, staged=True)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1) / args.steps)
    for kind in ("rpn", "rcnn"):
        a, b = ms[kind, "f32"], ms[kind, "bf16"]
        print("  %s.step(): fp32 trunk %.2f ms [%s], bf16 trunk %.2f ms [%s]; fp32 / bf16 = %.2f; bf16 faster in %d of %d rounds"
              % ("RPNTrainer" if kind == "rpn" else "RCNNTrainer", float(np.median(a)), " ".join("%.2f" % v for v in a), float(np.median(b)),
                 " ".join("%.2f" % v for v in b), float(np.median(a)) / float(np.median(b)), sum(y < x_ for x_, y in zip(a, b)), len(a)))
    print("  stage split of RCNNTrainer.step() (ms, median over every timed step):   fp32 trunk   bf16 trunk")
    per = {}
    for dt in ("f32", "bf16"):
        per[dt] = {s: [] for s in STAGES}
        for ev in events["rcnn", dt]:
            for (_, a), (name, b) in zip(ev, ev[1:]):
                per[dt][name].append(a.elapsed_time(b))
    for s in STAGES:
        if per["f32"][s]:
            print("    %-15s %38.3f %12.3f" % (s, float(np.median(per["f32"][s])), float(np.median(per["bf16"][s]))))
    print("  peak device memory of the process (four trainers resident): %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--part", choices=("kernels", "steps"), default=None)
    ap.add_argument("--only", choices=("kernels", "steps"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet16_train_micro.txt"))
    args = ap.parse_args()
    if args.part == "kernels":
        return part_kernels(args)
    if args.part == "steps":
        return part_steps(args)
    text, status = "", 0
    for part in ("kernels", "steps"):
        if args.only and part != args.only:
            continue
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(args.rounds),
               "--calls", str(args.calls), "--steps", str(args.steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        text += p.stdout
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:                                        # a fault, an abort or the time limit: nothing more is started on the GPU
            text += "the %s part ended with status %d\n" % (part, p.returncode)
            status = 1
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
