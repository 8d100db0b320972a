"""Train-mode BatchNormalization (csrc/bn_train.hip) in isolation at ResNet-101's real map shapes for a 600 x 1000 image, next to
frcnn_bias_grad_f32 on the same maps in the same run (the yardstick: a one-sum reduction over the same bytes), and the whole ResNet-101
RPN training step.  GPU only.

    python scripts/resnet_train_micro.py [--iters 50] [--rounds 5] [--steps 10] [--out profiles/resnet_train_micro.txt]

The driver starts each GPU part as a child process of its own under a time limit (`timeout -k 10 <seconds>`) and stops at the first part that
does not end cleanly; the parts print their tables, the driver writes them to --out.

Method (kernels part): for every distinct (C, H, W) of the trunk's 104 BatchNormalization layers the variants (forward, backward, bias_grad)
are interleaved over `rounds` rounds in one process; a round times `iters` back-to-back calls between two device events after `warmup`
untimed ones; a figure is the median over the rounds.  Bytes: forward 12 B per element (z read by both launches, y written; 16 with the
fused residual), backward 28 B (dy, y, z read by both launches, dz written; 32 with dres), bias_grad 4 B.  "per step" weights every shape by
the number of layers that have it.  Step part: `steps` RPNTrainer.step() calls between two events after 3 untimed ones."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bn_shapes(blocks=(3, 4, 23, 3), im_h=600, im_w=1000):
    """{(C, H, W, residual fused): number of BatchNormalization layers of that shape} over the whole trunk"""
    from chainer_faster_rcnn_amd.models.resnet import STAGES, block_names
    f = lambda v: (v - 1) // 2 + 1                                   # noqa: E731
    h, w = f(im_h), f(im_w)
    out = {(64, h, w, False): 1}
    h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    for (stage, cin, mid, cout, stride), n in zip(STAGES, blocks):
        if stride == 2:
            h, w = f(h), f(w)
        for b in block_names(n):
            for key in [(mid, h, w, False)] * 2 + [(cout, h, w, True)] + ([(cout, h, w, False)] if b == "a" else []):
                out[key] = out.get(key, 0) + 1
    return out


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters                          # us per call


def part_kernels(args):
    import torch
    import chainer_faster_rcnn_amd as pkg
    rt = pkg.runtime.default_runtime()
    print("resnet_train_micro / kernels: %s, %d rounds x %d calls per variant, interleaved (us per call: median over the rounds)" % (
        torch.cuda.get_device_name(0), args.rounds, args.iters))
    print("  %-22s %5s %9s | %9s %6s | %9s %6s | %9s %6s" % ("map (C x H x W)", "count", "MB", "fwd us", "TB/s", "bwd us", "TB/s", "bias_grad", "TB/s"))
    tot = dict(fwd=0.0, bwd=0.0, bg=0.0, fb=0.0, bb=0.0, z=0.0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for (C, H, W, res), count in sorted(bn_shapes().items(), key=lambda kv: -kv[0][1] * kv[0][2] * kv[0][0]):
        n = C * H * W
        z, dy, r = (torch.randn(1, C, H, W, device="cuda", generator=gen) for _ in range(3))
        gamma, beta = torch.rand(C, device="cuda", generator=gen) + 0.5, torch.zeros(C, device="cuda")
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y, mean, rstd = rt.bn_train_fwd(z, gamma, beta, residual=r if res else None, relu=True, running_mean=rm, running_var=rv)
        variants = {
            "fwd": lambda: rt.bn_train_fwd(z, gamma, beta, residual=r if res else None, relu=True, running_mean=rm, running_var=rv, out=y),
            "bwd": lambda: rt.bn_train_bwd(dy, y, z, gamma, mean, rstd, want_dres=res),
            "bg": lambda: rt.bias_grad(dy),
        }
        ts = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                ts[k].append(timed(fn, args.iters, args.warmup))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        fb, bb = (16 if res else 12) * n, (32 if res else 28) * n
        print("  %-22s %5d %9.1f | %9.1f %6.2f | %9.1f %6.2f | %9.1f %6.2f" % (
            "%d x %d x %d%s" % (C, H, W, " +res" if res else ""), count, n * 4 / 1e6, med["fwd"], fb / med["fwd"] / 1e6, med["bwd"], bb / med["bwd"] / 1e6,
            med["bg"], 4 * n / med["bg"] / 1e6))
        for k in ("fwd", "bwd", "bg"):
            tot[k] += count * med[k]
        tot["fb"] += count * fb
        tot["bb"] += count * bb
        tot["z"] += count * n * 4
        del z, dy, r, y
        torch.cuda.empty_cache()
    print("  per step (104 layers): pre-BN maps %.2f GB; BN forward %.2f ms (%.2f GB, %.2f TB/s), BN backward %.2f ms (%.2f GB, %.2f TB/s); "
          "bias_grad over the same maps %.2f ms (%.2f TB/s)" % (tot["z"] / 1e9, tot["fwd"] / 1e3, tot["fb"] / 1e9, tot["fb"] / tot["fwd"] / 1e6, tot["bwd"] / 1e3,
                                                                tot["bb"] / 1e9, tot["bb"] / tot["bwd"] / 1e6, tot["bg"] / 1e3, tot["z"] / tot["bg"] / 1e6))


def part_step(args):
    import torch
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.models import FasterRCNN, ResNet101
    from chainer_faster_rcnn_amd.train import RPNTrainer
    rt = pkg.runtime.default_runtime()
    params = synthetic.resnet_params(101, seed=2)
    rs = np.random.RandomState(3)
    head = synthetic.params(seed=1, rpn_ch=512, roi_feat=2048 * 49)
    params["RPN/rpn_conv_3x3/W"] = (rs.randn(512, 2048, 3, 3) * 0.01).astype(np.float32)
    params["RPN/rpn_conv_3x3/b"] = np.zeros(512, np.float32)
    for k in ("rpn_cls_score", "rpn_bbox_pred"):
        params["RPN/%s/W" % k], params["RPN/%s/b" % k] = head["RPN/%s/W" % k], head["RPN/%s/b" % k]
    model = FasterRCNN(trunk_class=ResNet101, rpn_in_ch=2048, rpn_mid_ch=512, feat_stride=32, runtime=rt)
    model.trunk.load_params(params, "trunk/")
    model.RPN.load_params(params, "RPN/")
    model.rpn_train = True
    tr = RPNTrainer(model)
    h, w = 600, 1000
    x = Variable(rt.mem.from_numpy(synthetic.image(seed=6, h=h, w=w) / 64.0))
    info = Variable(np.array([[h, w]], dtype=np.int32))
    gt = Variable(np.array([[[100, 80, 420, 380, 3], [500, 200, 900, 560, 7], [300, 300, 460, 520, 12]]], dtype=np.float32))
    np.random.seed(0)
    for _ in range(3):
        out = tr.step(x, info, gt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        out = tr.step(x, info, gt)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    print("resnet_train_micro / step: ResNet-101 RPNTrainer.step() at %d x %d, fp32, MomentumSGD: %.2f ms per step (%.2f img/s) over %d steps; "
          "arena %d floats; peak device memory %.2f GB; last loss %.4f" % (h, w, ms, 1e3 / ms, args.steps, tr.n_flat, torch.cuda.max_memory_allocated() / 1e9,
                                                                          tr.losses_host(out)["rpn_loss"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--part", choices=("kernels", "step"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_train_micro.txt"))
    args = ap.parse_args()
    if args.part == "kernels":
        return part_kernels(args)
    if args.part == "step":
        return part_step(args)
    text = ""
    for part, limit in (("kernels", 240), ("step", 300)):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--rounds", str(args.rounds), "--steps", str(args.steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        text += p.stdout + "\n"
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                                        # a fault, an abort or the time limit: nothing more is started on the GPU
            text += "part %s ended with status %d: stopped here\n" % (part, p.returncode)
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
