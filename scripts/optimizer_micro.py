"""The update launches in isolation at the two real arena sizes: n_flat of the VGG-16 RPNTrainer and of the RCNNTrainer (both constructed
here, not hard-coded), for frcnn_sgd_momentum_wd (the yardstick), Adam, AdaGrad and RMSprop (csrc/optimizer.hip), each plain and through a
loss scaler's state.  GPU only.

    python scripts/optimizer_micro.py [--iters 100] [--rounds 5] [--out profiles/optimizer_micro.txt]

Method: the variants are interleaved over `rounds` rounds in ONE process; a round times `iters` back-to-back launches of one variant
between two device events (after `warmup` untimed ones); a variant's figure is the median over the rounds, with the min - max spread
beside it.  Bandwidth = the bytes the rule has to move (20 B per parameter: w and one state read and written, grad read; Adam 28 B) over
that time; "vs SGD" is that bandwidth over the plain SGD kernel's of the same run.  An Adam time is the whole entry: the one-lane
prologue launch and the update launch."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"sgd": 20, "Adam": 28, "AdaGrad": 20, "RMSprop": 20}


def arena_sizes(rt):
    import torch
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import FasterRCNN
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    model = FasterRCNN(runtime=rt)
    model.load_params(synthetic.params(seed=1))
    model.rpn_train = True
    n_rpn = RPNTrainer(model).n_flat
    model.rpn_train, model.rcnn_train = False, True
    n_rcnn = RCNNTrainer(model).n_flat
    del model
    torch.cuda.empty_cache()
    return {"RPNTrainer": int(n_rpn), "RCNNTrainer": int(n_rcnn)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_micro.txt"))
    args = ap.parse_args()
    import torch
    import chainer_faster_rcnn_amd as pkg
    rt = pkg.runtime.default_runtime()
    sizes = arena_sizes(rt)
    lines = ["optimizer_micro: %s, %d rounds x %d launches per variant, interleaved (us per call: median [min - max] over the rounds)" % (
        torch.cuda.get_device_name(0), args.rounds, args.iters)]
    for who, n in sizes.items():
        gen = torch.Generator(device="cuda").manual_seed(1)
        w, g = (torch.randn(n, device="cuda", generator=gen) * 1e-2 for _ in range(2))
        s1, s2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        scaler = rt.mem.zeros((8,), "i32")
        rt.loss_scaler_init(scaler, 2.0 ** 10)
        opt = rt.mem.zeros((8,), "i32")
        rt.opt_state_init(opt)
        variants = {}
        for sc, tag in ((None, ""), (scaler, " (scaled)")):
            if sc is None:
                variants["sgd"] = lambda: rt.sgd_momentum_wd(w, g, s1, 1e-3, 0.9, 0.0005)
            else:
                variants["sgd" + tag] = lambda: rt.sgd_momentum_wd_scaled(w, g, s1, 1e-3, 0.9, 0.0005, scaler)
            variants["Adam" + tag] = lambda sc=sc: rt.opt_step("Adam", w, g, s1, s2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, opt_state=opt, scaler_state=sc)
            variants["AdaGrad" + tag] = lambda sc=sc: rt.opt_step("AdaGrad", w, g, s1, lr=1e-3, eps=1e-8, scaler_state=sc)
            variants["RMSprop" + tag] = lambda sc=sc: rt.opt_step("RMSprop", w, g, s1, lr=1e-2, beta1=0.99, eps=1e-8, scaler_state=sc)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                for _ in range(args.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        lines.append("")
        lines.append("%s arena: n_flat = %d floats (%.1f MB per buffer)" % (who, n, n * 4 / 1e6))
        lines.append("  %-20s %28s %10s %8s" % ("rule", "us per call", "TB/s", "vs SGD"))
        base = None
        for k, ts in times.items():
            med = float(np.median(ts))
            bw = BYTES[k.split(" ")[0]] * n / (med * 1e-6) / 1e12
            if k == "sgd":
                base = bw
            lines.append("  %-20s %10.1f [%7.1f - %7.1f] %10.2f %8.2f" % (k, med, min(ts), max(ts), bw, bw / base))
        del w, g, s1, s2
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
