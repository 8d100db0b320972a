"""The ResNet-101 stage-2 training step (RCNNTrainer on the BatchNormalization trunk) at 600 x 1000: MomentumSGD, device dropout, 300 proposals --
next to the two figures it can be read against, taken in the same process on the same box: RPNTrainer.step() on the SAME model, and the VGG-16
stage-2 step.  GPU only.

    python scripts/resnet_rcnn_train_micro.py [--steps 5] [--rounds 5] [--out profiles/resnet_rcnn_train_micro.txt]

The driver starts the GPU part as a child process under a time limit (`timeout -k 10 <seconds>`); the part prints its table, the driver writes it
to --out.

Method: the three variants are interleaved over `rounds` rounds in one process; in a round a variant runs one untimed step (on the ResNet model the
two trainers hand the trunk over to each other: the untimed step re-adopts it) and then `steps` steps between two device events; a figure is the
median over the rounds.  Stage split of the ResNet stage-2 step: a device event at every stage boundary of forward_backward (RCNNTrainer.stage_hook),
one after update(); a stage's figure is the median over every timed step of every round.  The events sit on the stream, so a stage also holds the
host time the GPU waited for (the one host round trip of the step, behind the ProposalLayer, lands in head_fwd / targets_loss)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("trunk_fwd", "rpn_proposals", "roi_pool_fwd", "head_fwd", "targets_loss", "head_bwd_small", "fc6_bwd", "roi_pool_bwd", "trunk_bwd", "update")


def resnet_model(rt):
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.models import FasterRCNN, ResNet101
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
    for n in ("fc6", "fc7", "cls_score", "bbox_pred"):
        getattr(model, n).set(head[n + "/W"], head[n + "/b"])
    return model


def part_step(args):
    import torch
    import chainer_faster_rcnn_amd as pkg
    from chainer_faster_rcnn_amd import synthetic
    from chainer_faster_rcnn_amd.chainer_compat import Variable
    from chainer_faster_rcnn_amd.models import FasterRCNN
    from chainer_faster_rcnn_amd.train import RCNNTrainer, RPNTrainer
    rt = pkg.runtime.default_runtime()
    h, w = 600, 1000
    info = Variable(np.array([[h, w]], dtype=np.int32))
    gt = Variable(np.array([[[100, 80, 420, 380, 3], [500, 200, 900, 560, 7], [300, 300, 460, 520, 12]]], dtype=np.float32))
    x_res = Variable(rt.mem.from_numpy(synthetic.image(seed=6, h=h, w=w) / 64.0))
    x_vgg = Variable(rt.mem.from_numpy(synthetic.image(seed=6, h=h, w=w)))
    res = resnet_model(rt)
    vgg = FasterRCNN(runtime=rt)
    vgg.load_params(synthetic.params(seed=1))
    vgg.rcnn_train = True
    res.rcnn_train = True
    rc = RCNNTrainer(res, dropout_rng="device")
    rp = RPNTrainer(res)
    vg = RCNNTrainer(vgg, dropout_rng="device")
    events = []

    def hook(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events[-1].append((name, e))

    def rcnn_step(tr, x, staged=False):
        if staged:
            events.append([])
            tr.stage_hook = hook
        out = tr.forward_backward(x, info, gt)
        tr.stage_hook = None
        tr.all_reduce()
        tr.update()
        if staged:
            hook("update")
        return out

    def run(name, steps, staged=False):
        if name == "resnet_rcnn":
            res.rcnn_train = True
            return [rcnn_step(rc, x_res, staged) for _ in range(steps)][-1]
        if name == "resnet_rpn":
            res.rpn_train = True
            return [rp.step(x_res, info, gt) for _ in range(steps)][-1]
        return [rcnn_step(vg, x_vgg) for _ in range(steps)][-1]

    np.random.seed(0)
    names = ("resnet_rcnn", "resnet_rpn", "vgg_rcnn")
    ms = {k: [] for k in names}
    last = {}
    for k in names:                                                   # workspaces, kept buffers, the first adoption
        run(k, 2)
    for _ in range(args.rounds):
        for k in names:
            run(k, 1)                                                 # untimed: the hand-over of the shared trunk
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = run(k, args.steps, staged=True)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    n_rois = int(last["resnet_rcnn"]["n_rois"])
    print("resnet_rcnn_train_micro: %s, %d rounds x %d steps per variant, interleaved (ms per step: median over the rounds; all rounds in brackets)" % (
        torch.cuda.get_device_name(0), args.rounds, args.steps))
    l = rc.losses_host(last["resnet_rcnn"])
    print("  ResNet-101 RCNNTrainer.step() at %d x %d, fp32, MomentumSGD, device dropout, %d proposals (%d kept rows): %.2f ms per step (%.2f img/s) [%s]; "
          "arena %d floats (%.2f GB each for W, G, v); last loss_cls %.4f loss_bbox %.4f" % (
              h, w, n_rois, int(last["resnet_rcnn"]["keep_inds"].shape[0]), med["resnet_rcnn"], 1e3 / med["resnet_rcnn"], " ".join("%.2f" % v for v in ms["resnet_rcnn"]),
              rc.n_flat, rc.n_flat * 4 / 1e9, l["loss_cls"], l["loss_bbox"]))
    print("  ResNet-101 RPNTrainer.step() on the same model: %.2f ms per step [%s]; arena %d floats" % (med["resnet_rpn"], " ".join("%.2f" % v for v in ms["resnet_rpn"]), rp.n_flat))
    print("  VGG-16 RCNNTrainer.step() at %d x %d, fp32, MomentumSGD, device dropout, %d proposals: %.2f ms per step [%s]; arena %d floats" % (
        h, w, int(last["vgg_rcnn"]["n_rois"]), med["vgg_rcnn"], " ".join("%.2f" % v for v in ms["vgg_rcnn"]), vg.n_flat))
    per = {s: [] for s in STAGES}
    for ev in events:
        for (_, a), (name, b) in zip(ev, ev[1:]):
            per[name].append(a.elapsed_time(b))
    total = sum(float(np.median(v)) for v in per.values() if v)
    print("  stage split of the ResNet-101 stage-2 step (ms, median over %d steps; sum %.2f):" % (len(events), total))
    for s in STAGES:
        print("    %-15s %8.3f" % (s, float(np.median(per[s]))) if per[s] else "    %-15s unmeasured" % s)
    print("  peak device memory of the process (the three trainers resident): %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=540)
    ap.add_argument("--part", choices=("step",), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_rcnn_train_micro.txt"))
    args = ap.parse_args()
    if args.part == "step":
        return part_step(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part", "step", "--steps", str(args.steps), "--rounds", str(args.rounds)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    text = p.stdout
    sys.stdout.write(p.stdout)
    if p.returncode != 0:                                            # a fault, an abort or the time limit: nothing more is started on the GPU
        text += "the step part ended with status %d\n" % p.returncode
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
