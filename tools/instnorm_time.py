#!/usr/bin/env python3
"""What instance normalisation costs: the InstanceNorm ResNet (--network resnet18IN) and --IN_test, 222 x 222.

    python tools/instnorm_time.py [--batch 32] [--steps 20] [--warmup 5] [--rounds 3] [--reps 20] [--out FILE]

1. Per IN site shape of ResNet18IN ([B, 64, 111, 111] stem, then 64 x 56^2, 128 x 28^2, 256 x 14^2, 512 x 7^2), forward and backward,
   HIP events around each, against the algorithmic bytes of include/ccst_instnorm.h's budget: forward 2 reads of x + 1 write of y
   (+ the residual read and the 1/16 mask write), backward 2 reads each of dy and x + 1 write of dx (+ the d_residual write and two
   1/16 mask reads).  Two forms: IN + ReLU (bn1 of a block, the stem) and IN + residual + ReLU (bn2 of a block).
2. The train step in images/s, B = --batch: ResNet18 (BatchNorm) and ResNet18IN eager, and ResNet18IN replayed from a HIP graph
   (fed._GraphedTrainStep), alternating in one process after warm-up and gc.freeze().
3. The same ResNetIN in stock PyTorch-ROCm (torch.nn, channels_last, torch.optim.SGD) on the same GPU.
4. The --IN_test eval forward of ResNet50 at B = 64 against its BatchNorm eval forward.
One JSON object on stdout (and in --out).
"""
import argparse
import copy
import gc
import json
import os
import statistics
import sys
import types

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SITES = [("stem", 64, 111), ("layer1", 64, 56), ("layer2", 128, 28), ("layer3", 256, 14), ("layer4", 512, 7)]


def _timed(fn, reps):
    """Median microseconds of fn() over reps calls, each between two events on the current stream."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def site_times(dev, B, reps):
    from ccst_amd import ops
    out = []
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, C, S in SITES:
        x = torch.relu(torch.randn(B, S, S, C, generator=g)).to(dev) * 3.0 + 0.5      # NHWC, a conv output of a ReLU'd input
        r = torch.randn(B, S, S, C, generator=g).to(dev)
        dy = torch.randn(B, S, S, C, generator=g).to(dev)
        gam, bet = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        nbytes = x.numel() * 4
        for form, res in (("relu", None), ("residual_relu", r)):
            holder = {}

            def fwd():
                holder["y"], holder["save"], holder["mask"] = ops.instnorm_fwd(x, gam, bet, res, True, 1e-5, want_mask=res is not None)

            fwd()
            us_f = _timed(fwd, reps)
            us_b = _timed(lambda: ops.instnorm_bwd(dy, x, holder["save"], gam, bet, True, mask=holder["mask"], want_dres=res is not None,
                                                   dgamma=dg, dbeta=db), reps)
            fb = 3 * nbytes + (nbytes + nbytes // 16 if res is not None else 0)
            bb = 5 * nbytes + (nbytes + nbytes // 8 if res is not None else 0)
            out.append({"site": name, "form": form, "shape_nhwc": [B, S, S, C], "tensor_MB": round(nbytes / 1e6, 1),
                        "fwd_us": round(us_f, 1), "fwd_bytes_MB": round(fb / 1e6, 1), "fwd_TBps": round(fb / us_f / 1e6, 2),
                        "bwd_us": round(us_b, 1), "bwd_bytes_MB": round(bb / 1e6, 1), "bwd_TBps": round(bb / us_b / 1e6, 2)})
        del x, r, dy, holder
        torch.cuda.empty_cache()
    return out


class _TorchBlock(nn.Module):
    """torchvision's v1.5 BasicBlock with InstanceNorm2d: the stock-PyTorch form of a ResNetIN block."""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.InstanceNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.InstanceNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return torch.relu(out + (self.downsample(x) if self.downsample is not None else x))


def torch_resnet18in(classes):
    layers, inplanes = [], 64
    for planes, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        ds = None
        if stride != 1 or inplanes != planes:
            ds = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.InstanceNorm2d(planes))
        layers += [_TorchBlock(inplanes, planes, stride, ds), _TorchBlock(planes, planes)]
        inplanes = planes
    return nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.InstanceNorm2d(64, affine=True), nn.ReLU(inplace=True),
                         nn.MaxPool2d(3, 2, 1), *layers, nn.AvgPool2d(7, 1), nn.Flatten(), nn.Linear(512, classes))


def step_rates(dev, B, steps, warmup, rounds):
    import bench_resnet
    from ccst_amd import fed
    from ccst_amd.nets import models
    forms = {}
    model, opt, loss_fun, x, y = bench_resnet.build(dev, "resnet18", batch=B)
    forms["resnet18"] = bench_resnet.make_step(model, opt, loss_fun, x, y)
    torch.manual_seed(1)
    mi = models.get_network("resnet18IN")(types.SimpleNamespace(dg_method=""), classes=7).to(dev).train()
    oi, li = fed.SGD(mi, lr=0.001), fed.CrossEntropyLoss()
    forms["resnet18in"] = bench_resnet.make_step(mi, oi, li, x, y)
    mg = copy.deepcopy(mi)
    og, lg = fed.SGD(mg, lr=0.001), fed.CrossEntropyLoss()
    eager_g = bench_resnet.make_step(mg, og, lg, x, y)
    for _ in range(3):
        eager_g()
    torch.cuda.synchronize()
    sums = (torch.zeros((), device=dev), torch.zeros((), device=dev, dtype=torch.int64))
    gs = fed._GraphedTrainStep(mg, og, lg, x, y, *sums)
    forms["resnet18in_replay"] = lambda: gs.run(x, y)
    tm = torch_resnet18in(7).to(dev).to(memory_format=torch.channels_last).train()
    topt, tce = torch.optim.SGD(tm.parameters(), lr=0.001), nn.CrossEntropyLoss()
    xt = x.contiguous(memory_format=torch.channels_last)

    def torch_step():
        topt.zero_grad()
        tce(tm(xt), y).backward()
        topt.step()
    forms["resnet18in_stock_torch"] = torch_step
    for step in forms.values():
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    rates = {k: [] for k in forms}
    for _ in range(rounds):
        for label, step in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            e1.synchronize()
            rates[label].append(B * steps / (e0.elapsed_time(e1) / 1e3))
    gc.unfreeze()
    out = {k: {"img_per_s": round(statistics.median(v), 1), "ms_per_step": round(B * 1e3 / statistics.median(v), 3),
               "rounds": [round(r, 1) for r in v]} for k, v in rates.items()}
    out["in_over_bn"] = round(out["resnet18in"]["ms_per_step"] / out["resnet18"]["ms_per_step"], 3)
    out["replay_in_over_bn"] = round(out["resnet18in_replay"]["ms_per_step"] / out["resnet18"]["ms_per_step"], 3)
    out["stock_over_in"] = round(out["resnet18in_stock_torch"]["ms_per_step"] / out["resnet18in"]["ms_per_step"], 3)
    return out


def in_test_eval(dev, reps):
    """ResNet50 eval forward at B = 64: BatchNorm vs the --IN_test swap (fed.swap_bn_for_in)."""
    import bench_resnet
    from ccst_amd import fed
    model, _, _, x, _ = bench_resnet.build(dev, "resnet50", batch=64)
    model.eval()
    res = {}
    with torch.no_grad():
        for label in ("batchnorm", "in_test"):
            if label == "in_test":
                fed.swap_bn_for_in(model, dev)
            for _ in range(3):
                model(x)
            us = _timed(lambda: model(x), reps)
            res[label] = {"ms": round(us / 1e3, 3), "img_per_s": round(64 / (us / 1e6), 1)}
    res["in_over_bn"] = round(res["in_test"]["ms"] / res["batchnorm"]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    res = {"batch": a.batch, "image": 222, "sites": site_times(dev, a.batch, a.reps),
           "train_step": step_rates(dev, a.batch, a.steps, a.warmup, a.rounds), "in_test_eval_resnet50_b64": in_test_eval(dev, a.reps)}
    for s in res["sites"]:
        print("%-7s %-13s %6.1f MB  fwd %7.1f us (%4.2f TB/s)  bwd %7.1f us (%4.2f TB/s)"
              % (s["site"], s["form"], s["tensor_MB"], s["fwd_us"], s["fwd_TBps"], s["bwd_us"], s["bwd_TBps"]), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
