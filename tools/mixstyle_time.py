#!/usr/bin/env python3
"""What MixStyle (--dg_method MixStyle) costs in the ResNet50 train step, B = 64, 222 x 222.

    python tools/mixstyle_time.py [--batch 64] [--steps 20] [--warmup 5] [--rounds 3] [--reps 20] [--out FILE]

1. Per site (the outputs of layer1..3: [B, 256, 56, 56], [B, 512, 28, 28], [B, 1024, 14, 14]): the forward (three launches: split
   partials, fp64 finalize, streaming pass) and the backward (one streaming launch), HIP events around each, against the algorithmic
   bytes -- forward 3 x the tensor (statistics read + stream read + write), backward 2 x (read dy, write dx).
2. The same MixStyle in stock PyTorch-ROCm ops (nets/layers.py's formula, autograd backward) on the same tensors.
3. The eager train step in images/s: plain ResNet50, MixStyleResNet at p = 1 and at p = 0.5, alternating in one process (rounds x
   steps each, after warm-up and gc.freeze(), as bench_resnet.py measures the plain step).
One JSON object on stdout (and in --out).
"""
import argparse
import gc
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SITES = [("layer1", 256, 56), ("layer2", 512, 28), ("layer3", 1024, 14)]


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
    from ccst_amd.nets import layers
    out = []
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, C, S in SITES:
        x = torch.relu(torch.randn(B, S, S, C, generator=g)).to(dev)           # NHWC, a closing BatchNorm + ReLU's output
        dy = torch.randn(B, S, S, C, generator=g).to(dev)
        lmda = torch.distributions.Beta(0.1, 0.1).sample((B,))
        perm = torch.randperm(B)
        draws = layers.pack_draws(lmda, perm, dev)
        holder = {}

        def fwd():
            holder["y"], holder["stat"] = ops.mixstyle_fwd(x, draws, 1e-6)

        fwd()
        us_f = _timed(fwd, reps)
        us_b = _timed(lambda: ops.mixstyle_bwd(dy, holder["stat"], draws), reps)
        # stock PyTorch on the same tensors (logical NCHW views of the NHWC buffers, as the ResNet hands them over)
        xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
        gt = dy.permute(0, 3, 1, 2)
        lam = lmda.to(dev).view(B, 1, 1, 1)
        p = perm.to(dev)

        def torch_fwd():
            mu = xt.mean(dim=[2, 3], keepdim=True)
            var = xt.var(dim=[2, 3], keepdim=True)
            sig = (var + 1e-6).sqrt()
            mu, sig = mu.detach(), sig.detach()
            x_normed = (xt - mu) / sig
            mu_mix = mu * lam + mu[p] * (1 - lam)
            sig_mix = sig * lam + sig[p] * (1 - lam)
            holder["yt"] = x_normed * sig_mix + mu_mix

        torch_fwd()
        ut_f = _timed(torch_fwd, reps)

        def torch_bwd():
            xt.grad = None
            holder["yt"].backward(gt, retain_graph=True)

        torch_bwd()
        ut_b = _timed(torch_bwd, reps)
        nbytes = x.numel() * 4
        out.append({"site": name, "shape_nhwc": [B, S, S, C], "tensor_MB": round(nbytes / 1e6, 1),
                    "fwd_us": round(us_f, 1), "fwd_GBps": round(3 * nbytes / us_f / 1e3, 0),
                    "bwd_us": round(us_b, 1), "bwd_GBps": round(2 * nbytes / us_b / 1e3, 0),
                    "torch_fwd_us": round(ut_f, 1), "torch_bwd_us": round(ut_b, 1)})
        del x, dy, xt, gt, holder
        torch.cuda.empty_cache()
    return out


def step_rates(dev, B, steps, warmup, rounds):
    sys.path.insert(0, ROOT)
    import bench_resnet
    from ccst_amd.nets import layers
    forms = {}
    for label, dg, p in (("plain", "", None), ("mixstyle_p1", "MixStyle", 1.0), ("mixstyle_p05", "MixStyle", 0.5)):
        model, opt, loss_fun, x, y = bench_resnet.build(dev, "resnet50", batch=B)
        if dg:                                                    # the same trunk and batch with MixStyle after layer1..3
            from ccst_amd.nets import resnet
            ms = resnet.MixStyleResNet(resnet.Bottleneck, [3, 4, 6, 3], classes=7, mixstyle_layers=["layer1", "layer2", "layer3"], mixstyle_p=p)
            ms.load_state_dict(model.state_dict())
            model = ms.to(dev).train()
            from ccst_amd import fed
            opt = fed.SGD(model, lr=0.001)
        assert isinstance(getattr(model, "mixstyle", None), (layers.MixStyle, type(None)))
        forms[label] = bench_resnet.make_step(model, opt, loss_fun, x, y)
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
    out["mixstyle_p1_extra_ms"] = round(out["mixstyle_p1"]["ms_per_step"] - out["plain"]["ms_per_step"], 3)
    out["mixstyle_p05_extra_ms"] = round(out["mixstyle_p05"]["ms_per_step"] - out["plain"]["ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    res = {"batch": a.batch, "image": 222, "sites": site_times(dev, a.batch, a.reps),
           "train_step": step_rates(dev, a.batch, a.steps, a.warmup, a.rounds)}
    for s in res["sites"]:
        print("%-7s %5.1f MB  fwd %7.1f us (%5.0f GB/s of 3x)  bwd %7.1f us (%5.0f GB/s of 2x)   torch fwd %7.1f us  bwd %7.1f us"
              % (s["site"], s["tensor_MB"], s["fwd_us"], s["fwd_GBps"], s["bwd_us"], s["bwd_GBps"], s["torch_fwd_us"], s["torch_bwd_us"]),
              file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
