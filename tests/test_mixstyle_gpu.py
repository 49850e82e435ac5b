"""GPU: MixStyle (include/ccst_mixstyle.h, ccst_amd.nets.layers.MixStyle, MixStyleResNet) against the reference's own outputs
(tests/golden/mixstyle_*.npz, tools/make_golden.py), against the same fp32 operations evaluated by torch, and in the ResNet train step,
fed.train and the fed_run.py CLI."""
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NOISE_MULT = 7.0          # tests/test_resnet_gpu.py::_model_case's multiplier of the fixtures' own fp32 noise


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def mixstyle_input(shape, seed):
    """tools/make_golden.py's recipe: per-(image, channel) means in [-1, 1], sigmas in [0.5, 2]; upstream gradient N(0, 1)."""
    rs = np.random.RandomState(seed)
    N, C, H, W = shape
    mu = rs.uniform(-1.0, 1.0, (N, C, 1, 1))
    sd = rs.uniform(0.5, 2.0, (N, C, 1, 1))
    x = (mu + sd * rs.standard_normal(shape)).astype(np.float32)
    g = rs.standard_normal(shape).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(g)


class DrawSpy(object):
    """Records every draw of ccst_amd.nets.layers.draw (None for a shut gate)."""

    def __init__(self, monkeypatch):
        from ccst_amd.nets import layers
        self.draws = []
        real = layers.draw

        def spy(*a, **k):
            d = real(*a, **k)
            self.draws.append(d)
            return d
        monkeypatch.setattr(layers, "draw", spy)


def words_max(words):
    return float(torch.tensor(int(words.max()), dtype=torch.int32).view(torch.float32))


def run_module(dev, ms, x, g):
    """One training forward + backward of our module on a channels_last device copy of x."""
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ms(xd)
    y.backward(g.to(dev).contiguous(memory_format=torch.channels_last))
    return xd, y


def close(got, ref, rel=2e-6):
    got, ref = got.detach().cpu(), torch.as_tensor(ref)
    if torch.isnan(ref).all():
        return bool(torch.isnan(got).all())
    return float((got - ref).abs().max()) <= rel * float(ref.abs().max())


def test_module_against_the_reference(dev, golden, monkeypatch):
    """Output and input gradient within 2e-6 of max |.| of the reference's, for 'random' and 'crossdomain' at several shapes (C % 64 != 0,
    HW = 1 -> NaN) and a p = 0.5 sequence; the same draws, and the generators left where the reference left them."""
    from ccst_amd import ops
    from ccst_amd.nets import layers
    g = golden("mixstyle_module")
    spy = DrawSpy(monkeypatch)
    for name in [str(c) for c in g["cases"]]:
        mix = name.split("_", 1)[1]
        shape, seed = tuple(int(v) for v in g[name + "/shape"]), int(g[name + "/seed"])
        x, gr = mixstyle_input(shape, seed)
        ms = layers.MixStyle(p=1.0, mix=mix).train()
        random.seed(seed)
        torch.manual_seed(seed)
        xd, y = run_module(dev, ms, x, gr)
        lmda, perm = spy.draws[-1]
        assert torch.equal(lmda, torch.from_numpy(g[name + "/lmda"])) and torch.equal(perm, torch.from_numpy(g[name + "/perm"])), name
        assert random.random() == float(g[name + "/probe_random"]) and torch.equal(torch.rand(4), torch.from_numpy(g[name + "/probe_torch"])), name
        assert close(y, g[name + "/y"]), (name, "y")
        assert close(xd.grad, g[name + "/dx"]), (name, "dx")
        if shape[2] * shape[3] == 1:
            assert bool(torch.isnan(y).all())               # unbiased variance of one element, as the reference
        else:
            assert words_max(ops.tagged_absmax(y)) == float(y.detach().abs().max()), name      # per-tensor words of y, exact
    shape, seed = tuple(int(v) for v in g["seq/shape"]), int(g["seq/seed"])
    ms = layers.MixStyle(p=0.5).train()
    random.seed(seed)
    torch.manual_seed(seed)
    for k in range(int(g["seq/K"])):
        x, gr = mixstyle_input(shape, seed + 1 + k)
        xd, y = run_module(dev, ms, x, gr)
        fired = spy.draws[-1] is not None
        assert fired == bool(g["seq/fired"][k]), k
        if not fired:
            assert y is xd                                   # a shut gate returns x itself
        assert close(y, g["seq/y"][k]) and close(xd.grad, g["seq/dx"][k]), k
    assert random.random() == float(g["seq/probe_random"]) and torch.equal(torch.rand(4), torch.from_numpy(g["seq/probe_torch"]))


@pytest.mark.parametrize("shape", [(8, 64, 6, 6), (6, 96, 5, 9), (4, 256, 17, 23), (3, 4, 9, 9)])
def test_kernels_are_the_fp32_operations(dev, shape):
    """Given the kernel's own mean / sigma: y is bit-equal to ((x - mu) / sigma) * sigma_mix + mu_mix and dx to (dy * sigma_mix) / sigma,
    each operation evaluated by torch on the device; mean / sigma within 1e-6 relative of fp64."""
    from ccst_amd import ops
    from ccst_amd.nets import layers
    N, C, H, W = shape
    x, gr = mixstyle_input(shape, 7 + C)
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev)
    dy = gr.permute(0, 2, 3, 1).contiguous().to(dev)
    torch.manual_seed(C)
    lmda = torch.distributions.Beta(0.1, 0.1).sample((N,))
    perm = torch.randperm(N)
    draws = layers.pack_draws(lmda, perm, dev)
    y, stat = ops.mixstyle_fwd(xh, draws, 1e-6)
    dx = ops.mixstyle_bwd(dy, stat, draws)
    mu, sd = stat[0].view(N, 1, 1, C), stat[1].view(N, 1, 1, C)
    lam = lmda.to(dev).view(N, 1, 1, 1)
    p = perm.to(dev)
    mu_mix = mu * lam + mu[p] * (1 - lam)
    sd_mix = sd * lam + sd[p] * (1 - lam)
    assert torch.equal(y, ((xh - mu) / sd) * sd_mix + mu_mix)
    assert torch.equal(dx, (dy * sd_mix) / sd)
    x64 = x.double()
    m64 = x64.mean(dim=(2, 3))
    s64 = (x64.var(dim=(2, 3)) + 1e-6).sqrt()
    # (a mean near zero has no relative error to speak of: the mean's is taken relative to max(|mean|, sigma))
    assert float(((stat[0].view(N, C).cpu().double() - m64) / torch.maximum(m64.abs(), s64)).abs().max()) <= 1e-6
    assert float(((stat[1].view(N, C).cpu().double() - s64) / s64).abs().max()) <= 1e-6


def test_statistics_do_not_depend_on_batch_mates(dev):
    from ccst_amd import ops
    from ccst_amd.nets import layers
    x, _ = mixstyle_input((6, 128, 14, 14), 21)
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev)
    _, whole = ops.mixstyle_fwd(xh, layers.pack_draws(torch.full((6,), 0.25), torch.tensor([3, 4, 5, 0, 1, 2]), dev))
    for n in range(6):
        _, alone = ops.mixstyle_fwd(xh[n:n + 1].contiguous(), layers.pack_draws(torch.full((1,), 0.25), torch.tensor([0]), dev))
        assert torch.equal(alone.view(2, 128), whole.view(2, 6, 128)[:, n]), n


def test_eval_deactivated_and_layouts(dev):
    """Eval and set_activation_status(False) return x itself; an NCHW-contiguous input goes through the layout plumbing (and gives the
    channels_last input's values); C % 4 != 0 raises."""
    from ccst_amd.nets import layers
    x, _ = mixstyle_input((4, 32, 7, 7), 5)
    xd = x.to(dev)
    ms = layers.MixStyle(p=1.0)
    assert ms.eval()(xd) is xd
    ms.train()
    ms.set_activation_status(False)
    assert ms(xd) is xd
    ms.set_activation_status(True)
    random.seed(1)
    torch.manual_seed(1)
    with torch.no_grad():
        a = ms(xd)                                            # NCHW in memory
    random.seed(1)
    torch.manual_seed(1)
    with torch.no_grad():
        b = ms(xd.contiguous(memory_format=torch.channels_last))
    assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="C % 4"):
        ms(torch.zeros(2, 6, 3, 3, device=dev))
    with pytest.raises(RuntimeError):
        layers.MixStyle(p=1.0, mix="crossdomain").train()(torch.zeros(3, 8, 3, 3, device=dev))


def _mixstyle_model_case(dev, g, arch, monkeypatch):
    """tests/test_resnet_gpu.py::_model_case for MixStyleResNet: one train step against the reference's, both generators seeded right
    before the train forward (the fixture's train_seed), the same gates at the three sites."""
    from ccst_amd import fed
    from ccst_amd.nets import models, resnet
    from oracle import resnet_ref as R
    seed, classes, nb, lr = int(g["seed"]), int(g["classes"]), int(g["nb"]), float(g["lr"])

    def tol(key):
        assert float(g["noise/" + key]) < 1e-4, ("fixture is ill-conditioned", key, float(g["noise/" + key]))
        return 1e-3

    model = models.get_network(arch)(types.SimpleNamespace(dg_method="MixStyle", mode="fedavg"), pretrained=False, classes=classes)
    assert isinstance(model, resnet.MixStyleResNet)
    model.mixstyle.p = float(g["mixstyle_p"])
    oracle = R.resnet18(classes) if arch == "resnet18" else R.resnet50(classes)
    model.load_state_dict(R.seeded_state_dict(oracle, seed, float(g["residual_gamma"]), float(g["fc_gain"])))
    model.to(dev)
    x, y = R.synth_batch(nb, 222, classes, seed=seed + 1)
    x, y = x.to(dev), y.to(dev)
    model.eval()
    with torch.no_grad():
        d = float((model(x).cpu() - torch.from_numpy(g["logit_eval"])).abs().max())
    assert d < tol("logit_eval"), "eval logits %g" % d
    model.train()
    opt = fed.SGD(model, lr=lr)
    ce = fed.CrossEntropyLoss()
    opt.zero_grad()
    spy = DrawSpy(monkeypatch)
    random.seed(int(g["train_seed"]))
    torch.manual_seed(int(g["train_seed"]))
    logit = model(x)
    assert [d_ is not None for d_ in spy.draws] == [float(v) <= float(g["mixstyle_p"]) for v in g["gates"]]
    loss = ce(logit, y)
    loss.backward()
    d = float((logit.detach().cpu() - torch.from_numpy(g["logit_train"])).abs().max())
    assert d < tol("logit_train"), "train logits %g" % d
    assert abs(float(loss.detach()) - float(g["loss"])) < tol("loss")
    named = dict(model.named_parameters())
    for k in g.files:
        if k.startswith("grad_abs/"):
            name = k[9:]
            got = float(named[name].grad.abs().sum())
            assert abs(got - float(g[k])) < 1e-3 * float(g[k]) + NOISE_MULT * float(g["noise/" + k]) + 1e-6, (name, got, float(g[k]))
        if k.startswith("grad_head/"):
            name = k[10:]
            ref = torch.from_numpy(g[k])
            got = named[name].grad.flatten()[:ref.numel()].cpu()
            scale = float(g["grad_abs/" + name]) / named[name].numel()
            d = float((got - ref).abs().max())
            noise = max(NOISE_MULT * float(g["noise/" + k]), 2.0 * float(g["noise_full/grad/" + name]))
            assert d < 1e-3 * max(scale, float(ref.abs().max())) + noise + 1e-6, (name, d)
    opt.step()
    sd = model.state_dict()
    for k in g.files:
        if k.startswith("state/"):
            ref = torch.from_numpy(np.asarray(g[k]))
            got = sd[k[6:]].cpu()
            if ref.dtype == torch.int64:
                assert int(got) == int(ref)
            else:
                assert float((got - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max())), k
    model.eval()
    with torch.no_grad():
        d = float((model(x).cpu() - torch.from_numpy(g["logit_after"])).abs().max())
    assert d < tol("logit_after"), "post-step logits %g" % d


@pytest.mark.parametrize("name,arch", [("mixstyle_resnet18_step", "resnet18"), ("mixstyle_resnet18_p1_step", "resnet18"),
                                       ("mixstyle_resnet50_step", "resnet50")])
def test_mixstyle_resnet_step_golden(dev, golden, monkeypatch, name, arch):
    _mixstyle_model_case(dev, golden(name), arch, monkeypatch)


def test_no_link_crosses_mixstyle_and_masks_stay_right(dev, monkeypatch):
    """A MixStyle output is a new tensor: it carries no MaskLink (the closing BatchNorm applies its own ReLU mask in its backward), and
    the step's gradients with the short-cuts on equal those with all of them off (2e-5 of each tensor's largest entry)."""
    from ccst_amd import fed, nn_ops
    from ccst_amd.nets import models, resnet
    from oracle import resnet_ref as R
    classes, nb = 7, 4
    sd = R.seeded_state_dict(R.resnet18(classes), 55, residual_gamma=0.25, fc_gain=8.0)
    x, y = R.synth_batch(nb, 222, classes, seed=56)
    x, y = x.to(dev), y.to(dev)
    saved = (nn_ops.MASK_LINK, nn_ops.MASK_LINK_STATS, resnet.USE_GRAD_SINK)

    def run(on):
        nn_ops.MASK_LINK, nn_ops.MASK_LINK_STATS, resnet.USE_GRAD_SINK = on, on, on
        model = models.get_network("resnet18")(types.SimpleNamespace(dg_method="MixStyle"), pretrained=False, classes=classes)
        model.load_state_dict(sd)
        model.mixstyle.p = 1.0
        model.to(dev).train()
        seen = []
        model.mixstyle.register_forward_hook(lambda _m, i, o: seen.append((getattr(i[0], "_ccst_mask_link", None) is not None,
                                                                           hasattr(o, "_ccst_mask_link"), o is i[0])))
        random.seed(3)
        torch.manual_seed(3)
        model.zero_grad()
        fed.CrossEntropyLoss()(model(x), y).backward()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()}, seen
    try:
        g_on, seen = run(True)
        g_off, _ = run(False)
    finally:
        nn_ops.MASK_LINK, nn_ops.MASK_LINK_STATS, resnet.USE_GRAD_SINK = saved
    assert seen == [(True, False, False)] * 3, seen        # each site's input carried a link; the output carries none
    for k in g_off:
        assert float((g_on[k] - g_off[k]).abs().max()) <= 2e-5 * float(g_off[k].abs().max()) + 1e-9, k


def test_mixstyle_step_runs_the_half_piece_forward_with_words(dev):
    """No |max| pass behind a MixStyle site: in a MixStyle ResNet50 train step every pointwise conv -- those reading a site's output
    included -- gets the |max| words of its input."""
    from ccst_amd import fed, ops
    from ccst_amd.nets import models
    torch.manual_seed(3)
    model = models.get_network("resnet50")(types.SimpleNamespace(dg_method="MixStyle"), pretrained=False, classes=7).to(dev)
    model.mixstyle.p = 1.0
    model.train()
    opt, loss_fun = fed.SGD(model, lr=0.01), fed.CrossEntropyLoss()
    x, y = torch.randn(2, 3, 222, 222, device=dev), torch.randint(0, 7, (2,), device=dev)
    outs = []
    model.mixstyle.register_forward_hook(lambda _m, _i, o: outs.append(o.permute(0, 2, 3, 1).data_ptr()))
    seen = []
    real = ops.conv2d_nhwc

    def spy(xx, pc, *a, **k):
        if k.get("want_stats") and pc.kh == 1:
            seen.append((xx.data_ptr(), k.get("x_absmax") is not None))
        return real(xx, pc, *a, **k)
    ops.conv2d_nhwc = spy
    try:
        opt.zero_grad()
        loss = loss_fun(model(x), y)
        fed.backward(loss)
        opt.step()
    finally:
        ops.conv2d_nhwc = real
    torch.cuda.synchronize()
    assert len(outs) == 3 and seen and all(w for _, w in seen)
    readers = [p for p, _ in seen if p in outs]
    assert len(readers) == 6, readers                      # layer{2,3,4}.0: conv1 and the downsample conv read a site's output
    assert bool(torch.isfinite(loss))


@pytest.mark.parametrize("mode", [True, "auto"])
def test_fed_train_never_captures_mixstyle(dev, monkeypatch, mode):
    """args.hip_graph on or auto: a model with an active MixStyle trains eagerly -- new draws every step, the eager loop's results bit
    for bit."""
    from ccst_amd import fed
    from ccst_amd.nets import models
    from oracle import resnet_ref as R
    monkeypatch.setattr(fed, "AUTO_PROBE", 1)
    loader = [R.synth_batch(4, 222, 7, seed=500 + i) for i in range(5)]
    out = {}
    for m in (False, mode):
        args = types.SimpleNamespace(mode="fedavg", dg_method="MixStyle", hip_graph=m)
        model = models.get_network("resnet18")(args, pretrained=False, classes=7)
        model.load_state_dict(R.seeded_state_dict(R.resnet18(7), 11))
        model.mixstyle.p = 0.9
        spy = DrawSpy(monkeypatch)
        random.seed(8)
        torch.manual_seed(8)
        r = fed.train(model, loader, fed.SGD(model, lr=0.01), fed.CrossEntropyLoss(), 1, dev, args, 0, None)
        steps = model.__dict__.get("_ccst_graph_steps", {})
        assert not [k for k in steps if k not in ("_sums", "_auto")], steps          # nothing captured
        assert len(spy.draws) == 3 * len(loader)
        out[m] = (r, list(spy.draws), {k: v.detach().clone() for k, v in model.state_dict().items()})
    (r0, d0, s0), (r1, d1, s1) = out[False], out[mode]
    lam = [d[0] for d in d0 if d is not None]
    assert len(lam) >= 2 and not all(torch.equal(lam[0], v) for v in lam[1:])       # fresh draws per step
    assert len(d0) == len(d1) and all((a is None and b is None) or (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])) for a, b in zip(d0, d1))
    assert r0 == r1
    for k, v in s0.items():
        assert torch.equal(v, s1[k]), k


def test_fed_run_cli_mixstyle(dev, tmp_path):
    """fed_run.py --dg_method MixStyle end to end on synthetic clients (with --hip_graph, which it declines): two rounds, checkpoint,
    --resume."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    base = [sys.executable, os.path.join(root, "federated", "fed_run.py"), "--mode", "fedavg", "--fusion_mode", "adain-overall-K3",
            "--source", "art_painting", "cartoon", "sketch", "--target", "photo", "--n_classes", "7", "--network", "resnet18",
            "--lr", "0.001", "--image_size", "222", "--batch", "4", "--synthetic", "8", "--save_path", str(tmp_path / "ckpt"),
            "--dg_method", "MixStyle", "--hip_graph"]
    out = subprocess.check_output(base + ["--iters", "2"], cwd=str(tmp_path), env=env, text=True)
    assert "Insert MixStyle after the following layers" in out and "=============Global iter is 1 ===============" in out
    assert out.count("| Train Loss:") == 6 and "| Global Test Class Acc:" in out
    d = tmp_path / "ckpt" / "pacs" / "fedavg_adain-overall-K3_MixStyle_resnet18_locIter1" / "Target_photo_seed_1"
    latest = torch.load(str(d / "fedavg_latest"), map_location="cpu")
    from oracle import resnet_ref as R
    assert int(latest["a_iter"]) == 1 and list(latest["server_model"].keys()) == list(R.resnet18(7).state_dict().keys())
    if not (d / "fedavg").exists():
        import shutil
        shutil.copy(str(d / "fedavg_latest"), str(d / "fedavg"))
    out2 = subprocess.check_output(base + ["--iters", "3", "--resume"], cwd=str(tmp_path), env=env, text=True)
    assert "Resume training from epoch 2" in out2 and "Global iter is 2" in out2
