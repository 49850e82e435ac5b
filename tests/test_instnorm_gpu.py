"""GPU: instance normalisation (include/ccst_instnorm.h, nets.resnet.InstanceNorm2d) against fp64 torch, bitwise determinism and
per-sample independence; the ResNetIN train step, fed.train / fed.test and --IN_test against the reference's own outputs
(tests/golden/resnet18in_step.npz, fed_loop_in.npz, in_test.npz; tools/make_golden.py); |max| words, HIP-graph replay and the CLI."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
NOISE_MULT = 7.0          # tests/test_resnet_gpu.py::_model_case's multiplier of the fixtures' own fp32 noise
ARGS = types.SimpleNamespace(dg_method="no_DG", mode="fedavg")
SHAPES = [(64, 111), (64, 56), (128, 28), (256, 14), (512, 7)]        # the ResNet18IN norm sites at 222 x 222
CONFIGS = [(True, False, True), (False, True, True), (True, True, False), (False, False, False)]     # (affine, residual, relu)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def in_input(N, C, H, seed, mean=1.0, sd=(0.5, 2.0)):
    g = torch.Generator().manual_seed(seed)
    mu = (torch.rand(N, C, 1, 1, generator=g) * 2 - 1) * mean
    s = sd[0] + (sd[1] - sd[0]) * torch.rand(N, C, 1, 1, generator=g)
    x = mu + s * torch.randn(N, C, H, H, generator=g)
    return x, torch.randn(N, C, H, H, generator=g), torch.randn(N, C, H, H, generator=g)


def cl(t, dev, grad=False):
    return t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def run_ours(dev, x, r, dy, affine, relu, w=None, b=None):
    """One forward + backward of nets.resnet.InstanceNorm2d; returns (y, dx, dres, dgamma, dbeta) on the host."""
    from ccst_amd.nets import resnet
    C = x.shape[1]
    m = resnet.InstanceNorm2d(C, affine=affine).to(dev).train()
    if affine:
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
    xd = cl(x, dev, True)
    rd = cl(r, dev, True) if r is not None else None
    y = m(xd, residual=rd, relu=relu)
    y.backward(cl(dy, dev))
    torch.cuda.synchronize()
    return (y.detach().cpu(), xd.grad.cpu(), rd.grad.cpu() if rd is not None else None,
            m.weight.grad.cpu() if affine else None, m.bias.grad.cpu() if affine else None)


def run_fp64(dev, x, r, dy, affine, relu, w=None, b=None, y32=None):
    """The same in fp64 torch.  y32: our output -- the ReLU then keeps exactly the elements ours kept (y32 > 0): a pre-activation within
    fp32 rounding of 0 may fall on either side, and one element on the other side moves its dx by O(|dy|)."""
    xd = x.to(dev).double().requires_grad_(True)
    wd = w.to(dev).double().requires_grad_(True) if affine else None
    bd = b.to(dev).double().requires_grad_(True) if affine else None
    rd = r.to(dev).double().requires_grad_(True) if r is not None else None
    y = F.instance_norm(xd, weight=wd, bias=bd, eps=1e-5)
    if rd is not None:
        y = y + rd
    if relu:
        y = torch.where(y32.to(dev) > 0, y, torch.zeros_like(y)) if y32 is not None else F.relu(y)
    y.backward(dy.to(dev).double())
    return (y.detach().cpu(), xd.grad.cpu(), rd.grad.cpu() if rd is not None else None,
            wd.grad.cpu() if affine else None, bd.grad.cpu() if affine else None)


def rel(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.mark.parametrize("C,H", SHAPES)
def test_op_against_fp64(dev, C, H):
    N = 32
    x, r, dy = in_input(N, C, H, seed=C + H)
    g = torch.Generator().manual_seed(7 * C)
    w, b = 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g)
    for affine, res, relu in CONFIGS:
        args = (x, r if res else None, dy, affine, relu, w, b)
        got = run_ours(dev, *args)
        ref = run_fp64(dev, *args, y32=got[0])
        tag = (C, H, affine, res, relu)
        assert rel(got[0], ref[0]) <= 4e-6, (tag, "y", rel(got[0], ref[0]))
        for i, name in ((1, "dx"), (2, "dres"), (3, "dgamma"), (4, "dbeta")):
            if ref[i] is not None:
                assert rel(got[i], ref[i]) <= 1e-5, (tag, name, rel(got[i], ref[i]))


@pytest.mark.parametrize("C,H", [(64, 56), (256, 14)])
def test_ill_conditioned_statistics(dev, C, H):
    """|mean| / sigma ~ 200 (means up to 20, sigmas 0.1): an E[x^2] - mu^2 form in fp32 loses the variance entirely here."""
    x, r, dy = in_input(8, C, H, seed=3 + C, mean=20.0, sd=(0.1, 0.1))
    w, b = torch.ones(C), torch.zeros(C)
    for affine, res, relu in CONFIGS:
        args = (x, r if res else None, dy, affine, relu, w, b)
        got = run_ours(dev, *args)
        ref = run_fp64(dev, *args, y32=got[0])
        assert rel(got[0], ref[0]) <= 4e-6, ("y", affine, res, relu, rel(got[0], ref[0]))
        for i in (1, 3, 4):
            if ref[i] is not None:
                assert rel(got[i], ref[i]) <= 1e-5, (i, affine, res, relu, rel(got[i], ref[i]))


def test_bitwise_determinism_and_independence(dev):
    """Two runs give the same bits; image n's y and dx are the same bits alone and beside batch-mates -- an outlier 2^17 brighter
    among them."""
    for C, H in [(64, 111), (128, 28), (512, 7)]:
        x, r, dy = in_input(6, C, H, seed=11 + C)
        x[3] *= 2.0 ** 17
        g = torch.Generator().manual_seed(C)
        w, b = 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g)
        for affine, res, relu in CONFIGS[:2]:
            a1 = run_ours(dev, x, r if res else None, dy, affine, relu, w, b)
            a2 = run_ours(dev, x, r if res else None, dy, affine, relu, w, b)
            for u, v in zip(a1, a2):
                assert u is None or torch.equal(u, v)
            for n in (0, 5):
                one = run_ours(dev, x[n:n + 1], r[n:n + 1] if res else None, dy[n:n + 1], affine, relu, w, b)
                assert torch.equal(one[0][0], a1[0][n]) and torch.equal(one[1][0], a1[1][n]), (C, H, n, affine, res)


def test_resnet18in_step_golden(dev, golden):
    from ccst_amd import fed
    from ccst_amd.nets import models
    from oracle import resnet_ref as R
    g = golden("resnet18in_step")
    seed, classes, nb, lr = int(g["seed"]), int(g["classes"]), int(g["nb"]), float(g["lr"])

    def tol(key):
        return 1e-3 + NOISE_MULT * float(g["noise/" + key])

    model = models.get_network("resnet18IN")(ARGS, classes=classes)
    model.load_state_dict(R.seeded_state_dict(model, seed, float(g["residual_gamma"]), float(g["fc_gain"])))
    model.to(dev)
    x, y = R.synth_batch(nb, 222, classes, seed=seed + 1)
    x, y = x.to(dev), y.to(dev)
    model.eval()
    with torch.no_grad():
        d = float((model(x).cpu() - torch.from_numpy(g["logit_eval"])).abs().max())
    assert d < tol("logit_eval"), "eval logits %g" % d
    model.train()
    opt, ce = fed.SGD(model, lr=lr), fed.CrossEntropyLoss()
    opt.zero_grad()
    logit = model(x)
    loss = ce(logit, y)
    fed.backward(loss)
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
            noise = max(NOISE_MULT * float(g["noise/" + k]), 2.0 * float(g["noise_full/grad/" + name]))
            assert float((got - ref).abs().max()) < 1e-3 * max(scale, float(ref.abs().max())) + noise + 1e-6, name
    opt.step()
    sd = model.state_dict()
    for k in g.files:
        if k.startswith("state/"):
            ref = torch.from_numpy(np.asarray(g[k]))
            assert float((sd[k[6:]].cpu() - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max())), k
    model.eval()
    with torch.no_grad():
        d = float((model(x).cpu() - torch.from_numpy(g["logit_after"])).abs().max())
    assert d < tol("logit_after"), "post-step logits %g" % d


def test_fed_loop_in_golden(dev, golden):
    """fed.train / fed.test on a small ResNetIN against the reference's own loops."""
    from ccst_amd import fed
    from ccst_amd.nets import resnet
    from oracle import resnet_ref as R
    g = golden("fed_loop_in")
    ours = resnet.ResNetIN(resnet.BasicBlock, [1, 1, 1, 1], classes=3)
    ours.load_state_dict(R.seeded_state_dict(ours, int(g["seed"])))
    train_loader = [R.synth_batch(int(n), 222, 3, seed=int(s)) for s, n in zip(g["train_seeds"], g["train_sizes"])]
    test_loader = [R.synth_batch(int(n), 222, 3, seed=int(s)) for s, n in zip(g["test_seeds"], g["test_sizes"])]
    ours.to(dev)
    opt, ce = fed.SGD(ours, lr=float(g["lr"])), fed.CrossEntropyLoss()
    tr1 = fed.train(ours, train_loader, opt, ce, 3, dev, ARGS, 0, None)
    te1 = fed.test(ours, test_loader, ce, dev, ARGS)
    tr2 = fed.train(ours, train_loader, opt, ce, 3, dev, ARGS, 1, None)
    te2 = fed.test(ours, train_loader, ce, dev, ARGS)
    for got, key in ((tr1, "train1"), (te1, "test1"), (tr2, "train2"), (te2, "test2")):
        assert abs(got[0] - float(g[key][0])) < 1e-3, (key, got, g[key])
        assert got[1] == float(g[key][1]), (key, got, g[key])
    sd = ours.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    for key, name in (("conv1_head", "conv1.weight"), ("fc_weight", "class_classifier.weight"), ("fc_bias", "class_classifier.bias"),
                      ("bn1_weight", "bn1.weight"), ("bn1_bias", "bn1.bias")):
        ref = torch.from_numpy(g[key]).flatten()
        got = sd[name].flatten()[:ref.numel()].cpu()
        assert float((got - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max())), key
    assert np.allclose(np.array([float(v.double().abs().sum()) for v in sd.values()]), g["key_abs"], rtol=1e-3)


def test_in_test_golden_and_following_communication(dev, golden):
    """fed.test(IN_test=True) on BatchNorm ResNets against the reference's test(): loss, accuracy, the state-dict keys afterwards, a
    second call identical; then the reference's communication() with the swapped server and BatchNorm clients."""
    import copy
    from ccst_amd import fed
    from ccst_amd.nets import resnet
    from oracle import resnet_ref as R
    g = golden("in_test")
    args = types.SimpleNamespace(dg_method="no_DG", mode="fedavg", IN_test=True)
    ce = fed.CrossEntropyLoss()
    for tag, block, layers in (("r18", resnet.BasicBlock, [1, 1, 1, 1]), ("r50", resnet.Bottleneck, [3, 4, 6, 3])):
        seed, classes = int(g[tag + "/seed"]), int(g[tag + "/classes"])
        oblock = R.BasicBlock if tag == "r18" else R.Bottleneck
        m = resnet.ResNet(block, layers, classes=classes)
        m.load_state_dict(R.seeded_state_dict(R.ResNet(oblock, layers, classes=classes), seed))
        m.to(dev)
        bn_copy = copy.deepcopy(m)
        assert list(m.state_dict()) == [str(k) for k in g[tag + "/bn_keys"]]
        loader = [R.synth_batch(n, 222, classes, seed=300 + seed + i) for i, n in enumerate((4, 2))]
        r1 = fed.test(m, loader, ce, dev, args)
        assert list(m.state_dict()) == [str(k) for k in g[tag + "/keys"]]
        r2 = fed.test(m, loader, ce, dev, args)
        assert r1 == r2
        for got, key in ((r1, "/test1"), (r2, "/test2")):
            assert abs(got[0] - float(g[tag + key][0])) < 1e-3, (tag, got, g[tag + key])
            assert got[1] == float(g[tag + key][1]), (tag, got, g[tag + key])
        if tag == "r18":
            clients = [copy.deepcopy(bn_copy) for _ in range(3)]
            for ci, c in enumerate(clients):
                rs = np.random.RandomState(400 + ci)
                with torch.no_grad():
                    for k, v in c.state_dict().items():
                        if "num_batches_tracked" in k:
                            v.fill_(5 + ci)
                        else:
                            v += torch.from_numpy(rs.normal(0, 0.02, tuple(v.shape)).astype(np.float32)).to(dev)
            srv, clients = fed.communication(args, m, clients, [float(w) for w in g["weights"]])
            torch.cuda.synchronize()
            assert list(srv.state_dict()) == [str(k) for k in g["comm/server_keys"]]
            ssum = np.array([float(v.double().sum()) for v in srv.state_dict().values()])
            sabs = np.array([float(v.double().abs().sum()) for v in srv.state_dict().values()])
            assert np.allclose(ssum, g["comm/server_sum"], rtol=1e-5, atol=1e-4) and np.allclose(sabs, g["comm/server_abs"], rtol=1e-5)
            for ci, c in enumerate(clients):
                assert list(c.state_dict()) == [str(k) for k in g["comm/client_keys"]]
                csum = np.array([float(v.double().sum()) for v in c.state_dict().values()])
                assert np.allclose(csum, g["comm/client%d_sum" % ci], rtol=1e-5, atol=1e-4), ci
            # the swapped server still evaluates and trains (its arena was rebuilt from the live modules)
            fed.test(srv, loader, ce, dev, args)


def test_resnet18in_step_passes_words(dev):
    """Every pointwise conv of a ResNetIN train step runs its half-piece forward with the |max| words of its input, and every weight
    gradient gets the words of its dy from the InstanceNorm backward in front of it."""
    from ccst_amd import fed, nn_ops, ops
    from ccst_amd.nets import models
    torch.manual_seed(3)
    model = models.get_network("resnet18IN")(ARGS, classes=7).to(dev).train()
    opt, loss_fun = fed.SGD(model, lr=0.01), fed.CrossEntropyLoss()
    x, y = torch.randn(2, 3, 222, 222, device=dev), torch.randint(0, 7, (2,), device=dev)
    fwd, bwd = [], []
    real_fwd, real_bwd = ops.conv2d_nhwc, nn_ops.conv_bwd_weight

    def spy_fwd(xx, pc, *a, **k):
        if pc.kh == 1:
            fwd.append(k.get("x_absmax") is not None)
        return real_fwd(xx, pc, *a, **k)

    def spy_bwd(d, xx, dy, *a, **k):
        bwd.append(k.get("dy_absmax") is not None)
        return real_bwd(d, xx, dy, *a, **k)
    ops.conv2d_nhwc, nn_ops.conv_bwd_weight = spy_fwd, spy_bwd
    try:
        opt.zero_grad()
        loss = loss_fun(model(x), y)
        fed.backward(loss)
        opt.step()
    finally:
        ops.conv2d_nhwc, nn_ops.conv_bwd_weight = real_fwd, real_bwd
    torch.cuda.synchronize()
    assert len(fwd) == 3 and all(fwd), fwd                   # the downsample convs of layer2..4
    assert len(bwd) == 20 and all(bwd), bwd                  # every conv of the net
    assert bool(torch.isfinite(loss))


def test_fed_train_hip_graph_matches_eager(dev):
    """fed.train(hip_graph=1) on a ResNetIN: the replayed steps give the eager loop's bits."""
    from ccst_amd import fed
    from ccst_amd.nets import models
    from oracle import resnet_ref as R
    loader = [R.synth_batch(4, 222, 7, seed=600 + i) for i in range(6)]
    out = {}
    for mode in (False, 1):
        args = types.SimpleNamespace(mode="fedavg", dg_method="no_DG", hip_graph=mode)
        model = models.get_network("resnet18IN")(args, classes=7)
        model.load_state_dict(R.seeded_state_dict(model, 12))
        r = fed.train(model, loader, fed.SGD(model, lr=0.01), fed.CrossEntropyLoss(), 1, dev, args, 0, None)
        steps = model.__dict__.get("_ccst_graph_steps", {})
        captured = [k for k in steps if k not in ("_sums", "_auto")]
        assert bool(captured) == bool(mode), steps
        out[mode] = (r, {k: v.detach().clone() for k, v in model.state_dict().items()})
    (r0, s0), (r1, s1) = out[False], out[1]
    assert r0 == r1
    for k, v in s0.items():
        assert torch.equal(v, s1[k]), k


def test_fed_run_cli_resnet18in_and_in_test(dev, tmp_path):
    """fed_run.py --network resnet18IN end to end on synthetic clients (fedavg, fedbn); then --test --IN_test on the checkpoint of a
    resnet18 run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)

    def cli(net, mode, extra, save):
        return [sys.executable, os.path.join(root, "federated", "fed_run.py"), "--mode", mode, "--fusion_mode", "adain-overall-K3",
                "--source", "art_painting", "cartoon", "sketch", "--target", "photo", "--n_classes", "7", "--network", net,
                "--lr", "0.001", "--image_size", "222", "--batch", "4", "--synthetic", "8", "--save_path", str(save)] + extra
    from oracle import resnet_ref as R
    for mode in ("fedavg", "fedbn"):
        out = subprocess.check_output(cli("resnet18IN", mode, ["--iters", "2"], tmp_path / ("in_" + mode)), cwd=str(tmp_path), env=env,
                                      text=True, timeout=900)
        assert out.count("| Train Loss:") == 6 and "| Global Test Class Acc:" in out, out
        d = tmp_path / ("in_" + mode) / "pacs" / ("%s_adain-overall-K3_no_DG_resnet18IN_locIter1" % mode) / "Target_photo_seed_1"
        latest = torch.load(str(d / ("%s_latest" % mode)), map_location="cpu")
        assert "bn1.weight" in latest["server_model"] and not [k for k in latest["server_model"] if "running" in k]
    save = tmp_path / "bn"
    subprocess.check_output(cli("resnet18", "fedavg", ["--iters", "2"], save), cwd=str(tmp_path), env=env, text=True, timeout=900)
    d = save / "pacs" / "fedavg_adain-overall-K3_no_DG_resnet18_locIter1" / "Target_photo_seed_1"
    if not (d / "fedavg").exists():
        import shutil
        shutil.copy(str(d / "fedavg_latest"), str(d / "fedavg"))
    assert list(torch.load(str(d / "fedavg"), map_location="cpu")["server_model"]) == list(R.resnet18(7).state_dict())
    out = subprocess.check_output(cli("resnet18", "fedavg", ["--test", "--IN_test"], save), cwd=str(tmp_path), env=env, text=True,
                                  timeout=600)
    assert "photo      | Test  Acc:" in out or "| Test  Acc:" in out, out
