"""CPU: MixStyle (--dg_method MixStyle) -- registries, the reference's host-side draws, the CLI gate and the extension C ABI
(include/ccst_mixstyle.h).  No GPU needed."""
import ctypes
import importlib.util
import os
import random
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(ccst_[a-z0-9_]+)\s*\(", text)))


@pytest.mark.parametrize("arch,dg", [("resnet18", "MixStyle"), ("resnet50", "mixstyle")])
def test_registries_build_mixstyle_resnet(arch, dg, capsys, golden):
    from ccst_amd.nets import layers, models, resnet
    from oracle import resnet_ref as R
    m = models.get_network(arch)(types.SimpleNamespace(dg_method=dg), pretrained=False, classes=7)
    assert type(m) is resnet.MixStyleResNet and isinstance(m, resnet.ResNet)
    assert "Insert MixStyle after the following layers: ['layer1', 'layer2', 'layer3']" in capsys.readouterr().out
    ref = R.resnet18(7) if arch == "resnet18" else R.resnet50(7)
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    assert m.mixstyle_layers == ["layer1", "layer2", "layer3"]
    ms = m.mixstyle
    assert isinstance(ms, layers.MixStyle) and (ms.p, ms.alpha, ms.eps, ms.mix) == (0.5, 0.1, 1e-6, "random")
    assert repr(ms) == str(golden("mixstyle_module")["repr"]) == "MixStyle(p=0.5, alpha=0.1, eps=1e-06, mix=random)"
    plain = resnet.MixStyleResNet(resnet.BasicBlock, [1, 1, 1, 1], classes=3)
    assert plain.mixstyle is None and plain.mixstyle_layers == []
    with pytest.raises(NotImplementedError):
        models.get_network(arch)(types.SimpleNamespace(dg_method="Jigsaw"), pretrained=False, classes=7)


def test_module_surface_on_the_host():
    from ccst_amd.nets import layers
    ms = layers.MixStyle(p=1.0)
    x = torch.randn(2, 8, 3, 3)
    assert ms.eval()(x) is x                          # eval: identity
    ms.train()
    ms.set_activation_status(False)
    assert ms(x) is x                                 # deactivated: identity
    ms.set_activation_status(True)
    ms.update_mix_method("crossdomain")
    assert ms.mix == "crossdomain" and repr(ms) == "MixStyle(p=1.0, alpha=0.1, eps=1e-06, mix=crossdomain)"
    with pytest.raises(RuntimeError, match="CUDA"):
        ms(x)                                         # training on the host: no CPU path
    random.seed(0)
    with pytest.raises(RuntimeError, match="even batch"):
        layers.draw("crossdomain", 1.0, ms.beta, 5)   # the reference fails on an odd batch too
    with pytest.raises(NotImplementedError):
        layers.draw("bogus", 1.0, ms.beta, 4)


def test_host_draws_are_the_references(golden):
    """With the reference's seeds the helper draws the same lambda and perm, and leaves random / torch where the reference's
    forward left them (the fixture's post-forward probes)."""
    from ccst_amd.nets import layers
    g = golden("mixstyle_module")
    for name in [str(c) for c in g["cases"]]:
        mix = name.split("_", 1)[1]
        B, seed = int(g[name + "/shape"][0]), int(g[name + "/seed"])
        ms = layers.MixStyle(p=1.0, mix=mix)
        random.seed(seed)
        torch.manual_seed(seed)
        lmda, perm = layers.draw(ms.mix, ms.p, ms.beta, B)
        assert lmda.dtype == torch.float32 and torch.equal(lmda, torch.from_numpy(g[name + "/lmda"])), name
        assert torch.equal(perm, torch.from_numpy(g[name + "/perm"])), name
        assert random.random() == float(g[name + "/probe_random"]), name
        assert torch.equal(torch.rand(4), torch.from_numpy(g[name + "/probe_torch"])), name
    ms = layers.MixStyle(p=0.5)
    seed = int(g["seq/seed"])
    random.seed(seed)
    torch.manual_seed(seed)
    B = int(g["seq/shape"][0])
    for k in range(int(g["seq/K"])):
        d = layers.draw(ms.mix, ms.p, ms.beta, B)
        assert (d is not None) == bool(g["seq/fired"][k]), k
        if d is not None:
            assert torch.equal(d[0], torch.from_numpy(g["seq/lmda"][k])) and torch.equal(d[1], torch.from_numpy(g["seq/perm"][k])), k
    assert random.random() == float(g["seq/probe_random"])
    assert torch.equal(torch.rand(4), torch.from_numpy(g["seq/probe_torch"]))


def _fed_run():
    spec = importlib.util.spec_from_file_location("ccst_fed_run_ms", os.path.join(ROOT, "federated", "fed_run.py"))
    fr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fr)
    return fr


def test_fed_run_accepts_mixstyle(monkeypatch, tmp_path):
    """--dg_method MixStyle passes main()'s method check and stops at the device check on a host without the GPU; Jigsaw is refused."""
    fr = _fed_run()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["fed_run.py", "--mode", "fedavg", "--network", "resnet18", "--synthetic", "4", "--save_path", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", base + ["--dg_method", "MixStyle"])
    with pytest.raises(SystemExit, match="MI355X"):
        fr.main()
    for mode in ("fedbn", "deepall"):
        monkeypatch.setattr(sys, "argv", base[:2] + [mode] + base[3:] + ["--dg_method", "MixStyle"])
        with pytest.raises(SystemExit, match="MI355X"):
            fr.main()
    for dg in ("Jigsaw", "RSC", "feddg"):
        monkeypatch.setattr(sys, "argv", base + ["--dg_method", dg])
        with pytest.raises(NotImplementedError):
            fr.main()


def test_fed_train_refuses_what_stays_out_of_scope():
    from ccst_amd import fed
    for dg in ("RSC", "Jigsaw"):
        with pytest.raises(NotImplementedError):
            fed.train(None, [], None, None, 1, "cpu", types.SimpleNamespace(dg_method=dg), 0, None)


def test_extension_abi_header_exports_and_binding():
    import __graft_entry__
    __graft_entry__.build()
    from ccst_amd import _lib
    syms = _header_symbols("ccst_mixstyle.h")
    assert syms == sorted(_lib.MIXSTYLE_EXPORTS) == ["ccst_mixstyle_abi_version", "ccst_mixstyle_bwd_f32", "ccst_mixstyle_fwd_f32"]
    assert not set(syms) & set(_lib.EXPORTS) and sorted(_lib.EXPORTS) == _header_symbols("ccst_hip.h")
    with open(os.path.join(ROOT, "include", "ccst_mixstyle.h")) as f:
        assert re.search(r"#define\s+CCST_MIXSTYLE_ABI_VERSION\s+1\b", f.read())
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), "libccst_hip.so does not export %s" % s
    assert _lib.load_mixstyle().ccst_mixstyle_abi_version() == _lib.MIXSTYLE_ABI_VERSION == 1
    assert _lib.load().ccst_abi_version() == 2


def test_extension_bad_arguments_return_errors_without_a_gpu():
    """Every check runs before a launch: fake (never dereferenced) device addresses are enough to reach each one."""
    from ccst_amd import _lib
    lib = _lib.load_mixstyle()
    P = ctypes.c_void_p
    x, lam, perm, y, mean, std, ws = (P(a) for a in (4096, 8192, 12288, 16384, 20480, 24576, 28672))
    nb = lib.ccst_stats_workspace_bytes(4, 8, 9)
    assert lib.ccst_mixstyle_fwd_f32(None, lam, perm, y, mean, std, 4, 8, 9, 1e-6, ws, nb, None, None) == -1
    assert b"null" in lib.ccst_last_error()
    assert lib.ccst_mixstyle_fwd_f32(x, lam, perm, y, mean, std, 4, 6, 9, 1e-6, ws, nb, None, None) == -1       # C % 4 != 0
    assert b"bad shape" in lib.ccst_last_error()
    assert lib.ccst_mixstyle_fwd_f32(x, lam, perm, y, mean, std, 0, 8, 9, 1e-6, ws, nb, None, None) == -1
    assert lib.ccst_mixstyle_fwd_f32(P(4100), lam, perm, y, mean, std, 4, 8, 9, 1e-6, ws, nb, None, None) == -1  # misaligned
    assert b"aligned" in lib.ccst_last_error()
    assert lib.ccst_mixstyle_fwd_f32(x, lam, perm, y, mean, std, 4, 8, 9, 1e-6, ws, nb - 1, None, None) == -2    # workspace
    assert b"workspace" in lib.ccst_last_error()
    assert lib.ccst_mixstyle_bwd_f32(x, None, lam, perm, y, 4, 8, 9, None) == -1
    assert lib.ccst_mixstyle_bwd_f32(x, std, lam, perm, y, 4, 10, 9, None) == -1
    assert lib.ccst_mixstyle_bwd_f32(x, std, lam, perm, y, 70000, 8, 9, None) == -1
