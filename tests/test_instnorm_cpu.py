"""CPU: the InstanceNorm ResNet (--network resnet18IN) and --IN_test -- registry, seeded construction against the reference's own
initial weights (tests/golden/resnet18in_init.npz, tools/make_golden.py), the CLI gate and the extension C ABI
(include/ccst_instnorm.h).  No GPU needed."""
import ctypes
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(ccst_[a-z0-9_]+)\s*\(", text)))


@pytest.mark.parametrize("dg", ["no_DG", "MixStyle"])
def test_registry_builds_resnet18in(golden, dg):
    from ccst_amd.nets import models, resnet
    g = golden("resnet18in_init")
    m = models.get_network("resnet18IN")(types.SimpleNamespace(dg_method=dg), pretrained=True, classes=int(g["classes"]))
    assert type(m) is resnet.ResNetIN and isinstance(m, resnet.ResNet)
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    assert [n for n, _ in m.named_modules()] == [str(k) for k in g["module_names"]]
    assert [type(mm).__name__ for _, mm in m.named_modules()][1:] == [str(t) for t in g["module_types"]][1:]
    norms = [(n, mm) for n, mm in m.named_modules() if isinstance(mm, nn.InstanceNorm2d)]
    assert [n for n, _ in norms] == [str(k) for k in g["norm_names"]]
    assert [bool(mm.affine) for _, mm in norms] == [bool(a) for a in g["norm_affine"]]
    assert [bool(mm.track_running_stats) for _, mm in norms] == [bool(t) for t in g["norm_track"]]
    assert all(isinstance(mm, resnet.InstanceNorm2d) and not isinstance(mm, nn.BatchNorm2d) for _, mm in norms)
    assert not [mm for mm in m.modules() if isinstance(mm, nn.BatchNorm2d)]
    assert m.counter_arena() is None


def test_seeded_construction_is_the_references(golden):
    """torch.manual_seed(s) then construction gives the reference's initial weights: the base constructor's draws, then the rebuilt
    trunk's, then the kaiming loop's."""
    from ccst_amd.nets import models
    g = golden("resnet18in_init")
    for seed in [int(s) for s in g["seeds"]]:
        torch.manual_seed(seed)
        m = models.get_network("resnet18IN")(types.SimpleNamespace(dg_method="no_DG"), classes=int(g["classes"]))
        sd = m.state_dict()
        ksum = np.array([float(v.double().sum()) for v in sd.values()])
        kabs = np.array([float(v.double().abs().sum()) for v in sd.values()])
        # (torch's CPU normal_ takes a vectorised path that depends on the host's instruction set: the same draws, rounded alike
        # only on the same kind of CPU -- so the sums are held to fp32 rounding, which any other draw would miss by far)
        assert np.allclose(ksum, g["key_sum_%d" % seed], rtol=1e-5, atol=1e-4), (seed, np.abs(ksum - g["key_sum_%d" % seed]).max())
        assert np.allclose(kabs, g["key_abs_%d" % seed], rtol=1e-5, atol=1e-4), (seed, np.abs(kabs - g["key_abs_%d" % seed]).max())


def test_blocks_take_torchvision_keywords():
    from ccst_amd.nets import resnet
    b = resnet.BasicBlock(64, 64)
    assert isinstance(b.bn1, resnet.BatchNorm2d) and isinstance(b.bn2, resnet.BatchNorm2d)
    b = resnet.BasicBlock(64, 64, norm_layer=nn.InstanceNorm2d)
    assert type(b.bn1) is resnet.InstanceNorm2d and not b.bn1.affine
    b = resnet.Bottleneck(64, 16, norm_layer=resnet.InstanceNorm2d)
    assert all(type(getattr(b, n)) is resnet.InstanceNorm2d for n in ("bn1", "bn2", "bn3"))
    with pytest.raises(ValueError):
        resnet.BasicBlock(64, 64, groups=2)
    with pytest.raises(ValueError):
        resnet.BasicBlock(64, 64, base_width=32)
    with pytest.raises(NotImplementedError):
        resnet.BasicBlock(64, 64, dilation=2)
    with pytest.raises(NotImplementedError):
        resnet.Bottleneck(64, 16, groups=32)
    with pytest.raises(NotImplementedError):
        resnet.BasicBlock(64, 64, norm_layer=nn.GroupNorm)
    # the default BatchNorm ResNet is unchanged: same keys as the oracle's
    from oracle import resnet_ref as R
    assert list(resnet.ResNet(resnet.BasicBlock, [2, 2, 2, 2], classes=3).state_dict()) == list(R.resnet18(3).state_dict())


def test_instance_norm_module_needs_the_gpu():
    from ccst_amd.nets import resnet
    m = resnet.InstanceNorm2d(8, affine=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        m(torch.zeros(1, 8, 3, 3))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 8, 3, 3), stats=torch.zeros(1))


def test_in_test_swap_on_the_host():
    """fed.test(IN_test=True) no longer refuses: the swap (fed_run.py:218-229) happens before the first batch needs a device -- every
    BatchNorm becomes an affine InstanceNorm2d holding its weight and bias, the keys lose the running statistics, and the parameter
    arena is dropped rather than trusted."""
    from ccst_amd import fed
    from ccst_amd.nets import models, resnet
    from oracle import resnet_ref as R
    m = models.get_network("resnet18")(types.SimpleNamespace(dg_method="no_DG"), pretrained=False, classes=3)
    m.load_state_dict(R.seeded_state_dict(R.resnet18(3), 5))
    bn = {n: (mm.weight.detach().clone(), mm.bias.detach().clone(), mm.eps, mm.momentum) for n, mm in m.named_modules()
          if isinstance(mm, nn.BatchNorm2d)}
    m.__dict__["_ccst_arena"] = object()
    args = types.SimpleNamespace(IN_test=True, dg_method="no_DG")
    with pytest.raises(ZeroDivisionError):
        fed.test(m, [], fed.CrossEntropyLoss(), "cpu", args)                            # an empty loader: 0 / 0 after the swap
    assert "_ccst_arena" not in m.__dict__
    mods = dict(m.named_modules())
    for n, (w, b, eps, mom) in bn.items():
        IN = mods[n]
        assert type(IN) is resnet.InstanceNorm2d and IN.affine and not IN.track_running_stats
        assert (IN.eps, IN.momentum) == (eps, mom) and torch.equal(IN.weight, w) and torch.equal(IN.bias, b)
    keys = list(m.state_dict())
    assert not [k for k in keys if "running" in k or "num_batches" in k]
    assert keys == [k for k in R.resnet18(3).state_dict() if not ("running" in k or "num_batches" in k)]
    assert not fed.swap_bn_for_in(m, "cpu")                      # a second call swaps nothing


def _fed_run():
    spec = importlib.util.spec_from_file_location("ccst_fed_run_in", os.path.join(ROOT, "federated", "fed_run.py"))
    fr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fr)
    return fr


def test_fed_run_accepts_resnet18in_and_in_test(monkeypatch, tmp_path):
    """--network resnet18IN and --IN_test pass main()'s checks and stop at the device check on a host without the GPU; what stays out of
    scope is still refused."""
    fr = _fed_run()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = ["fed_run.py", "--mode", "fedavg", "--synthetic", "4", "--save_path", str(tmp_path)]
    for extra in (["--network", "resnet18IN"], ["--network", "resnet18", "--IN_test"], ["--network", "resnet18IN", "--mode", "fedbn"],
                  ["--network", "resnet18", "--IN_test", "--test"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(SystemExit, match="MI355X"):
            fr.main()
    for extra in (["--dg_method", "Jigsaw"], ["--dg_method", "RSC"], ["--mode", "fedprox"], ["--tent_test"]):
        monkeypatch.setattr(sys, "argv", base + ["--network", "resnet18IN"] + extra)
        with pytest.raises(NotImplementedError):
            fr.main()


def test_extension_abi_header_exports_and_binding():
    import __graft_entry__
    __graft_entry__.build()
    from ccst_amd import _lib
    syms = _header_symbols("ccst_instnorm.h")
    assert syms == sorted(_lib.INSTNORM_EXPORTS) == ["ccst_instnorm_abi_version", "ccst_instnorm_bwd_f32", "ccst_instnorm_fwd_f32",
                                                     "ccst_instnorm_workspace_bytes"]
    assert not set(syms) & set(_lib.EXPORTS) and sorted(_lib.EXPORTS) == _header_symbols("ccst_hip.h")
    assert not set(syms) & set(_lib.MIXSTYLE_EXPORTS)
    with open(os.path.join(ROOT, "include", "ccst_instnorm.h")) as f:
        assert re.search(r"#define\s+CCST_INSTNORM_ABI_VERSION\s+1\b", f.read())
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), "libccst_hip.so does not export %s" % s
    assert _lib.load_instnorm().ccst_instnorm_abi_version() == _lib.INSTNORM_ABI_VERSION == 1
    assert _lib.load().ccst_abi_version() == 2


def test_extension_bad_arguments_return_errors_without_a_gpu():
    """Every check runs before a launch: fake (never dereferenced) device addresses are enough to reach each one."""
    from ccst_amd import _lib
    lib = _lib.load_instnorm()
    P = ctypes.c_void_p
    x, g, b, y, mk, mu, isd, ws, dx = (P(a) for a in (4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768, 36864))
    nb = lib.ccst_instnorm_workspace_bytes(4, 9, 8)
    assert nb > 0 and lib.ccst_instnorm_workspace_bytes(4, 9, 6) == 0
    # the workspace of one image is a function of (HW, C) only: N images need N times one image's
    assert lib.ccst_instnorm_workspace_bytes(32, 12321, 64) == 32 * lib.ccst_instnorm_workspace_bytes(1, 12321, 64)
    fwd = lib.ccst_instnorm_fwd_f32
    assert fwd(None, g, b, None, 0, y, None, mu, isd, 4, 9, 8, 1e-5, ws, nb, None, None) == -1
    assert b"null" in lib.ccst_last_error()
    assert fwd(x, g, b, None, 0, y, None, mu, isd, 4, 9, 6, 1e-5, ws, nb, None, None) == -1        # C % 4 != 0
    assert b"bad shape" in lib.ccst_last_error()
    assert fwd(x, g, b, None, 0, y, None, mu, isd, 0, 9, 8, 1e-5, ws, nb, None, None) == -1
    assert fwd(x, g, None, None, 0, y, None, mu, isd, 4, 9, 8, 1e-5, ws, nb, None, None) == -1     # gamma without beta
    assert b"gamma and beta" in lib.ccst_last_error()
    assert fwd(x, g, b, None, 0, y, mk, mu, isd, 4, 9, 8, 1e-5, ws, nb, None, None) == -1          # mask without relu
    assert fwd(P(4100), g, b, None, 0, y, None, mu, isd, 4, 9, 8, 1e-5, ws, nb, None, None) == -1  # misaligned
    assert b"aligned" in lib.ccst_last_error()
    assert fwd(x, g, b, None, 0, y, None, mu, isd, 4, 9, 8, 1e-5, ws, nb - 1, None, None) == -2    # workspace
    assert b"workspace" in lib.ccst_last_error()
    bwd = lib.ccst_instnorm_bwd_f32
    assert bwd(x, None, None, None, 0, g, b, mu, isd, dx, None, None, None, 1, 4, 9, 8, ws, nb, None, None) == -1
    assert bwd(x, x, None, None, 1, g, None, mu, isd, dx, None, None, None, 1, 4, 9, 8, ws, nb, None, None) == -1   # no way to the mask
    assert bwd(x, x, None, None, 1, g, b, mu, isd, dx, y, None, None, 1, 4, 9, 8, ws, nb, None, None) == -1        # residual: mask needed
    assert bwd(x, x, None, None, 0, None, None, mu, isd, dx, None, y, None, 1, 4, 9, 8, ws, nb, None, None) == -1  # dgamma, non-affine
    assert bwd(x, x, None, None, 0, g, b, mu, isd, dx, None, None, None, 1, 4, 9, 8, ws, nb - 8, None, None) == -2
    assert bwd(x, x, None, None, 0, g, b, mu, isd, dx, None, None, None, 1, 70000, 9, 8, ws, nb, None, None) == -1
