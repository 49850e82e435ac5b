"""Drop-in for nets/layers.py: MixStyle (Zhou et al., Domain Generalization with MixStyle, ICLR 2021) on HIP kernels.

The draws are the reference's, made on the host in its order from the same generators: the gate ``random.random()``, then
lambda ~ ``Beta(alpha, alpha).sample((B, 1, 1, 1))`` and ``torch.randperm`` on the CPU default generator -- so with the same seeds the
same images are mixed with the same weights, and both generators end in the same state.  The statistics, the mixing and the
re-normalisation run on the device (include/ccst_mixstyle.h): three launches forward, one backward.
"""
import random

import torch
import torch.nn as nn

from .. import nn_ops, ops


def draw(mix, p, beta, B):
    """The reference's draws for a batch of B in training: None when the gate leaves x unchanged, else (lambda float32 [B], perm int64
    [B]), both on the host.  'crossdomain' swaps the two halves of the batch, each shuffled; an odd B fails as it does there."""
    if random.random() > p:
        return None
    lmda = beta.sample((B, 1, 1, 1)).reshape(B)
    if mix == 'random':
        perm = torch.randperm(B)
    elif mix == 'crossdomain':
        perm = torch.arange(B - 1, -1, -1)
        perm_b, perm_a = perm.chunk(2)
        perm_b = perm_b[torch.randperm(B // 2)]
        perm_a = perm_a[torch.randperm(B // 2)]
        perm = torch.cat([perm_b, perm_a], 0)
        if perm.numel() != B:
            raise RuntimeError("MixStyle(mix='crossdomain') needs an even batch (got %d)" % B)
    else:
        raise NotImplementedError
    return lmda, perm


def pack_draws(lmda, perm, device):
    """lambda's fp32 bits and perm as ONE int32 [2B] device tensor: a single non-blocking copy out of pinned memory, no host sync
    (the pinned block is recycled only after the copy has run)."""
    B = perm.numel()
    if not bool(((perm >= 0) & (perm < B)).all()):
        raise RuntimeError("MixStyle: permutation index outside [0, %d)" % B)
    host = torch.empty(2 * B, dtype=torch.int32, pin_memory=True)
    host[:B] = lmda.to(torch.float32).view(torch.int32)
    host[B:] = perm.to(torch.int32)
    return host.to(device, non_blocking=True)


class MixStyle(nn.Module):
    """MixStyle (nets/layers.py:6-73).  Eval mode, a deactivated module and a closed gate return x itself."""

    def __init__(self, p=0.5, alpha=0.1, eps=1e-6, mix='random'):
        super().__init__()
        self.p = p
        self.beta = torch.distributions.Beta(alpha, alpha)
        self.eps = eps
        self.alpha = alpha
        self.mix = mix
        self._activated = True

    def __repr__(self):
        return f'MixStyle(p={self.p}, alpha={self.alpha}, eps={self.eps}, mix={self.mix})'

    def set_activation_status(self, status=True):
        self._activated = status

    def update_mix_method(self, mix='random'):
        self.mix = mix

    def forward(self, x):
        if not self.training or not self._activated:
            return x
        if not x.is_cuda:
            raise RuntimeError("ccst_amd.nets: MixStyle runs on CUDA (ROCm) tensors only; no CPU fallback")
        if x.dim() != 4 or x.shape[1] % 4 != 0:
            raise RuntimeError("ccst_amd.nets: MixStyle needs a 4-d tensor with C %% 4 == 0, got %s" % (tuple(x.shape),))
        d = draw(self.mix, self.p, self.beta, x.size(0))
        if d is None:
            return x
        y = nn_ops.MixStyleFn.apply(ops.from_api(x), pack_draws(d[0], d[1], x.device), float(self.eps))
        return ops.carry_absmax(y, ops.to_api(y))
