"""On-device counterparts of the reference's waveform transforms that sit directly in front of the frontend
(utilities/data/raw_transforms.py): the crops are views, PeakNormalization is a HIP kernel.  They take batched device
tensors ``(B, T)`` or ``(B, 1, T)`` (the reference versions run per clip on the CPU inside DataLoader workers)."""
import random

import torch

from . import _native


class RandomCrop:
    """raw_transforms.py:121-127 -- a random window of ``size`` samples (one offset per call, shared by the batch)."""

    def __init__(self, size: int):
        self.size = size

    def __call__(self, signal: torch.Tensor) -> torch.Tensor:
        start = random.randint(0, signal.shape[-1] - self.size)
        return signal[..., start: start + self.size]


class CenterCrop:
    """raw_transforms.py:130-140 -- the central ``size`` samples; shorter inputs pass unchanged."""

    def __init__(self, size: int):
        self.size = size

    def __call__(self, signal: torch.Tensor) -> torch.Tensor:
        if signal.shape[-1] > self.size:
            start = (signal.shape[-1] - self.size) // 2
            return signal[..., start: start + self.size]
        return signal


class PeakNormalization:
    """raw_transforms.py:334-345 -- ``torch_audiomentations.PeakNormalization(apply_to="only_too_loud_sounds", p=1)``:
    every clip whose peak |x| exceeds 1 is divided by its peak, quieter clips are returned unchanged.  (The third-party
    package is not in this image: its documented behaviour is restated, parity unpinned.)"""

    def __init__(self, sr: int = 16000):
        self.sr = sr                      # kept for signature compatibility; the operation does not depend on it

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return _native.peak_normalize(x)


class Mixup:
    """utilities/data/mixup.py:5-26 (``do_mixup``) restated for a batch on the device, with the mix itself done by a HIP kernel
    (``_native.mixup``: fp32 or int16 PCM in, fp32 out, bit for bit the reference's ``inputs * lam + inputs[perms] * (1 - lam)``).
    One weight per clip from Beta(alpha, alpha) -- drawn from ``numpy.random.RandomState(random_seed)`` as the reference does, so a
    fixed seed gives the reference's weights -- and one permutation of the batch from torch's generator.

    ``__call__(inputs, targets)`` returns ``(mixed_x, a, b, lam_or_None, perm, lam)``: the reference's four values -- multilabel:
    ``(mixed_x, mixed_y, None, None)``, any other mode: ``(mixed_x, y_a, y_b, lam)`` -- followed by the permutation and the weights,
    so that a caller can hand ``(inputs, perm, lam)`` to ``Leaf.forward_mixup`` instead of the mixed batch.  ``mix_inputs=False``
    skips the waveform kernel for exactly that use (``mixed_x`` is then None).  The targets are mixed with stock ops."""

    def __init__(self, alpha: float = 1., random_seed=1233, mode: str = "multilabel", mix_inputs: bool = True):
        self.alpha = alpha
        self.random_seed = random_seed
        self.mode = mode
        self.mix_inputs = mix_inputs

    def __call__(self, inputs: torch.Tensor, targets: torch.Tensor):
        import numpy as np
        random_state = np.random.RandomState(self.random_seed)      # (re-seeded per call, as the reference's do_mixup)
        bsize = len(inputs)
        lam = torch.from_numpy(random_state.beta(self.alpha, self.alpha, bsize)).to(inputs.device).float()
        perms = torch.randperm(bsize).to(inputs.device)
        mixed_x = _native.mixup(inputs, perms, lam) if self.mix_inputs else None
        if self.mode == "multilabel":
            mixed_y = targets * lam.view(bsize, 1) + targets[perms] * (1 - lam.view(bsize, 1))
            return mixed_x, mixed_y, None, None, perms, lam
        return mixed_x, targets, targets[perms], lam, perms, lam
