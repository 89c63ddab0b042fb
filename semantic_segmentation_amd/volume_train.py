"""The training loop of GenSeg-3D/train_unet.py:137-187 on raw (image, mask) pairs, every step on the device.

    criterion = CrossEntropyLoss(weight=torch.Tensor(BCE_WEIGHTS))             # train_unet.py:135, config.py:35
    optimizer = Adam(params=net.parameters())                                   # :137
    scheduler = CosineAnnealingLR(optimizer, T_max=500, eta_min=1e-9)           # :138

`VolumeTrainer` ties the pieces that exist one by one: volume.VolumePrep (the item transform of transforms.py: flips, normalise,
pad to a multiple of 16), the UNet3D engine, losses.weighted_cross_entropy (the criterion; in validation the same launch also
writes the arg-max label map), volume.label_dice (dice_score of :37-51), the fused optim.Adam.  The reference calls
`loss.item()` at every step (:159, :171); here the per-step losses stay on the device and each epoch / validation round reads
ONE number back.  Capturing the step into a hipGraph is not part of this module."""
from __future__ import annotations

from typing import Optional

import torch

from .losses import weighted_cross_entropy
from .optim import Adam
from .volume import VolumePrep, label_dice


class VolumeTrainer:
    """net: a UNet3D on the GPU; train_batches / val_batches: sequences (re-iterable) of raw (image, mask) pairs as
    VolumePrep.prepare takes them (image fp32 [D,H,W], [C,D,H,W] or [N,C,D,H,W]; mask integer class indices), on the GPU;
    class_weights: the criterion's weights (None = unweighted); lr / t_max / eta_min: Adam and CosineAnnealingLR as the reference
    sets them; prep: the training transform (default VolumePrep(flip_prob=0.5), transforms.py:69-76) -- validation uses the same
    object without flips."""

    def __init__(self, net, train_batches, val_batches, class_weights=(0.004, 0.996), lr: float = 1e-3, t_max: int = 500,
                 eta_min: float = 1e-9, prep: Optional[VolumePrep] = None):
        self.net = net
        self.train_batches, self.val_batches = train_batches, val_batches
        self.class_weights = None if class_weights is None else tuple(float(w) for w in class_weights)
        self.prep = prep if prep is not None else VolumePrep(flip_prob=0.5)
        self.optimizer = Adam(net.parameters(), lr=lr)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=t_max, eta_min=eta_min)
        self.best_dice = 0.0                                   # max_valid_dice of train_unet.py:141
        self.best_state = None
        self.history = []

    def train_epoch(self) -> float:
        """one pass over train_batches (train_unet.py:146-160) -> the mean training loss; one host sync, at the end"""
        self.net.train()
        losses = []
        for image, mask in self.train_batches:
            x, m, _ = self.prep.prepare(image, mask)
            self.optimizer.zero_grad()
            loss = weighted_cross_entropy(self.net(x), m, self.class_weights)
            loss.backward()
            self.optimizer.step()
            losses.append(loss.detach())
        self.scheduler.step()
        if not losses:
            return 0.0
        return float(torch.stack(losses).double().mean().item())

    def validate(self):
        """train_unet.py:161-175 -> (mean weighted CE, mean arg-max Dice) over val_batches: eval mode (and back to the mode found),
        per item one forward, one loss launch that also writes the label map, one label_dice; one host sync, at the end"""
        was_training = self.net.training
        self.net.eval()
        losses, scores = [], []
        try:
            with torch.no_grad():
                for image, mask in self.val_batches:
                    x, m, _ = self.prep.prepare(image, mask, flips=False)
                    loss, labels = weighted_cross_entropy(self.net(x), m, self.class_weights, labels=True)
                    losses.append(loss)
                    scores.append(label_dice(labels, m))
        finally:
            self.net.train(was_training)
        if not losses:
            return 0.0, 0.0
        both = torch.stack([torch.stack(losses).double().mean(), torch.stack(scores).double().mean()]).tolist()
        return float(both[0]), float(both[1])

    def fit(self, epochs: int, save_path: Optional[str] = None):
        """`epochs` rounds of train_epoch + validate; keeps (and, with save_path, writes) the state_dict of the best validation
        Dice as train_unet.py:182-187 does.  Returns the history: one (train loss, validation loss, validation Dice) per epoch."""
        for _ in range(int(epochs)):
            train_loss = self.train_epoch()
            val_loss, val_dice = self.validate()
            self.history.append((train_loss, val_loss, val_dice))
            if self.best_dice < val_dice:
                self.best_dice = val_dice
                self.best_state = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
                if save_path is not None:
                    torch.save(self.best_state, save_path)
        return self.history
