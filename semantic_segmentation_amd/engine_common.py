"""Host-side rules shared by the engines (unet_engine, block_engine, unet3d_engine, and the Pix2Pix plans pix2pix_engine, resnet_engine,
discriminator_engine): the compute dtype, the reuse policy of the 16-bit weight packs, the owner cache of a network's parameters and
the BatchNorm coefficient rule.  Nothing
here launches a kernel of its own beyond what ops.bn_finalize / ops.bn_eval_coeffs do; it imports none of the engines."""
from __future__ import annotations

import os

import torch

from . import ops

TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def compute_dtype(name=None):
    """(name, torch dtype) of the engines' 16-bit storage / MFMA type: the argument, else GSSEG_DTYPE, else fp16."""
    name = name or os.environ.get("GSSEG_DTYPE", "f16")
    if name not in TORCH_DT:
        raise ValueError("compute dtype must be 'f16' or 'bf16'")
    return name, TORCH_DT[name]


# Reuse of the 16-bit weight packs between forwards (GSSEG_PACK_CACHE):
#   "safe" (default, also "1"): a forward that keeps a graph (training: grad mode on and something requires grad) ALWAYS
#       re-packs -- one launch, ~0.1 ms at 31 M parameters, inside bench.py's timed region anyway.  Betty's darts hypergradient
#       perturbs the parameters through `p.data` (running_files/train_end2end_jsrt.py:287-292: Config(type="darts")), which
#       no version counter sees; with this default the stock script gets the perturbed weights.  Packs are reused only by
#       forwards without a graph (eval / torch.no_grad()), keyed on (data_ptr, _version): every torch in-place op, every
#       optimiser (torch's and optim.py's fused ones) and load_state_dict bump the version.
#   "versions": the version-keyed reuse for training forwards too (loops that never write through `.data`).
#   "0": never reuse.
_PC = os.environ.get("GSSEG_PACK_CACHE", "safe")
PACK_CACHE = _PC != "0"
PACK_CACHE_TRAINING = _PC == "versions"
_NOCACHE = [0]


def pack_key(t: torch.Tensor):
    """cache key of a pack made from tensor `t`; GSSEG_PACK_CACHE=0: a key that no earlier one equals"""
    if not PACK_CACHE:
        _NOCACHE[0] += 1
        return (_NOCACHE[0],)
    return (t.data_ptr(), t._version, t.dtype, tuple(t.shape))


def pack_reuse_allowed(need_grad: bool, trust_versions: bool = False) -> bool:
    """may a forward reuse the packs of an earlier one?  (see GSSEG_PACK_CACHE above; `trust_versions`: the engine's owner
    vouches that parameters only change through version-bumping ops -- harness.py does, it owns the optimisers)"""
    return PACK_CACHE and (PACK_CACHE_TRAINING or trust_versions or not need_grad)


class ParamIndex:
    """(name, owner module, leaf name) of every parameter and buffer of `self.net`, in registration order -- the order autograd
    sees them.  Walking the module tree costs ~0.7 ms per call on a UNet (0.1-0.2 ms on the Pix2Pix networks) and a step asks
    for it several times; the tree of these networks is static, while the tensors themselves may be swapped (`.to()`,
    `.half()`, a new nn.Parameter) -- so the OWNERS are cached and the tensors are read from them on every call."""

    def __init__(self, net):
        self.net = net

    def _index(self):
        idx = self.__dict__.get("_idx")
        if idx is None:
            mods = dict(self.net.named_modules())

            def owners(named):
                out = []
                for name, _ in named:
                    head, _, leaf = name.rpartition(".")
                    out.append((name, mods[head], leaf))
                return out
            idx = (owners(self.net.named_parameters()), owners(self.net.named_buffers()), mods)
            self.__dict__["_idx"] = idx
        return idx

    def param_items(self):
        """(name, Parameter) in registration order"""
        return [(n, m._parameters[leaf]) for n, m, leaf in self._index()[0]]

    def param_list(self):
        return [m._parameters[leaf] for _, m, leaf in self._index()[0]]

    def param_names(self):
        return [n for n, _, _ in self._index()[0]]

    def buffer_dict(self):
        return {n: m._buffers[leaf] for n, m, leaf in self._index()[1]}

    def submodule(self, key: str):
        return self._index()[2][key]


def bn_coeffs(bn, partials, ntiles, C, count, training, dev, nbt_pending=None, conv_bias=None):
    """(coef [4,C] fp32 = scale / shift / mean / invstd, batch_stats) of BatchNorm module `bn` from the conv-epilogue partial sums
    (batch statistics: train mode, or no running statistics) or from the running statistics (eval); in train mode it also
    updates running_mean / running_var / num_batches_tracked as torch does.
    nbt_pending: list collecting the `num_batches_tracked` counters of this pass -- the caller increments them with ONE foreach
    launch (_flush_nbt) instead of a 5-us kernel per BatchNorm layer; without it, or with momentum=None (cumulative average: the
    factor needs the new count now), the counter is incremented here.
    conv_bias: bias of the convolution in front, which the conv kernel did NOT add.  A bias in front of batch statistics cancels
    in the output; the statistics were taken before it and mean(y + b) = mean(y) + b, so it is folded into the running mean
    (train) or taken off it, i.e. added to the shift (eval)."""
    coef = torch.empty((4, C), dtype=torch.float32, device=dev)
    gamma, beta = bn._parameters["weight"].detach(), bn._parameters["bias"].detach()
    bufs = bn._buffers
    rm, rv, nbt = bufs.get("running_mean"), bufs.get("running_var"), bufs.get("num_batches_tracked")
    batch_stats = training or rm is None
    if batch_stats:
        mom = bn.momentum
        if training and nbt is not None:
            if nbt_pending is not None and mom is not None:
                nbt_pending.append(nbt)
            else:
                nbt.add_(1)
        if mom is None:
            mom = 1.0 / float(nbt.item()) if nbt is not None else 0.0      # (no counter: no running statistics to update either)
        upd = training and rm is not None
        ops.bn_finalize(partials, ntiles, C, count, gamma, beta, rm if upd else None, rv if upd else None, mom, bn.eps,
                        coef[0], coef[1], coef[2], coef[3])
        if upd and conv_bias is not None:
            rm.add_(conv_bias.detach(), alpha=mom)
    else:
        if conv_bias is not None:
            rm = (rm - conv_bias.detach()).contiguous()
        ops.bn_eval_coeffs(C, gamma, beta, rm, rv, bn.eps, coef[0], coef[1], coef[2], coef[3])
    return coef, batch_stats


def _flush_nbt(pending):
    """the one increment of the counters that bn_coeffs collected"""
    if pending:
        torch._foreach_add_(pending, 1)
        pending.clear()
