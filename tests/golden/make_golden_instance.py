"""Fixtures of the Pix2Pix networks under `--norm instance` from the ORIGINAL reference modules (read-only checkout, CPU), run
in DOUBLE: tests/golden/pix2pix_instance_{a,b}.npz.  As make_golden.py: weights are regenerated from the seed by
golden_util_instance.py (only checksums are stored) and loaded with load_state_dict(strict=True), which also proves that the
key set is the reference's.  Dropout is off (p = 0), so the train image is the eval image (InstanceNorm takes instance
statistics in both modes); the eval image is stored on its own.

Usage:  python tests/golden/make_golden_instance.py"""
import os
import sys

sys.dont_write_bytecode = True          # the reference checkout is read-only: no __pycache__ there

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = os.environ.get("GENSEG_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from golden_util import grad_summary, tensor_checksum  # noqa: E402
from golden_util_instance import (FIXTURES, fixture_inputs, seeded_discriminator_state_dict_instance,  # noqa: E402
                                  seeded_generator_state_dict_instance)

torch.set_num_threads(8)


def make(name, f):
    from models_pix2pix import networks
    norm = networks.get_norm_layer("instance")
    sdG = seeded_generator_state_dict_instance(f["seed_g"], f["cin"], f["cout"], f["D"], 64)
    sdD = seeded_discriminator_state_dict_instance(f["seed_d"], f["cin"] + f["cout"], 64, f["n_layers"])

    def gen():
        G = networks.UnetGenerator(f["cin"], f["cout"], f["D"], 64, norm_layer=norm, use_dropout=True)
        G.load_state_dict(sdG, strict=True)
        for m in G.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        return G.double()

    def disc():
        D = networks.NLayerDiscriminator(f["cin"] + f["cout"], 64, f["n_layers"], norm)
        D.load_state_dict(sdD, strict=True)
        return D.double()

    x, real, arch = fixture_inputs(f)
    x, real = x.double(), real.double()
    arch64 = arch.double().requires_grad_(True)
    networks.upconv_arch = arch64             # the cells read the module global at call time (networks.py:507-511)
    out = {"input": x.numpy(), "real": real.numpy(), "arch": arch.numpy()}
    G, D = gen().train(), disc().train()
    crit = networks.GANLoss("vanilla").double()
    fake = G(x)
    pred_fake = D(torch.cat((x, fake), 1))
    loss_G = crit(pred_fake, True) + torch.nn.L1Loss()(fake, real) * 100.0
    loss_G.backward()
    out["image"] = fake.detach().numpy()
    out["logits_fake"] = pred_fake.detach().numpy()
    out["loss_G"] = loss_G.item()
    for k, p in G.named_parameters():
        out["gsumG/" + k] = grad_summary(p.grad)
    out["arch_grad_G"] = arch64.grad.numpy().copy()
    D2 = disc().train()
    pf = D2(torch.cat((x, fake), 1).detach())
    pr = D2(torch.cat((x, real), 1))
    loss_D = (crit(pf, False) + crit(pr, True)) * 0.5
    loss_D.backward()
    out["logits_real"] = pr.detach().numpy()
    out["loss_D"] = loss_D.item()
    for k, p in D2.named_parameters():
        out["gsumD/" + k] = grad_summary(p.grad)
    with torch.no_grad():
        out["image_eval"] = gen().eval()(x).numpy()
    for k, v in sdG.items():
        out["wsumG/" + k] = tensor_checksum(v)
    for k, v in sdD.items():
        out["wsumD/" + k] = tensor_checksum(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss_G", loss_G.item(), "loss_D", loss_D.item(), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, f in FIXTURES.items():
        make(name, f)
