"""volume_train.VolumeTrainer, the loop of GenSeg-3D/train_unet.py:137-187, on three seeded synthetic scans of shape (13, 17, 21) --
no multiple of 16, so every item goes through the normalise / flip / pad kernel: one epoch equals the hand-written composition
of its parts bit for bit, two trainers with one seed agree bit for bit, the loss falls, `validate` equals its parts called
separately and leaves the network's mode as it found it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPE = (13, 17, 21)
WEIGHTS = (0.004, 0.996)


def scans(seed=5, n=3):
    """raw (image [D,H,W] fp32, mask [1,D,H,W] int64) pairs on the GPU: a bright ball of its own size and place in each scan, noise
    around it, zeros (background of a real scan) in one corner"""
    g = torch.Generator().manual_seed(seed)
    d, h, w = SHAPE
    zz, yy, xx = torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij")
    out = []
    for i in range(n):
        c = torch.tensor([4.0 + 2 * i, 6.0 + 3 * i, 8.0 + 2 * i])
        ball = ((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) < (3.0 + 0.5 * i) ** 2
        img = 0.5 * torch.randn(d, h, w, generator=g) + 3.0 * ball.float() + 1.0
        img[:2, :3, :4] = 0.0
        out.append((img.cuda(), ball.long().unsqueeze(0).cuda()))
    return out


def build(seed=3):
    """UNet3D(1, 2) with the narrow widths if the pair forward lays them out, else the default ones; seeded parameters"""
    from semantic_segmentation_amd.unet3d import UNet3D
    kw = dict(level_channels=[32, 64, 128], bottleneck_channel=256)
    try:
        UNet3D(1, 2, **kw).engine._pair_layout(16)
    except NotImplementedError:
        kw = {}
    torch.manual_seed(seed)
    return UNet3D(1, 2, **kw).cuda()


def trainer(net, data, seed=11, **kw):
    from semantic_segmentation_amd.volume import VolumePrep
    from semantic_segmentation_amd.volume_train import VolumeTrainer
    return VolumeTrainer(net, data, data, class_weights=WEIGHTS, prep=VolumePrep(flip_prob=0.5, seed=seed), **kw)


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))


def test_one_epoch_is_the_composition_of_its_parts():
    from semantic_segmentation_amd.losses import weighted_cross_entropy
    from semantic_segmentation_amd.optim import Adam
    from semantic_segmentation_amd.volume import VolumePrep
    data = scans()
    a, b = build(), build()
    assert same(a, b)
    tr = trainer(a, data, lr=1e-3, t_max=500, eta_min=1e-9)
    mean = tr.train_epoch()
    # by hand
    prep = VolumePrep(flip_prob=0.5, seed=11)
    opt = Adam(b.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=500, eta_min=1e-9)
    b.train()
    losses = []
    for image, mask in data:
        x, m, meta = prep.prepare(image, mask)
        assert tuple(x.shape) == (1, 1, 16, 32, 32) and tuple(m.shape) == (1, 16, 32, 32)
        opt.zero_grad()
        loss = weighted_cross_entropy(b(x), m, WEIGHTS)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    sched.step()
    torch.cuda.synchronize()
    assert same(a, b)
    assert mean == float(torch.stack(losses).double().mean().item())
    assert tr.optimizer.param_groups[0]["lr"] == opt.param_groups[0]["lr"] < 1e-3
    assert a.training


def test_two_trainers_with_one_seed_agree_bit_for_bit():
    data = scans()
    a, b = build(), build()
    ta, tb = trainer(a, data), trainer(b, data)
    la = [ta.train_epoch() for _ in range(2)]
    lb = [tb.train_epoch() for _ in range(2)]
    torch.cuda.synchronize()
    assert la == lb and same(a, b)


def test_training_loss_falls():
    data = scans()
    tr = trainer(build(), data)
    losses = [tr.train_epoch() for _ in range(8)]
    print("training loss per epoch:", losses)
    assert all(l == l for l in losses)
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize("training", [True, False])
def test_validate_is_loss_plus_label_dice(training):
    from semantic_segmentation_amd.losses import weighted_cross_entropy
    from semantic_segmentation_amd.volume import VolumePrep, label_dice
    data = scans()
    net = build()
    tr = trainer(net, data)
    tr.train_epoch()                                         # running statistics that differ from the initial ones
    net.train(training)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    vloss, vdice = tr.validate()
    assert net.training == training
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())          # eval mode: no statistic moved
    prep = VolumePrep()
    net.eval()
    ls, ds = [], []
    with torch.no_grad():
        for image, mask in data:
            x, m, _ = prep.prepare(image, mask, flips=False)
            logits = net(x)
            ls.append(weighted_cross_entropy(logits, m, WEIGHTS))                    # the loss alone
            ds.append(label_dice(first_maximum(logits), m))                          # the label map from its own kernel
    net.train(training)
    assert vloss == float(torch.stack(ls).double().mean().item())
    assert vdice == float(torch.stack(ds).double().mean().item())
    assert 0.0 <= vdice <= 1.0


def first_maximum(logits):
    """uint8 arg-max with the first maximum, as gs_labels_from_logits writes it"""
    from semantic_segmentation_amd import ops
    lab = torch.empty((logits.shape[0],) + tuple(logits.shape[2:]), dtype=torch.uint8, device=logits.device)
    ops.labels_from_logits(logits.contiguous(), lab)
    return lab


def test_fit_keeps_the_best_dice_state(tmp_path):
    data = scans()
    net = build()
    tr = trainer(net, data)
    path = str(tmp_path / "best.pth")
    hist = tr.fit(2, save_path=path)
    assert len(hist) == 2 and tr.best_dice == max([0.0] + [h[2] for h in hist])
    if tr.best_state is not None:
        saved = torch.load(path)
        assert all(torch.equal(saved[k].cuda(), v) for k, v in tr.best_state.items())
