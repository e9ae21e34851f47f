"""Generates the dice / focal loss fixtures under tests/golden/ from the REAL reference (imported through
oracle/ref_harness.py, dev container only):

    python tools/make_golden_losses.py [loss] [net] [fit]

  seg_losses_dice_focal.npz   loss level: logits, target, loss and d loss / d logits (fp32 and fp64) of the reference's
                              dice_loss / focal_loss classes and autograd (atomai/losses_metrics/losses.py:13-89)
  seg_<case>_dice|_focal.npz  net level: the recipe of oracle/make_golden.py:_seg_case with the criterion swapped
                              (x, y, first-step logits and gradients, 3 Adam-step losses; the init is pinned by seg_<case>.npz)
  seg_dice_focal_fit.npz      Segmentor(nb_classes).fit(..., loss=...) trajectories (4 cycles, batch 4, 4 x 32 x 48 frames)
Every array is emitted in fp32 and with the same modules ``.double()``'d, so each golden carries its own fp32 noise floor.
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")

# (name, kind, K, N, H, W, foreground fraction of a binary mask, (alpha, gamma))
LOSS_CASES = [
    ("dice_k1_3x24x37", "dice", 1, 3, 24, 37, 0.4, None),
    ("dice_k1_sparse_2x19x64", "dice", 1, 2, 19, 64, 0.03, None),
    ("dice_k2_2x19x64", "dice", 2, 2, 19, 64, None, None),
    ("dice_k3_3x24x37", "dice", 3, 3, 24, 37, None, None),
    ("dice_k4_2x19x64", "dice", 4, 2, 19, 64, None, None),
    ("dice_k5_3x24x37", "dice", 5, 3, 24, 37, None, None),
    ("focal_a0.5_g2_3x24x37", "focal", 1, 3, 24, 37, 0.4, (0.5, 2)),
    ("focal_a0.25_g1.5_2x19x64", "focal", 1, 2, 19, 64, 0.03, (0.25, 1.5)),
]


def make_loss(aoi):
    from atomai.losses_metrics import dice_loss, focal_loss
    out = {"cases": np.array([c[0] for c in LOSS_CASES])}
    for i, (name, kind, K, N, H, W, fg, par) in enumerate(LOSS_CASES):
        rs = np.random.RandomState(40 + i)
        logits = (2.0 * rs.randn(N, K, H, W)).astype(np.float32)
        if K == 1:
            target = (rs.rand(N, 1, H, W) < fg).astype(np.float32)
        else:
            target = rs.randint(0, K, (N, H, W)).astype(np.int64)
        out[name + "|logits"], out[name + "|target"] = logits, target
        if par is not None:
            out[name + "|params"] = np.array(par, dtype=np.float64)
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            crit = dice_loss() if kind == "dice" else focal_loss(*par)
            x = torch.from_numpy(logits).to(dt).requires_grad_(True)
            t = torch.from_numpy(target)
            if K == 1:
                t = t.to(dt)
            loss = crit(x, t)
            loss.backward()
            out[f"{name}|loss|{tag}"] = np.array(loss.item(), dtype=np.float64)
            out[f"{name}|dlogits|{tag}"] = x.grad.numpy().copy()
        print(name, "loss f32", out[name + "|loss|f32"], "f64", out[name + "|loss|f64"])
    np.savez_compressed(os.path.join(GOLD, "seg_losses_dice_focal.npz"), **out)


# (golden of the same net under 'ce', loss, model, nb_classes, nb_filters, B, H, seed, upsampling): oracle/make_golden.py:98-102
NET_CASES = [
    ("seg_unet_c3_nf4_b2_32", "dice", "Unet", 3, 4, 2, 32, 1, "bilinear"),
    ("seg_dilnet_c1_nf5_b2_32", "dice", "dilnet", 1, 5, 2, 32, 1, "bilinear"),
    ("seg_unet_c1_nf4_b2_16_nearest", "focal", "Unet", 1, 4, 2, 16, 2, "nearest"),
]


def make_net(aoi):
    from atomai.nets import init_fcnn_model
    from atomai.losses_metrics import select_loss
    from atomai.utils import set_train_rng
    for base, lossname, model, ncls, nf, B, H, seed, ups in NET_CASES:
        out = {}
        rs = np.random.RandomState(seed + 100)
        x = rs.rand(B, 1, H, H).astype(np.float32)
        if ncls == 1:
            y = (rs.rand(B, 1, H, H) > 0.5).astype(np.float32)
        else:
            y = rs.randint(0, ncls, (B, H, H)).astype(np.int64)
        out["x"], out["y"] = x, y
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            set_train_rng(seed)
            net, _ = init_fcnn_model(model, ncls, nb_filters=nf, upsampling=ups)
            net = net.to(dt)
            crit = select_loss(lossname)
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)
            xt = torch.from_numpy(x).to(dt)
            yt = torch.from_numpy(y) if ncls > 1 else torch.from_numpy(y).to(dt)
            losses = []
            for s in range(3):
                net.train()
                opt.zero_grad()
                logits = net(xt)
                loss = crit(logits, yt)
                loss.backward()
                if s == 0:
                    out["logits|" + tag] = logits.detach().numpy()
                    out.update({k + "|grad|" + tag: p.grad.detach().numpy().copy() for k, p in net.named_parameters()})
                opt.step()
                losses.append(loss.item())
            out["losses|" + tag] = np.array(losses)
        out["meta"] = np.array([ncls, nf, B, H, seed, 0])
        name = f"{base}_{lossname}"
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
        print(name, "losses f32", out["losses|f32"], "f64", out["losses|f64"])


FIT_CASES = [(3, "dice"), (1, "dice"), (1, "focal")]


def fit_data(ncls):
    """The data of a fit case (tests/_loss_checks.py draws the same)."""
    rs = np.random.RandomState(0)
    X = rs.rand(4, 32, 48).astype(np.float32)
    y = rs.randint(0, max(ncls, 2), (4, 32, 48))
    Xt = rs.rand(4, 32, 48).astype(np.float32)
    yt = rs.randint(0, max(ncls, 2), (4, 32, 48))
    return X, y, Xt, yt


def make_fit(aoi):
    out = {}
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())
    try:
        for ncls, lossname in FIT_CASES:
            X, y, Xt, yt = fit_data(ncls)
            m = aoi.models.Segmentor(nb_classes=ncls)
            m.fit(X, y, Xt, yt, loss=lossname, training_cycles=4, batch_size=4, swa=False, plot_training_history=False)
            tag = f"c{ncls}_{lossname}"
            out[tag + "|train_loss"] = np.array(m.loss_acc["train_loss"])
            out[tag + "|test_loss"] = np.array(m.loss_acc["test_loss"])
            out[tag + "|batch_idx_train"] = np.array(m.batch_idx_train)
            out[tag + "|batch_idx_test"] = np.array(m.batch_idx_test)
            print(tag, out[tag + "|train_loss"], out[tag + "|test_loss"])
    finally:
        os.chdir(cwd)
    np.savez_compressed(os.path.join(GOLD, "seg_dice_focal_fit.npz"), **out)


if __name__ == "__main__":
    aoi = ref_harness.import_reference()
    which = sys.argv[1:] or ["loss", "net", "fit"]
    for w in which:
        {"loss": make_loss, "net": make_net, "fit": make_fit}[w](aoi)
