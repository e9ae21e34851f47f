"""Shared bodies of the dice / focal loss tests (reference: atomai/losses_metrics/losses.py:13-89).  The SAME checks run
  * on the CPU through the SIMT emulator build of the kernel sources (`not gpu` tier, test_losses_emulated.py), and
  * on a real MI355X through libatomai_amd.so (`gpu` tier, test_losses_gpu.py),
against golden vectors generated from the real reference (tests/golden, tools/make_golden_losses.py)."""
import os

import numpy as np
import pytest
import torch

from _seg_checks import CASES, GOLD, REL_TOL, relmax

UPSTREAM = (1.0, 0.37)
NET_CASES = {                                   # golden -> (key of _seg_checks.CASES with the same net, loss)
    "seg_unet_c3_nf4_b2_32_dice": ("seg_unet_c3_nf4_b2_32", "dice"),
    "seg_dilnet_c1_nf5_b2_32_dice": ("seg_dilnet_c1_nf5_b2_32", "dice"),
    "seg_unet_c1_nf4_b2_16_nearest_focal": ("seg_unet_c1_nf4_b2_16_nearest", "focal"),
}
FIT_CASES = ((3, "dice"), (1, "dice"), (1, "focal"))


def loss_case_names():
    return [str(c) for c in np.load(os.path.join(GOLD, "seg_losses_dice_focal.npz"))["cases"]]


def _criterion(g, name):
    from atomai_amd.losses_metrics import dice_loss, focal_loss
    if name.startswith("dice"):
        return dice_loss()
    alpha, gamma = g[name + "|params"]
    return focal_loss(float(alpha), float(gamma))


def check_loss_level(name, device):
    """Loss and d loss / d logits of one golden case against the reference's classes and autograd in fp64: the loss within
    REL_TOL; the gradient error, normalised by max |dlogits|, within max(4 x the reference's own fp32-vs-fp64 error, 2e-5)
    (the rule of _seg_checks.check_net_case); upstream gradients 1 and 0.37; the same loss under torch.no_grad()."""
    g = np.load(os.path.join(GOLD, "seg_losses_dice_focal.npz"))
    crit = _criterion(g, name)
    target = torch.from_numpy(g[name + "|target"]).to(device)
    ref_loss, ref_dl = float(g[name + "|loss|f64"]), g[name + "|dlogits|f64"]
    gmax = np.abs(ref_dl).max()
    floor = np.abs(g[name + "|dlogits|f32"].astype(np.float64) - ref_dl).max() / gmax
    for up in UPSTREAM:
        x = torch.from_numpy(g[name + "|logits"]).to(device).requires_grad_(True)
        loss = crit(x, target)
        (loss * up).backward()
        loss = loss.detach()
        lerr = abs(float(loss) - ref_loss) / abs(ref_loss)
        gerr = np.abs(x.grad.cpu().numpy().astype(np.float64) - up * ref_dl).max() / (up * gmax)
        print(f"{name} upstream {up}: loss {float(loss):.8f} (reference fp64 {ref_loss:.8f}, rel {lerr:.2e}); dlogits error "
              f"{gerr:.2e} (reference-fp32 floor {floor:.2e})")
        assert loss.shape == () and loss.dtype == torch.float32
        assert lerr < REL_TOL, (name, float(loss), ref_loss)
        assert gerr <= max(4 * floor, 2e-5), (name, up, gerr, floor)
    with torch.no_grad():
        ev = crit(x, target)
    assert float(ev) == float(loss), (name, float(ev), float(loss))


def check_fused_vs_modular(device, kind, models):
    """net.forward_loss(x, y, criterion=dice_loss() / focal_loss()) (head + loss + their backward over the last activation,
    engine.PxLossNode) against criterion(net(x), y) + backward, in the form of _seg_checks.check_fused_head_and_loss: the
    loss within 2e-6 max(1, |loss|), every parameter and input gradient within 2e-5 gmax, upstream gradients 1 and 0.37.
    Returns {(model, classes): (what ran, what runs for the same net under 'ce')}: the dice / focal kernels take the heads
    amx_px_ce_train takes (amx_px_dice_train_supported mirrors amx_px_ce_train_supported)."""
    from atomai_amd.losses_metrics.losses import select_loss
    from atomai_amd.nets import init_fcnn_model
    rs = np.random.RandomState(7)
    kinds = {}
    for model, ncls, nf in models:
        crit = select_loss(kind)
        for gscale in UPSTREAM:
            torch.manual_seed(5)
            net, _ = init_fcnn_model(model, ncls, nb_filters=nf)
            net.to(device).train()
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.momentum = 0.0                           # (two forwards over the same batch)
            x = torch.from_numpy(rs.rand(3, 1, 24, 32).astype(np.float32)).to(device).requires_grad_(True)
            if ncls == 1:
                y = torch.from_numpy((rs.rand(3, 1, 24, 32) > 0.6).astype(np.float32)).to(device)
            else:
                y = torch.from_numpy(rs.randint(0, ncls, (3, 24, 32))).to(device)
            loss0 = crit(net(x), y)
            (loss0 * gscale).backward()
            loss0 = loss0.detach()
            ref = [p.grad.clone() for p in net.parameters()] + [x.grad.clone()]
            net.zero_grad()
            x.grad = None
            k, out = net.forward_loss(x, y, criterion=crit)
            loss1 = out if k == "loss" else crit(out, y)
            (loss1 * gscale).backward()
            loss1 = loss1.detach()
            with torch.no_grad():
                kinds[(model, ncls)] = (k, net.forward_loss(x, y)[0])
            got = [p.grad for p in net.parameters()] + [x.grad]
            gmax = max(float(t.abs().max()) for t in ref)
            worst = max(float((a - b).abs().max()) for a, b in zip(got, ref)) / gmax
            print(f"{kind} {model} K={ncls} nf={nf} upstream {gscale}: {k}; loss {float(loss1):.8f} vs modular "
                  f"{float(loss0):.8f}; worst gradient difference {worst:.2e} of gmax")
            assert abs(float(loss0) - float(loss1)) < 2e-6 * max(1.0, abs(float(loss0))), (model, float(loss0), float(loss1))
            for (name, _), a, b in zip(list(net.named_parameters()) + [("input", None)], got, ref):
                assert float((a - b).abs().max()) < 2e-5 * gmax, (model, ncls, name, float((a - b).abs().max()), gmax)
    net.eval()
    assert net.forward_loss(x, y, criterion=crit)[0] == "logits"        # eval(): no fused node
    return kinds


FUSED_MODELS = (("Unet", 3, 4), ("Unet", 2, 8), ("SegResNet", 3, 4), ("ResHedNet", 3, 4), ("dilnet", 4, 8), ("Unet", 1, 4),
                ("dilnet", 1, 8))               # the model list of _seg_checks.check_fused_head_and_loss


def check_fused_dice(device):
    from atomai_amd import _lib as L
    kinds = check_fused_vs_modular(device, "dice", FUSED_MODELS + (("Unet", 5, 4),))
    assert kinds[("Unet", 5)][0] == "logits"                    # more classes than the fused kernel takes
    assert L.load().amx_px_dice_train_supported(16, 5, 32) == 0 and L.load().amx_px_dice_train_supported(16, 3, 32) == 1
    assert all(k == ce for k, ce in kinds.values()), kinds       # the fused node ran wherever *_supported accepts the head
    assert [k for k, _ in kinds.values()].count("loss") >= 4, kinds


def check_fused_focal(device):
    kinds = check_fused_vs_modular(device, "focal", (("Unet", 1, 4), ("dilnet", 1, 8), ("SegResNet", 1, 4)))
    assert all(k == ce for k, ce in kinds.values()), kinds
    assert [k for k, _ in kinds.values()].count("loss") >= 2, kinds


def check_net_case(name, device):
    """_seg_checks.check_net_case restated with the criterion of select_loss('dice' | 'focal'): first-step logits, every
    gradient (global scale, relative to the reference's own fp32 noise) and the losses of three Adam steps."""
    from atomai_amd.nets import init_fcnn_model
    from atomai_amd.losses_metrics import select_loss
    from atomai_amd.optim import FusedAdam
    base, lossname = NET_CASES[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    ncls, nf, B, H, seed, _ = [int(v) for v in g["meta"]]
    model, kw = CASES[base]
    torch.manual_seed(seed)
    net, _ = init_fcnn_model(model, ncls, nb_filters=nf, **kw)
    net.to(device)
    x = torch.from_numpy(g["x"]).to(device)
    y = torch.from_numpy(g["y"]).to(device)
    crit = select_loss(lossname)
    opt = FusedAdam(net.parameters(), lr=1e-3)
    opt.prepare()
    losses = []
    for s in range(3):
        net.train()
        opt.zero_grad()
        logits = net(x)
        loss = crit(logits, y)
        loss.backward()
        if s == 0:
            assert relmax(logits.detach().cpu().numpy(), g["logits|f64"]) < REL_TOL
            gmax = max(np.abs(g[k + "|grad|f64"]).max() for k, _ in net.named_parameters())
            worst = (0.0, "", 0.0)
            for k, p in net.named_parameters():
                ref = g[k + "|grad|f64"]
                err = np.abs(p.grad.cpu().numpy() - ref).max() / gmax
                ref32 = np.abs(g[k + "|grad|f32"] - ref).max() / gmax
                worst = max(worst, (err, k, ref32))
                assert err <= max(4 * ref32, 2e-5), (k, err, ref32)
            print(f"{name}: worst gradient error {worst[0]:.2e} ({worst[1]}; reference-fp32 floor {worst[2]:.2e})")
        opt.step()
        losses.append(loss.item())
    print(f"{name}: losses {losses} reference fp64 {list(g['losses|f64'])}")
    np.testing.assert_allclose(losses, g["losses|f64"], rtol=REL_TOL)


def fit_data(ncls):
    """The data tools/make_golden_losses.py:fit_data draws."""
    rs = np.random.RandomState(0)
    X = rs.rand(4, 32, 48).astype(np.float32)
    y = rs.randint(0, max(ncls, 2), (4, 32, 48))
    Xt = rs.rand(4, 32, 48).astype(np.float32)
    yt = rs.randint(0, max(ncls, 2), (4, 32, 48))
    return X, y, Xt, yt


def _fit(ncls, lossname, tmp_path, tag=""):
    import atomai_amd as aoi
    X, y, Xt, yt = fit_data(ncls)
    m = aoi.models.Segmentor(nb_classes=ncls)
    m.fit(X, y, Xt, yt, loss=lossname, training_cycles=4, batch_size=4, swa=False, plot_training_history=False,
          filename=str(tmp_path / f"m{tag}"))
    return m


def check_fit_trajectory(ncls, lossname, tmp_path):
    """Segmentor(nb_classes).fit(..., loss=...) against the reference's CPU run: the same batch schedule; the losses to the
    tolerances test_seg_gpu.test_config1_loss_trajectory applies to its golden (first steps REL_TOL, all train 1e-3, test
    5e-3)."""
    g = np.load(os.path.join(GOLD, "seg_dice_focal_fit.npz"))
    tag = f"c{ncls}_{lossname}"
    m = _fit(ncls, lossname, tmp_path)
    assert type(m.criterion).__name__ == f"{lossname}_loss"
    assert list(m.batch_idx_train) == list(g[tag + "|batch_idx_train"])
    assert list(m.batch_idx_test) == list(g[tag + "|batch_idx_test"])
    print(f"{tag}: train {m.loss_acc['train_loss']} reference {list(g[tag + '|train_loss'])}; test "
          f"{m.loss_acc['test_loss']} reference {list(g[tag + '|test_loss'])}")
    np.testing.assert_allclose(m.loss_acc["train_loss"][:3], g[tag + "|train_loss"][:3], rtol=REL_TOL)
    np.testing.assert_allclose(m.loss_acc["train_loss"], g[tag + "|train_loss"], rtol=1e-3)
    np.testing.assert_allclose(m.loss_acc["test_loss"], g[tag + "|test_loss"], rtol=5e-3)


def check_fit_determinism(tmp_path, ncls=3):
    """Two identical dice fits: bit-identical train_loss and final state_dict (no floating-point atomics, fixed trees)."""
    runs = []
    for i in range(2):
        m = _fit(ncls, "dice", tmp_path, tag=str(i))
        runs.append((list(m.loss_acc["train_loss"]), {k: v.clone() for k, v in m.net.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def check_api(device):
    import atomai_amd as aoi
    from atomai_amd.losses_metrics import select_loss
    assert "dice_loss" in aoi.losses_metrics.__all__ and "focal_loss" in aoi.losses_metrics.__all__
    d, f = select_loss("dice"), select_loss("focal")              # no nb_classes needed, as in the reference
    assert isinstance(d, aoi.losses_metrics.dice_loss) and d.eps == 1e-7
    assert isinstance(f, aoi.losses_metrics.focal_loss) and (f.alpha, f.gamma, f.logits) == (0.5, 2, True)
    assert isinstance(d, torch.nn.Module) and isinstance(f, torch.nn.Module)
    logits = torch.zeros(2, 3, 8, 10, device=device)
    with pytest.raises(ValueError):                               # int64 multi-class target: target size != input size
        f(logits, torch.zeros(2, 8, 10, dtype=torch.int64, device=device))
    with pytest.raises(ValueError):                               # shapes, not just numel
        d(logits, torch.zeros(2, 10, 8, dtype=torch.int64, device=device))
    with pytest.raises(ValueError):
        d(logits[:, :1], torch.zeros(2, 8, 10, device=device))
    with pytest.raises(NotImplementedError):
        select_loss("nll")
    with pytest.raises(NotImplementedError):
        aoi.losses_metrics.focal_loss(with_logits=False)
    # labels of any integer type, and a float mask truncated as .long() does
    x3 = torch.randn(2, 3, 8, 10, device=device)
    y3 = torch.randint(0, 3, (2, 8, 10), device=device)
    assert float(d(x3, y3)) == float(d(x3, y3.to(torch.int32))) == float(d(x3, y3.to(torch.uint8)))
    x1 = torch.randn(2, 1, 8, 10, device=device)
    y1 = (torch.rand(2, 1, 8, 10, device=device) > 0.5)
    assert float(d(x1, y1.float())) == float(d(x1, y1.long())) == float(d(x1, y1.float() * 1.5))


# ---- the formulas of the reference restated in fp64 torch (host), for sizes no golden file holds
def dice_ref(logits, labels, dtype=torch.float64, eps=1e-7):
    """(loss, dlogits) in `dtype`.  K == 1: bins (foreground, background) over every pixel; K >= 2: one bin per (class, image
    COLUMN) — the reference sums over dims (0, 2) of (N,K,H,W) only (losses.py:85) — and the mean over the K * W ratios."""
    x = logits.detach().to(dtype).cpu().requires_grad_(True)
    K = x.shape[1]
    if K == 1:
        y = labels.detach().cpu().squeeze(1).long()
        onehot = torch.stack([(y == 1), (y == 0)], 1).to(dtype)
        s = torch.sigmoid(x)
        probas = torch.cat([s, 1 - s], 1)
        dims = (0, 2, 3)
    else:
        y = labels.detach().cpu().long()
        onehot = torch.nn.functional.one_hot(y, K).permute(0, 3, 1, 2).to(dtype)
        probas = torch.softmax(x, 1)
        dims = (0, 2)
    inter = (probas * onehot).sum(dims)
    card = (probas + onehot).sum(dims)
    loss = 1 - (2 * inter / (card + eps)).mean()
    loss.backward()
    return float(loss.detach()), x.grad


def focal_ref(logits, labels, dtype=torch.float64, alpha=0.5, gamma=2):
    x = logits.detach().to(dtype).cpu().requires_grad_(True)
    c = torch.nn.functional.binary_cross_entropy_with_logits(x, labels.detach().to(dtype).cpu())
    pt = torch.exp(-c)
    loss = alpha * (1 - pt) ** gamma * c
    loss.backward()
    return float(loss.detach()), x.grad


def check_full_size(device, K, N=4, H=512, W=512):
    """512^2, batch 4: K = 3 (K * W = 1536 bins of 2048 values) / K = 1 (2 bins of 1 M values) against the restated formulas
    in fp64 on the host; the bounds of the loss-level check, the floor being the same formulas in fp32 torch."""
    from atomai_amd.losses_metrics import dice_loss, focal_loss
    rs = np.random.RandomState(11 + K)
    x = torch.from_numpy((2.0 * rs.randn(N, K, H, W)).astype(np.float32))
    if K == 1:
        y = torch.from_numpy((rs.rand(N, 1, H, W) < 0.03).astype(np.float32))
    else:
        y = torch.from_numpy(rs.randint(0, K, (N, H, W)))
    todo = [("dice", dice_loss(), dice_ref)] + ([("focal", focal_loss(), focal_ref)] if K == 1 else [])
    for nm, crit, ref in todo:
        ref_loss, ref_dl = ref(x, y)
        floor = float((ref(x, y, torch.float32)[1].double() - ref_dl).abs().max()) / float(ref_dl.abs().max())
        xd = x.to(device).requires_grad_(True)
        loss = crit(xd, y.to(device))
        loss.backward()
        loss = loss.detach()
        gmax = float(ref_dl.abs().max())
        gerr = float((xd.grad.cpu().double() - ref_dl).abs().max()) / gmax
        lerr = abs(float(loss) - ref_loss) / abs(ref_loss)
        print(f"{nm} K={K} {N}x{H}x{W}: loss {float(loss):.8f} (fp64 {ref_loss:.8f}, rel {lerr:.2e}); dlogits error {gerr:.2e} "
              f"(torch-fp32 floor {floor:.2e})")
        assert lerr < REL_TOL
        assert gerr <= max(4 * floor, 2e-5), (nm, K, gerr, floor)


def check_many_classes(device, K=11, N=2, H=9, W=21):
    """More classes than a thread holds in registers (8): the re-reading forms of amx_dice_sums / amx_dice_bwd."""
    from atomai_amd.losses_metrics import dice_loss
    rs = np.random.RandomState(3)
    x = torch.from_numpy((2.0 * rs.randn(N, K, H, W)).astype(np.float32))
    y = torch.from_numpy(rs.randint(0, K, (N, H, W)))
    ref_loss, ref_dl = dice_ref(x, y)
    floor = float((dice_ref(x, y, torch.float32)[1].double() - ref_dl).abs().max()) / float(ref_dl.abs().max())
    xd = x.to(device).requires_grad_(True)
    loss = dice_loss()(xd, y.to(device))
    loss.backward()
    gerr = float((xd.grad.cpu().double() - ref_dl).abs().max()) / float(ref_dl.abs().max())
    print(f"dice K={K}: loss {float(loss.detach()):.8f} (fp64 {ref_loss:.8f}); dlogits error {gerr:.2e} (torch-fp32 floor {floor:.2e})")
    assert abs(float(loss.detach()) - ref_loss) / abs(ref_loss) < REL_TOL
    assert gerr <= max(4 * floor, 2e-5), (gerr, floor)
