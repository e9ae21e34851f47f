"""Generates the DenoisingAutoencoder fixtures under tests/golden/ from the REAL reference (imported through
oracle/ref_harness.py, dev container only; never imported by a test):

    python tools/make_denoiser_golden.py

  denoiser_<case>.npz   one per case of CASES, key scheme of imspec_*.npz: the initial state dict (``<key>|init``), x, y,
                        the training-mode output (``out|f32``, ``out|f64``), per-parameter gradients of the first step
                        (``<key>|grad|f32|f64``), BatchNorm running statistics after it (``<key>|bn1|...``), three
                        Adam-step losses (``losses|...``) and the eval-mode output after them (``eval_out|...``);
                        ``data_seed`` and ``margins`` = (smallest |LeakyReLU input|, smallest gap between the two largest
                        values of a pooling window, the reference's fp32 noise on those tensors), see below
  denoiser_fit.npz      DenoisingAutoencoder.fit of the reference on rs = RandomState(0): 20 clean 16 x 16 images and their
                        noisy copies, split 16 / 4, batch_size 4, once with swa=False (4 cycles) and once with the default
                        swa=True (30 cycles, keys ``...|swa``: the reference averages the weights of the last 30 cycles
                        and fails with KeyError: 0 on a shorter run): the batch schedule, train / test losses, the same training steps repeated in float64
                        (``train_loss|f64``) and the fp32-vs-fp64 drift of the reference over those cycles (``drift``),
                        predict(noisy[:5]) and predict(noisy[0]) of both runs, the checkpoint's prediction and keys
  ref_denoiser_ckpt.tar the checkpoint that the swa=False fit wrote
Every net case runs in fp32 and with the same modules ``.double()``'d, so each golden carries its own fp32 noise floor.

The net has two kinds of decision that fp32 noise can flip against float64: the sign of a LeakyReLU input and the winner
of a 2 x 2 pooling window.  The data of a case are therefore drawn from the first seed (counted from 0) at which the
float64 evaluation decides every one of them by more than the largest fp32-vs-float64 difference on those tensors — the
rule of tests/_imspec_checks.find_default_data_seed; the seed and the margins are printed and recorded.
TEST INFRASTRUCTURE ONLY.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 1
# name -> (encoder_filters, decoder_filters, encoder_layers, decoder_layers, use_batch_norm, upsampling_mode, input shape)
CASES = {
    "denoiser_a": ([4, 6, 8], [8, 6, 4], [1, 2, 2], [2, 2, 1], False, "nearest", (2, 1, 16, 24)),
    "denoiser_b": ([4, 6, 8], [8, 6, 4], [1, 2, 2], [2, 2, 1], True, "bilinear", (4, 1, 16, 16)),
    "denoiser_c": ([5, 12], [12, 12], [2, 1], [1, 2], True, "nearest", (3, 1, 8, 12)),
}
FIT_ARCH = dict(encoder_filters=[4, 6, 8], decoder_filters=[8, 6, 4], encoder_layers=[1, 2, 2], decoder_layers=[2, 2, 1])


def _build(aoi, case, dtype):
    ef, df, el, dl, bn, up, _ = case
    m = aoi.models.DenoisingAutoencoder(ef, df, el, dl, use_batch_norm=bn, upsampling_mode=up, seed=SEED)
    return m.net.to("cpu").to(dtype), m.meta_state_dict


def _data(shape, seed):
    rs = np.random.RandomState(seed)
    y = rs.rand(*shape).astype(np.float32)
    x = (y + 0.1 * rs.randn(*shape)).astype(np.float32)
    return x, y


def _decisions(net, x):
    """Training-mode forward -> (inputs of every LeakyReLU, inputs of every MaxPool2d), through forward hooks."""
    lre, pool, hooks = [], [], []
    for m in net.modules():
        if isinstance(m, torch.nn.LeakyReLU):
            hooks.append(m.register_forward_hook(lambda mod, i, o: lre.append(i[0].detach().clone())))
        elif isinstance(m, torch.nn.MaxPool2d):
            hooks.append(m.register_forward_hook(lambda mod, i, o: pool.append(i[0].detach().clone())))
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with torch.no_grad():
        net(x)
    net.load_state_dict(state)                              # (BatchNorm running statistics as before)
    for h in hooks:
        h.remove()
    return lre, pool


def _pool_gap(t):
    n, c, h, w = t.shape
    win = t.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    top = win.sort(dim=-1, descending=True).values
    return float((top[..., 0] - top[..., 1]).min())


def margins(aoi, case, x):
    n64, _ = _build(aoi, case, torch.float64)
    n32, _ = _build(aoi, case, torch.float32)
    l64, p64 = _decisions(n64, torch.from_numpy(x).double())
    l32, p32 = _decisions(n32, torch.from_numpy(x).float())
    lre = min(float(t.abs().min()) for t in l64)
    gap = min([_pool_gap(t) for t in p64] or [float("inf")])
    noise = max(float((a.double() - b).abs().max()) for a, b in zip(l32 + p32, l64 + p64))
    return lre, gap, noise


def find_data_seed(aoi, case, limit=20000):
    for seed in range(limit):
        x, _ = _data(case[-1], seed)
        lre, gap, noise = margins(aoi, case, x)
        if lre > noise and gap > noise:
            return seed, (lre, gap, noise)
    raise AssertionError("no seed below the limit")


def net_case(aoi, name, case, steps=3):
    out = {}
    seed, (lre, gap, noise) = find_data_seed(aoi, case)
    print(f"{name}: data seed {seed}: smallest |LeakyReLU input| {lre:.3e}, smallest pooling gap {gap:.3e}, "
          f"reference fp32 noise {noise:.3e}")
    x, y = _data(case[-1], seed)
    out["x"], out["y"] = x, y
    out["data_seed"], out["margins"] = np.array(seed), np.array([lre, gap, noise])
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        net, meta = _build(aoi, case, torch.float32)
        if tag == "f32":
            out.update({k + "|init": v.detach().numpy().copy() for k, v in net.state_dict().items()})
            out["meta_keys"] = np.array(list(meta.keys()))
        net = net.to(dt)
        crit = torch.nn.MSELoss()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        xt, yt = torch.from_numpy(x).to(dt), torch.from_numpy(y).to(dt)
        losses = []
        for s in range(steps):
            net.train()
            opt.zero_grad()
            pred = net(xt)
            loss = crit(pred, yt)
            loss.backward()
            if s == 0:
                out["out|" + tag] = pred.detach().numpy()
                out.update({k + "|grad|" + tag: p.grad.detach().numpy().copy() for k, p in net.named_parameters()})
            opt.step()
            losses.append(loss.item())
            if s == 0:
                out.update({k + "|bn1|" + tag: v.detach().numpy().copy()
                            for k, v in net.state_dict().items() if "running" in k})
        out["losses|" + tag] = np.array(losses)
        net.eval()
        with torch.no_grad():
            out["eval_out|" + tag] = net(xt).numpy()
    out["meta"] = np.array([SEED])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    gmax = max(np.abs(v).max() for k, v in out.items() if k.endswith("|grad|f64"))
    gnoise = max(np.abs(out[k[:-3] + "f32"] - v).max() for k, v in out.items() if k.endswith("|grad|f64")) / gmax
    print(name, "losses f32", out["losses|f32"], "f64", out["losses|f64"], "gradient noise", gnoise,
          os.path.getsize(os.path.join(GOLD, name + ".npz")), "bytes")


def fit_case(aoi):
    rs = np.random.RandomState(0)
    clean = rs.rand(20, 16, 16).astype(np.float32)
    noisy = (clean + 0.1 * rs.randn(20, 16, 16)).astype(np.float32)
    out = {"clean": clean, "noisy": noisy}
    cwd, tmp = os.getcwd(), tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        scheds = {}
        for tag, cycles, kw in (("", 4, dict(swa=False)), ("|swa", 30, dict())):
            m = aoi.models.DenoisingAutoencoder(**FIT_ARCH)
            m.fit(noisy[:16, None], clean[:16, None], noisy[16:, None], clean[16:, None], training_cycles=cycles,
                  batch_size=4, filename=os.path.join(tmp, "ref_denoiser"), plot_training_history=False, **kw)
            out["batch_idx_train" + tag] = np.array(m.batch_idx_train)
            out["batch_idx_test" + tag] = np.array(m.batch_idx_test)
            out["train_loss|f32" + tag] = np.array(m.loss_acc["train_loss"])
            out["test_loss|f32" + tag] = np.array(m.loss_acc["test_loss"])
            out["pred5" + tag] = m.predict(noisy[:5])
            out["pred1" + tag] = m.predict(noisy[0])
            out["meta_keys" + tag] = np.array(list(m.meta_state_dict.keys()))
            if not tag:
                ckpt = os.path.join(tmp, "ref_denoiser_metadict_final.tar")
                shutil.copy(ckpt, os.path.join(GOLD, "ref_denoiser_ckpt.tar"))
                lm = aoi.models.load_model(ckpt)
                out["ckpt|pred5"], out["ckpt|pred1"] = lm.predict(noisy[:5]), lm.predict(noisy[0])
                out["ckpt|meta_keys"] = np.array(sorted(torch.load(ckpt, weights_only=False).keys()))
            scheds[tag] = [int(i) for i in m.batch_idx_train]
        # the same training steps in float64: the reference's own fp32-vs-fp64 drift over these cycles
        for tag, sched in scheds.items():
            net = aoi.models.DenoisingAutoencoder(**FIT_ARCH).net.to("cpu").double()
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)
            crit = torch.nn.MSELoss()
            l64 = []
            for i in sched:
                xb = torch.from_numpy(noisy[:16, None][4 * i: 4 * i + 4]).double()
                yb = torch.from_numpy(clean[:16, None][4 * i: 4 * i + 4]).double()
                net.train()
                opt.zero_grad()
                loss = crit(net(xb), yb)
                loss.backward()
                opt.step()
                l64.append(loss.item())
            out["train_loss|f64" + tag] = np.array(l64)
            out["drift" + tag] = np.array(np.abs(out["train_loss|f32" + tag] - out["train_loss|f64" + tag]).max()
                                          / np.abs(out["train_loss|f64" + tag]).max())
    finally:
        os.chdir(cwd)
    np.savez_compressed(os.path.join(GOLD, "denoiser_fit.npz"), **out)
    print("fit: schedule", out["batch_idx_train"], out["batch_idx_test"], "train f32", out["train_loss|f32"], "f64",
          out["train_loss|f64"], "drift", float(out["drift"]), "swa run: last losses", out["train_loss|f32|swa"][-3:],
          out["train_loss|f64|swa"][-3:], "drift", float(out["drift|swa"]), "checkpoint",
          os.path.getsize(os.path.join(GOLD, "ref_denoiser_ckpt.tar")), "bytes")


if __name__ == "__main__":
    aoi = ref_harness.import_reference()
    for name, case in CASES.items():
        net_case(aoi, name, case)
    fit_case(aoi)
