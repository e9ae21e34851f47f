"""Generates the ImSpec (im2spec / spec2im) fixtures under tests/golden/ from the REAL reference (imported through
oracle/ref_harness.py, dev container only; never imported by a test):

    python tools/make_imspec_golden.py

  imspec_<case>.npz     one per case of CASES, key scheme of seg_*.npz: the initial state dict (``<key>|init``), x, y,
                        the training-mode output (``out|f32``, ``out|f64``), per-parameter gradients of the first step
                        (``<key>|grad|f32|f64``), BatchNorm running statistics after it (``<key>|bn1|...``), three
                        Adam-step losses (``losses|...``) and the eval-mode output after them (``eval_out|...``)
  imspec_fit.npz        ImSpec.fit of the reference on rs = RandomState(0): 40 images 8 x 8 -> 40 spectra of 16, split
                        32 / 8, batch_size 8, 4 cycles: the batch schedule, train / test losses, the same training steps
                        repeated in float64 (``train_loss|f64``) and the fp32-vs-fp64 drift of the reference over those
                        cycles (``drift``), predict(X[:5], norm=False) and the checkpoint's prediction
  ref_imspec_ckpt.tar   the checkpoint that fit wrote
Every net case runs in fp32 and with the same modules ``.double()``'d, so each golden carries its own fp32 noise floor.
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

SEED, B, LATENT = 1, 4, 3
NET_KW = dict(nblayers_encoder=2, nblayers_decoder=3, nbfilters_encoder=5, nbfilters_decoder=6)
CASES = {
    "imspec_i2s": ((8, 8), (16,), dict()),
    "imspec_s2i": ((16,), (8, 8), dict()),
    "imspec_i2s_updown": ((8, 8), (16,), dict(encoder_downsampling=2, decoder_upsampling=True)),
    "imspec_s2i_nobn": ((12,), (8, 8), dict(encoder_downsampling=2, decoder_upsampling=True, batch_norm=False)),
}


def _np(d, suffix=""):
    return {k + suffix: v.detach().cpu().numpy().copy() for k, v in d.items()}


def net_case(name, in_dim, out_dim, kw, steps=3):
    from atomai.nets import init_imspec_model
    from atomai.utils import set_train_rng
    out = {}
    rs = np.random.RandomState(SEED + 100)
    x = rs.rand(B, 1, *in_dim).astype(np.float32)
    y = rs.rand(B, 1, *out_dim).astype(np.float32)
    out["x"], out["y"] = x, y
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        set_train_rng(SEED)
        net, meta = init_imspec_model(in_dim, out_dim, LATENT, **NET_KW, **kw)
        if tag == "f32":
            out.update(_np(net.state_dict(), "|init"))
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
    out["meta"] = np.array([SEED, B, LATENT] + [NET_KW[k] for k in sorted(NET_KW)])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    gmax = max(np.abs(v).max() for k, v in out.items() if k.endswith("|grad|f64"))
    noise = max(np.abs(out[k[:-3] + "f32"] - v).max() for k, v in out.items() if k.endswith("|grad|f64")) / gmax
    print(name, "losses f32", out["losses|f32"], "f64", out["losses|f64"], "gradient noise", noise)


def fit_case(aoi):
    from atomai.nets import init_imspec_model
    from atomai.utils import set_train_rng
    rs = np.random.RandomState(0)
    X = rs.rand(40, 1, 8, 8).astype(np.float32)
    y = rs.rand(40, 1, 16).astype(np.float32)
    out = {"X": X, "y": y}
    cwd, tmp = os.getcwd(), tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        m = aoi.models.ImSpec((8, 8), (16,), latent_dim=LATENT, **NET_KW)
        m.fit(X[:32], y[:32], X[32:], y[32:], training_cycles=4, batch_size=8, filename=os.path.join(tmp, "ref_imspec"),
              plot_training_history=False)
        out["batch_idx_train"], out["batch_idx_test"] = np.array(m.batch_idx_train), np.array(m.batch_idx_test)
        out["train_loss|f32"], out["test_loss|f32"] = np.array(m.loss_acc["train_loss"]), np.array(m.loss_acc["test_loss"])
        out["pred"] = m.predict(X[:5], norm=False)
        out["pred_norm"] = m.predict(X[:5])
        ckpt = os.path.join(tmp, "ref_imspec_metadict_final.tar")
        shutil.copy(ckpt, os.path.join(GOLD, "ref_imspec_ckpt.tar"))
        lm = aoi.models.load_model(ckpt)
        out["ckpt|pred"] = lm.predict(X[:5], norm=False)
        out["ckpt|meta_keys"] = np.array(sorted(torch.load(ckpt, weights_only=False).keys()))
        # the same four training steps in float64: the reference's own fp32-vs-fp64 drift over these cycles
        set_train_rng(SEED)
        net, _ = init_imspec_model((8, 8), (16,), LATENT, **NET_KW)
        net = net.double()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        crit = torch.nn.MSELoss()
        l64 = []
        for e in range(4):
            i = int(m.batch_idx_train[e])
            xb, yb = torch.from_numpy(X[:32][8 * i: 8 * i + 8]).double(), torch.from_numpy(y[:32][8 * i: 8 * i + 8]).double()
            net.train()
            opt.zero_grad()
            loss = crit(net(xb), yb)
            loss.backward()
            opt.step()
            l64.append(loss.item())
        out["train_loss|f64"] = np.array(l64)
        out["drift"] = np.array(np.abs(out["train_loss|f32"] - out["train_loss|f64"]).max() / np.abs(out["train_loss|f64"]).max())
    finally:
        os.chdir(cwd)
    np.savez_compressed(os.path.join(GOLD, "imspec_fit.npz"), **out)
    print("fit: schedule", out["batch_idx_train"], out["batch_idx_test"], "train f32", out["train_loss|f32"], "f64",
          out["train_loss|f64"], "drift", float(out["drift"]), "checkpoint",
          os.path.getsize(os.path.join(GOLD, "ref_imspec_ckpt.tar")), "bytes")


if __name__ == "__main__":
    aoi = ref_harness.import_reference()
    for name, (in_dim, out_dim, kw) in CASES.items():
        net_case(name, in_dim, out_dim, kw)
    fit_case(aoi)
