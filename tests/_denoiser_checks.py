"""Shared bodies of the DenoisingAutoencoder tests: the fused 1x1-head + MSE kernel amx_px_mse_train (csrc/head.hip) through
the C ABI with the arguments engine.PxLossNode forms, the node against the modular path through a whole net, the net against
golden vectors written by the reference (tests/golden/denoiser_*.npz, tools/make_denoiser_golden.py) and the user API.
The SAME checks run
  * on the CPU through the SIMT emulator build of the kernel sources (`not gpu` tier, test_denoiser_emulated.py), and
  * on a real MI355X through libatomai_amd.so (`gpu` tier, test_denoiser_gpu.py)."""
import copy
import os
import pickletools
import warnings
import zipfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _head_checks import Head, _compare, _nan
from _imspec_checks import GOLD, REL_TOL, _train_and_judge, relmax
from _loss_checks import UPSTREAM


class _mse_head_on:
    """The 'mse' kind of engine.PxLossNode switched on for the enclosed code, whatever the default (engine.FUSE_PX_MSE)."""

    def __enter__(self):
        import atomai_amd.engine as eng
        self.eng, self.old = eng, eng.FUSE_PX_MSE
        eng.FUSE_PX_MSE = True

    def __exit__(self, *exc):
        self.eng.FUSE_PX_MSE = self.old
        return False

# name -> (Cs, C, (N, H, W), affine): the smallest geometries that reach each branch of px_ce_train_kernel<1, true, 3>
# (G = Cs / 4 lanes share a pixel, PL = 256 / G pixel lanes per workgroup, AMX_PX_BWD_UNROLL pixels in flight)
KERNEL_CASES = {
    "g4_3x37x29": (16, 16, (3, 37, 29), True),              # 3219 pixels: a multiple of neither PL nor 1024
    "g4_3x37x29_no_scale": (16, 16, (3, 37, 29), False),
    "g2_c5_1x1030x130": (8, 5, (1, 1030, 130), True),       # PL = 128, padded channels; the denoiser's own width
    "g8_1x45x23": (32, 32, (1, 45, 23), True),              # a single workgroup
    "g64_c250_1x37x9": (256, 250, (1, 37, 9), True),        # one wave per pixel, six xor-shuffle steps
    "g1_c3_1x5x3": (4, 3, (1, 5, 3), True),                 # fewer pixels (15) than pixel lanes (256)
}
FN = "amx_px_mse_train"


class MseHead(Head):
    """_head_checks.Head's inputs for a one-channel head (activation, negative BatchNorm scales or none, weights, bias)
    with a random-normal float target (N,1,H,W) in place of the binary mask."""

    def __init__(self, device, Cs, C, nhw, affine=True, seed=0):
        super().__init__(device, "mse", Cs, C, 1, nhw, affine=affine, seed=seed)
        rs = np.random.RandomState(seed + 1000)
        self.target = torch.from_numpy(rs.randn(nhw[0], 1, nhw[1], nhw[2]).astype(np.float32)).to(device)

    def buffers(self, drows=None):
        o = super().buffers(drows)
        return {k: o[k] for k in ("dxn", "part", "partb", "bstats", "lpart")}

    def args(self, fn, o, **over):
        """The argument tuple of amx_px_mse_train as engine.PxLossNode forms it; `over` replaces single arguments."""
        from atomai_amd import _lib as L
        assert fn == FN
        g = {"Cs": self.Cs, "C": self.C, "rows": self.rows, "rows_pix": self.rows_pix, "scale": self.scale,
             "shift": self.shift, "target": self.target}
        g.update(over)
        return (L.ptr(self.a), L.ptr(g["scale"]), L.ptr(g["shift"]), L.ptr(self.w), L.ptr(self.b), L.ptr(g["target"]),
                L.ptr(o["dxn"]), L.ptr(o["part"]), L.ptr(o["partb"]), L.ptr(o["bstats"]), L.ptr(o["lpart"]),
                self.N, self.H, self.W, g["C"], g["Cs"], g["rows"], g["rows_pix"], L.stream_ptr(self.a))

    def run(self):
        """The launches of engine.PxLossNode.__init__ (kind 'mse') -> {name: host tensor} of everything they wrote."""
        from atomai_amd import _lib as L
        o = self.buffers()
        L.call(FN, *self.args(FN, o))
        o["loss"] = _nan(self.device)
        L.call("amx_reduce_rows", L.ptr(o["lpart"]), self.rows, 1, 1, 1.0 / self.npix, L.ptr(o["loss"]),
               L.stream_ptr(self.a))
        return {k: v.detach().cpu() for k, v in o.items()}

    def reference(self, dtype):
        """The same operation in `dtype` torch on the host: p = xn w^T + b, loss = mean (p - t)^2, g = d loss / d p by
        autograd, and from g what amx_px_bwd produces (see _head_checks.Head.reference)."""
        C = self.C
        a = self.a.cpu()[:, :C].to(dtype)
        xn = a * self.scale.cpu()[:C].to(dtype) + self.shift.cpu()[:C].to(dtype) if self.affine else a
        w, b = self.w.cpu().to(dtype), self.b.cpu().to(dtype)
        p = (xn @ w.t() + b).reshape(-1).clone().requires_grad_(True)
        terms = (p - self.target.cpu().to(dtype).reshape(-1)) ** 2
        loss = terms.mean()
        loss.backward()
        t = torch.zeros(self.rows * self.rows_pix, dtype=dtype)
        t[:self.npix] = terms.detach()
        gf = p.grad.reshape(self.npix, 1)
        r = {"loss": float(loss.detach()), "lpart": t.reshape(self.rows, self.rows_pix).sum(1), "dxn": gf @ w,
             "dW": gf.t() @ xn, "db": gf.sum(0)}
        r["bstats"] = torch.stack([r["dxn"].sum(0), (r["dxn"] * a).sum(0)])
        return r


def check_kernel_case(name, device):
    """The judgement of _head_checks.check_case: every buffer fully written, the padding of dxn exactly 0, the loss within
    REL_TOL of fp64, dxn / dW / db / bstats / lpart within max(4 x the fp32-torch floor, 2e-5) of the largest fp64 entry,
    and a repeated call bit-identical."""
    Cs, C, nhw, affine = KERNEL_CASES[name]
    h = MseHead(device, Cs, C, nhw, affine=affine)
    o = h.run()
    for k, v in o.items():
        assert bool(torch.isfinite(v).all()), (name, k, int((~torch.isfinite(v)).sum()))
    assert not bool(o["dxn"][:, C:].any()), name
    r64, r32 = h.reference(torch.float64), h.reference(torch.float32)
    lerr = abs(float(o["loss"]) - r64["loss"]) / abs(r64["loss"])
    print(f"mse head {name} loss: {float(o['loss']):.8f} (fp64 {r64['loss']:.8f}, rel {lerr:.2e})")
    assert lerr < REL_TOL, (name, float(o["loss"]), r64["loss"])
    got = {"dxn": o["dxn"][:, :C], "dW": o["part"].double().sum(0)[:, :C], "db": o["partb"].double().sum(0),
           "bstats": o["bstats"].double().sum(0)[:, :C], "lpart": o["lpart"]}
    for what, v in got.items():
        _compare("mse " + name, what, v, r64[what], r32[what])
    again = h.run()
    for k, v in o.items():
        assert torch.equal(v.view(torch.int32), again[k].view(torch.int32)), (name, k)


REFUSALS = ("Cs12", "rows", "scale_without_shift", "shift_without_scale", "null_target")


def check_refusal(why, device):
    """Cs = 12 (G = 3, no power of two), rows x rows_pix < npix, one of scale / shift without the other, a NULL target:
    AmxError, and every (valid, NaN-filled) output buffer is untouched.  The unmodified call is accepted first."""
    from atomai_amd import _lib as L
    h = MseHead(device, 16, 10, (2, 30, 40))
    over = {"Cs12": {"Cs": 12}, "rows": {"rows_pix": (h.npix - 1) // h.rows}, "scale_without_shift": {"shift": None},
            "shift_without_scale": {"scale": None}, "null_target": {"target": None}}[why]
    L.call(FN, *h.args(FN, h.buffers()))
    o = h.buffers()
    with pytest.raises(L.AmxError):
        L.call(FN, *h.args(FN, o, **over))
    for k, v in o.items():
        assert bool(torch.isnan(v).all()), (why, k)


# ---------------------------------------------------------------- the node against the modular path through a whole net
def check_net_beyond_one_tile(device, last_filters, expect):
    """_head_checks.check_net_beyond_one_tile for the denoiser: forward_loss against MSELoss()(net(x), y) with BatchNorm
    momentum 0 at every UPSTREAM scale, input 2 x 1 x 264 x 72 (W = 72 > PL = 64, N H = 528 > 512 image rows).  Last
    decoder filters 16 (G = 4): the fused node runs ('loss'); 12 (G = 3): it declines ('logits'), same values."""
    from atomai_amd.losses_metrics.losses import select_loss
    from atomai_amd.nets import DenoiserNet
    rs = np.random.RandomState(7)
    shape = (2, 1, 264, 72)
    crit = select_loss("mse")
    for gscale in UPSTREAM:
        torch.manual_seed(5)
        net = DenoiserNet([3, 4], [4, last_filters], [1, 1], [1, 1], True, "nearest")
        net.to(device).train()
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 0.0                                 # (two forwards over the same batch)
        x = torch.from_numpy(rs.rand(*shape).astype(np.float32)).to(device).requires_grad_(True)
        y = torch.from_numpy(rs.randn(*shape).astype(np.float32)).to(device)
        loss0 = crit(net(x), y)
        (loss0 * gscale).backward()
        loss0 = loss0.detach()
        ref = [p.grad.clone() for p in net.parameters()] + [x.grad.clone()]
        net.zero_grad()
        x.grad = None
        with _mse_head_on():
            k, out = net.forward_loss(x, y, criterion=crit)
        assert k == expect, k
        loss1 = out if k == "loss" else crit(out, y)
        (loss1 * gscale).backward()
        loss1 = loss1.detach()
        got = [p.grad for p in net.parameters()] + [x.grad]
        gmax = max(float(t.abs().max()) for t in ref)
        worst = max(float((a - b).abs().max()) for a, b in zip(got, ref)) / gmax
        print(f"mse denoiser last filters {last_filters} {shape} upstream {gscale}: {k} {float(loss1):.8f} vs modular "
              f"{float(loss0):.8f}; worst gradient difference {worst:.2e} of gmax")
        assert abs(float(loss0) - float(loss1)) < 2e-6 * max(1.0, abs(float(loss0))), (float(loss0), float(loss1))
        for (pname, _), a, b in zip(list(net.named_parameters()) + [("input", None)], got, ref):
            assert float((a - b).abs().max()) < 2e-5 * gmax, (pname, float((a - b).abs().max()), gmax)


# ---------------------------------------------------------------- net cases against the reference goldens
# name -> (encoder_filters, decoder_filters, encoder_layers, decoder_layers, use_batch_norm, upsampling_mode, fused head?)
NET_CASES = {
    "denoiser_a": ([4, 6, 8], [8, 6, 4], [1, 2, 2], [2, 2, 1], False, "nearest", True),
    "denoiser_b": ([4, 6, 8], [8, 6, 4], [1, 2, 2], [2, 2, 1], True, "bilinear", True),
    # padded channels, a first block that is not the one-layer fast path, a head (G = 3) the fused node must decline
    "denoiser_c": ([5, 12], [12, 12], [2, 1], [1, 2], True, "nearest", False),
}
META_KEYS = ["model_type", "encoder_filters", "decoder_filters", "encoder_layers", "decoder_layers", "use_batch_norm",
             "upsampling_mode", "weights"]


def check_net_case(name, device):
    """Net parity against the reference golden: state-dict keys, shapes (in order) and initial values under the same seed,
    then _imspec_checks._train_and_judge (training-mode output within REL_TOL of fp64, first-step gradients against fp64
    relative to the golden's own fp32 noise, running statistics after one step, three Adam-step losses, the eval output);
    and the fused step (forward_loss) on a copy of the net: its loss and gradients under the same first-step rules."""
    import atomai_amd as aoi
    ef, df, el, dl, bn, up, fused = NET_CASES[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    lre, gap, noise = g["margins"]
    print(f"{name}: data seed {int(g['data_seed'])}, smallest |LeakyReLU input| {lre:.3e}, pooling gap {gap:.3e}, "
          f"reference fp32 noise {noise:.3e}")
    assert lre > noise and gap > noise
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net, meta = aoi.models.denoiser.init_denoising_autoencoder(
            encoder_filters=ef, decoder_filters=df, encoder_layers=el, decoder_layers=dl, use_batch_norm=bn,
            upsampling_mode=up, seed=int(g["meta"][0]))
    assert list(meta) == META_KEYS == [str(k) for k in g["meta_keys"]]
    net.cpu()
    sd = net.state_dict()
    assert [k + "|init" for k in sd] == [k for k in g.files if k.endswith("|init")]      # the same keys, in order
    for k, v in sd.items():
        assert tuple(v.shape) == g[k + "|init"].shape and np.array_equal(v.numpy(), g[k + "|init"]), k
    net.to(device)
    names = [k for k, _ in net.named_parameters()]
    x, y = torch.from_numpy(g["x"]).to(device), torch.from_numpy(g["y"]).to(device)
    ref = dict(out=g["out|f64"], grads={k: g[k + "|grad|f64"] for k in names},
               ref32={k: np.abs(g[k + "|grad|f32"] - g[k + "|grad|f64"]).max() for k in names},
               bn1={k[:-8]: g[k] for k in g.files if k.endswith("|bn1|f64")}, losses=g["losses|f64"],
               eval=g["eval_out|f32"])
    # ---- the fused step on a copy (the forward pass moves the BatchNorm running statistics)
    from atomai_amd.losses_metrics import select_loss
    twin = copy.deepcopy(net).train()
    crit = select_loss("mse")
    with _mse_head_on():
        kind, out = twin.forward_loss(x, y, criterion=crit)
    assert kind == ("loss" if fused else "logits"), (name, kind)
    loss = out if kind == "loss" else crit(out, y)
    loss.backward()
    np.testing.assert_allclose(loss.item(), ref["losses"][0], rtol=REL_TOL)
    gmax = max(np.abs(v).max() for v in ref["grads"].values())
    for k, p in twin.named_parameters():
        err = np.abs(p.grad.cpu().numpy() - ref["grads"][k]).max() / gmax
        print(f"  fused step grad {k}: err {err:.3e} ref32 {ref['ref32'][k] / gmax:.3e}")
        assert err <= max(4 * ref["ref32"][k] / gmax, 2e-5), (k, err)
    for k, v in twin.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), ref["bn1"][k], rtol=REL_TOL, atol=1e-6)
    _train_and_judge(net, x, y, ref, device)


# ---------------------------------------------------------------- model level
FIT_ARCH = dict(encoder_filters=[4, 6, 8], decoder_filters=[8, 6, 4], encoder_layers=[1, 2, 2], decoder_layers=[2, 2, 1])


def _fit_data():
    g = np.load(os.path.join(GOLD, "denoiser_fit.npz"))
    return g, g["noisy"], g["clean"]


def _fit(tmp_path, tag, noisy, clean, cycles, **kw):
    import atomai_amd as aoi
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # (no GPU in the emulator tier; the channel axis)
        m = aoi.models.DenoisingAutoencoder(**FIT_ARCH)
        m.fit(noisy[:16], clean[:16], noisy[16:], clean[16:], training_cycles=cycles, batch_size=4,
              filename=os.path.join(str(tmp_path), tag), plot_training_history=False, **kw)
    return m


def _torch_only(o):
    if isinstance(o, dict):
        return all(_torch_only(v) for v in o.values())
    if isinstance(o, (list, tuple)):
        return all(_torch_only(v) for v in o)
    return isinstance(o, (torch.Tensor, int, float, bool, str, type(None), torch.optim.Optimizer))


def _pickled_globals(path):
    """Every module.name a torch.save file refers to (read from the pickle's opcodes, nothing is imported)."""
    with zipfile.ZipFile(path) as z:
        data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    out, strs = set(), []
    for op, arg, _ in pickletools.genops(data):
        if op.name == "GLOBAL":
            out.add(arg.replace(" ", "."))
        elif op.name in ("SHORT_BINUNICODE", "BINUNICODE", "UNICODE"):
            strs.append(arg)
        elif op.name == "STACK_GLOBAL":
            out.add(strs[-2] + "." + strs[-1])
    return out


def check_determinism(device, tmp_path):
    """Two identical fits: equal loss lists, bit-equal weights."""
    _, noisy, clean = _fit_data()
    runs = []
    for _ in range(2):
        m = _fit(tmp_path, "det", noisy, clean, 4, swa=False)
        runs.append((list(m.loss_acc["train_loss"]), list(m.loss_acc["test_loss"]),
                     {k: v.detach().cpu().clone() for k, v in m.net.state_dict().items()}))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k, v in runs[0][2].items():
        assert torch.equal(v, runs[1][2][k]), k


def check_api(device, tmp_path):
    """DenoisingAutoencoder.fit / predict / save_model / load_model / the reference's checkpoint / load_weights /
    init_denoising_autoencoder / denoise_images, against the reference's run of the same recipe (denoiser_fit.npz)."""
    import atomai_amd as aoi
    from atomai_amd.trainers import trainer as T
    g, noisy, clean = _fit_data()
    # ---- swa=False, 4 cycles; the trainer's steps went through the fused node
    calls = []
    orig = aoi.nets.DenoiserNet.forward_loss

    def spy(self, *a, **k):
        r = orig(self, *a, **k)
        calls.append(r[0])
        return r
    aoi.nets.DenoiserNet.forward_loss = spy
    try:
        with _mse_head_on():
            m = _fit(tmp_path, "dn", noisy, clean, 4, swa=False)
    finally:
        aoi.nets.DenoiserNet.forward_loss = orig
    assert calls == ["loss"] * 4 and T.FUSE_LOSS
    assert list(m.batch_idx_train) == list(g["batch_idx_train"]) and list(m.batch_idx_test) == list(g["batch_idx_test"])
    tl = np.array(m.loss_acc["train_loss"])
    print("train losses", tl, "reference f64", g["train_loss|f64"], "drift", float(g["drift"]))
    np.testing.assert_allclose(tl[0], g["train_loss|f64"][0], rtol=REL_TOL)
    np.testing.assert_allclose(tl[1:], g["train_loss|f64"][1:], rtol=max(4 * float(g["drift"]), REL_TOL))
    np.testing.assert_allclose(m.loss_acc["test_loss"], g["test_loss|f32"], rtol=max(4 * float(g["drift"]), REL_TOL))
    assert repr(m.criterion) == "MSELoss()"
    assert list(m.meta_state_dict) == [str(k) for k in g["meta_keys"]]
    for k, v in m.net.state_dict().items():                      # refreshed after run()
        assert m.meta_state_dict["weights"][k].data_ptr() == v.data_ptr(), k
    pred5, pred1 = m.predict(noisy[:5]), m.predict(noisy[0])
    assert pred5.shape == g["pred5"].shape == (5, 16, 16) and pred5.dtype == np.float32
    assert pred1.shape == g["pred1"].shape == (16, 16)
    # (weights after four Adam steps of fp32 training: the loose rule of _imspec_checks._train_and_judge's eval output)
    assert relmax(pred5, g["pred5"].astype(np.float64)) < 2e-2 and relmax(pred1, g["pred1"].astype(np.float64)) < 2e-2
    assert np.array_equal(m.predict(noisy[:5, None]), pred5)
    assert relmax(m.predict(noisy[:5], num_batches=2), pred5.astype(np.float64)) < REL_TOL
    # ---- the default swa=True over the shortest run the reference's averaging takes (30 cycles)
    ms = _fit(tmp_path, "dn_swa", noisy, clean, 30)
    assert ms.swa and sorted(ms.running_weights) == list(range(30))
    assert list(ms.batch_idx_train) == list(g["batch_idx_train|swa"])
    ts = np.array(ms.loss_acc["train_loss"])
    print("swa run: last train losses", ts[-3:], "reference f64", g["train_loss|f64|swa"][-3:], "drift",
          float(g["drift|swa"]))
    np.testing.assert_allclose(ts[0], g["train_loss|f64|swa"][0], rtol=REL_TOL)
    np.testing.assert_allclose(ts[1:], g["train_loss|f64|swa"][1:], rtol=max(4 * float(g["drift|swa"]), REL_TOL))
    ps = ms.predict(noisy[:5])
    assert ps.shape == g["pred5|swa"].shape and relmax(ps, g["pred5|swa"].astype(np.float64)) < 2e-2
    assert relmax(ms.predict(noisy[0]), g["pred1|swa"].astype(np.float64)) < 2e-2
    assert list(ms.meta_state_dict) == [str(k) for k in g["meta_keys|swa"]]
    # ---- checkpoint written here: torch types only, reloads to bit-equal weights
    ck = os.path.join(str(tmp_path), "dn_metadict_final.tar")
    loaded = torch.load(ck, weights_only=False)
    assert sorted(loaded.keys()) == sorted(str(k) for k in g["ckpt|meta_keys"])
    assert type(loaded["optimizer"]) is torch.optim.Adam and loaded["use_batch_norm"] is False
    assert _torch_only(loaded)
    mods = {n.split(".")[0] for n in _pickled_globals(ck)}
    assert mods <= {"torch", "collections", "builtins", "__builtin__", "_codecs"} and "torch" in mods, mods
    m2 = aoi.models.load_model(ck)
    assert isinstance(m2, aoi.models.DenoisingAutoencoder) and not m2.net.training
    for k, v in m.net.state_dict().items():
        assert torch.equal(v.cpu(), m2.net.state_dict()[k].cpu()), k
    assert np.array_equal(m2.predict(noisy[:5]), pred5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m3 = aoi.models.DenoisingAutoencoder(**FIT_ARCH, seed=3)
    m3.load_weights(ck)
    assert np.array_equal(m3.predict(noisy[:5]), pred5)
    # ---- the checkpoint the reference wrote
    mr = aoi.models.load_model(os.path.join(GOLD, "ref_denoiser_ckpt.tar"))
    assert isinstance(mr, aoi.models.DenoisingAutoencoder) and not mr.net.training
    p5, p1 = mr.predict(noisy[:5]), mr.predict(noisy[0])
    assert p5.shape == g["ckpt|pred5"].shape and p1.shape == g["ckpt|pred1"].shape
    assert relmax(p5, g["ckpt|pred5"].astype(np.float64)) < REL_TOL
    assert relmax(p1, g["ckpt|pred1"].astype(np.float64)) < REL_TOL
    # a checkpoint without the "use_batch_norm" entry is rebuilt WITH BatchNorm (the reference loader's default)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mb = aoi.models.DenoisingAutoencoder(**FIT_ARCH, use_batch_norm=True)
    meta = {k: v for k, v in mb.meta_state_dict.items() if k != "use_batch_norm"}
    torch.save(meta, os.path.join(str(tmp_path), "nokey.tar"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert any("running_mean" in k for k in aoi.models.load_model(
            os.path.join(str(tmp_path), "nokey.tar")).net.state_dict())
    # ---- no test set: 15 % split off; denoise_images; init_denoising_autoencoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        md, pd = aoi.models.denoise_images(noisy, clean, training_cycles=2, batch_size=3, swa=False, **FIT_ARCH,
                                           filename=os.path.join(str(tmp_path), "di"), plot_training_history=False)
        assert pd is None and len(md.loss_acc["train_loss"]) == 2 and len(md.loss_acc["test_loss"]) == 2
        md, pd = aoi.models.denoise_images(noisy[:16], clean[:16], noisy[16:], clean[16:], training_cycles=2, batch_size=4,
                                           swa=False, **FIT_ARCH, filename=os.path.join(str(tmp_path), "di"),
                                           plot_training_history=False)
        assert pd.shape == (4, 16, 16)
        net, meta = aoi.models.denoiser.init_denoising_autoencoder(**FIT_ARCH)
    assert isinstance(net, aoi.nets.DenoiserNet) and isinstance(net, torch.nn.Sequential) and list(meta) == META_KEYS


def check_preprocess():
    """utils.preprocess_denoiser_data: the reference's warnings, float32 output, TypeError / ValueError cases."""
    from atomai_amd.utils import preprocess_denoiser_data
    rs = np.random.RandomState(1)
    a, b = rs.rand(6, 8, 8), rs.rand(3, 8, 8)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = preprocess_denoiser_data(a, a + 1, b, b + 1)
    assert [str(x.message) for x in w] == [f"Adding channel dimension of 1 to {s} images" for s in
                                           ("noisy training", "clean training", "noisy test", "clean test")]
    assert all(x.category is UserWarning for x in w)
    assert [tuple(t.shape) for t in out] == [(6, 1, 8, 8)] * 2 + [(3, 1, 8, 8)] * 2
    assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 for t in out)
    assert torch.equal(out[1], torch.from_numpy(a + 1).float()[:, None])
    with warnings.catch_warnings(record=True) as w:                           # torch input, channel axis present
        warnings.simplefilter("always")
        t4 = [torch.from_numpy(v[:, None]) for v in (a, a, b, b)]
        out = preprocess_denoiser_data(*t4)
    assert not w and all(t.dtype == torch.float32 and t.ndim == 4 for t in out)
    with warnings.catch_warnings(record=True) as w:                           # only one stack lacks the axis
        warnings.simplefilter("always")
        preprocess_denoiser_data(a[:, None], a[:, None], b, b[:, None])
    assert [str(x.message) for x in w] == ["Adding channel dimension of 1 to noisy test images"]
    with pytest.raises(TypeError):
        preprocess_denoiser_data(a, torch.from_numpy(a), b, b)
    with pytest.raises(TypeError):
        preprocess_denoiser_data(a.tolist(), a, b, b)
    with pytest.raises(ValueError, match="training"):
        preprocess_denoiser_data(a[:, None], a[:5, None], b[:, None], b[:, None])
    with pytest.raises(ValueError, match="test"):
        preprocess_denoiser_data(a[:, None], a[:, None], b[:, None], b[:, None, :, :7])


def check_refuses_indivisible_input(device, tmp_path):
    """H or W not divisible by 2 ** (len(encoder_filters) - 1): an AssertionError that names the factor, from the net in
    both modes, from the fused step, and from fit before any training."""
    import atomai_amd as aoi
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = aoi.models.DenoisingAutoencoder(**FIT_ARCH)
    x = torch.rand(2, 1, 16, 18, device=device)
    for mode in (m.net.train, m.net.eval):
        mode()
        with pytest.raises(AssertionError, match="divisible by 4"):
            m.net(x)
    m.net.train()
    with pytest.raises(AssertionError, match="divisible by 4"):
        m.net.forward_loss(x, x.clone())
    with pytest.raises(AssertionError, match="divisible by 4"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(np.zeros((8, 18, 16), np.float32), np.zeros((8, 18, 16), np.float32), np.zeros((4, 18, 16), np.float32),
              np.zeros((4, 18, 16), np.float32), training_cycles=1, batch_size=4,
              filename=os.path.join(str(tmp_path), "bad"))
    assert m.optimizer is None and not m.loss_acc["train_loss"]
    # a net without poolings takes any size
    from atomai_amd.nets import DenoiserNet
    torch.manual_seed(0)
    n1 = DenoiserNet([3], [4], [1], [1]).to(device).eval()
    with torch.no_grad():
        assert n1(torch.rand(1, 1, 7, 9, device=device)).shape == (1, 1, 7, 9)


def check_forward_hooks(device):
    """A forward hook on a child (a ConvBlock, a MaxPool2d, an UpsampleBlock, the final Conv2d, the decoder itself) sees
    that child's input and output; the net's output is that of the single-tape path; the pooling and the 1x1 convolution
    of the block-by-block path run on the HIP kernels (their ATen forwards are never entered)."""
    from atomai_amd.nets import DenoiserNet
    torch.manual_seed(2)
    net = DenoiserNet([4, 6], [6, 4], [1, 2], [2, 1], True, "bilinear").to(device).eval()
    x = torch.rand(2, 1, 8, 12, device=device)
    with torch.no_grad():
        plain = net(x)
    seen = {}
    targets = {"block": net[0][0], "pool": net[0][1], "up": net[1][1], "px": net[1][3], "decoder": net[1]}
    hooks = [mod.register_forward_hook(lambda mod, i, o, k=k: seen.__setitem__(k, (i[0].detach().cpu(), o.detach().cpu())))
             for k, mod in targets.items()]
    aten = []
    orig_pool, orig_conv = torch.nn.MaxPool2d.forward, torch.nn.Conv2d.forward
    torch.nn.MaxPool2d.forward = lambda self, t: aten.append("pool") or orig_pool(self, t)
    torch.nn.Conv2d.forward = lambda self, t: aten.append("conv") or orig_conv(self, t)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.no_grad():
                hooked = net(x)
    finally:
        torch.nn.MaxPool2d.forward, torch.nn.Conv2d.forward = orig_pool, orig_conv
        for h in hooks:
            h.remove()
    assert not aten, aten
    assert set(seen) == set(targets)
    assert torch.equal(seen["block"][0], x.cpu()) and seen["block"][1].shape == (2, 4, 8, 12)
    assert torch.equal(seen["pool"][0], seen["block"][1])
    assert torch.equal(seen["pool"][1], F.max_pool2d(seen["pool"][0], 2, 2))
    assert seen["up"][0].shape == (2, 6, 4, 6) and seen["up"][1].shape == (2, 6, 8, 12)
    assert torch.equal(seen["px"][1], hooked.cpu()) and torch.equal(seen["decoder"][1], hooked.cpu())
    assert seen["px"][0].shape == (2, 4, 8, 12) and seen["decoder"][0].shape == (2, 6, 4, 6)
    w, b = net[1][3].weight.detach().double().cpu(), net[1][3].bias.detach().double().cpu()
    assert relmax(seen["px"][1].numpy(), F.conv2d(seen["px"][0].double(), w, b).numpy()) < 1e-5
    assert relmax(hooked.cpu().numpy(), plain.double().cpu().numpy()) < 1e-5
    with torch.no_grad():                                       # hooks removed: the single-tape path again, same bits
        assert torch.equal(net(x), plain)
