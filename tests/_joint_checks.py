"""Shared bodies of the joint-VAE (jVAE / jrVAE) tests: emulator tier on CPU, gpu tier on the MI355X.

Goldens: tests/golden/joint_kernels.npz, vae_joint.npz and ref_jrvae_ckpt.tar, written by tools/make_golden_joint.py from
the live reference, every number in fp32 and in fp64.  Bounds: REL_TOL = 1e-4 is the project's target; "floor" is the
golden's own fp32-vs-fp64 difference, i.e. what two correct fp32 implementations may differ by; errors and floors are
normalised by the largest entry of the fp64 tensor."""
import hashlib
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_TOL = 1e-4

# the cases of tools/make_golden_joint.py (all B = 6, 32-wide nets unless stated)
_W = dict(numhidden_encoder=32, numhidden_decoder=32)
CASES = {
    "jvae16": dict(cls="jVAE", in_dim=(16, 16), ctor=dict(discrete_dim=[10], **_W), fit=dict()),
    "jrvae16": dict(cls="jrVAE", in_dim=(16, 16), ctor=dict(discrete_dim=[3, 5], **_W), fit=dict()),
    "jrvae16_nt_skip": dict(cls="jrVAE", in_dim=(16, 16), ctor=dict(discrete_dim=[2], translation=False, skip=True, **_W),
                            fit=dict()),
    "jvae16_conv": dict(cls="jVAE", in_dim=(16, 16), ctor=dict(conv_encoder=True, numhidden_encoder=8,
                                                               numhidden_decoder=32), fit=dict()),
    "jrvae12_rgb_ce": dict(cls="jrVAE", in_dim=(12, 12, 3), ctor=dict(**_W), fit=dict(), loss="ce"),
    "jvae16_cap": dict(cls="jVAE", in_dim=(16, 16), ctor=dict(**_W),
                       fit=dict(cont_capacity=[5.0, 100, 2.0], disc_capacity=[1.0, 50, 3.0], temperature=0.4)),
}

_cache = {}


def golden(fname):
    if fname not in _cache:
        _cache[fname] = dict(np.load(os.path.join(GOLD, fname)))
    return _cache[fname]


def kernel_cases():
    return [str(c) for c in golden("joint_kernels.npz")["cases"]]


def model_cases():
    cases = [str(c) for c in golden("vae_joint.npz")["cases"]]
    assert cases == list(CASES)
    return cases


def _close(got, g, key, what):
    """|got - fp64| / max|fp64| < max(REL_TOL, 2 x floor); an all-zero fp64 tensor must be met exactly."""
    ref, f32 = g[key + "|f64"].astype(np.float64), g[key + "|f32"].astype(np.float64)
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), what
    scale = np.abs(ref).max()
    if scale == 0.0:
        assert not got.any(), (what, got)
        return 0.0
    err, floor = np.abs(got - ref).max() / scale, np.abs(f32 - ref).max() / scale
    print(f"{what}: error {err:.2e}, golden fp32 floor {floor:.2e}")
    assert err < max(REL_TOL, 2 * floor), (what, err, floor)
    return err


def check_joint_kernels(name, device):
    """Softmax heads, Gumbel-Softmax sample and kld_discrete, values and gradients, of one joint_kernels.npz case."""
    from atomai_amd._joint import gumbel_softmax, kl_discrete_rows, seg_softmax
    from atomai_amd.losses_metrics import kld_discrete
    g = golden("joint_kernels.npz")
    sizes = [int(k) for k in g[name + "|sizes"]]
    tau = float(g[name + "|tau"])
    t = lambda k: torch.from_numpy(g[f"{name}|{k}"]).to(device)
    lg = t("logits").requires_grad_(True)
    alpha = seg_softmax(lg, sizes)
    alpha.retain_grad()
    heads = [alpha] if len(sizes) == 1 else list(alpha.split(sizes, 1))
    us = t("u").split(sizes, 1)
    y = torch.cat([gumbel_softmax(a, u, tau) for a, u in zip(heads, us)], 1)
    kls = torch.cat([kld_discrete(a) for a in heads])
    assert kls.shape == (len(sizes),) and kld_discrete(heads[0]).shape == (1,)
    _close(alpha, g, name + "|alpha", "alpha")
    _close(y, g, name + "|y", "sample")
    _close(kls, g, name + "|kl", "kld_discrete")
    # the packed form the models' default path uses: all heads in one launch, per-sample sums
    rows = kl_discrete_rows(alpha.detach(), sizes)
    assert rows.shape == (lg.shape[0],)
    ref = float(g[name + "|kl|f64"].sum())
    if ref == 0.0:
        assert not rows.any()
    else:
        floor = abs(float(g[name + "|kl|f32"].astype(np.float64).sum()) - ref) / abs(ref)
        assert abs(float(rows.double().mean()) - ref) / abs(ref) < max(REL_TOL, 2 * floor)
    (y * t("dy")).sum().backward(retain_graph=True)
    _close(alpha.grad, g, name + "|dalpha_sample", "d sample / d alpha")
    _close(lg.grad, g, name + "|dlogits_sample", "d sample / d logits")
    sample_grads = (alpha.grad.clone(), lg.grad.clone())
    alpha.grad, lg.grad = None, None
    (kls * t("ckl")).sum().backward()
    _close(alpha.grad, g, name + "|dalpha_kl", "d KL / d alpha")
    _close(lg.grad, g, name + "|dlogits_kl", "d KL / d logits")
    if sizes == [1]:                                         # a one-category head is deterministic: exact, not close
        assert torch.equal(y, torch.ones_like(y)) and torch.equal(alpha.detach(), torch.ones_like(y))
        assert not kls.detach().any() and not rows.any()
        assert not sample_grads[0].any() and not sample_grads[1].any() and not lg.grad.any()


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _build(name):
    import atomai_amd as aoi
    c = CASES[name]
    m = getattr(aoi.models, c["cls"])(c["in_dim"], latent_dim=2, seed=0, **c["ctor"])
    if m.coord:                                              # what jrVAE.fit sets before the loop
        m.dx_prior = 0.1
        m.kdict_["phi_prior"] = 0.1
    for k, v in c["fit"].items():
        m.kdict_[k] = v
    m.loss = c.get("loss", "mse")
    return m, c


def check_joint_case(name, device):
    """check_vae_case for a joint model: bit-equal initialisation, first-step gradients, three Adam-step ELBOs with the
    golden's noise injected through the step-by-step path, encode() shapes, alphas that sum to one."""
    from atomai_amd._joint import gumbel_softmax
    g = {k[len(name) + 1:]: v for k, v in golden("vae_joint.npz").items() if k.startswith(name + "|")}
    m, c = _build(name)
    for which, net in (("enc", m.encoder_net), ("dec", m.decoder_net)):
        sd = net.state_dict()
        assert {k for k in g if k.startswith(which + "|")} == {f"{which}|{k}|sha256" for k in sd}
        for k, v in sd.items():                              # RNG-order initialisation == reference, bit for bit
            assert _sha(v) == str(g[f"{which}|{k}|sha256"]), (which, k)
    x, sizes = g["x"], [int(k) for k in g["sizes"]]
    assert sizes == list(m.discrete_dim) == list(m.encoder_net.discrete_dim)
    eps_all, u_all = torch.from_numpy(g["eps"]).to(device), torch.from_numpy(g["u"]).to(device)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    m.compile_trainer((x, None), None, batch_size=x.shape[0])
    state = {"i": 0, "h": 0}
    m.reparameterize = lambda zm, zs: zm + zs * eps_all[state["i"]]

    def reparam_disc(alpha, tau):
        h = state["h"]
        state["h"] = (h + 1) % len(sizes)
        return gumbel_softmax(alpha, u_all[state["i"]][:, offs[h]:offs[h + 1]], tau)
    m.reparameterize_discrete = reparam_disc
    assert not m._default_sampling()
    xt = torch.from_numpy(x).to(device)
    elbos = []
    for s in range(3):
        state["i"], state["h"] = s, 0
        m.encoder_net.train(), m.decoder_net.train()
        m.optim.zero_grad()
        elbo = m.forward_compute_elbo(xt)
        (-elbo).backward()
        if s == 0:
            for which, net in (("enc", m.encoder_net), ("dec", m.decoder_net)):
                for k, p in net.named_parameters():
                    ref, floor = g[f"g{which}|{k}|f64"].astype(np.float64), float(g[f"g{which}|{k}|floor"])
                    err = np.abs(p.grad.cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-30)
                    assert err < max(REL_TOL, 2 * floor), (which, k, err, floor)
        m.optim.step()
        elbos.append(elbo.item())
    assert m.kdict_["num_iter"] == 3
    print(name, "ELBOs", elbos, "golden fp64", g["elbo|f64"])
    np.testing.assert_allclose(elbos, g["elbo|f64"], rtol=REL_TOL)
    with torch.no_grad():
        lat = m.encoder_net(xt)
    assert isinstance(lat, list) and len(lat) == 2 + len(sizes)
    np.testing.assert_allclose(lat[0].cpu().numpy(), g["zmean|f64"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(torch.cat(lat[2:], 1).cpu().numpy(), g["alphas|f64"], rtol=2e-3, atol=2e-4)
    zm, zs, al = m.encode(x)
    Z = m.z_dim - sum(sizes)
    assert zm.shape == g["zmean|f64"].shape == (x.shape[0], Z) and zs.shape == zm.shape
    assert al.shape == g["alphas|f64"].shape == (x.shape[0], sum(sizes))
    for h in range(len(sizes)):
        assert np.abs(al[:, offs[h]:offs[h + 1]].sum(1) - 1.0).max() < 1e-6


def check_default_path_equals_step_path(device):
    """forward_compute_elbo with stock reparameterize / reparameterize_discrete takes the one-launch path (csrc/joint.hip
    amx_joint_latent_*); overriding either selects the reference's step-by-step dataflow.  Under the same seed both
    must draw the same noise (one normal_() of (B, Z), then one uniform_() per head) and give the same ELBO and
    gradients."""
    import atomai_amd as aoi
    configs = [("jVAE", {}), ("jrVAE", dict(translation=True)), ("jrVAE", dict(translation=False))]
    for cls, kw in configs:
        m = getattr(aoi.models, cls)((16, 16), latent_dim=2, discrete_dim=[3, 5], seed=0, numhidden_encoder=32,
                                     numhidden_decoder=32, **kw)
        if m.coord:
            m.dx_prior, m.kdict_["phi_prior"] = 0.1, 0.1
        assert m._default_sampling() and m.fused_latent
        x = torch.rand(6, 16, 16).to(device)
        params = list(m.encoder_net.parameters()) + list(m.decoder_net.parameters())
        res = []
        for fused in (True, False):
            torch.manual_seed(3)
            for p in params:
                p.grad = None
            if not fused:                                        # an instance-level override selects the step-by-step path
                m.reparameterize = lambda zm, zs: zm + zs * zm.new(zm.size(0), zm.size(1)).normal_()
                assert not m._default_sampling()
            m.encoder_net.train(), m.decoder_net.train()
            m.kdict_["num_iter"] = 0                             # both at the same point of the capacity schedule
            elbo = m.forward_compute_elbo(x)
            (-elbo).backward()
            res.append((elbo.item(), [p.grad.detach().cpu().clone() for p in params]))
        assert abs(res[0][0] - res[1][0]) < 1e-5 * abs(res[1][0]), (cls, kw, res[0][0], res[1][0])
        for a, b in zip(res[0][1], res[1][1]):
            assert float((a - b).abs().max()) <= 1e-5 * max(1e-6, float(b.abs().max())), (cls, kw)


def check_api(device, tmp_path):
    """fit -> checkpoint -> load_model round trip, decode, the reference-written checkpoint, the error paths and the
    unchanged construction of VAE / rVAE."""
    import atomai_amd as aoi
    from atomai_amd.nets import init_VAE_nets
    X = np.random.RandomState(0).rand(8, 8, 8).astype(np.float32)
    for cls, kw in (("jrVAE", {}), ("jVAE", {})):
        m = getattr(aoi.models, cls)((8, 8), latent_dim=2, discrete_dim=[3], numhidden_encoder=16, numhidden_decoder=16, **kw)
        fname = str(tmp_path / cls)
        m.fit(X, training_cycles=2, batch_size=4, filename=fname, temperature=0.5)
        assert len(m.loss_history["train_loss"]) == 2 and m.kdict_["num_iter"] == 4 and m.kdict_["temperature"] == 0.5
        ck = torch.load(fname + ".tar", weights_only=False)
        assert {"encoder", "decoder", "optimizer", "num_iter", "discrete_dim"} <= set(ck.keys())
        assert ck["discrete_dim"] == [3] and ck["num_iter"] == 4
        m2 = aoi.models.load_model(fname + ".tar")
        assert type(m2) is type(m) and m2.kdict_["num_iter"] == 4
        for a, b in zip(m.encode(X), m2.encode(X)):
            assert np.array_equal(a, b)
        n_cont = 2                                               # decode takes [content latents | one-hot of every head]
        z = np.concatenate([np.zeros((5, n_cont), np.float32), np.eye(3, dtype=np.float32)[[0, 1, 2, 0, 1]]], 1)
        assert m.decode(z).shape == (5, 8, 8)
        with pytest.raises(ValueError):
            m.fit(X, np.zeros(8, dtype=np.int64), training_cycles=1, batch_size=4, filename=fname)
        with pytest.raises(ValueError):
            m.forward_compute_elbo(torch.from_numpy(X[:4]).to(device), torch.zeros(4, dtype=torch.long).to(device))
        with pytest.raises(NotImplementedError):
            m.fit(X, training_cycles=1, batch_size=4, filename=fname, recording=True)
        with pytest.raises(NotImplementedError):
            m.reconstruct(X[:1])
    # a checkpoint written by the reference's jrVAE.fit
    g = golden("vae_joint.npz")
    ref = aoi.models.load_model(os.path.join(GOLD, "ref_jrvae_ckpt.tar"))
    assert type(ref) is aoi.models.jrVAE and ref.kdict_["num_iter"] == int(g["ckpt|num_iter"])
    assert ref.discrete_dim == [3] and ref.translation
    got = ref.encode(g["ckpt|x"], num_batches=2)
    assert len(got) == 3
    for a, k in zip(got, ("zmean", "zlogsd", "alphas")):
        np.testing.assert_allclose(a, g["ckpt|" + k], rtol=1e-4, atol=1e-6)
    # limits of csrc/joint.hip are refused at construction
    with pytest.raises(ValueError):
        aoi.models.jVAE((8, 8), discrete_dim=[2] * 17, numhidden_encoder=16, numhidden_decoder=16)
    with pytest.raises(ValueError):
        aoi.models.jrVAE((8, 8), discrete_dim=[4097], numhidden_encoder=16, numhidden_decoder=16)
    with pytest.raises(ValueError):
        aoi.models.jVAE((8, 8), discrete_dim=[3, 0], numhidden_encoder=16, numhidden_decoder=16)
    # the plain models are built exactly as before
    for dd in (None, []):
        enc, dec, meta = init_VAE_nets((8, 8), 2, 3, dd, 0, numhidden_encoder=16, numhidden_decoder=16)
        assert type(enc).__name__ == "fcEncoderNet" and type(dec).__name__ == "rDecoderNet"
        assert list(enc.state_dict()) == ["dense.0.weight", "dense.0.bias", "dense.2.weight", "dense.2.bias",
                                          "fc11.weight", "fc11.bias", "fc12.weight", "fc12.bias"]
        assert dec.coord_latent.fc_latent.in_features == 2 and meta["discrete_dim"] == dd
        assert list(meta) == ["model_type", "in_dim", "latent_dim", "coord", "conv_encoder", "numlayers_encoder",
                              "numlayers_decoder", "numhidden_encoder", "numhidden_decoder", "skip", "nb_classes",
                              "discrete_dim", "sigmoid_out", "softplus_out"]
    v = aoi.models.VAE((8, 8), latent_dim=2, nb_classes=3, numhidden_encoder=16, numhidden_decoder=16)
    assert v.z_dim == 2 and v.decoder_net.decoder[0].in_features == 5 and len(v.encode(X)) == 2
    r = aoi.models.rVAE((8, 8), latent_dim=2, numhidden_encoder=16, numhidden_decoder=16)
    assert r.z_dim == 5 and r.metadict["discrete_dim"] is None and "conv_decoder" not in r.metadict
    # joint nets: the reference's module tree, the decoder fed [content | samples] and no class one-hot
    enc, dec, meta = init_VAE_nets((8, 8), 2, 3, [3, 4], 5, numhidden_encoder=16, numhidden_decoder=16)
    assert type(enc).__name__ == "jfcEncoderNet" and dec.coord_latent.fc_latent.in_features == 2 + 7
    assert [k for k in enc.state_dict() if k.startswith("fc13")] == ["fc13.0.weight", "fc13.0.bias", "fc13.1.weight",
                                                                     "fc13.1.bias"]
    assert meta["discrete_dim"] == [3, 4] and meta["nb_classes"] == 5
    enc, _, _ = init_VAE_nets((8, 8), 2, 0, [3], 0, conv_encoder=True, numhidden_encoder=4, numhidden_decoder=16)
    assert type(enc).__name__ == "jconvEncoderNet" and "conv.block.0.weight" in enc.state_dict()


def check_c_abi_limits(device):
    """The C entry points refuse segment tables beyond the limits stated in include/atomai_amd.h."""
    from atomai_amd import _joint as J, _lib as L
    a = torch.full((2, 4), 0.25).to(device)
    out = torch.empty_like(a)
    for sizes in ([1] * (J.MAX_HEADS + 1), [J.MAX_D + 1], [2, 0, 2], []):
        with pytest.raises(L.AmxError):
            L.call("amx_segsoftmax_fwd", L.ptr(a), J._segs(sizes) if sizes else None, len(sizes), 2, L.ptr(out),
                   L.stream_ptr(a))


# ---------------------------------------------------------------------------------------------- gpu tier only
def joint_oracle_elbo(enc, dec, x, eps, u, x_coord, sizes, tau, dx_prior=0.1, phi_prior=0.1,
                      cont_capacity=(5.0, 25000, 30), disc_capacity=(5.0, 25000, 30), num_iter=1):
    """jrVAE.forward_compute_elbo (translation on, fc encoder, 2 + 2 layers, 'mse'), training mode, with the noise
    injected, in stock torch ops of the dtype of its inputs (jrvae.py:105-152, vitrainer.py:237-248,
    vi_losses.py:60-74, 179-251)."""
    from oracle import vae_oracle as vo
    F = torch.nn.functional
    B = x.shape[0]
    h = x.reshape(B, -1)
    for i in range(2):
        h = torch.tanh(F.linear(h, enc[f"dense.{2 * i}.weight"], enc[f"dense.{2 * i}.bias"]))
    z_mean, z_logsd = F.linear(h, enc["fc11.weight"], enc["fc11.bias"]), F.linear(h, enc["fc12.weight"], enc["fc12.bias"])
    alphas = [torch.softmax(F.linear(h, enc[f"fc13.{j}.weight"], enc[f"fc13.{j}.bias"]), dim=1) for j in range(len(sizes))]
    z = z_mean + torch.exp(z_logsd) * eps
    coords = vo.transform_coordinates(x_coord.expand(B, *x_coord.shape), z[:, 0], (z[:, 1:3] * dx_prior).unsqueeze(1))
    ys, kl_disc, o = [], 0.0, 0
    for a, K in zip(alphas, sizes):
        gum = -torch.log(-torch.log(u[:, o:o + K] + 1e-12) + 1e-12)
        ys.append(torch.softmax((torch.log(a + 1e-12) + gum) / tau, dim=1))
        kl_disc = kl_disc + (a * (torch.log(a + 1e-12) - math.log(1.0 / K + 1e-12))).sum(1).mean()
        o += K
    x_rec = vo.r_decoder(dec, coords, torch.cat([z[:, 3:]] + ys, 1), tuple(x.shape[1:]), 2, False)
    kl_cont = vo.kld_normal(z_mean[:, 1:], z_logsd[:, 1:]).mean() + vo.kld_rot(phi_prior, z_logsd[:, 0]).mean()
    ccap = min(cont_capacity[0] * num_iter / float(cont_capacity[1]), cont_capacity[0])
    dcap = min(disc_capacity[0] * num_iter / float(disc_capacity[1]), disc_capacity[0], sum(math.log(K) for K in sizes))
    return (-vo.reconstruction("mse", x, x_rec).mean() - cont_capacity[2] * torch.abs(kl_cont - ccap)
            - disc_capacity[2] * torch.abs(dcap - kl_disc))


def check_full_shape_vs_oracle(B=128):
    """jrVAE 64 x 64, default 128-wide nets, discrete_dim=[10] at bs 128 on the DEFAULT (one-launch) path against the
    oracle graph on the same GPU in fp64 (= the reference) and in fp32 (= the floor): the recipe and bounds of
    test_rvae_config4_vs_oracle_on_device.  The noise of the default path is reproduced by drawing from the same seed in
    the same order."""
    import atomai_amd as aoi
    m = aoi.models.jrVAE((64, 64), latent_dim=2, discrete_dim=[10], seed=0)
    m.dx_prior, m.kdict_["phi_prior"] = 0.1, 0.1
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.rand(B, 64, 64).astype(np.float32)).cuda()
    assert m._default_sampling()
    m.encoder_net.train(), m.decoder_net.train()
    torch.manual_seed(7)
    elbo = m.forward_compute_elbo(x)
    (-elbo).backward()
    torch.manual_seed(7)
    eps = torch.empty(B, 5, device="cuda").normal_()
    u = torch.empty(B, 10, device="cuda").uniform_()

    def oracle(dtype):
        enc = OrderedDict((k, v.detach().to(dtype).requires_grad_(True)) for k, v in m.encoder_net.state_dict().items())
        dec = OrderedDict((k, v.detach().to(dtype).requires_grad_(True)) for k, v in m.decoder_net.state_dict().items())
        ref = joint_oracle_elbo(enc, dec, x.to(dtype), eps.to(dtype), u.to(dtype), m.x_coord.to(dtype), [10], 0.67)
        (-ref).backward()
        grads = {("enc", k): v.grad.double() for k, v in enc.items()}
        grads.update({("dec", k): v.grad.double() for k, v in dec.items()})
        return float(ref), grads
    e64, g64 = oracle(torch.float64)
    e32, g32 = oracle(torch.float32)
    torch.cuda.empty_cache()
    assert abs(elbo.item() - e64) / abs(e64) < 1e-5, (elbo.item(), e64, e32)
    gmax = max(float(g.abs().max()) for g in g64.values())
    report = []
    for which, net in (("enc", m.encoder_net), ("dec", m.decoder_net)):
        for k, p in net.named_parameters():
            ref = g64[(which, k)]
            err = float((p.grad.double() - ref).abs().max()) / gmax
            floor = float((g32[(which, k)] - ref).abs().max()) / gmax
            bound = max(0.1 * REL_TOL, 2 * floor)
            report.append((err / bound, f"{which}.{k}", err, floor))
            assert err < bound, (which, k, err, floor)
    worst = max(report)
    print(f"jrVAE 64x64 [10], bs {B}: ELBO rel. error {abs(elbo.item() - e64) / abs(e64):.2e} (oracle fp32: "
          f"{abs(e32 - e64) / abs(e64):.2e}); worst gradient error {worst[2]:.2e} of the global scale ({worst[1]}; "
          f"oracle-fp32 floor of that tensor {worst[3]:.2e}, largest floor {max(r[3] for r in report):.2e})")
