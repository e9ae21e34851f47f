"""Generates the joint-VAE (jVAE / jrVAE) fixtures under tests/golden/ from the REAL reference (imported through
oracle/ref_harness.py, dev container only):

    python tools/make_golden_joint.py [kernels] [models]

  joint_kernels.npz    kernel level: logits, uniform noise u, tau and upstream gradients; the reference's softmax heads,
                       ``viBaseTrainer.reparameterize_discrete`` and ``kld_discrete`` with their autograd gradients
  vae_joint.npz        model level, one entry per case of CASES: x, injected eps (3, B, Z) and u (3, B, D), first-step
                       gradients, three Adam-step ELBOs, final z_mean / alphas; plus the encode() output of the checkpoint
  ref_jrvae_ckpt.tar   a checkpoint written by the reference's jrVAE.fit (8 x 8 patches, 16-wide nets, discrete_dim=[3])
Everything is computed in fp32 and with the same modules ``.double()``'d, so each golden carries its own fp32 noise
floor.  To keep the file small the model-level goldens hold, per parameter tensor, the fp64 gradient ROUNDED to fp32
(6e-8 relative, far below the 1e-4 the tests ask for), the floor max|g32 - g64| / max|g64| as a number, and the SHA-256
of the initial tensor's bytes instead of the tensor (bit-equality is what the tests check).
TEST INFRASTRUCTURE ONLY.
"""
import contextlib
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


@contextlib.contextmanager
def injected_uniform(u: torch.Tensor):
    """Inside, ``Tensor.uniform_()`` fills with ``u`` instead of drawing: the only way to feed known noise to the
    reference's ``reparameterize_discrete``, which draws its own."""
    orig = torch.Tensor.uniform_

    def fill(self, *a, **k):
        assert self.shape == u.shape
        return self.copy_(u.to(self.dtype))
    torch.Tensor.uniform_ = fill
    try:
        yield
    finally:
        torch.Tensor.uniform_ = orig


# ---------------------------------------------------------------------------------------------- kernel level
SEG_TABLES = [[1], [2], [3, 5], [10], [64], [65], [7, 1, 130]]
TAUS = [0.67, 0.1]
# extra: one head whose logits span +-40 (issue), and one spanning +-60, where exp(-120) IS 0 in fp32 so the +1e-12 guards
# see an exact zero
EXTRA = [("span40", [6], 40.0), ("span60", [6], 60.0)]


def kernel_case_name(sizes, tau, tag=None):
    return (tag or "t" + "_".join(str(k) for k in sizes)) + f"|tau{tau}"


def make_kernels(aoi):
    from atomai.losses_metrics.vi_losses import kld_discrete
    from atomai.trainers import viBaseTrainer
    B = 3
    out, names = {}, []
    rs = np.random.RandomState(11)
    todo = [(None, s, None) for s in SEG_TABLES] + EXTRA
    for tag, sizes, span in todo:
        for tau in TAUS:
            name = kernel_case_name(sizes, tau, tag)
            names.append(name)
            D = sum(sizes)
            logits = (2.0 * rs.randn(B, D)).astype(np.float32)
            if span is not None:
                logits = np.stack([rs.permutation(np.linspace(-span, span, D)) for _ in range(B)]).astype(np.float32)
            u = rs.rand(B, D).astype(np.float32)
            dy = rs.randn(B, D).astype(np.float32)
            ckl = rs.randn(len(sizes)).astype(np.float32)          # upstream gradient of every head's kld_discrete
            out[name + "|sizes"] = np.array(sizes)
            out[name + "|tau"] = np.array(tau)
            out[name + "|logits"], out[name + "|u"], out[name + "|dy"], out[name + "|ckl"] = logits, u, dy, ckl
            offs = np.concatenate([[0], np.cumsum(sizes)])
            for dt, t in ((torch.float32, "f32"), (torch.float64, "f64")):
                lg = torch.from_numpy(logits).to(dt).requires_grad_(True)
                alphas = [torch.softmax(lg[:, offs[h]:offs[h + 1]], dim=1) for h in range(len(sizes))]
                for a in alphas:
                    a.retain_grad()
                ys = []
                for h, a in enumerate(alphas):
                    with injected_uniform(torch.from_numpy(u[:, offs[h]:offs[h + 1]])):
                        ys.append(viBaseTrainer.reparameterize_discrete(a, tau))
                y = torch.cat(ys, 1)
                kls = torch.cat([kld_discrete(a) for a in alphas])
                out[f"{name}|alpha|{t}"] = torch.cat(alphas, 1).detach().numpy()
                out[f"{name}|y|{t}"] = y.detach().numpy()
                out[f"{name}|kl|{t}"] = kls.detach().numpy()
                (y * torch.from_numpy(dy).to(dt)).sum().backward(retain_graph=True)
                out[f"{name}|dalpha_sample|{t}"] = torch.cat([a.grad for a in alphas], 1).numpy().copy()
                out[f"{name}|dlogits_sample|{t}"] = lg.grad.numpy().copy()
                lg.grad = None
                for a in alphas:
                    a.grad = None
                (kls * torch.from_numpy(ckl).to(dt)).sum().backward()
                out[f"{name}|dalpha_kl|{t}"] = torch.cat([a.grad for a in alphas], 1).numpy().copy()
                out[f"{name}|dlogits_kl|{t}"] = lg.grad.numpy().copy()
            print(name, "kl f32", out[name + "|kl|f32"], "f64", out[name + "|kl|f64"],
                  "min alpha f32", out[name + "|alpha|f32"].min())
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(GOLD, "joint_kernels.npz"), **out)


# ---------------------------------------------------------------------------------------------- model level
W = dict(numhidden_encoder=32, numhidden_decoder=32)
CASES = {
    "jvae16": dict(cls="jVAE", in_dim=(16, 16), ctor=dict(discrete_dim=[10], **W), fit=dict()),
    "jrvae16": dict(cls="jrVAE", in_dim=(16, 16), ctor=dict(discrete_dim=[3, 5], **W), fit=dict()),
    "jrvae16_nt_skip": dict(cls="jrVAE", in_dim=(16, 16), ctor=dict(discrete_dim=[2], translation=False, skip=True, **W),
                            fit=dict()),
    "jvae16_conv": dict(cls="jVAE", in_dim=(16, 16), ctor=dict(conv_encoder=True, numhidden_encoder=8,
                                                               numhidden_decoder=32), fit=dict()),
    "jrvae12_rgb_ce": dict(cls="jrVAE", in_dim=(12, 12, 3), ctor=dict(**W), fit=dict(), loss="ce"),
    "jvae16_cap": dict(cls="jVAE", in_dim=(16, 16), ctor=dict(**W),
                       fit=dict(cont_capacity=[5.0, 100, 2.0], disc_capacity=[1.0, 50, 3.0], temperature=0.4)),
}
B_MODEL, STEPS = 6, 3


def digest(a: np.ndarray) -> np.ndarray:
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def _model_run(aoi, name, c, seed):
    """One case with data seed ``seed`` -> (dict of arrays, list of (|KL - C|, |KL32 - KL64|) per step and channel)."""
    import atomai.losses_metrics.vi_losses as vl
    out = {}
    rs = np.random.RandomState(seed)
    in_dim = c["in_dim"]
    x = rs.rand(B_MODEL, *in_dim).astype(np.float32)
    probe = getattr(aoi.models, c["cls"])(in_dim, latent_dim=2, seed=0, **c["ctor"])
    sizes = list(probe.discrete_dim)
    Z = probe.z_dim - sum(sizes)
    eps_all = rs.randn(STEPS, B_MODEL, Z).astype(np.float32)
    u_all = rs.rand(STEPS, B_MODEL, sum(sizes)).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    out["x"], out["eps"], out["u"], out["sizes"] = x, eps_all, u_all, np.array(sizes)
    record = {}
    orig_cap = vl.infocapacity
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        m = getattr(aoi.models, c["cls"])(in_dim, latent_dim=2, seed=0, **c["ctor"])
        if tag == "f32":
            for which, net in (("enc", m.encoder_net), ("dec", m.decoder_net)):
                for k, v in net.state_dict().items():
                    out[f"{which}|{k}|sha256"] = digest(v.numpy())
        m.encoder_net.to(dt), m.decoder_net.to(dt)
        if hasattr(m, "x_coord"):
            m.x_coord = m.x_coord.to(dt)
        if hasattr(m, "translation"):                          # what jrVAE.fit sets before the loop (jrvae.py:203-204)
            m.dx_prior = 0.1
            m.kdict_["phi_prior"] = 0.1
        for k, v in c["fit"].items():
            m.kdict_[k] = v
        m.loss = c.get("loss", "mse")
        m.compile_trainer((x, None), None, batch_size=B_MODEL)
        state = {"i": 0, "h": 0}

        def reparam(z_mean, z_sd, st=state, d=dt):
            return z_mean + z_sd * torch.from_numpy(eps_all[st["i"]]).to(d)

        def reparam_disc(alpha, tau, st=state, mm=m):
            h = st["h"]
            st["h"] = (h + 1) % len(sizes)
            with injected_uniform(torch.from_numpy(u_all[st["i"]][:, offs[h]:offs[h + 1]])):
                return type(mm).reparameterize_discrete(alpha, tau)
        m.reparameterize, m.reparameterize_discrete = reparam, reparam_disc
        kls = []

        def cap_probe(kl_cont, cont_capacity, kl_disc=None, disc_capacity=None, disc_dims=None, num_iter=0):
            cc = min(cont_capacity[0] * num_iter / float(cont_capacity[1]), cont_capacity[0])
            dc = min(disc_capacity[0] * num_iter / float(disc_capacity[1]), disc_capacity[0],
                     sum(float(np.log(d)) for d in disc_dims))
            kls.append((float(kl_cont), cc, float(kl_disc), dc))
            return orig_cap(kl_cont, cont_capacity, kl_disc, disc_capacity, disc_dims, num_iter)
        vl.infocapacity = cap_probe
        try:
            xt = torch.from_numpy(x).to(dt)
            elbos = []
            for s in range(STEPS):
                state["i"], state["h"] = s, 0
                m.encoder_net.train(), m.decoder_net.train()
                m.optim.zero_grad()
                elbo = m.forward_compute_elbo(xt)
                (-elbo).backward()
                if s == 0:
                    for which, net in (("enc", m.encoder_net), ("dec", m.decoder_net)):
                        for k, p in net.named_parameters():
                            record[(which, k, tag)] = p.grad.numpy().astype(np.float64).copy()
                m.optim.step()
                elbos.append(elbo.item())
        finally:
            vl.infocapacity = orig_cap
        record[("kls", tag)] = kls
        out[f"elbo|{tag}"] = np.array(elbos)
        with torch.no_grad():
            lat = m.encoder_net(xt)
        out[f"zmean|{tag}"], out[f"zlogsd|{tag}"] = lat[0].numpy(), lat[1].numpy()
        out[f"alphas|{tag}"] = torch.cat(lat[2:], 1).numpy()
    for (which, k, tag) in [key for key in record if len(key) == 3 and key[2] == "f64"]:
        g64, g32 = record[(which, k, "f64")], record[(which, k, "f32")]
        out[f"g{which}|{k}|f64"] = g64.astype(np.float32)
        out[f"g{which}|{k}|floor"] = np.array(np.abs(g32 - g64).max() / max(np.abs(g64).max(), 1e-300))
    margins = []
    for (kc32, cc, kd32, dcap), (kc64, _, kd64, _) in zip(record[("kls", "f32")], record[("kls", "f64")]):
        margins += [(abs(kc64 - cc), abs(kc32 - kc64)), (abs(kd64 - dcap), abs(kd32 - kd64))]
    out["kl_cont|f64"] = np.array([k[0] for k in record[("kls", "f64")]])
    out["kl_disc|f64"] = np.array([k[2] for k in record[("kls", "f64")]])
    return out, margins


def make_ckpt(aoi, out):
    """A checkpoint written by the reference's own jrVAE.fit, and its encode() output on 4 patches."""
    rs = np.random.RandomState(21)
    X = rs.rand(8, 8, 8).astype(np.float32)
    tmp = tempfile.mkdtemp()
    m = aoi.models.jrVAE((8, 8), latent_dim=2, discrete_dim=[3], seed=0, numhidden_encoder=16, numhidden_decoder=16)
    m.fit(X, training_cycles=2, batch_size=4, filename=os.path.join(tmp, "ref_jrvae_ckpt"))
    shutil.copy(os.path.join(tmp, "ref_jrvae_ckpt.tar"), os.path.join(GOLD, "ref_jrvae_ckpt.tar"))
    xq = rs.rand(4, 8, 8).astype(np.float32)
    zm, zs, al = m.encode(xq, num_batches=2)
    out["ckpt|x"], out["ckpt|zmean"], out["ckpt|zlogsd"], out["ckpt|alphas"] = xq, zm, zs, al
    out["ckpt|num_iter"] = np.array(m.kdict_["num_iter"])
    print("checkpoint", os.path.getsize(os.path.join(GOLD, "ref_jrvae_ckpt.tar")), "bytes; num_iter", m.kdict_["num_iter"])


def make_models(aoi):
    out = {"cases": np.array(list(CASES))}
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())
    try:
        for i, (name, c) in enumerate(CASES.items()):
            seed = 100 + 10 * i
            while True:
                arrays, margins = _model_run(aoi, name, c, seed)
                # |KL - C| has a kink at KL = C: keep every recorded step at least 100 fp32-noise widths away from it
                if all(gap >= 100 * noise for gap, noise in margins):
                    break
                print(name, "data seed", seed, "too close to the kink of |KL - C|:", margins)
                seed += 1
            arrays["seed"] = np.array(seed)
            out.update({f"{name}|{k}": v for k, v in arrays.items()})
            print(name, "seed", seed, "elbo f32", arrays["elbo|f32"], "f64", arrays["elbo|f64"],
                  "min gap/noise", min(g / max(n, 1e-300) for g, n in margins))
        make_ckpt(aoi, out)
    finally:
        os.chdir(cwd)
    np.savez_compressed(os.path.join(GOLD, "vae_joint.npz"), **out)
    print("vae_joint.npz", os.path.getsize(os.path.join(GOLD, "vae_joint.npz")), "bytes")


if __name__ == "__main__":
    aoi = ref_harness.import_reference()
    for w in sys.argv[1:] or ["kernels", "models"]:
        {"kernels": make_kernels, "models": make_models}[w](aoi)
