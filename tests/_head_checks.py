"""Shared bodies of the fused head-and-loss tests: amx_px_ce_train (CE / BCE), amx_px_dice_sums -> amx_dice_finalize ->
amx_px_dice_train (dice) and amx_px_bce_sum -> amx_focal_from_bce -> amx_px_focal_train (focal), csrc/head.hip and dice.hip,
called through the C ABI with the arguments engine.PxLossNode passes, against the same formulas in fp64 torch on the host.
The SAME checks run
  * on the CPU through the SIMT emulator build of the kernel sources (`not gpu` tier, test_head_emulated.py), and
  * on a real MI355X through libatomai_amd.so (`gpu` tier, test_head_gpu.py).
The geometries are the smallest that reach each branch of the kernels (G = Cs / 4 lanes share a pixel, PL = 256 / G pixel
lanes per workgroup): more than one column block of px_dice_sums_kernel with a partial last one, several image rows per
thread with a ragged DICE_U group and empty workgroups, every tail form of the PL * U pixel loop of px_ce_train_kernel,
G up to 64 (one wave per pixel, six xor-shuffle steps), padded channels, negative BatchNorm scales and no scales at all."""
import numpy as np
import pytest
import torch

from _loss_checks import UPSTREAM, dice_ref, focal_ref
from _seg_checks import REL_TOL

DICE_EPS, FOCAL = 1e-7, (0.5, 2)

# name -> (kind, Cs, C, K, (N, H, W), options)
CASES = {
    # G = 4, PL = 64: W = PL + 8 (a partial second column block); N H = 600 > 512 rows -> 2 image rows per workgroup,
    # workgroups 300 .. 511 of the sums kernel own no row
    "dice_g4_k3_3x200x72": ("dice", 16, 16, 3, (3, 200, 72), {}),
    "dice_g4_k3_3x200x72_no_scale": ("dice", 16, 16, 3, (3, 200, 72), {"affine": False}),
    # C < Cs; W = 2 PL + 8; a class absent from some columns (I_j = 0, C_j the sum of probabilities only)
    "dice_g4_c13_k4_2x300x136": ("dice", 16, 13, 4, (2, 300, 136), {"absent": True}),
    # G = 2, PL = 128: 3 image rows per workgroup, a ragged DICE_U group
    "dice_g2_c5_k2_1x1030x130": ("dice", 8, 5, 2, (1, 1030, 130), {}),
    "dice_g16_k3_1x520x24": ("dice", 64, 64, 3, (1, 520, 24), {}),          # PL = 16, W = PL + 8
    # G = 64: one wave per pixel, PL = 4; padded channels
    "dice_g64_c250_k2_1x37x9": ("dice", 256, 250, 2, (1, 37, 9), {}),
    "dice_g64_c250_k4_1x37x9": ("dice", 256, 250, 4, (1, 37, 9), {}),
    "ce_g64_c250_k2_1x37x9": ("ce", 256, 250, 2, (1, 37, 9), {}),
    "ce_g64_c250_k4_1x37x9": ("ce", 256, 250, 4, (1, 37, 9), {}),
    # one class; 3219 pixels: a multiple of neither PL nor 1024; 16 rows of PL pixels per workgroup of the sums kernel
    "dice_g4_k1_3x37x29": ("dice", 16, 16, 1, (3, 37, 29), {}),
    "focal_g4_k1_3x37x29": ("focal", 16, 16, 1, (3, 37, 29), {}),
    "bce_g4_k1_3x37x29": ("ce", 16, 16, 1, (3, 37, 29), {}),
    "ce_g4_k3_3x37x29": ("ce", 16, 16, 3, (3, 37, 29), {}),
    "bce_g8_k1_1x45x23": ("ce", 32, 32, 1, (1, 45, 23), {}),                # a single workgroup
    # fewer pixels (15) than pixel lanes (PL = 256)
    "ce_g1_c3_k2_1x5x3": ("ce", 4, 3, 2, (1, 5, 3), {}),
    "dice_g1_c3_k2_1x5x3": ("dice", 4, 3, 2, (1, 5, 3), {}),
}


def _nan(device, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=device)


class Head:
    """Inputs of one fused head call, drawn as the issue of this suite prescribes: the last activation a [npix][Cs] (NHWC,
    random normal in the channels < C, zeros in the padding), BatchNorm scale / shift [Cs] with some NEGATIVE scales (or
    none), px weights [K][C] and bias [K], and an int64 class map (N,H,W) (K >= 2) or a float mask (N,1,H,W) (K == 1; for
    dice with the values 0, 1 and 1.5 — the latter truncates to 1 as .long() does)."""

    def __init__(self, device, kind, Cs, C, K, nhw, affine=True, absent=False, seed=0):
        from atomai_amd import _lib as L
        N, H, W = nhw
        rs = np.random.RandomState(seed)
        npix = N * H * W
        a = np.zeros((npix, Cs), np.float32)
        a[:, :C] = rs.randn(npix, C)
        scale = (0.5 + rs.rand(Cs)) * np.where(rs.rand(Cs) < 0.4, -1.0, 1.0)
        scale[0] = -abs(scale[0])
        shift = 0.3 * rs.randn(Cs)
        w = 1.5 * rs.randn(K, C) / np.sqrt(C)
        b = 0.2 * rs.randn(K)
        if K == 1:
            y = (rs.rand(N, 1, H, W) < 0.4).astype(np.float32)
            if kind == "dice":
                y[rs.rand(N, 1, H, W) < 0.1] = 1.5
        else:
            y = rs.randint(0, K, (N, H, W))
            if absent:                                           # class K - 1 never occurs in columns 3 .. W / 2
                sub = y[:, :, 3:W // 2]
                sub[sub == K - 1] = 0
        f32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(device)
        self.device, self.kind, self.Cs, self.C, self.K, self.N, self.H, self.W = device, kind, Cs, C, K, N, H, W
        self.npix, self.affine = npix, affine
        self.a, self.w, self.b = f32(a), f32(w), f32(b)
        self.scale, self.shift = (f32(scale), f32(shift)) if affine else (None, None)
        self.target = f32(y) if K == 1 else torch.from_numpy(y).to(device)
        lib = L.load()
        self.rows, self.rows_pix = lib.amx_rows_for(npix), lib.amx_rows_pix(npix)
        self.drows = lib.amx_dice_rows(N, H, W, K)
        self.B = lib.amx_dice_bins(K, W)

    def buffers(self, drows=None):
        """Every output buffer of the family, pre-filled with NaN."""
        d, K, Cs = self.device, self.K, self.Cs
        return {"dxn": _nan(d, self.npix, Cs), "part": _nan(d, self.rows, K, Cs), "partb": _nan(d, self.rows, K),
                "bstats": _nan(d, self.rows, 2, Cs), "lpart": _nan(d, self.rows),
                "dpart": _nan(d, drows or self.drows, 2 * self.B), "bpart": _nan(d, drows or self.drows, 4)}

    def args(self, fn, o, table=None, dfdc=None, **over):
        """The argument tuple of entry point `fn` as engine.PxLossNode forms it; `over` replaces single arguments."""
        from atomai_amd import _lib as L
        g = {"Cs": self.Cs, "C": self.C, "K": self.K, "rows": self.rows, "rows_pix": self.rows_pix, "drows": self.drows,
             "shift": self.shift}
        g.update(over)
        head = (L.ptr(self.a), L.ptr(self.scale), L.ptr(g["shift"]), L.ptr(self.w), L.ptr(self.b))
        ti, tf = L.ptr(self.target if self.K > 1 else None), L.ptr(self.target if self.K == 1 else None)
        geom = (self.N, self.H, self.W, g["C"], g["Cs"])
        grads = (L.ptr(o["dxn"]), L.ptr(o["part"]), L.ptr(o["partb"]), L.ptr(o["bstats"]))
        sp = L.stream_ptr(self.a)
        if fn == "amx_px_ce_train":
            return (*head, ti, tf, *grads, L.ptr(o["lpart"]), *geom, g["K"], g["rows"], g["rows_pix"], sp)
        if fn == "amx_px_dice_sums":
            return (*head, ti, tf, L.ptr(o["dpart"]), g["drows"], *geom, g["K"], sp)
        if fn == "amx_px_dice_train":
            return (*head, ti, tf, L.ptr(table), *grads, *geom, g["K"], g["rows"], g["rows_pix"], sp)
        if fn == "amx_px_bce_sum":
            return (*head, tf, L.ptr(o["bpart"]), g["drows"], *geom, sp)
        if fn == "amx_px_focal_train":
            return (*head, tf, L.ptr(dfdc), *grads, L.ptr(o["lpart"]), *geom, g["rows"], g["rows_pix"], sp)
        raise KeyError(fn)

    def run(self):
        """The launches of engine.PxLossNode.__init__ -> {name: host tensor} of everything the kernels wrote."""
        from atomai_amd import _lib as L
        from atomai_amd.losses_metrics import losses
        o = self.buffers()
        sp = L.stream_ptr(self.a)
        if self.kind == "dice":
            B, drows, nch = losses.dice_launch_plan(self.N, self.K, self.H, self.W)
            assert (B, drows) == (self.B, self.drows)
            L.call("amx_px_dice_sums", *self.args("amx_px_dice_sums", o))
            o["table"], o["loss"] = losses.dice_table_and_loss(o["dpart"], B, drows, nch, DICE_EPS, sp)
            L.call("amx_px_dice_train", *self.args("amx_px_dice_train", o, table=o["table"]))
            del o["lpart"], o["bpart"]
        elif self.kind == "focal":
            L.call("amx_px_bce_sum", *self.args("amx_px_bce_sum", o))
            c = _nan(self.device, 1)
            L.call("amx_reduce_rows", L.ptr(o["bpart"]), self.drows, 4, 1, 1.0 / self.npix, L.ptr(c), sp)
            o["loss"], dfdc = losses.focal_scalars(c, *FOCAL)
            L.call("amx_px_focal_train", *self.args("amx_px_focal_train", o, dfdc=dfdc))
            del o["dpart"]
        else:
            L.call("amx_px_ce_train", *self.args("amx_px_ce_train", o))
            o["loss"] = _nan(self.device)
            L.call("amx_reduce_rows", L.ptr(o["lpart"]), self.rows, 1, 1, 1.0 / self.npix, L.ptr(o["loss"]), sp)
            del o["dpart"], o["bpart"]
        return {k: v.detach().cpu() for k, v in o.items()}

    def reference(self, dtype):
        """The same operation in `dtype` torch on the host: xn = a scale + shift, logits = xn W^T + b, the loss, and from
        g = d loss / d logits: dxn = g W, dW = g^T xn, db = sum g, bstats = (sum dxn, sum dxn a_raw); plus the partial sums
        the kernels expose (loss terms per workgroup of rows_pix pixels, the dice bin sums, the BCE total)."""
        C, K, N, H, W = self.C, self.K, self.N, self.H, self.W
        a = self.a.cpu()[:, :C].to(dtype)
        xn = a * self.scale.cpu()[:C].to(dtype) + self.shift.cpu()[:C].to(dtype) if self.affine else a
        w, b = self.w.cpu().to(dtype), self.b.cpu().to(dtype)
        logits = (xn @ w.t() + b).reshape(N, H, W, K).permute(0, 3, 1, 2).contiguous()
        y = self.target.cpu()
        r = {}
        terms = None
        if self.kind == "dice":
            r["loss"], g = dice_ref(logits, y, dtype, DICE_EPS)
            if K == 1:
                yl = y.squeeze(1).long()
                onehot = torch.stack([(yl == 1), (yl == 0)], 1).to(dtype)
                s = torch.sigmoid(logits)
                probas, dims = torch.cat([s, 1 - s], 1), (0, 2, 3)
            else:
                onehot = torch.nn.functional.one_hot(y, K).permute(0, 3, 1, 2).to(dtype)
                probas, dims = torch.softmax(logits, 1), (0, 2)
            r["dice_I"] = (probas * onehot).sum(dims).reshape(-1)            # bin (k, w) at k W + w, as the table
            r["dice_C"] = (probas + onehot).sum(dims).reshape(-1)
        elif self.kind == "focal":
            r["loss"], g = focal_ref(logits, y, dtype, *FOCAL)
            terms = torch.nn.functional.binary_cross_entropy_with_logits(logits, y.to(dtype), reduction="none")
            r["bce_total"] = terms.sum().reshape(1)
        else:
            x = logits.clone().requires_grad_(True)
            if K == 1:
                terms = torch.nn.functional.binary_cross_entropy_with_logits(x, y.to(dtype), reduction="none")
            else:
                terms = torch.nn.functional.cross_entropy(x, y, reduction="none")
            loss = terms.mean()
            loss.backward()
            r["loss"], g, terms = float(loss.detach()), x.grad, terms.detach()
        if terms is not None:                                    # pixel p = (n H + h) W + w belongs to workgroup p / rows_pix
            t = torch.zeros(self.rows * self.rows_pix, dtype=dtype)
            t[:self.npix] = terms.reshape(-1)
            r["lpart"] = t.reshape(self.rows, self.rows_pix).sum(1)
        gf = g.permute(0, 2, 3, 1).reshape(self.npix, K)
        r["dxn"] = gf @ w
        r["dW"] = gf.t() @ xn
        r["db"] = gf.sum(0)
        r["bstats"] = torch.stack([r["dxn"].sum(0), (r["dxn"] * a).sum(0)])
        return r


def _compare(tag, what, got, ref64, ref32):
    """The project's gradient rule (_loss_checks.check_loss_level): the error against fp64, normalised by the largest fp64
    entry of the tensor, within max(4 x the error of the fp32 evaluation of the same reference, 2e-5)."""
    norm = float(ref64.abs().max())
    assert norm > 0, (tag, what)
    err = float((got.double() - ref64).abs().max()) / norm
    floor = float((ref32.double() - ref64).abs().max()) / norm
    print(f"head {tag} {what}: error {err:.2e} (torch-fp32 floor {floor:.2e}, err/floor {err / max(floor, 1e-30):.2f})")
    assert err <= max(4 * floor, 2e-5), (tag, what, err, floor)


def check_case(name, device):
    kind, Cs, C, K, nhw, opt = CASES[name]
    h = Head(device, kind, Cs, C, K, nhw, **opt)
    o = h.run()
    for k, v in o.items():                                       # nothing is left unwritten
        assert bool(torch.isfinite(v).all()), (name, k, int((~torch.isfinite(v)).sum()))
    assert not bool(o["dxn"][:, C:].any()), name                 # the padding of dxn is exactly 0
    r64, r32 = h.reference(torch.float64), h.reference(torch.float32)
    lerr = abs(float(o["loss"]) - r64["loss"]) / abs(r64["loss"])
    print(f"head {name} loss: {float(o['loss']):.8f} (fp64 {r64['loss']:.8f}, rel {lerr:.2e})")
    assert lerr < REL_TOL, (name, float(o["loss"]), r64["loss"])
    got = {"dxn": o["dxn"][:, :C], "dW": o["part"].double().sum(0)[:, :C], "db": o["partb"].double().sum(0),
           "bstats": o["bstats"].double().sum(0)[:, :C]}
    if "lpart" in o:
        got["lpart"] = o["lpart"]
    if "dpart" in o:
        sums = o["dpart"].double().sum(0)
        got["dice_I"], got["dice_C"] = sums[:h.B], sums[h.B:]
        if opt.get("absent"):
            W = nhw[2]
            assert not bool(got["dice_I"].reshape(K, W)[K - 1, 3:W // 2].any())     # no pixel of the class: exactly 0
    if "bpart" in o:
        got["bce_total"] = o["bpart"][:, 0].double().sum().reshape(1)
        assert not bool(o["bpart"][:, 1:].any())
    for what, v in got.items():
        _compare(name, what, v, r64[what], r32[what])
    again = h.run()                                              # no floating-point atomics: bit-identical when repeated
    for k, v in o.items():
        assert torch.equal(v.view(torch.int32), again[k].view(torch.int32)), (name, k)


# ---------------------------------------------------------------- argument checks: refused before anything is launched
REFUSALS = [(fn, why) for fn, whys in (
    ("amx_px_ce_train", ("Cs12", "K5", "rows", "shift")),
    ("amx_px_dice_sums", ("Cs12", "K5", "drows", "shift")),
    ("amx_px_dice_train", ("Cs12", "K5", "rows", "shift")),
    ("amx_px_bce_sum", ("Cs12", "drows", "shift")),
    ("amx_px_focal_train", ("Cs12", "rows", "shift"))) for why in whys]


def check_refusal(fn, why, device):
    """Cs = 12 (G = 3, no power of two), K = 5, rows x rows_pix < npix, dice rows other than amx_dice_rows, scale without
    shift: AmxError, and every (valid, NaN-filled) output buffer is untouched."""
    from atomai_amd import _lib as L
    K = 1 if fn in ("amx_px_bce_sum", "amx_px_focal_train") else 3
    h = Head(device, "dice", 16, 10, K, (2, 30, 40))
    over = {"Cs12": {"Cs": 12}, "K5": {"K": 5}, "rows": {"rows_pix": (h.npix - 1) // h.rows},
            "drows": {"drows": h.drows + 1}, "shift": {"shift": None}}[why]
    o = h.buffers(drows=h.drows + 1)
    table, dfdc = torch.zeros(h.B, 2, device=device), torch.ones(1, device=device)
    L.call(fn, *h.args(fn, h.buffers(drows=h.drows + 1), table=table, dfdc=dfdc))      # the unmodified call is accepted
    with pytest.raises(L.AmxError):
        L.call(fn, *h.args(fn, o, table=table, dfdc=dfdc, **over))
    for k, v in o.items():
        assert bool(torch.isnan(v).all()), (fn, why, k)


# ---------------------------------------------------------------- amx_scale_unless_one_multi
def check_scale_unless_one_multi(device):
    """Four buffers of unequal lengths (together more than one grid of 4096 x 256 threads), and three with the fourth
    NULL / 0: an upstream scalar of 1 leaves every bit as it was, 0.37 gives fl(x * 0.37f) in every element."""
    from atomai_amd import _lib as L
    rs = np.random.RandomState(2)
    lens = (4096 * 256 + 1000, 37, 3, 513)
    for nbuf in (4, 3):
        for up in UPSTREAM:
            src = [torch.from_numpy(rs.randn(n).astype(np.float32)) for n in lens[:nbuf]]
            x = [t.clone().to(device) for t in src] + [None] * (4 - nbuf)
            g = torch.tensor([up], dtype=torch.float32, device=device)
            segs = [v for t in x for v in (L.ptr(t), t.numel() if t is not None else 0)]
            L.call("amx_scale_unless_one_multi", *segs, L.ptr(g), L.stream_ptr(g))
            for t, s in zip(x, src):
                want = s if up == 1.0 else s * torch.tensor(up, dtype=torch.float32)
                assert torch.equal(t.cpu().view(torch.int32), want.view(torch.int32)), (nbuf, up, t.numel())


# ---------------------------------------------------------------- the engine's own plumbing beyond one tile
def check_net_beyond_one_tile(device, kind, model=("Unet", 3, 16), shape=(2, 1, 264, 72)):
    """_seg_checks.check_fused_head_and_loss ('ce') / _loss_checks.check_fused_vs_modular ('dice') with their assertions, on
    the default 16 filters (G = 4, PL = 64) and an input with W = 72 > PL and N H = 528 > 512 image rows: engine.PxLossNode
    itself through more than one column block and more than one image row per thread."""
    from atomai_amd.losses_metrics.losses import select_loss
    from atomai_amd.nets import init_fcnn_model
    rs = np.random.RandomState(7)
    name, ncls, nf = model
    N, _, H, W = shape
    crit = select_loss("ce", ncls) if kind == "ce" else select_loss(kind)
    for gscale in UPSTREAM:
        torch.manual_seed(5)
        net, _ = init_fcnn_model(name, ncls, nb_filters=nf)
        net.to(device).train()
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 0.0                                 # (two forwards over the same batch)
        x = torch.from_numpy(rs.rand(*shape).astype(np.float32)).to(device).requires_grad_(True)
        y = torch.from_numpy(rs.randint(0, ncls, (N, H, W))).to(device)
        loss0 = crit(net(x), y)
        (loss0 * gscale).backward()
        loss0 = loss0.detach()
        ref = [p.grad.clone() for p in net.parameters()] + [x.grad.clone()]
        net.zero_grad()
        x.grad = None
        k, loss1 = net.forward_loss(x, y) if kind == "ce" else net.forward_loss(x, y, criterion=crit)
        assert k == "loss", k                                    # the fused node ran
        (loss1 * gscale).backward()
        loss1 = loss1.detach()
        got = [p.grad for p in net.parameters()] + [x.grad]
        gmax = max(float(t.abs().max()) for t in ref)
        worst = max(float((a - b).abs().max()) for a, b in zip(got, ref)) / gmax
        print(f"{kind} {name} K={ncls} nf={nf} {shape} upstream {gscale}: loss {float(loss1):.8f} vs modular "
              f"{float(loss0):.8f}; worst gradient difference {worst:.2e} of gmax")
        assert abs(float(loss0) - float(loss1)) < 2e-6 * max(1.0, abs(float(loss0))), (float(loss0), float(loss1))
        for (pname, _), a, b in zip(list(net.named_parameters()) + [("input", None)], got, ref):
            assert float((a - b).abs().max()) < 2e-5 * gmax, (pname, float((a - b).abs().max()), gmax)
