"""Shared bodies of the ImSpec (im2spec / spec2im) tests.  The SAME checks run
  * on the CPU through the SIMT emulator build of the kernel sources (`not gpu` tier), and
  * on a real MI355X through libatomai_amd.so (`gpu` tier),
against golden vectors written by the reference (tests/golden/imspec_*.npz, tools/make_imspec_golden.py) and against
float64 torch on the CPU."""
import os
import warnings

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_TOL = 1e-4          # north_star: "within 1e-4 rel fp32"
SLOPE = 0.1             # lrelu_a of every ImSpec block (atomai/nets/ed.py:61-63, 125-138)

# name -> (in_dim, out_dim, kwargs of SignalED); seed 1, B = 4, latent_dim = 3, filters 5 / 6, layers 2 / 3
CASES = {
    "imspec_i2s": ((8, 8), (16,), dict()),
    "imspec_s2i": ((16,), (8, 8), dict()),
    "imspec_i2s_updown": ((8, 8), (16,), dict(encoder_downsampling=2, decoder_upsampling=True)),
    "imspec_s2i_nobn": ((12,), (8, 8), dict(encoder_downsampling=2, decoder_upsampling=True, batch_norm=False)),
}
NET_KW = dict(nblayers_encoder=2, nblayers_decoder=3, nbfilters_encoder=5, nbfilters_decoder=6)
LATENT = 3

# (N, L, Cin, Cout, k, dil): see the docstring of check_conv1d_kernels
KERNEL_SHAPES = [
    (2, 16, 1, 5, 3, 1),
    (3, 37, 6, 6, 3, 3),
    (2, 16, 6, 1, 3, 1),
    (2, 200, 20, 33, 3, 4),
    (5, 13, 4, 4, 3, 2),
    (2, 3, 4, 4, 3, 4),
    (2, 16, 1, 1, 1, 1),
    (2, 40, 8, 8, 3, 9),
    (3, 700, 4, 8, 3, 2),          # N * L = 2100: three statistics rows (the last one partial), nine weight-gradient rows
    (1, 500, 8, 8, 3, 400),
]


def relmax(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def r4(c):
    return (c + 3) // 4 * 4


def r16(c):
    return (c + 15) // 16 * 16


def _lib():
    from atomai_amd import _lib as L
    return L


def _nlc(x_ncl, device):
    """(N, C, L) float64/32 CPU tensor -> channels-last [N][L][Cs] fp32 on `device`, padding channels zero."""
    N, C, Ln = x_ncl.shape
    t = torch.zeros((N, Ln, r4(C)), dtype=torch.float32)
    t[..., :C] = x_ncl.permute(0, 2, 1).float()
    return t.to(device).contiguous()


def _pad(v, n, device):
    out = torch.zeros(n, dtype=torch.float32)
    out[: v.numel()] = v.float()
    return out.to(device)


def _pack1d(w, cin, mode, device):
    L = _lib()
    cout, _, taps = w.shape
    wd = w.float().to(device).contiguous()
    n = L.load().amx_pack_weights1d_size(cout, r4(cin), taps)
    dst = torch.empty(n, dtype=torch.float32, device=device)
    L.call("amx_pack_weights1d", L.ptr(wd), L.ptr(dst), cout, cin, r4(cin), taps, mode, L.stream_ptr(dst))
    return dst


def conv1d_problem(N, Ln, cin, cout, k, dil, seed=0):
    """Random raw input with a pending affine of NON-ZERO shift, weights, bias, upstream gradient; and the float64
    reference: y = lrelu(conv1d(scale * x + shift)), its BatchNorm batch statistics and autograd's three gradients."""
    gen = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(N, cin, Ln, generator=gen, dtype=torch.float64).float().double()
    scale = (0.5 + torch.rand(cin, generator=gen, dtype=torch.float64)).float().double()
    shift = (0.3 + torch.rand(cin, generator=gen, dtype=torch.float64)).float().double()
    w = (torch.randn(cout, cin, k, generator=gen, dtype=torch.float64) / (cin * k) ** 0.5).float().double()
    b = torch.randn(cout, generator=gen, dtype=torch.float64).float().double()
    dy = torch.randn(N, cout, Ln, generator=gen, dtype=torch.float64).float().double()
    # the value the layer sees: fp32 product of fp32 factors is NOT exact, so the reference forms it in float64 from the
    # same fp32 inputs (the kernel's fused multiply-add rounds once; the difference is within the tolerance)
    xin = (x * scale[None, :, None] + shift[None, :, None]).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = F.conv1d(xin, wr, br, stride=1, padding=dil if k == 3 else 0, dilation=dil if k == 3 else 1)
    y = F.leaky_relu(pre, SLOPE)
    (y * dy).sum().backward()
    dpre = torch.where(pre > 0, dy, dy * SLOPE).detach()
    return dict(x=x, scale=scale, shift=shift, w=w, b=b, dy=dy, y=y.detach(), dpre=dpre, dx=xin.grad, dw=wr.grad,
                db=br.grad, mean=y.detach().mean((0, 2)), var=y.detach().var((0, 2), unbiased=False))


def _close(got, want, what):
    """The linear-layer rule of tests/_seg_checks.py: 2e-5 * max(1, max|ref|) absolute."""
    tol = 2e-5 * max(1.0, float(want.abs().max()))
    err = float((got.double().cpu() - want).abs().max())
    assert err <= tol, (what, err, tol)


def run_conv1d_fwd(pr, device, dil, want_stats=True):
    """amx_conv1d_fwd through the C ABI -> (y [N][L][cos], (mean, var) merged by amx_bn_finalize or None)."""
    L = _lib()
    N, cin, Ln = pr["x"].shape
    cout, _, k = pr["w"].shape
    cos, cop = r4(cout), r16(cout)
    x = _nlc(pr["x"], device)
    sc, sh = _pad(pr["scale"], r4(cin), device), _pad(pr["shift"], r4(cin), device)
    wpk = _pack1d(pr["w"], cin, 0, device)
    bias = pr["b"].float().to(device)
    y = torch.full((N, Ln, cos), float("nan"), dtype=torch.float32, device=device)
    npix = N * Ln
    rows, rows_pix = L.load().amx_rows_for(npix), L.load().amx_rows_pix(npix)
    stats = torch.zeros((rows, 2, cop), dtype=torch.float32, device=device) if want_stats else None
    sp = L.stream_ptr(y)
    L.call("amx_conv1d_fwd", L.ptr(x), L.ptr(sc), L.ptr(sh), 1.0, r4(cin), L.ptr(wpk), L.ptr(bias), L.ptr(y),
           L.ptr(stats), N, Ln, cout, k, dil if k == 3 else 1, SLOPE, rows, rows_pix, sp)
    if not want_stats:
        return y, None
    gamma, beta = torch.ones(cout, device=device), torch.zeros(cout, device=device)
    scale, shift = torch.empty(cos, device=device), torch.empty(cos, device=device)
    mean, invstd = torch.empty(cos, device=device), torch.empty(cos, device=device)
    L.call("amx_bn_finalize", L.ptr(stats), rows, cop, 1, N, 1, Ln, rows_pix, L.ptr(gamma), L.ptr(beta), None, None,
           0.1, 0.0, cout, cos, L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd), sp)
    return y, (mean[:cout], 1.0 / invstd[:cout] ** 2)


def check_conv1d_kernels(device, shape):
    """amx_conv1d_fwd (forward, statistics, data gradient) and amx_conv1d_wgrad through the C ABI against float64
    torch.nn.functional.conv1d (+ bias, LeakyReLU 0.1) and its autograd, on inputs that carry a pending affine with a
    non-zero shift (a shift that leaked into the halo, or across a sample boundary, shows as an O(1) error).

    Shapes (N, L, Cin -> Cout, k, dil), each chosen for one failure:
      (2, 16, 1->5, 3, 1) first layer; (3, 37, 6->6, 3, 3) odd length, odd dilation; (2, 16, 6->1, 3, 1) one output
      channel; (2, 200, 20->33, 3, 4) channel counts across the 16 / 32 blocks, several position tiles with the halo
      across their borders; (5, 13, 4->4, 3, 2) N * L = 65: a tile spans a sample boundary; (2, 3, 4->4, 3, 4) dilation
      larger than the signal: only the centre tap sees data; (2, 16, 1->1, 1, 1) the decoder's `out` layer;
      (2, 40, 8->8, 3, 9) dilation beyond the 2-D limit; (3, 700, 4->8, 3, 2) more than one statistics row;
      (1, 500, 8->8, 3, 400) a staged window above 64 KB of LDS (864 positions x 20 floats), in all three launches."""
    L = _lib()
    N, Ln, cin, cout, k, dil = shape
    pr = conv1d_problem(N, Ln, cin, cout, k, dil)
    cos = r4(cout)
    y, (mean, var) = run_conv1d_fwd(pr, device, dil)
    assert not torch.isnan(y).any()
    _close(y[..., :cout].permute(0, 2, 1), pr["y"], "y")
    assert float(y[..., cout:].abs().max() if cos > cout else 0.0) == 0.0          # padding channels stay zero
    np.testing.assert_allclose(mean.cpu().double().numpy(), pr["mean"].numpy(), rtol=REL_TOL)
    np.testing.assert_allclose(var.cpu().double().numpy(), pr["var"].numpy(), rtol=REL_TOL)
    y2, _ = run_conv1d_fwd(pr, device, dil, want_stats=False)                   # the launch plan without statistics
    assert torch.equal(y, y2)

    # ---- data gradient: the same kernel on the flipped / transposed image, no affine, no bias, no activation
    d = dil if k == 3 else 1
    dpre = _nlc(pr["dpre"], device)
    wpk1 = _pack1d(pr["w"], cin, 1, device)
    dx = torch.full((N, Ln, r4(cin)), float("nan"), dtype=torch.float32, device=device)
    sp = L.stream_ptr(dx)
    L.call("amx_conv1d_fwd", L.ptr(dpre), None, None, 1.0, cos, L.ptr(wpk1), None, L.ptr(dx), None, N, Ln, cin, k, d,
           1.0, 0, 0, sp)
    _close(dx[..., :cin].permute(0, 2, 1), pr["dx"], "dx")

    # ---- weight / bias gradient: partial rows -> amx_reduce_rows_chunked -> amx_wgrad_reduce; two runs, same bits
    x = _nlc(pr["x"], device)
    sc, sh = _pad(pr["scale"], r4(cin), device), _pad(pr["shift"], r4(cin), device)
    rows = L.load().amx_conv1d_wgrad_rows(N, Ln)
    ci_pad, co_pad = r16(r4(cin)), r16(cout)
    got = []
    for _ in range(2):
        part = torch.full((rows, k, ci_pad, co_pad), float("nan"), dtype=torch.float32, device=device)
        bpart = torch.full((rows, co_pad), float("nan"), dtype=torch.float32, device=device)
        L.call("amx_conv1d_wgrad", L.ptr(x), L.ptr(sc), L.ptr(sh), 1.0, r4(cin), L.ptr(dpre), L.ptr(part), L.ptr(bpart),
               N, Ln, cout, k, d, rows, sp)
        red = torch.empty((1, k * ci_pad * co_pad), dtype=torch.float32, device=device)
        L.call("amx_reduce_rows_chunked", L.ptr(part), rows, k * ci_pad * co_pad, 1, L.ptr(red), sp)
        dw = torch.empty((cout, cin, k), dtype=torch.float32, device=device)
        L.call("amx_wgrad_reduce", L.ptr(red), 1, k, ci_pad, co_pad, cin, r4(cin), 0, cout, L.ptr(dw), sp)
        db = torch.empty(cout, dtype=torch.float32, device=device)
        L.call("amx_reduce_rows", L.ptr(bpart), rows, co_pad, cout, 1.0, L.ptr(db), sp)
        got.append((dw, db))
    _close(got[0][0], pr["dw"], "dw")
    _close(got[0][1], pr["db"], "db")
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def check_conv1d_vs_conv2d(device, dil):
    """amx_conv1d_fwd == amx_conv2d_fwd on the same data viewed as an H = 1 image with the three taps embedded in the
    middle row of a zero 3x3 weight (the summation order differs: tolerance of check_conv1d_kernels, not bit equality)."""
    L = _lib()
    N, Ln, cin, cout = 2, 37, 6, 6
    pr = conv1d_problem(N, Ln, cin, cout, 3, dil, seed=7)
    y1, _ = run_conv1d_fwd(pr, device, dil, want_stats=False)
    cos = r4(cout)
    w2 = torch.zeros(cout, cin, 3, 3, dtype=torch.float32)
    w2[:, :, 1, :] = pr["w"].float()
    w2 = w2.to(device)
    n = L.load().amx_pack_weights_size(cout, r4(cin), 0, 9, 0)
    wpk = torch.empty(n, dtype=torch.float32, device=device)
    sp = L.stream_ptr(wpk)
    L.call("amx_pack_weights", L.ptr(w2), L.ptr(wpk), cout, cin, r4(cin), 0, 0, 9, 0, sp)
    x = _nlc(pr["x"], device)
    sc, sh = _pad(pr["scale"], r4(cin), device), _pad(pr["shift"], r4(cin), device)
    bias = pr["b"].float().to(device)
    y2 = torch.full((N, 1, Ln, cos), float("nan"), dtype=torch.float32, device=device)
    L.call("amx_conv2d_fwd", L.ptr(x), L.ptr(sc), L.ptr(sh), r4(cin), None, None, None, 0, L.ptr(wpk), L.ptr(bias),
           None, L.ptr(y2), cos, None, 0, None, N, 1, Ln, cout, 9, dil, SLOPE, sp)
    want = y2.view(N, Ln, cos).double().cpu()
    tol = 2e-5 * max(1.0, float(want.abs().max()))
    assert float((y1.double().cpu() - want).abs().max()) <= tol
    _close(y1[..., :cout].permute(0, 2, 1), pr["y"], "y")


def check_conv1d_refusals(device):
    """AMX_BADARG only for what the kernel cannot do, and the message names the argument."""
    L = _lib()
    pr = conv1d_problem(1, 8, 4, 4, 3, 1)
    x = _nlc(pr["x"], device)
    wpk = _pack1d(pr["w"], 4, 0, device)
    y = torch.empty((1, 8, 4), dtype=torch.float32, device=device)
    sp = L.stream_ptr(y)
    for taps, dil, word in ((2, 1, "taps"), (3, 0, "dil")):
        try:
            L.call("amx_conv1d_fwd", L.ptr(x), None, None, 1.0, 4, L.ptr(wpk), None, L.ptr(y), None, 1, 8, 4, taps, dil,
                   SLOPE, 0, 0, sp)
        except L.AmxError as e:
            assert word in str(e), str(e)
        else:
            raise AssertionError("expected a refusal")
    # a window that cannot be staged: 64 + 2 * dil positions of 64 (+ 4) channels beyond 160 KB
    assert L.load().amx_conv1d_supported(64, 64, 4096, 3, 4) == 1
    assert L.load().amx_conv1d_supported(64, 64, 4096, 3, 1000) == 0
    assert L.load().amx_conv1d_supported(64, 64, 512, 3, 1000) == 1          # dil >= L: centre tap only, no window
    # the boundary: (64 + 2 * dil) positions x (64 + 4) floats + the 4 KB reduction buffer <= 160 KB  <=>  dil <= 261;
    # the weight gradient adds its 64 x (64 + 4) gradient tile and 3 x 64 flags                    <=>  dil <= 235
    assert L.load().amx_conv1d_supported(64, 64, 4096, 3, 261) == 1
    assert L.load().amx_conv1d_supported(64, 64, 4096, 3, 262) == 0
    assert L.load().amx_conv1d_wgrad_supported(64, 64, 4096, 3, 235) == 1
    assert L.load().amx_conv1d_wgrad_supported(64, 64, 4096, 3, 236) == 0


def check_conv1d_node_refuses_up_front(device):
    """A 1-D layer whose forward fits but whose weight gradient does not (64 -> 64 channels, dilation 250) is refused
    when the layer is built on a tape that needs gradients, before any launch, with the dilation named; without
    gradients the same layer runs and equals float64 torch."""
    from atomai_amd.nets.blocks import DilatedBlock
    L = _lib()
    torch.manual_seed(3)
    blk = DilatedBlock(1, 64, 64, [250], [250], lrelu_a=SLOPE).to(device)
    x = torch.randn(1, 64, 300)
    blk.train()
    try:
        blk(x.to(device).requires_grad_(True))
    except L.AmxError as e:
        assert "dilation = 250" in str(e) and "weight gradient" in str(e), str(e)
    else:
        raise AssertionError("expected a refusal")
    blk.eval()
    with torch.no_grad():
        got = blk(x.to(device))
    conv = blk.atrous_module[0]
    pre = F.conv1d(x.double(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), padding=250,
                   dilation=250)
    _close(got, pre + F.leaky_relu(pre, SLOPE), "dilated sum")


# ====================================================================================== pointwise kernels
def check_pointwise_kernels(device):
    """amx_upsample1d2x_fwd / _bwd, amx_avgpool_fwd (1-D k = 2 on L = 13, 2-D k = 2 on 9 x 8) and amx_mse_fwd_bwd against
    float64 torch at rtol 1e-6."""
    L = _lib()
    gen = torch.Generator().manual_seed(3)
    # nearest x2 along L
    N, C, Ln = 3, 6, 13
    v = torch.randn(N, C, Ln, generator=gen)
    vt = _nlc(v, device)
    u = torch.empty((N, 2 * Ln, r4(C)), dtype=torch.float32, device=device)
    sp = L.stream_ptr(u)
    L.call("amx_upsample1d2x_fwd", L.ptr(vt), L.ptr(u), N, Ln, r4(C), sp)
    want = F.interpolate(v.double(), scale_factor=2, mode="nearest")
    np.testing.assert_allclose(u[..., :C].permute(0, 2, 1).cpu().double().numpy(), want.numpy(), rtol=1e-6)
    du = torch.randn(N, C, 2 * Ln, generator=gen)
    vd = v.double().requires_grad_(True)
    (F.interpolate(vd, scale_factor=2, mode="nearest") * du.double()).sum().backward()
    dut = _nlc(du, device)
    dv = torch.empty((N, Ln, r4(C)), dtype=torch.float32, device=device)
    L.call("amx_upsample1d2x_bwd", L.ptr(dut), L.ptr(dv), N, Ln, r4(C), sp)
    np.testing.assert_allclose(dv[..., :C].permute(0, 2, 1).cpu().double().numpy(), vd.grad.numpy(), rtol=1e-6)
    # average pooling, floor semantics
    x1 = torch.randn(4, 1, 13, generator=gen)
    y1 = torch.empty((4, 6), dtype=torch.float32, device=device)
    L.call("amx_avgpool_fwd", L.ptr(x1.to(device)), L.ptr(y1), 4, 1, 13, 1, 2, sp)
    np.testing.assert_allclose(y1.cpu().double().numpy(), F.avg_pool1d(x1.double(), 2, 2)[:, 0].numpy(), rtol=1e-6)
    x2 = torch.randn(3, 1, 9, 8, generator=gen)
    y2 = torch.empty((3, 4, 4), dtype=torch.float32, device=device)
    L.call("amx_avgpool_fwd", L.ptr(x2.to(device)), L.ptr(y2), 3, 9, 8, 2, 2, sp)
    np.testing.assert_allclose(y2.cpu().double().numpy(), F.avg_pool2d(x2.double(), 2, 2)[:, 0].numpy(), rtol=1e-6)
    # MSE, more than one block of the first stage
    n = 3 * 4096 + 17
    p, t = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    rows = L.load().amx_mse_rows(n)
    assert rows == 4
    grad = torch.empty(n, dtype=torch.float32, device=device)
    part = torch.empty(rows, dtype=torch.float32, device=device)
    loss = torch.empty((), dtype=torch.float32, device=device)
    L.call("amx_mse_fwd_bwd", L.ptr(p.to(device)), L.ptr(t.to(device)), L.ptr(grad), L.ptr(part), n, rows, sp)
    L.call("amx_reduce_rows", L.ptr(part), rows, 1, 1, 1.0 / n, L.ptr(loss), sp)
    pd = p.double().requires_grad_(True)
    ref = F.mse_loss(pd, t.double())
    ref.backward()
    np.testing.assert_allclose(float(loss), float(ref.detach()), rtol=1e-6)
    np.testing.assert_allclose(grad.cpu().double().numpy(), pd.grad.numpy(), rtol=1e-6)


def check_upsample_carries_affine(device):
    """The nearest upsample that carries the producer's affine on == (bit for bit) the upsample of the materialised
    tensor, in 1-D and in 2-D; a source without a pending affine takes the path it always took."""
    from atomai_amd.engine import Act, Tape
    L = _lib()
    gen = torch.Generator().manual_seed(11)
    for ndim, shape in ((1, (2, 1, 7, 8)), (2, (2, 5, 6, 8))):
        C = 6
        t = torch.randn(*shape, generator=gen)
        t[..., C:] = 0
        t = t.to(device)
        scale, shift = _pad(torch.rand(C, generator=gen) + 0.5, 8, device), _pad(torch.rand(C, generator=gen) + 0.3, 8, device)
        tape = Tape(False, False)
        up = (lambda a: tape.upsample1d(a, "nearest")) if ndim == 1 else (lambda a: tape.upsample(a, "nearest"))
        carried = up(Act(t, C, scale, shift))
        assert carried.scale is scale and carried.shift is shift
        got = tape.output(carried).value
        mat = torch.empty_like(t)
        L.call("amx_affine_nhwc", L.ptr(t), L.ptr(scale), L.ptr(shift), L.ptr(mat), t.numel() // 8, 8, L.stream_ptr(t))
        plain = up(Act(mat, C))
        assert plain.scale is None
        want = tape.output(plain).value
        assert torch.equal(got, want)
        ref = F.interpolate((t[..., :C].double().cpu() * scale[:C].double().cpu() + shift[:C].double().cpu())
                            .permute(0, 3, 1, 2), scale_factor=(1, 2) if ndim == 1 else 2, mode="nearest")
        np.testing.assert_allclose(got.double().cpu().numpy(), ref.numpy(), rtol=1e-6)
        # backward: the gradient an Act holds is that of the value its consumers see (after the affine), so the carried
        # affine changes nothing: the source receives the sum of its children, as without one
        tape = Tape(True, True)
        src = Act(t, C, scale, shift, needs_grad=True)
        out = up(src)
        g = torch.randn(*out.t.shape, generator=gen).to(device)
        out.grad = g
        tape.nodes[-1].backward(tape)
        gd = g.double().cpu()
        want = gd[:, :, 0::2] + gd[:, :, 1::2] if ndim == 1 else (gd[:, 0::2, 0::2] + gd[:, 0::2, 1::2]
                                                                    + gd[:, 1::2, 0::2] + gd[:, 1::2, 1::2])
        np.testing.assert_allclose(src.grad.double().cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6)


def check_mse_loss(device):
    """losses_metrics.MSELoss: prints as MSELoss(), is what select_loss('mse') returns, equals torch (value and gradient)
    on the kernel path and defers to its parent — same value, same warning — for a shape-mismatched pair."""
    from atomai_amd.losses_metrics import MSELoss, select_loss
    crit = select_loss("mse")
    assert isinstance(crit, MSELoss) and isinstance(crit, torch.nn.MSELoss) and repr(crit) == "MSELoss()"
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(4, 1, 16, generator=gen).to(device).requires_grad_(True)
    t = torch.randn(4, 1, 16, generator=gen).to(device)
    loss = crit(p, t)
    loss.backward()
    pd = p.detach().double().cpu().requires_grad_(True)
    ref = F.mse_loss(pd, t.double().cpu())
    ref.backward()
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-6)
    np.testing.assert_allclose(p.grad.double().cpu().numpy(), pd.grad.numpy(), rtol=1e-6)
    t2 = torch.randn(4, 16, generator=gen).to(device)                      # broadcasts against (4, 1, 16): parent class
    with warnings.catch_warnings(record=True) as w1:
        warnings.simplefilter("always")
        a = crit(p.detach(), t2)
    with warnings.catch_warnings(record=True) as w2:
        warnings.simplefilter("always")
        b = torch.nn.MSELoss()(p.detach(), t2)
    assert torch.equal(a, b)
    assert [str(x.message) for x in w1] == [str(x.message) for x in w2] and len(w1) == 1
    assert torch.equal(MSELoss(reduction="sum")(p.detach(), t), torch.nn.MSELoss(reduction="sum")(p.detach(), t))


# ====================================================================================== nets
def signal_ed_f64(sd, x, in_dim, out_dim, training, batch_norm=True, encoder_downsampling=0, decoder_upsampling=False,
                  momentum=0.1, eps=1e-5, pre=None):
    """Plain-torch functional statement of SignalED (atomai/nets/ed.py:20-228) in float64 on the CPU, written from the
    module tree alone: `sd` maps state-dict keys to float64 tensors.  Returns (output, {running-stat key: new value}).
    The `not gpu` tier pins it against the reference goldens at 1e-10; the GPU tier uses it as the yardstick of the
    default architecture (the role oracle/vae_oracle.py plays for the VAEs).  `pre`: a list that receives every LeakyReLU
    input (detached), for default_inputs_clear_the_kink."""
    nd = len(in_dim), len(out_dim)
    new_stats = {}

    def conv(h, prefix, i, ndim, dil=1):
        w, b = sd[f"{prefix}.{i}.weight"], sd[f"{prefix}.{i}.bias"]
        f = F.conv2d if ndim == 2 else F.conv1d
        h = f(h, w, b, stride=1, padding=dil if w.shape[-1] == 3 else 0, dilation=dil)
        if pre is not None:
            pre.append(h.detach())
        return h

    def bnorm(h, key):
        dims = [0] + list(range(2, h.ndim))
        shape = [1, -1] + [1] * (h.ndim - 2)
        if training:
            mean, var = h.mean(dims), h.var(dims, unbiased=False)
            n = h.numel() / h.shape[1]
            new_stats[key + ".running_mean"] = (1 - momentum) * sd[key + ".running_mean"] + momentum * mean.detach()
            new_stats[key + ".running_var"] = ((1 - momentum) * sd[key + ".running_var"]
                                               + momentum * var.detach() * n / max(n - 1, 1))
        else:
            mean, var = sd[key + ".running_mean"], sd[key + ".running_var"]
        return (h - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * sd[key + ".weight"].view(shape) \
            + sd[key + ".bias"].view(shape)

    def conv_block(h, prefix, nlayers, ndim):
        per = 3 if batch_norm else 2
        for j in range(nlayers):
            h = F.leaky_relu(conv(h, prefix, per * j, ndim), SLOPE)
            if batch_norm:
                h = bnorm(h, f"{prefix}.{per * j + 2}")
        return h

    # ---- encoder
    h = x
    if encoder_downsampling:
        k = encoder_downsampling
        h = F.avg_pool2d(h, k, k) if nd[0] == 2 else F.avg_pool1d(h, k, k)
    n_enc = len([k for k in sd if k.startswith("encoder.conv.block.") and k.endswith(".weight") and sd[k].ndim > 1])
    h = conv_block(h, "encoder.conv.block", n_enc, nd[0])
    z = F.linear(h.reshape(h.shape[0], -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"])
    # ---- decoder
    nf = sd["decoder.conv.block.0.weight"].shape[1]
    dims = [s // 4 for s in out_dim] if decoder_upsampling else list(out_dim)
    h = F.linear(z, sd["decoder.fc.weight"], sd["decoder.fc.bias"]).reshape(-1, nf, *dims)
    if decoder_upsampling:
        h = F.interpolate(conv_block(h, "decoder.deconv1.block", 1, nd[1]), scale_factor=2, mode="nearest")
        h = F.interpolate(conv_block(h, "decoder.deconv2.block", 1, nd[1]), scale_factor=2, mode="nearest")
    per = 3 if batch_norm else 2
    n_dil = len([k for k in sd if k.startswith("decoder.dilblock.atrous_module.") and k.endswith(".weight")
                 and sd[k].ndim > 1])
    total = 0
    for j in range(n_dil):                              # DilatedBlock: the sum of EVERY sub-layer output
        h = conv(h, "decoder.dilblock.atrous_module", per * j, nd[1], dil=j + 1)
        total = total + h
        h = F.leaky_relu(h, SLOPE)
        total = total + h
        if batch_norm:
            h = bnorm(h, f"decoder.dilblock.atrous_module.{per * j + 2}")
            total = total + h
    h = conv_block(total, "decoder.conv.block", 1, nd[1])
    f = F.conv2d if nd[1] == 2 else F.conv1d
    return f(h, sd["decoder.out.weight"], sd["decoder.out.bias"]), new_stats


def f64_step(sd32, x, y, in_dim, out_dim, dtype=torch.float64, **kw):
    """One training-mode evaluation of signal_ed_f64 with autograd -> (output, loss, {key: gradient}, new running stats);
    dtype=torch.float32 gives the functional's own fp32 noise."""
    sd = {k: v.detach().to(dtype).cpu().clone() for k, v in sd32.items()}
    params = [k for k in sd if "running" not in k and "num_batches_tracked" not in k]
    for k in params:
        sd[k].requires_grad_(True)
    out, stats = signal_ed_f64(sd, x.to(dtype).cpu(), in_dim, out_dim, True, **kw)
    loss = F.mse_loss(out, y.to(dtype).cpu())
    loss.backward()
    return out.detach(), loss.item(), {k: sd[k].grad for k in params}, stats


def check_f64_statement_vs_golden(name):
    """signal_ed_f64 == the reference in float64 (output, loss, gradients, running statistics) at 1e-10."""
    in_dim, out_dim, kw = CASES[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sd = {k[:-5]: torch.from_numpy(g[k]) for k in g.files if k.endswith("|init")}
    out, loss, grads, stats = f64_step(sd, torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), in_dim, out_dim, **kw)
    assert relmax(out.numpy(), g["out|f64"]) < 1e-10
    assert abs(loss - g["losses|f64"][0]) <= 1e-10 * abs(g["losses|f64"][0])
    gmax = max(np.abs(g[k + "|grad|f64"]).max() for k in grads)
    for k, v in grads.items():
        assert np.abs(v.numpy() - g[k + "|grad|f64"]).max() / gmax < 1e-10, k
    for k, v in stats.items():
        np.testing.assert_allclose(v.numpy(), g[k + "|bn1|f64"], rtol=1e-10, atol=1e-12)
    assert len(stats) == len([k for k in g.files if k.endswith("|bn1|f64")])


def _train_and_judge(net, x, y, ref, device):
    """The criteria of tests/_seg_checks.py::check_net_case on three FusedAdam steps of `net`.  `ref`: out / grads (fp64),
    per-parameter fp32 noise `ref32` (or None: the floor alone), running statistics after one step, the three losses and
    the eval output after them (or None)."""
    from atomai_amd.losses_metrics import select_loss
    from atomai_amd.optim import FusedAdam
    crit = select_loss("mse")
    opt = FusedAdam(net.parameters(), lr=1e-3)
    opt.prepare()
    losses = []
    for s in range(3):
        net.train()
        opt.zero_grad()
        pred = net(x)
        loss = crit(pred, y)
        loss.backward()
        if s == 0:
            assert relmax(pred.detach().cpu().numpy(), ref["out"]) < REL_TOL
            gmax = max(np.abs(v).max() for v in ref["grads"].values())
            for k, p in net.named_parameters():
                err = np.abs(p.grad.cpu().numpy() - ref["grads"][k]).max() / gmax
                ref32 = ref["ref32"][k] / gmax if ref["ref32"] is not None else 0.0
                print(f"  grad {k}: err {err:.3e} ref32 {ref32:.3e}")
                assert err <= max(4 * ref32, 2e-5), (k, err, ref32)
        opt.step()
        if s == 0:
            for k, v in net.state_dict().items():
                if "running" in k:
                    np.testing.assert_allclose(v.cpu().numpy(), ref["bn1"][k], rtol=REL_TOL, atol=1e-6)
                if "num_batches_tracked" in k:
                    assert int(v) == 1
        losses.append(loss.item())
        if ref["losses"] is None:
            np.testing.assert_allclose(losses[0], ref["loss0"], rtol=REL_TOL)
            break
    if ref["losses"] is not None:
        np.testing.assert_allclose(losses, ref["losses"], rtol=REL_TOL)
        st = opt.state_dict()["state"]
        assert set(st[0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and float(st[0]["step"]) == 3
    if ref["eval"] is not None:
        net.eval()
        with torch.no_grad():
            ev = net(x).cpu().numpy()
        assert relmax(ev, ref["eval"].astype(np.float64)) < 2e-2        # parameters after Adam steps: loose


def check_net_case(name, device):
    """Net parity against the reference golden: initial state dict bit-equal under the same seed, training-mode output,
    first-step gradients (against fp64, relative to the reference's own fp32 noise), running statistics, three Adam-step
    losses, the optimizer state's format, the eval output after the steps."""
    from atomai_amd.nets import init_imspec_model
    in_dim, out_dim, kw = CASES[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    torch.manual_seed(int(g["meta"][0]))
    net, meta = init_imspec_model(in_dim, out_dim, LATENT, **NET_KW, **kw)
    sd = net.state_dict()
    assert sorted(k + "|init" for k in sd) == sorted(k for k in g.files if k.endswith("|init"))
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g[k + "|init"]), k
    assert meta["model_type"] == "imspec" and meta["batchnorm"] == kw.get("batch_norm", True)
    assert list(meta)[:4] == ["model_type", "in_dim", "out_dim", "latent_dim"]
    net.to(device)
    names = [k for k, _ in net.named_parameters()]
    ref = dict(out=g["out|f64"], grads={k: g[k + "|grad|f64"] for k in names},
               ref32={k: np.abs(g[k + "|grad|f32"] - g[k + "|grad|f64"]).max() for k in names},
               bn1={k[:-8]: g[k] for k in g.files if k.endswith("|bn1|f64")}, losses=g["losses|f64"],
               eval=g["eval_out|f32"])
    _train_and_judge(net, torch.from_numpy(g["x"]).to(device), torch.from_numpy(g["y"]).to(device), ref, device)


# LeakyReLU has a kink at 0: where a pre-activation of the float64 yardstick lies closer to 0 than fp32 arithmetic can
# resolve, ANY correct fp32 evaluation may land on the other side, its derivative there is 0.1 instead of 1 (or the
# reverse) and one such element moves a weight gradient by ~1e-4 of the gradient scale: float64 is then no yardstick for
# that element.  The default architecture has ~9e5 LeakyReLU inputs per step: torch's own fp32 evaluation of
# signal_ed_f64 flipped a sign against its float64 one for 8 of 116 data draws (a flip needs a pre-activation within the
# TYPICAL fp32 error, ~5e-7, of zero).  The data of the default-architecture check are therefore drawn from the smallest
# generator seed (counted from 0, parameters from torch.manual_seed(1)) at which the yardstick is well-posed for every
# fp32 evaluation, not only for torch's: every LeakyReLU input of the float64 evaluation is farther from 0 than the
# LARGEST difference between the fp32 and the float64 evaluation of any LeakyReLU input (~7e-6, the reference's own
# worst fp32 noise).  That bound is an order of magnitude above the typical error, which is why the first seeds that
# meet it are 636 and 318 although nine draws in ten are free of flips in torch.  What the check sees is thereby limited
# to data without a sign decision inside fp32 noise: at any other draw a correct fp32 network may differ from float64 by
# ~1e-4 of the gradient scale in one channel, and the 2e-5 criterion would measure the draw, not the kernels.  The
# rule looks at the CPU yardstick alone and find_default_data_seed states it as code.  The fp32 noise depends a little on
# the host's convolution algorithm, so the value measured when the seed was found is recorded next to it, and
# default_inputs_clear_the_kink asserts, in both tiers, that the float64 margin (host-independent) exceeds it.
DEFAULT_DATA_SEED = {((16, 16), (64,)): (636, 7.305e-06), ((64,), (16, 16)): (318, 6.545e-06)}


def _default_problem(in_dim, out_dim, seed):
    from atomai_amd.nets import init_imspec_model
    torch.manual_seed(1)
    net, _ = init_imspec_model(in_dim, out_dim, 10)
    gen = torch.Generator().manual_seed(seed)
    x, y = torch.rand(8, 1, *in_dim, generator=gen), torch.rand(8, 1, *out_dim, generator=gen)
    return net, x, y


def kink_margin(sd, x, in_dim, out_dim):
    """(smallest |LeakyReLU input| of signal_ed_f64 in float64, largest fp32-vs-float64 difference of such an input)."""
    p64, p32 = [], []
    with torch.no_grad():
        signal_ed_f64({k: v.detach().double().cpu() for k, v in sd.items()}, x.double(), in_dim, out_dim, True, pre=p64)
        signal_ed_f64({k: v.detach().float().cpu() for k, v in sd.items()}, x.float(), in_dim, out_dim, True, pre=p32)
    margin = min(float(b.abs().min()) for b in p64)
    noise = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return margin, noise


def find_default_data_seed(in_dim, out_dim, limit=20000):
    """The rule behind DEFAULT_DATA_SEED (not run by the suite: some seconds of CPU per direction)."""
    for seed in range(limit):
        net, x, _ = _default_problem(in_dim, out_dim, seed)
        margin, noise = kink_margin(net.state_dict(), x, in_dim, out_dim)
        if margin > noise:
            return seed
    raise AssertionError("no seed below the limit")


def default_inputs_clear_the_kink(in_dim, out_dim):
    seed, recorded = DEFAULT_DATA_SEED[(tuple(in_dim), tuple(out_dim))]
    net, x, _ = _default_problem(in_dim, out_dim, seed)
    margin, noise = kink_margin(net.state_dict(), x, in_dim, out_dim)
    print(f"  smallest |LeakyReLU input| {margin:.3e}, fp32 noise of the yardstick: recorded {recorded:.3e}, here {noise:.3e}")
    assert margin > recorded, (margin, recorded)


def check_default_architecture(device, in_dim, out_dim):
    """GPU tier: the default architecture (3 / 4 layers, 64 / 64 filters), latent_dim 10, B = 8, one training step against
    signal_ed_f64 on the CPU, with the criteria of check_net_case (ref32: the same functional evaluated in fp32), on data
    at which float64 is a yardstick for an fp32 LeakyReLU network (DEFAULT_DATA_SEED)."""
    default_inputs_clear_the_kink(in_dim, out_dim)
    net, x, y = _default_problem(in_dim, out_dim, DEFAULT_DATA_SEED[(tuple(in_dim), tuple(out_dim))][0])
    out, loss, grads, stats = f64_step(net.state_dict(), x, y, in_dim, out_dim)
    g32 = f64_step(net.state_dict(), x, y, in_dim, out_dim, dtype=torch.float32)[2]
    ref = dict(out=out.numpy(), grads={k: v.numpy() for k, v in grads.items()},
               ref32={k: float((g32[k].double() - grads[k]).abs().max()) for k in grads},
               bn1={k: v.numpy() for k, v in stats.items()}, losses=None, loss0=loss, eval=None)
    net.to(device)
    _train_and_judge(net, x.to(device), y.to(device), ref, device)


# ====================================================================================== model level
def _fit_data():
    g = np.load(os.path.join(GOLD, "imspec_fit.npz"))
    return g, g["X"], g["y"]


def check_determinism(device, tmp_path):
    """Two fits of 5 cycles from seed 1: equal loss lists, bit-equal parameters."""
    import atomai_amd as aoi
    _, X, y = _fit_data()
    runs = []
    for _ in range(2):
        m = aoi.models.ImSpec((8, 8), (16,), latent_dim=3)
        m.fit(X[:32], y[:32], X[32:], y[32:], training_cycles=5, batch_size=8, plot_training_history=False,
              filename=os.path.join(str(tmp_path), "det"))
        runs.append((list(m.loss_acc["train_loss"]), list(m.loss_acc["test_loss"]),
                     {k: v.detach().cpu().clone() for k, v in m.net.state_dict().items()}))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k, v in runs[0][2].items():
        assert torch.equal(v, runs[1][2][k]), k


def check_api(device, tmp_path):
    """ImSpec.fit / predict / save_model / load_model / the reference's checkpoint / the refusals."""
    import atomai_amd as aoi
    g, X, y = _fit_data()
    fn = os.path.join(str(tmp_path), "imspec")
    m = aoi.models.ImSpec((8, 8), (16,), latent_dim=LATENT, **NET_KW)
    m.fit(X[:32], y[:32], X[32:], y[32:], training_cycles=4, batch_size=8, filename=fn, plot_training_history=False)
    assert list(m.batch_idx_train) == list(g["batch_idx_train"]) and list(m.batch_idx_test) == list(g["batch_idx_test"])
    tl = np.array(m.loss_acc["train_loss"])
    print("train losses", tl, "reference f64", g["train_loss|f64"], "drift", float(g["drift"]))
    np.testing.assert_allclose(tl[0], g["train_loss|f64"][0], rtol=REL_TOL)
    np.testing.assert_allclose(tl[1:], g["train_loss|f64"][1:], rtol=max(4 * float(g["drift"]), REL_TOL))
    assert len(m.loss_acc["test_loss"]) == 4 and repr(m.criterion) == "MSELoss()"
    pred = m.predict(X[:5], norm=False)
    assert pred.shape == (5, 16) and pred.dtype == np.float32
    assert m.predict(X[:5, 0]).shape == (5, 16) and m.predict(X[0, 0], norm=True, verbose=False).shape == (1, 16)
    # ---- checkpoint written here: torch types only, reloads to the same predictions bit for bit
    ck = fn + "_metadict_final.tar"
    loaded = torch.load(ck, weights_only=False)
    assert sorted(loaded.keys()) == sorted(str(k) for k in g["ckpt|meta_keys"])
    assert type(loaded["optimizer"]) is torch.optim.Adam and loaded["batchnorm"] is True

    def torch_only(o):
        if isinstance(o, dict):
            return all(torch_only(v) for v in o.values())
        if isinstance(o, (list, tuple)):
            return all(torch_only(v) for v in o)
        return isinstance(o, (torch.Tensor, int, float, bool, str, type(None), torch.optim.Optimizer))
    assert torch_only(loaded)
    m2 = aoi.models.load_model(ck)
    assert isinstance(m2, aoi.models.ImSpec) and not m2.net.training
    assert np.array_equal(m2.predict(X[:5], norm=False, verbose=False), pred)
    m.save_model(os.path.join(str(tmp_path), "again"))
    assert np.array_equal(aoi.models.load_model(os.path.join(str(tmp_path), "again.tar")).predict(X[:5], norm=False), pred)
    # ---- the checkpoint the reference wrote
    mr = aoi.models.load_model(os.path.join(GOLD, "ref_imspec_ckpt.tar"))
    assert relmax(mr.predict(X[:5], norm=False), g["ckpt|pred"].astype(np.float64)) < REL_TOL
    assert relmax(mr.predict(X[:5]), g["pred_norm"].astype(np.float64)) < REL_TOL
    # ---- a BatchNorm-free model survives the round trip (the reference's loader drops "batchnorm")
    m3 = aoi.models.ImSpec((16,), (8, 8), latent_dim=2, batch_norm=False, **NET_KW)
    m3.fit(y[:32], X[:32], y[32:], X[32:], training_cycles=2, batch_size=8, filename=fn + "_nobn", swa=True,
           plot_training_history=False)
    m4 = aoi.models.load_model(fn + "_nobn_metadict_final.tar")
    assert not any("running" in k for k in m4.net.state_dict())
    p3 = m3.predict(y[:3], norm=False)
    assert p3.shape == (3, 8, 8) and np.array_equal(m4.predict(y[:3], norm=False), p3)
    # ---- full_epoch, and inputs without the channel axis (a warning each, then the same training)
    m5 = aoi.models.ImSpec((8, 8), (16,), latent_dim=LATENT, **NET_KW)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m5.fit(X[:32, 0], y[:32, 0], X[32:, 0], y[32:, 0], training_cycles=2, batch_size=8, full_epoch=True,
               filename=fn + "_fe", plot_training_history=False)
    msgs = [str(x.message) for x in w]
    for what in ("training images", "test images", "training spectra", "test spectra"):
        assert f"Adding a channel dimension of 1 to {what}" in msgs
    assert len(m5.loss_acc["train_loss"]) == 2
    # ---- refusals
    for bad in (dict(in_dim=(8, 9)), dict(out_dim=(15,))):
        mb = aoi.models.ImSpec(bad.get("in_dim", (8, 8)), bad.get("out_dim", (16,)), latent_dim=2, **NET_KW)
        try:
            mb.fit(X[:32], y[:32], X[32:], y[32:], training_cycles=1, batch_size=8)
        except AssertionError as e:
            assert "dimensions of the model must match" in str(e)
        else:
            raise AssertionError("expected an AssertionError")
    try:
        aoi.models.ImSpec((8, 8), (16,), latent_dim=2, **NET_KW).fit(X[:32], y[:32], X[32:], y[32:], training_cycles=1,
                                                                  batch_size=8, gauss_noise=[20, 60])
    except NotImplementedError:
        pass
    else:
        raise AssertionError("expected NotImplementedError")
    assert aoi.transforms.imspec_augmentor((8, 8), (16,)) is None
    try:
        aoi.nets.ConvBlock(3, 1, 1, 4)
    except AssertionError:
        pass
    else:
        raise AssertionError("expected an AssertionError")
    for cls, args in ((aoi.nets.UpsampleBlock, (1, 4, 4)), (aoi.nets.ResBlock, (1, 4, 4))):
        try:
            cls(*args)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("expected NotImplementedError")
    x_req = torch.rand(2, 1, 8, 8, device=device, requires_grad=True)
    try:
        aoi.nets.SignalEncoder((8, 8), 2, 1, 4, downsampling=2).to(device)(x_req)
    except NotImplementedError as e:
        assert "gradient" in str(e)
    else:
        raise AssertionError("expected NotImplementedError")
