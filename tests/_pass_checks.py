"""Shared bodies of the tests of the HBM-bound "pass" kernels that sit between the convolutions: csrc/spatial.hip (max-pool
forward / backward, pool backward with the first layer's weight-gradient sums, x2 upsample backward, DilatedBlock sum),
res.hip (residual-block output, LeakyReLU backward), resize.hip (resize-and-concatenate), the BatchNorm part of bn.hip
(eval affine, backward reduce -> finalize -> apply -> bias sums) and the layout converters / copies of pack.hip, each called
through the C ABI with the arguments engine.py passes, against plain torch / numpy on the host.  The SAME checks run
  * on the CPU through the SIMT emulator build of the kernel sources (`not gpu` tier, test_pass_emulated.py), and
  * on a real MI355X through libatomai_amd.so (`gpu` tier, test_pass_gpu.py).
The geometries are the smallest that reach each branch (G = Cs / 4 channel groups, PL = 256 / G pixel lanes): odd heights
and widths, G that divides neither 256 nor 32, ragged tails of the unrolled loops, a second grid-stride trip, padded
channels, NEGATIVE producer scales and no scales at all.

Kernels that branch on a comparison (arg-max of a pool window, `> 0` of a LeakyReLU) get DYADIC inputs: activations k / 8
in [-4, 4], scales from {+-0.25, +-0.5, +-1, +-1.5}, shifts k / 16.  a * scale + shift is then exact in fp32 and in fp64
(a multiple of 1 / 32 below 8), so ties inside pool windows and exact zeros at the LeakyReLU are decided identically in
both precisions, and every output with at most one fp32 rounding must equal a float32 numpy restatement BIT FOR BIT.
Everything compared with fp64 uses the project's rule: error <= max(4 x the error of the fp32 evaluation of the same torch
reference, 2e-5), both normalised by the largest fp64 magnitude of that output."""
import contextlib
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _seg_checks import REL_TOL

f32 = np.float32
SENTINEL = 12345.0
WORST = {}                                   # kernel -> (err / bound, err / floor or None), for the report of a run


def _nan(device, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=device)


def _dev(v, device):
    return torch.from_numpy(np.array(v, dtype=np.float32, order="C")).to(device)        # (a copy: kernels write into some)


def _host(t):
    return t.detach().cpu().numpy()


def _t(v, dtype):
    return torch.from_numpy(np.array(v, order="C")).to(dtype)                  # (a copy, whatever the dtype)


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _finite(tag, **tensors):
    for k, v in tensors.items():                                  # nothing of a NaN-filled output is left unwritten
        v = np.asarray(v)
        assert np.isfinite(v).all(), (tag, k, int((~np.isfinite(v)).sum()))


def _compare(kernel, tag, what, got, ref64, ref32):
    got, ref64, ref32 = (np.asarray(v, dtype=np.float64) for v in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (kernel, tag, what, got.shape, ref64.shape, ref32.shape)
    norm = float(np.abs(ref64).max())
    assert norm > 0, (kernel, tag, what)
    err = float(np.abs(got - ref64).max()) / norm
    floor = float(np.abs(ref32 - ref64).max()) / norm
    bound = max(4 * floor, 2e-5)
    ratio = err / floor if floor > 0 else None
    print(f"pass {kernel} {tag} {what}: error {err:.2e} (torch-fp32 floor {floor:.2e}, err/floor "
          f"{'n/a' if ratio is None else '%.2f' % ratio}, err/bound {err / bound:.3f})")
    w = WORST.get(kernel, (0.0, None))
    WORST[kernel] = (max(w[0], err / bound), ratio if w[1] is None else (w[1] if ratio is None else max(w[1], ratio)))
    assert err <= bound, (kernel, tag, what, err, floor)


def report():
    for k in sorted(WORST):
        b, r = WORST[k]
        print(f"pass-worst {k}: err/bound {b:.3f}, err/floor {'n/a' if r is None else '%.2f' % r}")


# ---------------------------------------------------------------- input draws
def dyadic_act(rs, shape, zero_frac=0.0):
    """Multiples of 1/8 in [-4, 4]; zero_frac of them exactly 0."""
    a = rs.randint(-32, 33, shape, dtype=np.int8).astype(f32) / f32(8)
    if zero_frac:
        a[rs.rand(*shape) < zero_frac] = 0.0
    return a


def draw_affine(rs, Cs, dyadic):
    """Producer scale / shift [Cs]: ~40 % negative scales, channel 0 always negative."""
    sign = np.where(rs.rand(Cs) < 0.4, -1.0, 1.0)
    sign[0] = -1.0
    if dyadic:
        return (sign * rs.choice([0.25, 0.5, 1.0, 1.5], Cs)).astype(f32), (rs.randint(-16, 17, Cs) / 16.0).astype(f32)
    return (sign * (0.5 + rs.rand(Cs))).astype(f32), (0.3 * rs.randn(Cs)).astype(f32)


def _tied_windows(rs, a):
    """Copies one element of ~30 % of the 2x2 windows over another one (or over all of them): exact ties, among them ties
    for the maximum.  With a negative scale a tie of the raw minimum is a tie of the normalised maximum."""
    N, H, W, Cs = a.shape
    Ho, Wo = H // 2, W // 2
    for n in range(N):
        for yo in range(Ho):
            for xo in range(Wo):
                win = a[n, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2]             # view [2][2][Cs]
                u = rs.rand(Cs)
                flat = win.reshape(4, Cs)                                    # (a copy: non-contiguous view)
                order = np.argsort(flat, 0)
                hi, lo = order[3], order[0]
                c = np.arange(Cs)
                m = u < 0.1                                                  # the maximum twice
                k = rs.randint(0, 4, Cs)
                flat[k[m], c[m]] = flat[hi[m], c[m]]
                m = (u >= 0.1) & (u < 0.2)                                   # the minimum twice
                flat[k[m], c[m]] = flat[lo[m], c[m]]
                m = (u >= 0.2) & (u < 0.3)                                   # all four equal
                flat[:, m] = flat[0, m]
                a[n, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2] = flat.reshape(2, 2, Cs)
    a[0, 0:2, 0:2, 0] = a[0, 0, 0, 0]                                        # (one tie for the maximum whatever the draw)
    return a


# ================================================================ 1. max-pool forward / backward
# name -> (N, H, W, Cs)
POOL_CASES = {
    "minimal_2x2x2_g1": (2, 2, 2, 4),
    "odd_h_odd_w_g5_2x7x5": (2, 7, 5, 20),                       # G = 5 divides neither 256 nor 32
    "odd_w_g13_1x6x9": (1, 6, 9, 52),
    "odd_h_g4_3x9x4": (3, 9, 4, 16),
    "13_workgroups_g16_2x22x18": (2, 22, 18, 64),
    "g128_all_threads_write_bstats_1x6x4": (1, 6, 4, 512),
}
# 33 024 windows x 16 groups > 2048 x 256 slots: a second grid-stride trip of pool_bwd_kernel with bstats
POOL_SECOND_TRIP = (2, 258, 256, 64)


class Pool:
    def __init__(self, device, nhwc, seed=0, ties=True):
        N, H, W, Cs = nhwc
        rs = np.random.RandomState(seed)
        a = dyadic_act(rs, (N, H, W, Cs))
        if ties and N * H * W * Cs < 1 << 20:
            a = _tied_windows(rs, a)
        self.N, self.H, self.W, self.Cs, self.device = N, H, W, Cs, device
        self.a = a
        self.scale, self.shift = draw_affine(rs, Cs, True)
        self.g = rs.randn(N, H // 2, W // 2, Cs).astype(f32)
        self.skip = rs.randn(N, H, W, Cs).astype(f32)
        self.x = rs.randn(N, H, W).astype(f32)                                # the net input (first-layer weight gradient)
        self.d = {k: _dev(getattr(self, k), device) for k in ("a", "scale", "shift", "g", "skip", "x")}

    def v32(self, affine):
        """fl32(a * scale + shift): exact for the dyadic draws."""
        return (self.a * self.scale + self.shift).astype(f32) if affine else self.a

    def windows(self, affine):
        N, H, W, Cs = self.a.shape
        Ho, Wo = H // 2, W // 2
        v = self.v32(affine)[:, :2 * Ho, :2 * Wo]
        return v.reshape(N, Ho, 2, Wo, 2, Cs).transpose(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, 4, Cs)   # scan order k = 2 dy + dx

    def restate(self, affine, skip):
        """float32 numpy restatement: (pooled, dy).  np.argmax returns the FIRST maximum."""
        N, H, W, Cs = self.a.shape
        Ho, Wo = H // 2, W // 2
        win = self.windows(affine)
        am = win.argmax(3)
        routed = np.where(np.arange(4).reshape(1, 1, 1, 4, 1) == am[:, :, :, None, :], self.g[:, :, :, None, :], f32(0))
        routed = routed.astype(f32).reshape(N, Ho, Wo, 2, 2, Cs).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, Cs)
        dy = self.skip.copy() if skip else np.zeros_like(self.a)
        dy[:, :2 * Ho, :2 * Wo] = dy[:, :2 * Ho, :2 * Wo] + routed           # skip + 0 where nothing is routed, as the kernel
        return win.max(3), dy

    def reference(self, dtype, affine, skip):
        """F.max_pool2d and autograd through it in `dtype`, NHWC: pooled, dy, (sum dy, sum dy a_raw)."""
        a = _t(self.a, dtype)
        v = (a * _t(self.scale, dtype) + _t(self.shift, dtype)) if affine else a.clone()
        v = v.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        p = F.max_pool2d(v, 2, 2)
        (dy,) = torch.autograd.grad(p, v, _t(self.g, dtype).permute(0, 3, 1, 2).contiguous())
        dy = dy.permute(0, 2, 3, 1)
        if skip:
            dy = dy + _t(self.skip, dtype)
        return {"pooled": p.detach().permute(0, 2, 3, 1).numpy(), "dy": dy.numpy(),
                "bstats": torch.stack([dy.sum((0, 1, 2)), (dy * a).sum((0, 1, 2))]).numpy()}

    def fwd(self, affine):
        from atomai_amd import _lib as L
        d = self.d
        y = _nan(self.device, self.N, self.H // 2, self.W // 2, self.Cs)
        L.call("amx_pool2x2_fwd", L.ptr(d["a"]), L.ptr(d["scale"] if affine else None), L.ptr(d["shift"] if affine else None),
               L.ptr(y), self.N, self.H, self.W, self.Cs, L.stream_ptr(y))
        return _host(y)

    def bwd(self, affine, skip, bstats):
        from atomai_amd import _lib as L
        d = self.d
        rows = L.load().amx_pool2x2_bwd_rows(self.N, self.H, self.W, self.Cs)
        numel = self.N * self.H * self.W * self.Cs               # (NaN guard behind dy: two image rows)
        flat = _nan(self.device, numel + 2 * (self.W + 2) * self.Cs)
        dy = flat[:numel].view(self.N, self.H, self.W, self.Cs)
        bs = _nan(self.device, rows, 2, self.Cs) if bstats else None
        L.call("amx_pool2x2_bwd", L.ptr(d["g"]), L.ptr(d["a"]), L.ptr(d["scale"] if affine else None),
               L.ptr(d["shift"] if affine else None), L.ptr(d["skip"] if skip else None), L.ptr(dy), L.ptr(bs),
               self.N, self.H, self.W, self.Cs, L.stream_ptr(dy))
        assert bool(torch.isnan(flat[numel:]).all()), "amx_pool2x2_bwd wrote behind dy"
        return _host(dy), (_host(bs) if bstats else None)


def _pool_rows_rule(N, H, W, Cs):
    return min((N * ((H + 1) // 2) * ((W + 1) // 2) * (Cs // 4) + 255) // 256, 2048)


def check_pool_case(name, device, combos=None):
    from atomai_amd import _lib as L
    nhwc = POOL_SECOND_TRIP if name == "second_trip" else POOL_CASES[name]
    N, H, W, Cs = nhwc
    G = Cs // 4
    p = Pool(device, nhwc)
    assert L.load().amx_pool2x2_bwd_rows(N, H, W, Cs) == _pool_rows_rule(N, H, W, Cs)
    if name == "second_trip":
        assert N * ((H + 1) // 2) * ((W + 1) // 2) * G > 2048 * 256
    else:                                                        # the draw holds what it is meant to hold
        win = p.windows(True)
        top2 = np.sort(win, 3)[:, :, :, 2:]
        assert (top2[:, :, :, 0] == top2[:, :, :, 1]).any(), "no tie for the maximum in any window"
    can_bstats = 256 % G == 0 and G <= 128
    if combos is None:
        combos = [(af, sk, bs) for af in (True, False) for sk in (True, False) for bs in ((False, True) if can_bstats else (False,))]
    for affine in sorted({c[0] for c in combos}):
        y = p.fwd(affine)
        _finite(name, pooled=y)
        want, _ = p.restate(affine, False)
        assert _bits_equal(y, want), (name, "pooled", affine)
        r64, r32 = p.reference(torch.float64, affine, False), p.reference(torch.float32, affine, False)
        _compare("pool2x2_fwd", name, f"pooled affine={affine}", y, r64["pooled"], r32["pooled"])
    first = True
    for affine, skip, bstats in combos:
        tag = f"affine={affine} skip={skip} bstats={bstats}"
        dy, bs = p.bwd(affine, skip, bstats)
        _finite(name, dy=dy)
        _, want = p.restate(affine, skip)
        assert _bits_equal(dy, want), (name, "dy", tag, float(np.abs(dy - want).max()))
        if H & 1:                                                # the odd last row / column gets the skip gradient only
            assert _bits_equal(dy[:, H - 1], p.skip[:, H - 1] if skip else np.zeros_like(dy[:, H - 1])), (name, tag)
        if W & 1:
            assert _bits_equal(dy[:, :, W - 1], p.skip[:, :, W - 1] if skip else np.zeros_like(dy[:, :, W - 1])), (name, tag)
        r64, r32 = p.reference(torch.float64, affine, skip), p.reference(torch.float32, affine, skip)
        _compare("pool2x2_bwd", name, f"dy {tag}", dy, r64["dy"], r32["dy"])
        if bstats:
            _finite(name, bstats=bs)
            _compare("pool2x2_bwd", name, f"bstats {tag}", bs.astype(np.float64).sum(0), r64["bstats"], r32["bstats"])
        if first:                                                # fixed-order reductions: bit-identical when repeated
            dy2, bs2 = p.bwd(affine, skip, bstats)
            assert _bits_equal(dy, dy2) and (bs is None or _bits_equal(bs, bs2)), (name, tag)
            first = False
    if not can_bstats:                                           # G = 5, 13: a thread would not keep its channel group
        d = p.d
        dy, bs = _nan(device, N, H, W, Cs), _nan(device, _pool_rows_rule(N, H, W, Cs), 2, Cs)
        with pytest.raises(L.AmxError):
            L.call("amx_pool2x2_bwd", L.ptr(d["g"]), L.ptr(d["a"]), L.ptr(d["scale"]), L.ptr(d["shift"]), L.ptr(d["skip"]),
                   L.ptr(dy), L.ptr(bs), N, H, W, Cs, L.stream_ptr(dy))
        assert bool(torch.isnan(dy).all()) and bool(torch.isnan(bs).all())


def check_pool_engine_fallback(device, Cout=18, shape=(2, 3, 6, 10)):
    """ConvBlock -> max_pool2d on ONE tape, training step at Cs = 20 (G = 5): amx_pool2x2_bwd cannot emit the BatchNorm-backward
    sums, engine.PoolNode.backward must leave them to amx_bn_bwd_reduce, and dgamma / dbeta (and every other gradient) must
    still be those of the same layers in fp64 torch."""
    import copy
    from atomai_amd import engine, _lib as L
    from atomai_amd.nets import ConvBlock
    from atomai_amd.nets._function import run_tape
    torch.manual_seed(3)
    rs = np.random.RandomState(3)
    blk = ConvBlock(2, 1, shape[1], Cout, batch_norm=True)
    with torch.no_grad():
        bn = blk.block[2]
        sign = np.where(rs.rand(Cout) < 0.4, -1.0, 1.0)
        sign[0] = -1.0
        bn.weight.copy_(torch.from_numpy((sign * (0.5 + rs.rand(Cout))).astype(f32)))
        bn.bias.copy_(torch.from_numpy((0.3 * rs.randn(Cout)).astype(f32)))
    refs = {dt: copy.deepcopy(blk).to(dt) for dt in (torch.float64, torch.float32)}
    x = torch.from_numpy(rs.randn(*shape).astype(f32))
    gy = torch.from_numpy(rs.randn(shape[0], Cout, shape[2] // 2, shape[3] // 2).astype(f32))
    out = {}
    for dt, m in refs.items():
        xr = x.clone().to(dt).requires_grad_(True)
        conv, act, bnr = m.block[0], m.block[1], m.block[2]
        pre = F.conv2d(xr, conv.weight, conv.bias, padding=1)
        if dt == torch.float64:                                  # fp64 is a yardstick only away from the kink and from ties
            assert float(pre.detach().abs().min()) > 1e-5
        z = F.batch_norm(F.leaky_relu(pre, act.negative_slope), None, None, bnr.weight, bnr.bias, True, 0.1, bnr.eps)
        if dt == torch.float64:
            w = z.detach().unfold(2, 2, 2).unfold(3, 2, 2).reshape(*z.shape[:2], shape[2] // 2, shape[3] // 2, 4)
            top = w.sort(-1).values
            assert float((top[..., 3] - top[..., 2]).min()) > 1e-5
        y = F.max_pool2d(z, 2, 2)
        y.backward(gy.to(dt))
        out[dt] = dict(y=y.detach(), x=xr.grad, **{k: p.grad for k, p in m.named_parameters()})
    blk.to(device).train()
    calls = []
    orig = L.call

    def spy(name, *a):
        calls.append((name, a))
        return orig(name, *a)

    def build(tape, xin):
        node, act = blk._emit_input(tape, xin)
        return node, tape.output(tape.pool(act))
    xd = x.clone().to(device).requires_grad_(True)
    L.call = spy
    engine.L.call = spy
    try:
        y = run_tape(build, xd, list(blk.parameters()), True)
        y.backward(gy.to(device))
    finally:
        L.call = orig
        engine.L.call = orig
    names = [c[0] for c in calls]
    assert "amx_pool2x2_bwd" in names and "amx_bn_bwd_reduce" in names, names
    pb = [a for n, a in calls if n == "amx_pool2x2_bwd"][0]
    assert not pb[6].value, "bstats must be NULL at G = 5"        # (the 7th argument)
    got = dict(y=y.detach(), x=xd.grad, **{k: p.grad for k, p in blk.named_parameters()})
    r64, r32 = out[torch.float64], out[torch.float32]
    for k in got:
        _compare("engine.PoolNode(G=5)", "convblock_pool", k, _host(got[k]), r64[k].numpy(), r32[k].numpy())


# ================================================================ 2. pool backward + first-layer weight gradient
WG1_SHAPES = ((2, 6, 10), (1, 34, 18), (3, 2, 2))
WG1_GROUPS = (1, 2, 4, 8, 16)
SLOPE = 0.01


def _wg1_reference(p, dtype, affine, skip, k):
    """dy by the fp64 routing of case 1, then S1 = sum lrelu'(a) dy x_t, S2 = sum lrelu'(a) a x_t, S3 = sum lrelu'(a) x_t over
    the zero-padded 3x3 patches of x (t = 9: x_t = 1), as the header comment of pool_bwd_wgrad1_kernel defines them."""
    r = p.reference(dtype, affine, skip)
    a, dy = _t(p.a, dtype), _t(r["dy"], dtype)
    lp = torch.where(a > 0, torch.ones((), dtype=dtype), torch.full((), SLOPE, dtype=dtype))
    xp = F.pad(_t(p.x, dtype), (1, 1, 1, 1))
    H, W = p.H, p.W
    X = torch.stack([xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)] + [torch.ones_like(_t(p.x, dtype))])
    S = torch.stack([torch.einsum("tnhw,nhwc->tc", X, u) for u in (lp * dy, lp * a, lp)])            # [3][10][Cs]
    out = {"bstats": r["bstats"], "S": S.numpy(), "S1": S[0].numpy()}
    if k is not None:
        kk = _t(k, dtype)
        out["combined"] = (kk[0] * S[0] + kk[1] * S[1] + kk[2] * S[2]).numpy()
    return out


def check_pool_wgrad1(shape, G, device):
    from atomai_amd import _lib as L
    N, H, W = shape
    Cs = 4 * G
    p = Pool(device, (N, H, W, Cs), seed=G + H)
    p.a[p.a == 0.5] = 0.0                                        # exact zeros at the LeakyReLU test (lrelu'(0) = slope)
    p.d["a"] = _dev(p.a, device)
    assert (p.a == 0).any()
    rs = np.random.RandomState(11)
    k = rs.randn(3, Cs).astype(f32)
    kd = _dev(k, device)
    assert L.load().amx_pool2x2_bwd_wgrad1_supported(H, W, Cs, 1) == 1
    rows = L.load().amx_pool2x2_bwd_rows(N, H, W, Cs)
    d = p.d
    for affine, skip in ((True, True), (False, False), (True, False)):
        tag = f"{N}x{H}x{W} G={G} affine={affine} skip={skip}"
        outs = []
        for _ in range(2):
            bs, part3 = _nan(device, rows, 2, Cs), _nan(device, rows, 3, 10, Cs)
            L.call("amx_pool2x2_bwd_wgrad1", L.ptr(d["g"]), L.ptr(d["a"]), L.ptr(d["scale"] if affine else None),
                   L.ptr(d["shift"] if affine else None), L.ptr(d["skip"] if skip else None), L.ptr(d["x"]), SLOPE,
                   L.ptr(bs), L.ptr(part3), N, H, W, Cs, L.stream_ptr(bs))
            tot, tot1 = _nan(device, 10, Cs), _nan(device, 10, Cs)
            L.call("amx_conv1_wgrad_combine", L.ptr(part3), rows, Cs, L.ptr(kd[0]), L.ptr(kd[1]), L.ptr(kd[2]), L.ptr(tot),
                   L.stream_ptr(bs))
            L.call("amx_conv1_wgrad_combine", L.ptr(part3), rows, Cs, None, None, None, L.ptr(tot1), L.stream_ptr(bs))
            outs.append([_host(t) for t in (bs, part3, tot, tot1)])
        for u, v in zip(*outs):
            assert _bits_equal(u, v), tag
        bs, part3, tot, tot1 = outs[0]
        _finite(tag, bstats=bs, part3=part3, combined=tot, S1=tot1)
        r64, r32 = (_wg1_reference(p, dt, affine, skip, k) for dt in (torch.float64, torch.float32))
        got = {"bstats": bs.astype(np.float64).sum(0), "S": part3.astype(np.float64).sum(0), "combined": tot, "S1": tot1}
        for what, v in got.items():
            _compare("pool2x2_bwd_wgrad1", tag, what, v, r64[what], r32[what])
        # without k1..k3 the combine kernel returns S1: the fp64 sum of the rows in order, rounded once
        s1 = np.zeros((10, Cs))
        for r_ in range(rows):
            s1 += part3[r_, 0].astype(np.float64)
        assert _bits_equal(tot1, s1.astype(f32)), tag


def check_pool_wgrad1_domain(device):
    """amx_pool2x2_bwd_wgrad1_supported against its documented domain (even H and W, dilation 1, G a power of two <= 16), and
    the entry point refuses what it does not support."""
    from atomai_amd import _lib as L
    lib = L.load()
    for (H, W, Cs, dil), want in (((6, 10, 16, 1), 1), ((2, 2, 4, 1), 1), ((6, 10, 64, 1), 1), ((7, 10, 16, 1), 0),
                                  ((6, 9, 16, 1), 0), ((6, 10, 128, 1), 0), ((6, 10, 12, 1), 0), ((6, 10, 16, 2), 0),
                                  ((6, 10, 6, 1), 0), ((0, 10, 16, 1), 0)):
        assert lib.amx_pool2x2_bwd_wgrad1_supported(H, W, Cs, dil) == want, (H, W, Cs, dil)
    for H, W, Cs in ((7, 10, 16), (6, 9, 16), (6, 10, 128), (6, 10, 12)):
        p = Pool(device, (1, H, W, Cs), ties=False)
        rows = max(lib.amx_pool2x2_bwd_rows(1, H, W, Cs), 1)
        bs, part3 = _nan(device, rows, 2, Cs), _nan(device, rows, 3, 10, Cs)
        d = p.d
        with pytest.raises(L.AmxError):
            L.call("amx_pool2x2_bwd_wgrad1", L.ptr(d["g"]), L.ptr(d["a"]), L.ptr(d["scale"]), L.ptr(d["shift"]), L.ptr(d["skip"]),
                   L.ptr(d["x"]), SLOPE, L.ptr(bs), L.ptr(part3), 1, H, W, Cs, L.stream_ptr(bs))
        assert bool(torch.isnan(bs).all()) and bool(torch.isnan(part3).all())


# ================================================================ 3. upsample backward
# name -> (N, h, w, Cs)
UP_CASES = {
    "g7_tx4_ty8_ragged_tiles_2x5x7": (2, 5, 7, 28),
    "every_clamp_at_once_1x1x1": (1, 1, 1, 4),
    "one_row_3x1x3": (3, 1, 3, 4),
    "g50_tx1_ty5_1x9x2": (1, 9, 2, 200),
    "g256_ty1_1x3x2": (1, 3, 2, 1024),
}


def check_upsample_bwd(name, device):
    from atomai_amd import _lib as L
    N, h, w, Cs = UP_CASES[name]
    rs = np.random.RandomState(5)
    du = rs.randn(N, 2 * h, 2 * w, Cs).astype(f32)
    dud = _dev(du, device)
    for mode, mname in ((0, "bilinear"), (1, "nearest")):
        outs = []
        for _ in range(2):
            dv = _nan(device, N, h, w, Cs)
            L.call("amx_upsample2x_bwd", L.ptr(dud), L.ptr(dv), N, h, w, Cs, mode, L.stream_ptr(dud))
            outs.append(_host(dv))
        assert _bits_equal(*outs), (name, mname)
        _finite(name, dv=outs[0])
        ref = {}
        for dt in (torch.float64, torch.float32):
            v = torch.zeros(N, Cs, h, w, dtype=dt, requires_grad=True)
            kw = {"align_corners": False} if mode == 0 else {}
            u = F.interpolate(v, scale_factor=2, mode=mname, **kw)
            u.backward(_t(du, dt).permute(0, 3, 1, 2).contiguous())
            ref[dt] = v.grad.permute(0, 2, 3, 1).numpy()
        _compare("upsample2x_bwd", name, mname, outs[0], ref[torch.float64], ref[torch.float32])


# ================================================================ 4. resize-and-concatenate
# name -> (h, w, H, W)
RESIZE_CASES = {
    "non_integer_ratio_5x3_to_22x13": (5, 3, 22, 13),
    "times_two_11x6_to_22x12": (11, 6, 22, 12),
    "one_pixel_1x1_to_4x7": (1, 1, 4, 7),
    "identity_7x9": (7, 9, 7, 9),
    "downscale_9x8_to_4x3": (9, 8, 4, 3),
}


def check_resize_cat(name, device, N=2, Cs=4, Cd=8):
    from atomai_amd import _lib as L
    h, w, H, W = RESIZE_CASES[name]
    rs = np.random.RandomState(9)
    for C in (1, 3):
        for coff in (0, 1, 5):
            for mode, mname in ((0, "bilinear"), (1, "nearest")):
                for affine in (True, False):
                    tag = f"C={C} coff={coff} {mname} affine={affine}"
                    dyadic = mode == 1                           # nearest copies fl32(fma(a, scale, shift)): exact when dyadic
                    src = np.full((N, h, w, Cs), np.nan, f32)    # the padding channels c >= C are never read
                    src[..., :C] = dyadic_act(rs, (N, h, w, C)) if dyadic else rs.randn(N, h, w, C)
                    sc, sh = draw_affine(rs, Cs, dyadic)
                    srcd, scd, shd = _dev(src, device), _dev(sc, device), _dev(sh, device)
                    dst = torch.full((N, H, W, Cd), SENTINEL, dtype=torch.float32, device=device)
                    L.call("amx_resize_cat_fwd", L.ptr(srcd), L.ptr(scd if affine else None), L.ptr(shd if affine else None),
                           N, h, w, Cs, C, L.ptr(dst), H, W, Cd, coff, mode, L.stream_ptr(dst))
                    got = _host(dst)
                    keep = np.ones(Cd, bool)
                    keep[coff:coff + C] = False
                    assert (got[..., keep] == SENTINEL).all(), (name, tag, "a channel outside the slice was written")
                    ref = {}
                    for dt in (torch.float64, torch.float32):
                        v = _t(src[..., :C], dt)
                        if affine:
                            v = v * _t(sc[:C], dt) + _t(sh[:C], dt)
                        kw = {"align_corners": False} if mode == 0 else {}
                        ref[dt] = F.interpolate(v.permute(0, 3, 1, 2).contiguous(), size=(H, W), mode=mname,
                                                **kw).permute(0, 2, 3, 1).numpy()
                    if mode == 1:                                # (ATen's nearest index rule is float32 arithmetic too)
                        assert _bits_equal(got[..., coff:coff + C], ref[torch.float32]), (name, tag)
                    else:
                        _compare("resize_cat_fwd", name, tag, got[..., coff:coff + C], ref[torch.float64], ref[torch.float32])
                    if affine:
                        continue                                 # the backward takes no affine: once per (C, coff, mode)
                    ddst = rs.randn(N, H, W, Cd).astype(f32)
                    dd = _dev(ddst, device)
                    outs = []
                    for _ in range(2):
                        dsrc = _nan(device, N, h, w, Cs)
                        L.call("amx_resize_cat_bwd", L.ptr(dd), N, H, W, Cd, coff, C, L.ptr(dsrc), h, w, Cs, mode,
                               L.stream_ptr(dd))
                        outs.append(_host(dsrc))
                    assert _bits_equal(*outs), (name, tag)
                    _finite(name, dsrc=outs[0])
                    assert not outs[0][..., C:].any(), (name, tag, "padded channels of dsrc must be 0")
                    for dt in (torch.float64, torch.float32):
                        v = torch.zeros(N, C, h, w, dtype=dt, requires_grad=True)
                        kw = {"align_corners": False} if mode == 0 else {}
                        F.interpolate(v, size=(H, W), mode=mname, **kw).backward(
                            _t(ddst[..., coff:coff + C], dt).permute(0, 3, 1, 2).contiguous())
                        ref[dt] = v.grad.permute(0, 2, 3, 1).numpy()
                    _compare("resize_cat_bwd", name, tag, outs[0][..., :C], ref[torch.float64], ref[torch.float32])


# ================================================================ 5. DilatedBlock sum
def _dilated_call(fn, device, a, sc, sh, n, slope, accumulate, wpre, wact, out, npix, Cs, whole_null=False):
    from atomai_amd import _lib as L
    PP = ctypes.c_void_p * 4
    pa = PP(*([t.data_ptr() for t in a[:n]] + [0] * (4 - n)))
    ps = PP(*[(t.data_ptr() if t is not None else 0) for t in sc])
    ph = PP(*[(t.data_ptr() if t is not None else 0) for t in sh])
    if whole_null:
        ps = ph = None
    if fn == "amx_dilated_sum":
        L.call(fn, pa, ps, ph, n, slope, accumulate, L.ptr(out), npix, Cs, L.stream_ptr(out))
    else:
        L.call(fn, pa, ps, ph, n, slope, accumulate, float(wpre), float(wact), L.ptr(out), npix, Cs, L.stream_ptr(out))


def check_dilated_sum(device, npix, Cs, ns=(1, 3, 4), tag=""):
    """out (+)= sum_i [ wpre pre_i + wact a_i + bn_i ], pre_i = a_i > 0 ? a_i : a_i / slope, bn_i = a_i scale_i + shift_i or
    nothing where scale_i is NULL (the formula of the kernel's comment) in fp64."""
    rs = np.random.RandomState(13)
    a = [rs.randn(npix, Cs).astype(f32) for _ in range(4)]
    aff = [draw_affine(rs, Cs, False) for _ in range(4)]
    out0 = rs.randn(npix, Cs).astype(f32)
    ad = [_dev(v, device) for v in a]
    scd, shd = [_dev(s, device) for s, _ in aff], [_dev(s, device) for _, s in aff]

    def ref(dt, n, slope, acc, wpre, wact, has):
        o = _t(out0, dt).clone() if acc else torch.zeros(npix, Cs, dtype=dt)
        for i in range(n):
            v = _t(a[i], dt)
            o = o + wpre * torch.where(v > 0, v, v / slope) + wact * v
            if has[i]:
                o = o + (v * _t(aff[i][0], dt) + _t(aff[i][1], dt))
        return o.numpy()
    for n in ns:
        for acc in (0, 1):
            for wpre, wact in ((1, 1), (2, 1), (1, 0)):
                for slope in (0.01, 1.0):
                    for pattern in ("mixed", "none"):
                        has = [pattern == "mixed" and i % 2 == 0 for i in range(4)]      # some scale[k] NULL inside one call
                        sc = [s if h_ else None for s, h_ in zip(scd, has)]
                        sh = [s if h_ else None for s, h_ in zip(shd, has)]
                        t = f"{tag}npix={npix} Cs={Cs} n={n} acc={acc} w=({wpre},{wact}) slope={slope} scales={pattern}"
                        outs = []
                        for fn in ("amx_dilated_sum_ex", "amx_dilated_sum_ex") + (("amx_dilated_sum",) if (wpre, wact) == (1, 1) else ()):
                            out = _dev(out0, device) if acc else _nan(device, npix, Cs)
                            _dilated_call(fn, device, ad, sc, sh, n, slope, acc, wpre, wact, out, npix, Cs,
                                          whole_null=(pattern == "none" and n == 3))
                            outs.append(_host(out))
                        for o in outs[1:]:                       # repeatable; amx_dilated_sum is the wpre = wact = 1 form
                            assert _bits_equal(outs[0], o), t
                        _finite(t, out=outs[0])
                        _compare("dilated_sum_ex", t, "out", outs[0], ref(torch.float64, n, slope, acc, wpre, wact, has),
                                 ref(torch.float32, n, slope, acc, wpre, wact, has))


# ================================================================ 6. residual-block passes
def _res_inputs(rs, npix, Cs):
    t = dyadic_act(rs, (npix, Cs))
    sc, sh = draw_affine(rs, Cs, True)
    r = dyadic_act(rs, (npix, Cs))
    g = rs.randn(npix, Cs).astype(f32)
    return t, sc, sh, r, g


def check_res_passes(device, npix, Cs, tag=""):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(17)
    t, sc, sh, r, g = _res_inputs(rs, npix, Cs)
    sh[1] = 0.0
    t[::3, 1] = 0.0                                                          # exact zeros at the sign test of lrelu_bwd
    td, scd, shd, gd = (_dev(v, device) for v in (t, sc, sh, g))
    for affine in (True, False):
        z0 = (t * sc + sh).astype(f32) if affine else t                      # exact
        rr = r.copy()
        m = rs.rand(npix, Cs) < 0.1
        m[0, 0] = True
        rr[m] = -z0[m]                                                       # exact zeros at the `> 0` test
        z = (z0 + rr).astype(f32)                                            # exact: multiples of 1/32 below 16
        assert (z == 0).any()
        rd = _dev(rr, device)
        for slope in (0.01, 0.2):
            tg = f"{tag}npix={npix} Cs={Cs} affine={affine} slope={slope}"
            outs = []
            for _ in range(2):
                y = _nan(device, npix, Cs)
                L.call("amx_res_out_fwd", L.ptr(td), L.ptr(scd if affine else None), L.ptr(shd if affine else None), L.ptr(rd),
                       slope, npix, Cs, L.ptr(y), L.stream_ptr(y))
                outs.append(_host(y))
            assert _bits_equal(*outs), tg
            want = np.where(z > 0, z, z * f32(slope)).astype(f32)
            assert _bits_equal(outs[0], want), (tg, "res_out")
            ref = {dt: F.leaky_relu(_t(z0, dt) + _t(rr, dt), slope).numpy() for dt in (torch.float64, torch.float32)}
            _compare("res_out_fwd", tg, "out", outs[0], ref[torch.float64], ref[torch.float32])
            # amx_lrelu_bwd: the sign of z = ref * scale + shift (ref alone without the affine)
            refin = t
            zz = (refin * sc + sh).astype(f32) if affine else refin
            assert (zz == 0).any()
            dwant = np.where(zz > 0, g, g * f32(slope)).astype(f32)
            refd = _dev(refin, device)
            for two in (True, False):
                din, din2 = _nan(device, npix, Cs), (_nan(device, npix, Cs) if two else None)
                L.call("amx_lrelu_bwd", L.ptr(gd), L.ptr(refd), L.ptr(scd if affine else None), L.ptr(shd if affine else None),
                       slope, npix, Cs, L.ptr(din), L.ptr(din2), L.stream_ptr(din))
                assert _bits_equal(_host(din), dwant), (tg, "din", two)
                if two:
                    assert _bits_equal(_host(din2), dwant), (tg, "din2")
            ref = {}
            for dt in (torch.float64, torch.float32):
                zt = _t(zz, dt).requires_grad_(True)
                F.leaky_relu(zt, slope).backward(_t(g, dt))
                ref[dt] = zt.grad.numpy()
            _compare("lrelu_bwd", tg, "din", _host(din), ref[torch.float64], ref[torch.float32])
            # the identity engine.ResOutNode.backward relies on: lrelu_bwd(ref = the block's OUTPUT, no affine) is the
            # gradient through leaky_relu at the pre-activation z (LeakyReLU keeps the sign)
            outd = _dev(outs[0], device)
            din = _nan(device, npix, Cs)
            L.call("amx_lrelu_bwd", L.ptr(gd), L.ptr(outd), None, None, slope, npix, Cs, L.ptr(din), None, L.stream_ptr(din))
            assert _bits_equal(_host(din), np.where(z > 0, g, g * f32(slope)).astype(f32)), (tg, "identity")


# ================================================================ 7. BatchNorm affine and backward chain
def check_bn_eval_affine(device):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(19)
    eps = 1e-5
    for Cs, C in ((4, 3), (20, 18), (68, 65), (256, 250)):
        gamma, beta = draw_affine(rs, C, False)
        rm = rs.randn(C).astype(f32)
        rv = (10.0 ** rs.uniform(-6, 1, C)).astype(f32)
        rv[1] = 1e-6
        dev = [_dev(v, device) for v in (gamma, beta, rm, rv)]
        scale, shift = _nan(device, Cs), _nan(device, Cs)
        L.call("amx_bn_eval_affine", *[L.ptr(v) for v in dev], eps, C, Cs, L.ptr(scale), L.ptr(shift), L.stream_ptr(scale))
        scale, shift = _host(scale), _host(shift)
        _finite(f"Cs={Cs}", scale=scale, shift=shift)
        assert not scale[C:].any() and not shift[C:].any(), "padded channels normalise to exactly 0"
        ref = {}
        for dt in (torch.float64, torch.float32):
            g_, b_, m_, v_ = (_t(v, dt) for v in (gamma, beta, rm, rv))
            s = g_ / torch.sqrt(v_ + eps)
            ref[dt] = (s.numpy(), (b_ - m_ * s).numpy())
        _compare("bn_eval_affine", f"Cs={Cs} C={C}", "scale", scale[:C], ref[torch.float64][0], ref[torch.float32][0])
        _compare("bn_eval_affine", f"Cs={Cs} C={C}", "shift", shift[:C], ref[torch.float64][1], ref[torch.float32][1])


# name -> (npix, Cs, C)
BN_CASES = {
    "fewer_pixels_than_lanes_15_c3": (15, 4, 3),
    "exactly_one_block_1024_g4": (1024, 16, 16),
    "second_block_of_one_pixel_1025_g4": (1025, 16, 16),
    "pl51_one_idle_thread_ragged_u_3219_g5": (3219, 20, 18),
    "pl19_nine_idle_threads_2146_g13": (2146, 52, 50),
    "pl4_1100_g64": (1100, 256, 250),
    "pl1_1030_g256": (1030, 1024, 1024),
}
BN_EPS = 1e-5


class BnChain:
    def __init__(self, device, npix, Cs, C, seed=23):
        rs = np.random.RandomState(seed)
        self.device, self.npix, self.Cs, self.C = device, npix, Cs, C
        pad = lambda v: np.concatenate([v, np.zeros((npix, Cs - C), f32)], 1)
        # dyadic activations (the lrelu' factor compares a with 0), uniform over [-4, 4]: |mean| <= std in every channel, so
        # the cancellation in sdya - mean * sdy is the reference's problem as much as the kernel's
        self.a = pad(dyadic_act(rs, (npix, C), zero_frac=0.05))
        self.dy = pad(rs.randn(npix, C).astype(f32))
        self.gx = pad(rs.randn(npix, C).astype(f32))
        self.gamma, self.beta = draw_affine(rs, C, False)
        a64 = self.a[:, :C].astype(np.float64)
        assert (np.abs(a64.mean(0)) <= a64.std(0)).all()
        self.mean = np.zeros(Cs, f32)
        self.invstd = np.zeros(Cs, f32)
        self.mean[:C] = a64.mean(0)
        self.invstd[:C] = 1.0 / np.sqrt(a64.var(0) + BN_EPS)
        self.d = {k: _dev(getattr(self, k), device) for k in ("a", "dy", "gx", "gamma", "mean", "invstd")}

    def run(self, gx, bn):
        """engine.ConvNode._bn_bwd_sums + _materialise_dpre: reduce -> finalize -> apply -> reduce_rows."""
        from atomai_amd import _lib as L
        d, npix, Cs, C, dev = self.d, self.npix, self.Cs, self.C, self.device
        sp = L.stream_ptr(d["a"])
        rows = L.load().amx_rows_for(npix)
        o = {}
        kk = (None, None, None)
        if bn:
            o["part"] = _nan(dev, rows, 2, Cs)
            L.call("amx_bn_bwd_reduce", L.ptr(d["dy"]), L.ptr(d["a"]), npix, Cs, L.ptr(o["part"]), sp)
            o["dgamma"], o["dbeta"], o["k"] = _nan(dev, C), _nan(dev, C), _nan(dev, 3, Cs)
            k = o["k"]
            L.call("amx_bn_bwd_finalize", L.ptr(o["part"]), rows, Cs, Cs, C, npix, L.ptr(d["gamma"]), L.ptr(d["mean"]),
                   L.ptr(d["invstd"]), L.ptr(o["dgamma"]), L.ptr(o["dbeta"]), L.ptr(k[0]), L.ptr(k[1]), L.ptr(k[2]), sp)
            kk = (L.ptr(k[0]), L.ptr(k[1]), L.ptr(k[2]))
        o["dpre"], o["bias_part"] = _nan(dev, npix, Cs), _nan(dev, rows, Cs)
        L.call("amx_bn_bwd_apply", L.ptr(d["dy"]), L.ptr(d["a"]), L.ptr(d["gx"] if gx else None), *kk, SLOPE, npix, Cs,
               L.ptr(o["dpre"]), L.ptr(o["bias_part"]), sp)
        o["db"] = _nan(dev, C)
        L.call("amx_reduce_rows", L.ptr(o["bias_part"]), rows, Cs, C, 1.0, L.ptr(o["db"]), sp)
        return {k: _host(v) for k, v in o.items()}

    def reference(self, dt, gx, bn):
        """Autograd of F.batch_norm(F.leaky_relu(pre), training=True) with pre = a > 0 ? a : a / slope; a DilatedBlock's extra
        gradient gx reaches pre directly and (under a BatchNorm, where the activation is a summed sub-layer of its own)
        through the activation as well: dpre = gx + lrelu'(a) (gx + d bn).  Without a BatchNorm: dpre = gx + lrelu'(a) dy."""
        C = self.C
        a, dy, g_ = (_t(getattr(self, k)[:, :C], dt) for k in ("a", "dy", "gx"))
        pre = torch.where(a > 0, a, a / SLOPE).requires_grad_(True)
        act = F.leaky_relu(pre, SLOPE)
        gamma, beta = _t(self.gamma, dt).requires_grad_(True), _t(self.beta, dt).requires_grad_(True)
        if bn:
            y = F.batch_norm(act.t().reshape(1, C, -1), None, None, gamma, beta, True, 0.1, BN_EPS).reshape(C, -1).t()
            loss = (y * dy).sum()
            if gx:
                loss = loss + (g_ * (pre + act)).sum()
        else:
            loss = (act * dy).sum()
            if gx:
                loss = loss + (g_ * pre).sum()
        loss.backward()
        r = {"dpre": pre.grad.numpy(), "db": pre.grad.sum(0).numpy()}
        if bn:
            r["dgamma"], r["dbeta"] = gamma.grad.numpy(), beta.grad.numpy()
        return r


def check_bn_chain(name, device):
    npix, Cs, C = BN_CASES[name]
    b = BnChain(device, npix, Cs, C)
    assert (b.a[:, :C] == 0).any()
    first = True
    for bn in (True, False):
        for gx in (True, False):
            tag = f"bn={bn} gx={gx}"
            o = b.run(gx, bn)
            _finite(name, **o)
            assert not o["dpre"][:, C:].any(), (name, tag, "padded channels of dpre")
            if bn:
                assert not o["k"][:, C:].any(), (name, tag, "k1..k3 of the padded channels")
            r64, r32 = b.reference(torch.float64, gx, bn), b.reference(torch.float32, gx, bn)
            for what in r64:
                got = o[what][:, :C] if what == "dpre" else o[what]
                _compare("bn_bwd_chain" if bn else "bn_bwd_apply(no bn)", name, f"{what} {tag}", got, r64[what], r32[what])
            if not bn and not gx:                                # dpre = lrelu'(a) dy: one rounding
                want = np.where(b.a > 0, b.dy, b.dy * f32(SLOPE)).astype(f32)
                assert _bits_equal(o["dpre"], want), (name, tag)
            if first:
                again = b.run(gx, bn)
                for k_, v in o.items():
                    assert _bits_equal(v, again[k_]), (name, tag, k_)
                first = False


def check_rows_rule(device):
    """amx_rows_for / amx_rows_pix against pick_ppb's rule: 1024 pixels per row, doubled until at most 4096 rows."""
    from atomai_amd import _lib as L
    lib = L.load()
    for npix in (1, 1024, 1025, 4096 * 1024, 4096 * 1024 + 1, 3 * 4096 * 1024 + 5):
        ppb = 1024
        while (npix + ppb - 1) // ppb > 4096:
            ppb *= 2
        assert (lib.amx_rows_for(npix), lib.amx_rows_pix(npix)) == ((npix + ppb - 1) // ppb, ppb), npix
    assert (lib.amx_rows_for(4096 * 1024 + 1), lib.amx_rows_pix(4096 * 1024 + 1)) == (2049, 2048)


# ================================================================ 8. layout and copies
LAYOUT_CASES = ((2, 3, 4, 5, 7), (1, 50, 52, 3, 2), (3, 8, 8, 1, 1))      # (N, C, Cs, H, W)


def check_layout(device, cases=LAYOUT_CASES):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(29)
    for N, C, Cs, H, W in cases:
        x = rs.randn(N, C, H, W).astype(f32)
        xd = _dev(x, device)
        t = _nan(device, N, H, W, Cs)
        L.call("amx_nchw_to_nhwc", L.ptr(xd), L.ptr(t), N, C, Cs, H, W, L.stream_ptr(xd))
        th = _host(t)
        assert _bits_equal(th[..., :C], x.transpose(0, 2, 3, 1)), (N, C, Cs, H, W)
        assert not th[..., C:].any() and np.isfinite(th).all(), "the padding is zero"
        src = np.full((N, H, W, Cs), np.nan, f32)                # the padding is not read on the way back
        src[..., :C] = rs.randn(N, H, W, C)
        back = _nan(device, N, C, H, W)
        L.call("amx_nhwc_to_nchw", L.ptr(_dev(src, device)), L.ptr(back), N, C, Cs, H, W, L.stream_ptr(back))
        assert _bits_equal(_host(back), src[..., :C].transpose(0, 3, 1, 2)), (N, C, Cs, H, W)
        rt = _nan(device, N, C, H, W)
        L.call("amx_nhwc_to_nchw", L.ptr(t), L.ptr(rt), N, C, Cs, H, W, L.stream_ptr(rt))
        assert _bits_equal(_host(rt), x), "round trip"


def check_add_inplace(device, ns=(4, 1028)):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(31)
    for n in ns:
        a, b = rs.randn(n).astype(f32), rs.randn(n).astype(f32)
        ad, bd = _dev(a, device), _dev(b, device)
        L.call("amx_add_inplace", L.ptr(ad), L.ptr(bd), n, L.stream_ptr(ad))
        assert _bits_equal(_host(ad), a + b), n
        assert _bits_equal(_host(bd), b), n


def check_copy16(device):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(37)
    for nbytes, max_wgs in ((16, 128), (4112, 128), (1 << 20, 3)):           # 1 MiB on 3 workgroups: a grid-stride loop
        src = rs.randn(nbytes // 4).astype(f32)
        sd, dd = _dev(src, device), _nan(device, nbytes // 4 + 4)
        L.call("amx_copy16", L.ptr(sd), L.ptr(dd), nbytes, max_wgs, L.stream_ptr(sd))
        got = _host(dd)
        assert _bits_equal(got[:nbytes // 4], src) and np.isnan(got[nbytes // 4:]).all(), nbytes


# ================================================================ argument checks: refused before anything is launched
REFUSALS = [(fn, why) for fn, whys in (
    ("amx_pool2x2_fwd", ("Cs6", "H1", "shift")),
    ("amx_pool2x2_bwd", ("Cs6", "W1", "shift", "bstats_g256")),
    ("amx_pool2x2_bwd_wgrad1", ("shift", "no_bstats")),
    ("amx_conv1_wgrad_combine", ("k2", "rows0")),
    ("amx_upsample2x_bwd", ("Cs1028", "Cs6", "mode2", "h0")),
    ("amx_dilated_sum_ex", ("n0", "n5", "slope0", "Cs6")),
    ("amx_dilated_sum", ("n0", "n5", "slope0")),
    ("amx_res_out_fwd", ("Cs6", "shift", "npix0")),
    ("amx_lrelu_bwd", ("Cs6", "shift", "npix0")),
    ("amx_resize_cat_fwd", ("C5", "coff", "mode2", "shift", "h0")),
    ("amx_resize_cat_bwd", ("C5", "coff", "mode2", "H0")),
    ("amx_bn_eval_affine", ("Cs_lt_C", "no_rv")),
    ("amx_bn_bwd_reduce", ("Cs1028", "Cs6", "npix0")),
    ("amx_bn_bwd_finalize", ("stride", "no_k3")),
    ("amx_bn_bwd_apply", ("Cs1028", "k2", "npix0")),
    ("amx_nchw_to_nhwc", ("Cs_lt_C", "Cs6")),
    ("amx_nhwc_to_nchw", ("Cs_lt_C", "Cs6")),
    ("amx_add_inplace", ("n6", "n0")),
    ("amx_copy16", ("nbytes24", "src_misaligned", "dst_misaligned", "wgs0"))) for why in whys]


def check_refusal(fn, why, device):
    """Every AMX_BADARG branch of the pass kernels' entry points: the unmodified call is accepted, the modified one raises
    AmxError and leaves every (valid, NaN-filled) output buffer untouched."""
    from atomai_amd import _lib as L
    rs = np.random.RandomState(41)
    N, H, W, Cs, C = 1, 4, 6, 8, 5
    npix = N * H * W
    big = 1028 if "1028" in why or why == "bstats_g256" else Cs              # buffers large enough for the refused geometry
    rnd = lambda *s: _dev(rs.randn(*s), device)
    a, g, skip, x = rnd(N, H, W, big), rnd(N, H // 2, W // 2, big), rnd(N, H, W, big), rnd(N, H, W)
    sc, sh = rnd(big), rnd(big)
    hi = rnd(N, 2 * H, 2 * W, big)
    kd = rnd(3, big)
    PP = ctypes.c_void_p * 4
    PP5 = ctypes.c_void_p * 5

    def outs():
        return {"y": _nan(device, N, 2 * H, 2 * W, big), "y2": _nan(device, N, H, W, big), "bs": _nan(device, 8, 2, big),
                "part3": _nan(device, 8, 3, 10, big), "v": _nan(device, 16, big), "v2": _nan(device, 4, big)}

    def args(o, w):
        sp = L.stream_ptr(a)
        P = L.ptr
        m = lambda key, val, dflt: val if w == key else dflt
        if fn == "amx_pool2x2_fwd":
            return (P(a), P(sc), m("shift", None, P(sh)), P(o["y"]), N, m("H1", 1, H), W, m("Cs6", 6, Cs), sp)
        if fn == "amx_pool2x2_bwd":
            bst = P(o["bs"]) if w == "bstats_g256" else None
            return (P(g), P(a), P(sc), m("shift", None, P(sh)), P(skip), P(o["y2"]), bst, N, H, m("W1", 1, W),
                    m("bstats_g256", 1024, m("Cs6", 6, Cs)), sp)
        if fn == "amx_pool2x2_bwd_wgrad1":
            return (P(g), P(a), P(sc), m("shift", None, P(sh)), P(skip), P(x), SLOPE, m("no_bstats", None, P(o["bs"])),
                    P(o["part3"]), N, H, W, Cs, sp)
        if fn == "amx_conv1_wgrad_combine":
            p3 = rnd(2, 3, 10, Cs)
            return (P(p3), m("rows0", 0, 2), Cs, P(kd[0]), m("k2", None, P(kd[1])), P(kd[2]), P(o["v"]), sp)
        if fn == "amx_upsample2x_bwd":
            return (P(hi), P(o["y2"]), N, m("h0", 0, H), W, m("Cs1028", 1028, m("Cs6", 6, Cs)), m("mode2", 2, 0), sp)
        if fn in ("amx_dilated_sum_ex", "amx_dilated_sum"):
            n = m("n0", 0, m("n5", 5, 2))
            pa = PP5(*[a.data_ptr()] * 5)
            ps, ph = PP5(*[sc.data_ptr()] * 5), PP5(*[sh.data_ptr()] * 5)
            head = (pa, ps, ph, n, m("slope0", 0.0, SLOPE), 0)
            tail = (P(o["y2"]), npix, m("Cs6", 6, Cs), sp)
            return head + ((1.0, 1.0) if fn == "amx_dilated_sum_ex" else ()) + tail
        if fn == "amx_res_out_fwd":
            return (P(a), P(sc), m("shift", None, P(sh)), P(skip), SLOPE, m("npix0", 0, npix), m("Cs6", 6, Cs), P(o["y2"]), sp)
        if fn == "amx_lrelu_bwd":
            return (P(skip), P(a), P(sc), m("shift", None, P(sh)), SLOPE, m("npix0", 0, npix), m("Cs6", 6, Cs), P(o["y2"]),
                    P(o["y"]), sp)
        if fn == "amx_resize_cat_fwd":                           # dst [N][2H][2W][Cs], slice [coff, coff + C)
            return (P(a), P(sc), m("shift", None, P(sh)), N, m("h0", 0, H), W, Cs, m("C5", Cs + 1, 3), P(o["y"]), 2 * H, 2 * W,
                    Cs, m("coff", Cs - 2, 1), m("mode2", 2, 0), sp)
        if fn == "amx_resize_cat_bwd":
            return (P(hi), N, m("H0", 0, 2 * H), 2 * W, Cs, m("coff", Cs - 2, 1), m("C5", Cs + 1, 3), P(o["y2"]), H, W, Cs,
                    m("mode2", 2, 0), sp)
        if fn == "amx_bn_eval_affine":
            rv = _dev(rs.rand(Cs) + 0.5, device)
            return (P(sc), P(sh), P(kd[0]), m("no_rv", None, P(rv)), 1e-5, m("Cs_lt_C", Cs + 1, C), Cs, P(o["v"]), P(o["v2"]), sp)
        if fn == "amx_bn_bwd_reduce":
            return (P(skip), P(a), m("npix0", 0, npix), m("Cs1028", 1028, m("Cs6", 6, Cs)), P(o["bs"]), sp)
        if fn == "amx_bn_bwd_finalize":
            part = rnd(2, 2, Cs)
            k = o["v"]
            return (P(part), 2, m("stride", C - 1, Cs), Cs, C, npix, P(sc), P(sh), P(kd[0]), P(o["v2"][0]), P(o["v2"][1]),
                    P(k[0]), P(k[1]), m("no_k3", None, P(k[2])), sp)
        if fn == "amx_bn_bwd_apply":
            return (P(skip), P(a), None, P(kd[0]), m("k2", None, P(kd[1])), P(kd[2]), SLOPE, m("npix0", 0, npix),
                    m("Cs1028", 1028, Cs), P(o["y2"]), P(o["bs"]), sp)
        if fn == "amx_nchw_to_nhwc":
            return (P(x), P(o["y2"]), N, m("Cs_lt_C", Cs + 1, 1), m("Cs6", 6, Cs), H, W, sp)
        if fn == "amx_nhwc_to_nchw":
            return (P(a), P(o["y2"]), N, m("Cs_lt_C", Cs + 1, C), m("Cs6", 6, Cs), H, W, sp)
        if fn == "amx_add_inplace":
            return (P(o["y2"]), P(a), m("n6", 6, m("n0", 0, 8)), sp)
        if fn == "amx_copy16":
            src = ctypes.c_void_p(a.data_ptr() + (4 if w == "src_misaligned" else 0))
            dst = ctypes.c_void_p(o["y2"].data_ptr() + (4 if w == "dst_misaligned" else 0))
            return (src, dst, m("nbytes24", 24, 32), m("wgs0", 0, 4), sp)
        raise KeyError(fn)
    o = outs()
    if fn == "amx_add_inplace":
        o["y2"].zero_()
    L.call(fn, *args(o, None))                                   # the unmodified call is accepted
    o = outs()
    with pytest.raises(L.AmxError):
        L.call(fn, *args(o, why))
    for k, v in o.items():
        assert bool(torch.isnan(v).all()), (fn, why, k)


# ================================================================ 9. the second grid-stride trip of the capped launches
def _second_trip_elems(cap, per):
    """Smallest multiple of `per` float4 / scalar slots that exceeds cap x 256 by about three workgroups."""
    return -(-(cap * 256 + 3 * 256) // per)


def check_second_trip(kernel, device):
    """One case per capped launch at the smallest element count past its block cap, Cs = 12 (G = 3 divides no power of two, so
    the channel group of a slot changes from trip to trip)."""
    from atomai_amd import _lib as L
    rs = np.random.RandomState(43)
    Cs, G = 12, 3
    if kernel == "pool2x2_fwd":
        Ho, Wo = _second_trip_elems(16384, G), 1
        assert 16384 * 256 < Ho * Wo * G < 16384 * 256 + 5 * 256
        a = dyadic_act(rs, (1, 2 * Ho, 2 * Wo, Cs))
        sc, sh = draw_affine(rs, Cs, True)
        y = _nan(device, 1, Ho, Wo, Cs)
        ad = _dev(a, device)
        L.call("amx_pool2x2_fwd", L.ptr(ad), L.ptr(_dev(sc, device)), L.ptr(_dev(sh, device)), L.ptr(y), 1, 2 * Ho, 2 * Wo, Cs,
               L.stream_ptr(y))
        v = (a * sc + sh).astype(f32)
        want = v.reshape(1, Ho, 2, Wo, 2, Cs).max((2, 4))
        assert _bits_equal(_host(y), want)
        return
    if kernel in ("dilated_sum_ex", "res_out_fwd", "lrelu_bwd", "affine_nhwc", "add_inplace"):
        cap = {"affine_nhwc": 8192, "add_inplace": 8192}.get(kernel, 16384)
        npix = _second_trip_elems(cap, G)
        assert npix * G > cap * 256 and npix * G < cap * 256 + 5 * 256
        if kernel in ("res_out_fwd", "lrelu_bwd"):
            check_res_passes_once(device, npix, Cs, kernel)
        elif kernel == "dilated_sum_ex":
            check_dilated_sum_once(device, npix, Cs)
        elif kernel == "add_inplace":
            check_add_inplace(device, ns=(npix * Cs,))
        else:
            a = rs.randn(npix, Cs).astype(f32)
            sc, sh = draw_affine(rs, Cs, False)
            y = _nan(device, npix, Cs)
            ad = _dev(a, device)
            L.call("amx_affine_nhwc", L.ptr(ad), L.ptr(_dev(sc, device)), L.ptr(_dev(sh, device)), L.ptr(y), npix, Cs,
                   L.stream_ptr(y))
            ref = {dt: (_t(a, dt) * _t(sc, dt) + _t(sh, dt)).numpy() for dt in (torch.float64, torch.float32)}
            got = _host(y)
            _finite(kernel, y=got)
            _compare("affine_nhwc", "second_trip", "y", got, ref[torch.float64], ref[torch.float32])
        return
    if kernel == "nchw_to_nhwc":
        hw = _second_trip_elems(4096, Cs)
        check_layout_one(device, 1, 10, Cs, 2, -(-hw // 2), to_nhwc=True)
        return
    if kernel == "nhwc_to_nchw":
        hw = _second_trip_elems(4096, 10)
        check_layout_one(device, 1, 10, Cs, 2, -(-hw // 2), to_nhwc=False)
        return
    raise KeyError(kernel)


SECOND_TRIP = ("pool2x2_fwd", "dilated_sum_ex", "res_out_fwd", "lrelu_bwd", "affine_nhwc", "add_inplace", "nchw_to_nhwc",
               "nhwc_to_nchw")


def check_res_passes_once(device, npix, Cs, kernel):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(47)
    t, sc, sh, r, g = _res_inputs(rs, npix, Cs)
    td, scd, shd = _dev(t, device), _dev(sc, device), _dev(sh, device)
    slope = 0.01
    if kernel == "res_out_fwd":
        z = ((t * sc + sh).astype(f32) + r).astype(f32)
        y = _nan(device, npix, Cs)
        L.call("amx_res_out_fwd", L.ptr(td), L.ptr(scd), L.ptr(shd), L.ptr(_dev(r, device)), slope, npix, Cs, L.ptr(y),
               L.stream_ptr(y))
        assert _bits_equal(_host(y), np.where(z > 0, z, z * f32(slope)).astype(f32))
    else:
        z = (t * sc + sh).astype(f32)
        din = _nan(device, npix, Cs)
        L.call("amx_lrelu_bwd", L.ptr(_dev(g, device)), L.ptr(td), L.ptr(scd), L.ptr(shd), slope, npix, Cs, L.ptr(din), None,
               L.stream_ptr(din))
        assert _bits_equal(_host(din), np.where(z > 0, g, g * f32(slope)).astype(f32))


def check_dilated_sum_once(device, npix, Cs):
    rs = np.random.RandomState(53)
    a = rs.randn(npix, Cs).astype(f32)
    sc, sh = draw_affine(rs, Cs, False)
    ad, scd, shd = _dev(a, device), _dev(sc, device), _dev(sh, device)
    out = _nan(device, npix, Cs)
    _dilated_call("amx_dilated_sum_ex", device, [ad], [scd, None, None, None], [shd, None, None, None], 1, 0.01, 0, 1.0, 1.0, out,
                  npix, Cs)
    ref = {}
    for dt in (torch.float64, torch.float32):
        v = _t(a, dt)
        ref[dt] = (torch.where(v > 0, v, v / 0.01) + v + (v * _t(sc, dt) + _t(sh, dt))).numpy()
    got = _host(out)
    _finite("dilated_sum_ex second_trip", out=got)
    _compare("dilated_sum_ex", "second_trip", "out", got, ref[torch.float64], ref[torch.float32])


def check_layout_one(device, N, C, Cs, H, W, to_nhwc):
    from atomai_amd import _lib as L
    rs = np.random.RandomState(59)
    if to_nhwc:
        assert N * H * W * Cs > 4096 * 256
        x = rs.randn(N, C, H, W).astype(f32)
        t = _nan(device, N, H, W, Cs)
        xd = _dev(x, device)
        L.call("amx_nchw_to_nhwc", L.ptr(xd), L.ptr(t), N, C, Cs, H, W, L.stream_ptr(xd))
        th = _host(t)
        assert _bits_equal(th[..., :C], x.transpose(0, 2, 3, 1)) and not th[..., C:].any()
    else:
        assert N * C * H * W > 4096 * 256
        src = np.full((N, H, W, Cs), np.nan, f32)
        src[..., :C] = rs.randn(N, H, W, C)
        back = _nan(device, N, C, H, W)
        L.call("amx_nhwc_to_nchw", L.ptr(_dev(src, device)), L.ptr(back), N, C, Cs, H, W, L.stream_ptr(back))
        assert _bits_equal(_host(back), src[..., :C].transpose(0, 3, 1, 2))


# ================================================================ 10. one training step with trained BatchNorm state
# model -> (nb_filters, nb_classes)
TRAINED_NETS = {"Unet": (4, 3), "SegResNet": (4, 3), "dilnet": (5, 1)}
TRAINED_SHAPE = (2, 1, 24, 40)


class _PoolProbe:
    """Stands in for torch.nn.functional inside oracle.seg_oracle: records, for every F.max_pool2d, the smallest gap between
    the two largest values of a 2x2 window."""

    def __init__(self, gaps):
        self._gaps = gaps

    def __getattr__(self, name):
        return getattr(F, name)

    def max_pool2d(self, x, k, s):
        n, c, h, w = x.shape
        win = x.detach()[:, :, :h // 2 * 2, :w // 2 * 2].unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, h // 2, w // 2, 4)
        top = win.sort(-1).values
        self._gaps.append(float((top[..., 3] - top[..., 2]).min()))
        return F.max_pool2d(x, k, s)


def min_pool_gap(model, sd, x):
    """Smallest gap between the two largest values of any 2x2 pooling window of a training-mode forward of the oracle."""
    from oracle import seg_oracle as so
    gaps = []
    so.F = _PoolProbe(gaps)
    try:
        with torch.no_grad():
            so.net_forward(model, so.cast(sd, x.dtype), x, True)
    finally:
        so.F = F
    return min(gaps)


def _trained_problem(model, seed):
    """init_fcnn_model, then a BatchNorm state as training leaves it: about half of every weight negative, biases off 0,
    running statistics off (0, 1)."""
    from atomai_amd.nets import init_fcnn_model
    nf, ncls = TRAINED_NETS[model]
    torch.manual_seed(seed)
    net, _ = init_fcnn_model(model, ncls, nb_filters=nf)
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
                m.weight.mul_(torch.from_numpy((sign * (0.5 + rs.rand(n))).astype(f32)))
                m.bias.add_(torch.from_numpy((0.3 * rs.randn(n)).astype(f32)))
                m.running_mean.add_(torch.from_numpy((0.2 * rs.randn(n)).astype(f32)))
                m.running_var.mul_(torch.from_numpy((0.5 + rs.rand(n)).astype(f32)))
    B, _, H, W = TRAINED_SHAPE
    x = torch.from_numpy(rs.rand(*TRAINED_SHAPE).astype(f32))
    y = (torch.from_numpy(rs.randint(0, ncls, (B, H, W))) if ncls > 1
         else torch.from_numpy((rs.rand(B, 1, H, W) > 0.5).astype(f32)))
    return net, x, y


def trained_margins(model, seed):
    """(smallest |LeakyReLU input|, smallest pool-window gap) of the float64 oracle alone."""
    from oracle import seg_oracle as so
    net, x, _ = _trained_problem(model, seed)
    sd = OrderedDict((k, v.clone().double()) for k, v in net.state_dict().items())
    return so.min_abs_preactivation(model, OrderedDict(sd), x.double()), min_pool_gap(model, OrderedDict(sd), x.double())


def find_trained_seed(model, limit=200):
    """The rule behind TRAINED_SEED (not run by the suite): the smallest seed at which the float64 oracle is a yardstick for an
    fp32 evaluation — every LeakyReLU input farther than 1e-5 from 0 (check_vs_oracle_small's guard) and, in every 2x2 pooling
    window, the two largest values more than 1e-5 apart.  It looks at the oracle alone, never at the kernels."""
    for seed in range(limit):
        kink, gap = trained_margins(model, seed)
        if kink > 1e-5 and gap > 1e-5:
            return seed
    raise AssertionError("no seed below the limit")


TRAINED_SEED = {"Unet": 2, "SegResNet": 0, "dilnet": 2}                 # = find_trained_seed(model)


def check_trained_bn_step(model, device):
    """check_vs_oracle_small with its tolerances on a non-square input and a trained BatchNorm state: negative scales reach
    the arg-max of pool_bwd_kernel, the sign test of lrelu_bwd and the loaders of resize / dilated-sum in TRAINING mode."""
    from oracle import seg_oracle as so
    from atomai_amd.losses_metrics import select_loss
    nf, ncls = TRAINED_NETS[model]
    seed = TRAINED_SEED[model]
    kink, gap = trained_margins(model, seed)
    print(f"pass trained {model} seed {seed}: smallest |LeakyReLU input| {kink:.3e}, smallest pool-window gap {gap:.3e}")
    assert kink > 1e-5 and gap > 1e-5, (model, seed, kink, gap)
    net, x, y = _trained_problem(model, seed)
    sd = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    assert any(bool((v < 0).any()) for k, v in sd.items() if k.endswith(".weight") and v.ndim == 1)
    net.to(device).train()
    logits = net(x.to(device))
    loss = select_loss("ce", ncls)(logits, y.to(device))
    loss.backward()
    y64 = y if ncls > 1 else y.double()
    ref_loss, ref_logits, ref_grads = so.loss_and_grads(model, so.cast(sd, torch.float64), x.double(), y64, ncls)
    from _seg_checks import relmax
    lrel = relmax(_host(logits), ref_logits.numpy())
    print(f"pass trained {model}: logits rel {lrel:.2e}, loss {loss.item():.8f} (fp64 {float(ref_loss):.8f})")
    assert lrel < REL_TOL
    assert abs(loss.item() - float(ref_loss)) / abs(float(ref_loss)) < 1e-5
    gmax = max(float(g.abs().max()) for g in ref_grads.values())
    worst = 0.0
    for k, p in net.named_parameters():
        err = float((p.grad.cpu().double() - ref_grads[k]).abs().max()) / gmax
        worst = max(worst, err)
        assert err < 2e-5, (model, k, err)
    print(f"pass trained {model}: worst gradient error {worst:.2e} of gmax")
