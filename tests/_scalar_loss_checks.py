"""Shared bodies of the scalar-loss and IoU kernel tests (csrc/head.hip: ce_fwd_bwd_kernel, ce_fwd_bwd_generic_kernel,
bce_fwd_bwd_kernel, scale_unless_one_kernel, iou_hist_kernel, iou_hist_generic_kernel) through their wrappers
(losses_metrics/losses.py: CrossEntropyLoss, BCEWithLogitsLoss; metrics.py: IoU) against fp64 torch / a numpy restatement of
the reference (atomai/losses_metrics/metrics.py:16-95), at the shapes where such kernels go wrong: HW below, at and
beyond one workgroup, grid strides that cross image boundaries (LOSS_BLOCKS 3 and 1), the last register-resident and the
first generic class count, saturating logits, no gradient requested, several blocks per image, more classes than the
privatised histogram holds, labels out of range.

Bound of the losses (the project's rule, _seg_checks.check_net_case): an error is within max(4 x floor, 2e-6), the floor being
the error of stock torch in fp32 against fp64 on the same input.  The loss error is relative; the gradient error is divided
by max |dlogits_ref|.  The IoU histograms are integers and are compared exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

BLOCKS = (4096, 3, 1)                     # losses.LOSS_BLOCKS: the product default; 3 and 1: every thread takes several pixels
TOL = 2e-6                                # (the figure of _seg_checks.check_loss_upstream_gradient)
FLT_MIN = 1.1754944e-38


def _with_blocks(nblk, fn):
    from atomai_amd.losses_metrics import losses
    old = losses.LOSS_BLOCKS[0]
    losses.LOSS_BLOCKS[0] = nblk
    try:
        return fn()
    finally:
        losses.LOSS_BLOCKS[0] = old


def _reference(fn, x, t, up=1.0):
    """(loss fp64, dlogits fp64, fp32 floor of the loss (relative), fp32 floor of dlogits (/ max |dlogits|)) of stock torch."""
    out = []
    for dt in (torch.float64, torch.float32):
        xr = x.detach().clone().to(dt).requires_grad_(True)
        loss = fn(xr, t if t.dtype == torch.int64 else t.to(dt))
        (loss * up).backward()
        out.append((float(loss.detach().double()), xr.grad.double().numpy()))
    (l64, g64), (l32, g32) = out
    return l64, g64, abs(l32 - l64) / abs(l64), np.abs(g32 - g64).max() / np.abs(g64).max()


def _run(crit, x, t, device, up=1.0, grad=True):
    xd = x.detach().clone().to(device).requires_grad_(grad)
    loss = crit(xd, t.to(device))
    if grad:
        (loss * up).backward() if up != 1.0 else loss.backward()
    return loss.detach().cpu(), (xd.grad.cpu() if grad else None)


def _check_against_fp64(tag, crit, ref, x, t, device, up=1.0):
    """One (input, LOSS_BLOCKS) point: value and gradient within the bound, shape and dtype of the loss, the dx == nullptr
    path (no_grad and requires_grad=False) bit-equal to the training loss, two calls bit-identical, everything finite."""
    l64, g64, lfloor, gfloor = ref
    loss, grad = _run(crit, x, t, device, up)
    lerr = abs(float(loss.double()) - l64) / abs(l64)
    gerr = np.abs(grad.double().numpy() - g64).max() / np.abs(g64).max()
    print(f"{tag}: loss {float(loss):.9g} (fp64 {l64:.9g}) rel {lerr:.2e} (fp32 floor {lfloor:.2e}); dlogits error "
          f"{gerr:.2e} (fp32 floor {gfloor:.2e})")
    assert loss.shape == () and loss.dtype == torch.float32, tag
    assert grad.shape == x.shape and grad.dtype == torch.float32, tag
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), tag
    assert lerr <= max(4 * lfloor, TOL), (tag, lerr, lfloor)
    assert gerr <= max(4 * gfloor, TOL), (tag, gerr, gfloor)
    with torch.no_grad():
        ev = crit(x.clone().to(device).requires_grad_(True), t.to(device)).cpu()
    frozen, none = _run(crit, x, t, device, grad=False)
    assert none is None
    assert ev.shape == () and ev.dtype == torch.float32 and not ev.requires_grad, tag
    assert torch.equal(ev, loss) and torch.equal(frozen, loss), (tag, float(ev), float(frozen), float(loss))
    loss2, grad2 = _run(crit, x, t, device, up)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad), tag
    return loss, grad


# ------------------------------------------------------------------------------------------------ cross entropy
# (N, K, H, W): K = 2 (never built by select_loss), 8 = MAXCLS (last register-resident count), 9 (first generic count), 11;
# HW = 3 (one wave spans five images), HW = 256 (exactly one workgroup), HW = 257 (one pixel into the second)
CE_SHAPES = [(3, 2, 7, 37), (2, 8, 9, 31), (2, 9, 5, 13), (1, 11, 33, 17), (5, 3, 1, 3), (2, 3, 16, 16), (1, 4, 1, 257)]
CE_SATURATED = [(2, 8, 9, 31), (2, 9, 5, 13), (1, 11, 33, 17), (3, 2, 7, 37)]      # both kernels (K <= 8 and K > 8)
BIG = 1e4


def ce_case_ids():
    return ["x".join(map(str, s)) for s in CE_SHAPES]


def ce_inputs(shape, kind):
    """Logits `scale * randn` and targets that cover every class.  kind 'sat' overwrites the first six pixels (image 0) with
    the fixed saturating block: one logit at +1e4 and the rest at -1e4 with the target on the large logit (first and last
    class) and off it (twice), all logits equal (0, and +1e4)."""
    N, K, H, W = shape
    rs = np.random.RandomState(1000 * K + N * H * W)
    scale = {"randn1": 1.0, "randn30": 30.0, "sat": 1.0}[kind]
    x = (scale * rs.randn(N, K, H, W)).astype(np.float32)
    t = rs.randint(0, K, (N, H, W))
    npix = N * H * W
    first = 0
    if kind == "sat":
        first = 6
        xf, tf = x.reshape(N, K, H * W), t.reshape(N, H * W)
        for p, (hot, tgt) in enumerate([(0, 0), (K - 1, K - 1), (1, 0), (K - 1, K - 2)]):
            xf[0, :, p] = -BIG
            xf[0, hot, p] = BIG
            tf[0, p] = tgt
        xf[0, :, 4], tf[0, 4] = 0.0, K - 1
        xf[0, :, 5], tf[0, 5] = BIG, 0
    where = first + rs.permutation(npix - first)[:K]
    t.reshape(-1)[where] = np.arange(K)
    assert set(t.reshape(-1).tolist()) == set(range(K))
    return torch.from_numpy(x), torch.from_numpy(t)


def check_ce_vs_fp64(shape, device):
    from atomai_amd.losses_metrics.losses import CrossEntropyLoss
    crit = CrossEntropyLoss()
    kinds = ["randn1", "randn30"] + (["sat"] if shape in CE_SATURATED else [])
    for kind in kinds:
        x, t = ce_inputs(shape, kind)
        ref = _reference(F.cross_entropy, x, t)
        for nblk in BLOCKS:
            _with_blocks(nblk, lambda: _check_against_fp64(f"ce {shape} {kind} blocks {nblk}", crit, ref, x, t, device))


def check_ce_saturated_pixels(device):
    """The fixed block alone, pixel by pixel (N = 6 images of one pixel): 0 where the target is on the +1e4 logit, 2e4
    where it is off, log K where all logits are equal; the gradient one-hot differences, never NaN."""
    from atomai_amd.losses_metrics.losses import CrossEntropyLoss
    for K in (2, 8, 9):
        x, t = ce_inputs((2, K, 1, 20), "sat")
        x, t = x[0, :, 0, :6].t().reshape(6, K, 1, 1).contiguous(), t[0, 0, :6].reshape(6, 1, 1).contiguous()
        ref = F.cross_entropy(x.double(), t, reduction="none").reshape(6)
        assert ref.tolist()[:4] == [0.0, 0.0, 2 * BIG, 2 * BIG]
        for p in range(6):
            loss, grad = _run(CrossEntropyLoss(), x[p:p + 1], t[p:p + 1], device)
            want = float(ref[p])
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), (K, p)
            assert abs(float(loss) - want) <= 2e-6 * want, (K, p, float(loss), want)
            xr = x[p:p + 1].double().requires_grad_(True)
            F.cross_entropy(xr, t[p:p + 1]).backward()
            assert np.abs(grad.double().numpy() - xr.grad.numpy()).max() <= TOL, (K, p)


def check_ce_wrapper(device):
    """A permuted NHWC view and a sliced target give what their contiguous copies give; wrong targets raise ValueError."""
    from atomai_amd.losses_metrics.losses import CrossEntropyLoss
    crit = CrossEntropyLoss()
    for shape in ((2, 3, 5, 7), (2, 9, 5, 7)):
        x, t = ce_inputs(shape, "randn1")
        N, K, H, W = shape
        loss0, grad0 = _run(crit, x, t, device)
        nhwc = x.permute(0, 2, 3, 1).contiguous().to(device)
        wide = torch.full((N, H, 2 * W + 1), K + 5, dtype=torch.int64)
        wide[:, :, 1::2] = t
        view = nhwc.permute(0, 3, 1, 2).requires_grad_(True)
        tview = wide.to(device)[:, :, 1::2]
        assert not view.is_contiguous() and not tview.is_contiguous()
        loss1 = crit(view, tview)
        loss1.backward()
        assert torch.equal(loss1.detach().cpu(), loss0)
        assert view.grad.shape == x.shape and torch.equal(view.grad.cpu(), grad0)
    xd, td = x.to(device), t.to(device)
    for bad in (td.int(), td.float(), td.bool()):
        with pytest.raises(ValueError):
            crit(xd, bad)
    for bad in (td[:, :-1], td[:1], td.unsqueeze(1), td.reshape(N, W, H), td.reshape(-1)):
        with pytest.raises(ValueError):
            crit(xd, bad)


def check_ce_abi_rejects(device):
    """amx_ce_fwd_bwd refuses K = 1 (BCE's case) and rows = 0 before anything is launched."""
    from atomai_amd import _lib as L
    x, t = ce_inputs((2, 3, 4, 5), "randn1")
    x, t = x.to(device), t.to(device)
    part = torch.zeros(4, dtype=torch.float32, device=device)
    sp = L.stream_ptr(x)
    L.call("amx_ce_fwd_bwd", L.ptr(x), L.ptr(t), L.ptr(None), L.ptr(part), 1, 2, 3, 20, sp)        # (the valid call)
    with pytest.raises(L.AmxError):
        L.call("amx_ce_fwd_bwd", L.ptr(x), L.ptr(t), L.ptr(None), L.ptr(part), 1, 2, 1, 20, sp)
    with pytest.raises(L.AmxError):
        L.call("amx_ce_fwd_bwd", L.ptr(x), L.ptr(t), L.ptr(None), L.ptr(part), 0, 2, 3, 20, sp)


# ------------------------------------------------------------------------------------------------ BCE with logits
BCE_SHAPES = [(1,), (255,), (256,), (257,), (3, 33, 9)]
BCE_FIXED = [0.0, 1e-8, -1e-8, 17.0, -17.0, 40.0, -40.0, 88.7, -88.7, 100.0, -100.0, 1e4, -1e4]
BCE_BIG = 4096 * 256 + 5                # the smallest size at which the default LOSS_BLOCKS makes a second grid-stride pass


def bce_case_ids():
    return ["x".join(map(str, s)) for s in BCE_SHAPES]


def bce_inputs(shape, kind):
    n = int(np.prod(shape))
    rs = np.random.RandomState(7 * n + 1)
    t = (rs.rand(*shape) > 0.5).astype(np.float32)
    if kind == "confident":              # x = 20 (2t - 1): mean loss log1p(e^-20) = 2.06e-9, which logf(1 + e) returns as 0
        x = 20.0 * (2.0 * t - 1.0)
    else:
        x = {"randn1": 1.0, "randn40": 40.0}[kind] * rs.randn(*shape)
        soft = rs.rand(*shape) < 0.25    # (a quarter of the targets strictly inside (0, 1))
        t = np.where(soft, rs.rand(*shape), t).astype(np.float32)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(t)


def bce_exact(x, t):
    """(per-element loss, sigmoid(x) - t) in fp64 by the cancellation-free forms max(x, 0) - x t + log1p(e^-|x|) and
    1 / (1 + e^-x) | e^x / (1 + e^x).  Stock torch's own fp64 loss, (1 - t) x - logsigmoid(x), cancels where |x| is large
    and the loss small (x = -40, t = 0 gives 0 instead of 4.25e-18), and its fp32 floor there is 50 % and more."""
    x, t = x.double().numpy(), t.double().numpy()
    e = np.exp(-np.abs(x))
    return np.maximum(x, 0) - x * t + np.log1p(e), np.where(x >= 0, 1 / (1 + e), e / (1 + e)) - t


def check_bce_vs_fp64(shape, device):
    """The rule of the module against stock torch, and, because the fp32 floor of stock torch is about 0.5 for the loss and
    1.0 for the gradient of the 'confident' input (see bce_exact), which would let any loss between 0 and 3 x the truth
    pass: the loss within TOL of the cancellation-free fp64 value too, and the gradient within TOL of it on the scale of
    its range (dlogits = (sigmoid - t) / n lies in [-1 / n, 1 / n], and fp32 resolves sigmoid to 6e-8)."""
    from atomai_amd.losses_metrics.losses import BCEWithLogitsLoss
    crit = BCEWithLogitsLoss()
    n = int(np.prod(shape))
    for kind in ("randn1", "randn40", "confident"):
        x, t = bce_inputs(shape, kind)
        ref = _reference(F.binary_cross_entropy_with_logits, x, t)
        le, ge = bce_exact(x, t)
        exact = float(le.mean())
        if kind == "confident":
            assert abs(exact - np.log1p(np.exp(-20.0))) < 1e-9 * exact
        for nblk in BLOCKS:
            tag = f"bce {shape} {kind} blocks {nblk}"
            loss, grad = _with_blocks(nblk, lambda: _check_against_fp64(tag, crit, ref, x, t, device))
            lerr = abs(float(loss.double()) - exact) / exact
            gerr = np.abs(grad.double().numpy() * n - ge).max()
            print(f"{tag}: against the cancellation-free fp64 forms: loss rel {lerr:.2e}, n * dlogits error {gerr:.2e}")
            assert lerr <= TOL, (tag, float(loss), exact)
            assert gerr <= TOL, (tag, gerr)


def check_bce_fixed_vector(device):
    """0, +-1e-8, +-17 (where 1 + e^-x rounds to 1 in fp32), +-40, +-88.7 (the edge of expf's range), +-100, +-1e4 against
    targets 0, 1 and 0.3: the whole vector under the rule of the module, then element by element (each alone, so that the
    1e4 terms cannot hide the small ones) against bce_exact: the loss to TOL relative (none of the elements cancels in the
    kernel's form: x - x t is exact for t = 0 and 1 and far from 0 for t = 0.3), the gradient to TOL of its range 1, and
    relative to itself where t = 0 (e / (1 + e) does not cancel).  A result below fp32's normal range (log1p(e^-x) of
    x = 88.7, 100, 1e4) may be flushed: the format resolves it to FLT_MIN at best."""
    from atomai_amd.losses_metrics.losses import BCEWithLogitsLoss
    crit = BCEWithLogitsLoss()
    x = torch.tensor(BCE_FIXED * 3, dtype=torch.float32)
    t = torch.tensor([0.0] * 13 + [1.0] * 13 + [0.3] * 13, dtype=torch.float32)
    ref = _reference(F.binary_cross_entropy_with_logits, x, t)
    for nblk in BLOCKS:
        _with_blocks(nblk, lambda: _check_against_fp64(f"bce fixed vector blocks {nblk}", crit, ref, x, t, device))
    le, ge = bce_exact(x, t)
    worst = (0.0, 0.0, 0.0)
    for i in range(x.numel()):
        xi, ti = x[i:i + 1], t[i:i + 1]
        loss, grad = _run(crit, xi, ti, device)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), (float(xi), float(ti))
        lerr = abs(float(loss.double()) - le[i])
        gerr = abs(float(grad.double()) - ge[i])
        if le[i] >= FLT_MIN:
            worst = max(worst, (lerr / le[i], float(xi), float(ti)))
        assert lerr <= max(TOL * le[i], FLT_MIN), (float(xi), float(ti), float(loss), le[i])
        assert gerr <= TOL, (float(xi), float(ti), float(grad), ge[i])
        if float(ti) == 0.0:
            assert gerr <= max(TOL * abs(ge[i]), FLT_MIN), (float(xi), float(grad), ge[i])
    print("bce fixed vector, element by element: worst loss rel %.2e at x = %g, t = %g" % worst)


def check_bce_target_dtypes(device):
    """bool and int64 targets are cast by the wrapper: the result of the same targets in fp32, bit for bit."""
    from atomai_amd.losses_metrics.losses import BCEWithLogitsLoss
    crit = BCEWithLogitsLoss()
    x, t = bce_inputs((3, 33, 9), "confident")
    x = x + torch.from_numpy(np.random.RandomState(5).randn(3, 33, 9).astype(np.float32))
    loss0, grad0 = _run(crit, x, t, device)
    for cast in (torch.bool, torch.int64):
        loss1, grad1 = _run(crit, x, t.to(cast), device)
        assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0), cast
    with pytest.raises(ValueError):
        crit(x.to(device), t.to(device)[:2])


def check_bce_second_pass(device):
    """4096 * 256 + 5 elements at the default LOSS_BLOCKS, upstream gradient 0.37: five threads of bce_fwd_bwd_kernel and of
    scale_unless_one_kernel take a second element; the last five gradients are compared on their own as well."""
    from atomai_amd.losses_metrics import losses
    assert losses.LOSS_BLOCKS[0] == 4096, "this check is about the product default"
    crit = losses.BCEWithLogitsLoss()
    rs = np.random.RandomState(11)
    x = (3.0 * rs.randn(BCE_BIG)).astype(np.float32)
    x[-5:] = [0.5, -0.5, 2.0, -2.0, 0.0]                             # (the second pass: gradients that are not small)
    x = torch.from_numpy(x)
    t = torch.from_numpy((rs.rand(BCE_BIG) > 0.5).astype(np.float32))
    l64, g64, lfloor, gfloor = _reference(F.binary_cross_entropy_with_logits, x, t, up=0.37)
    loss, grad = _run(crit, x, t, device, up=0.37)
    lerr = abs(float(loss.double()) - l64) / abs(l64)
    err = np.abs(grad.double().numpy() - g64) / np.abs(g64).max()
    print(f"bce {BCE_BIG} upstream 0.37: loss {float(loss):.9g} (fp64 {l64:.9g}) rel {lerr:.2e} (fp32 floor {lfloor:.2e}); "
          f"dlogits error {err.max():.2e}, last five {err[-5:].max():.2e} (fp32 floor {gfloor:.2e})")
    assert loss.shape == () and loss.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    assert lerr <= max(4 * lfloor, TOL), (lerr, lfloor)
    assert err.max() <= max(4 * gfloor, TOL), (err.max(), gfloor)
    frozen, _ = _run(crit, x, t, device, grad=False)
    assert torch.equal(frozen, loss)


# ------------------------------------------------------------------------------------------------ IoU histograms
MARGIN = 1e-4                             # |p - thresh| of every probability of every pixel, in fp64
# name: (N, K, H, W, thresh, activation, truth)
IOU_CASES = {
    "two_blocks_per_image": (2, 3, 70, 61, .5, 1, "int"),          # HW = 4270 > 4096: two blocks add into one histogram
    "binary_float_truth": (1, 1, 66, 65, .5, 1, "float"),
    "binary_int_truth": (1, 1, 66, 65, .5, 1, "int"),
    "two_classes": (2, 2, 9, 11, .5, 1, "int"),
    "eight_classes": (2, 8, 20, 24, .2, 1, "int"),                 # MAXCLS, class sums above K - 1 are clipped to 0
    "nine_classes_probabilities": (2, 9, 66, 65, .2, 0, "int"),    # generic kernel, two blocks per image
    "k32_privatised": (1, 32, 12, 12, .05, 1, "int"),              # last K whose counts are privatised in LDS
    "k33_global_atomics": (1, 33, 12, 12, .05, 1, "int"),          # first K on global atomics only
    "k40_global_atomics": (1, 40, 10, 12, .03, 1, "int"),
    "k33_two_images": (2, 33, 6, 11, .05, 1, "int"),               # a label K of image 0 must not land in image 1's counts
    "binary_probabilities": (2, 1, 17, 19, .6, 0, "float"),
}


def _probabilities64(x, K, activation):
    x = torch.from_numpy(x).double()
    if not activation:
        return x.numpy()
    return (torch.softmax(x, 1) if K > 1 else torch.sigmoid(x)).numpy()


def iou_inputs(name):
    """(pred fp32 (N,K,H,W), truth) of one case.  Exact equality of integer counts is a fair demand only away from the
    threshold (the device's expf may differ from the host's in the last bits): every pixel one of whose probabilities, in
    fp64, lies within MARGIN of the threshold is replaced by a fixed safe vector, and none may remain."""
    N, K, H, W, thresh, activation, truth = IOU_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    # logits of scale 2 (several classes above a low threshold: class sums, clipped ones among them) and, pixel by
    # pixel, of scale 8 (one class dominates: every class occurs as a prediction)
    sharp = np.where(rs.rand(N, 1, H, W) < 0.5, 2.0, 8.0)
    if activation:
        x = (sharp * rs.randn(N, K, H, W)).astype(np.float32)
        safe = np.zeros(K, np.float32)
        safe[K // 2] = 8.0                                    # softmax: 0.987 .. 0.9996 there, below 3.4e-4 elsewhere; sigmoid .9997
    elif K > 1:
        x = torch.softmax(torch.from_numpy(sharp * rs.randn(N, K, H, W)), 1).numpy().astype(np.float32)
        safe = np.full(K, 0.1 / (K - 1), np.float32)
        safe[K // 2] = 0.9
    else:
        x = rs.rand(N, K, H, W).astype(np.float32)
        safe = np.full(K, 0.9, np.float32)
    near = (np.abs(_probabilities64(x, K, activation) - thresh) < MARGIN).any(1)          # (N,H,W)
    x = np.where(near[:, None], safe[None, :, None, None], x).astype(np.float32)
    assert not (np.abs(_probabilities64(x, K, activation) - thresh) < MARGIN).any(), name
    Kc = max(K, 2)
    if truth == "int":
        t = rs.randint(0, Kc, (N, H, W))
        flat = t.reshape(N, -1)
        for n in range(N):                                    # labels outside [0, Kc) are skipped (metrics.py:74)
            flat[n, 3 + n:11 + n] = [-1, Kc, Kc + 3, -7, -1, Kc, Kc + 3, -7]
    else:
        t = rs.randint(0, 2, (N, 1, H, W)).astype(np.float32)
        flat = t.reshape(N, -1)
        for n in range(N):                                    # .long() truncates: 0, 1, 0 (-0.5 -> 0), 2 (skipped)
            flat[n, 5 + n:13 + n] = [0.9, 1.7, -0.5, 2.0, 0.9, 1.7, -0.5, 2.0]
    return torch.from_numpy(x), torch.from_numpy(t)


def iou_reference_hist(pred, true, thresh, activation):
    """The reference's IoU.__init__ + compute_hist (metrics.py:16-79) per image, in numpy: fp32 softmax / sigmoid on the
    host, p > thresh (cv2.threshold THRESH_BINARY on an fp32 image), sum_k k [p_k > thresh] with sums above K - 1 set to 0
    (squeeze_channels(clip=True)), labels truncated by .long(), a Kc x Kc count over the labels in [0, Kc).
    Returns (hist int64 (N,Kc,Kc), number of pixels whose class sum was clipped)."""
    N, K = pred.shape[:2]
    p = pred.float().cpu()
    if activation:
        p = torch.softmax(p, 1) if K > 1 else torch.sigmoid(p)
    above = p.numpy() > np.float32(thresh)
    cls = (above * np.arange(K).reshape(1, K, 1, 1)).sum(1) if K > 1 else above[:, 0].astype(np.int64)
    clipped = int((cls > K - 1).sum()) if K > 1 else 0
    if K > 1:
        cls[cls > K - 1] = 0
    Kc = max(K, 2)
    lab = true.cpu().numpy().astype(np.int64).reshape(N, -1)          # (astype truncates toward zero, as .long() does)
    cls = cls.reshape(N, -1)
    hist = np.zeros((N, Kc, Kc), np.int64)
    for n in range(N):
        ok = (lab[n] >= 0) & (lab[n] < Kc)
        np.add.at(hist[n], (lab[n][ok], cls[n][ok]), 1)
    return hist, clipped


def _jaccard64(hist):
    total = hist.sum(0).astype(np.float64)
    inter = np.diag(total)
    jcd = inter / (total.sum(1) + total.sum(0) - inter + 1e-10)
    return float(jcd[~np.isnan(jcd)].mean())


def check_iou_hist(name, device):
    from atomai_amd.losses_metrics import IoU
    N, K, H, W, thresh, activation, truth = IOU_CASES[name]
    pred, true = iou_inputs(name)
    want, clipped = iou_reference_hist(pred, true, thresh, activation)
    Kc = max(K, 2)
    lab = true.numpy().astype(np.int64)
    in_range = int(((lab >= 0) & (lab < Kc)).sum())
    assert in_range == N * H * W - (2 * N if truth == "float" else 8 * N)       # (the planted labels; 0.9, 1.7, -0.5 stay)
    if K > 1 and thresh < 0.5:
        assert clipped > 0, "this case is meant to reach the clip of class sums above K - 1"
    assert (want.sum((0, 1)) > 0).sum() >= min(Kc, 3)                           # (no degenerate prediction map)
    m = IoU(true.to(device), pred.to(device), bool(activation), thresh)
    got = m.hist.cpu().numpy()
    print(f"iou {name}: {N}x{K}x{H}x{W} thresh {thresh} activation {activation}: {in_range} labelled pixels, {clipped} "
          f"clipped class sums, histogram mismatches {int((got != want).sum())}")
    assert m.hist.dtype == torch.int32 and got.shape == (N, Kc, Kc)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8].tolist())
    assert int(got.sum()) == in_range
    assert abs(m.evaluate() - _jaccard64(want)) < 1e-6, (name, m.evaluate(), _jaccard64(want))
    again = IoU(true.to(device), pred.to(device), bool(activation), thresh)             # nothing accumulates across calls
    assert np.array_equal(again.hist.cpu().numpy(), want)
    assert np.array_equal(m.hist.cpu().numpy(), want)


def check_iou_threshold_is_strict(device):
    """activation=False: the inputs are the probabilities themselves.  A probability equal to the threshold (as the fp32
    number the kernel compares with) is not counted, the next fp32 number above it is: in both kernels, with the counts
    privatised and on global atomics, and for K = 1.  One pixel per (class, value), every label 0, so the expected row is
    written down here; the restatement of the reference must agree with it too."""
    from atomai_amd.losses_metrics import IoU
    for K, thresh in ((1, 0.6), (3, 0.5), (8, 0.2), (9, 0.2), (33, 0.05)):
        th = np.float32(thresh)
        up, down = np.nextafter(th, np.float32(1)), np.nextafter(th, np.float32(0))
        assert down < th < up
        classes = [0] if K == 1 else sorted({1, K // 2, K - 1})
        Kc = max(K, 2)
        pixels, want = [], np.zeros((1, Kc, Kc), np.int64)
        for c in classes:
            for v in (th, up, down, up, th):
                px = np.zeros(K, np.float32)
                px[c] = v
                pixels.append(px)
                want[0, 0, (max(c, 1) if v > th else 0)] += 1
        x = np.stack(pixels, 1).reshape(1, K, 1, len(pixels))
        pred, true = torch.from_numpy(x), torch.zeros((1, 1, len(pixels)), dtype=torch.int64)
        assert np.array_equal(iou_reference_hist(pred, true, thresh, 0)[0], want)
        got = IoU(true.to(device), pred.to(device), False, thresh).hist.cpu().numpy()
        assert np.array_equal(got, want), (K, thresh, got[0, 0].tolist(), want[0, 0].tolist())
