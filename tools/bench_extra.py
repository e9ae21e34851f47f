"""Secondary workloads of BASELINE.json (configs[2..4]) — one JSON line each, written to gpurun_out/.
   python tools/bench_extra.py rvae|jrvae|predict|dkl|losses|imspec|denoiser|stat|knn|cluster|nmf|ica [--unfused-head]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import atomai_amd as aoi
from atomai_amd import _lib as L

PEAK = 157.3


def timed_calls(names):
    recs, orig = [], L.call

    def call(name, *a):
        if name not in names:
            return orig(name, *a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); r = orig(name, *a); e1.record()
        recs.append((name, e0, e1))
        return r
    L.call = call
    import atomai_amd.nets.ed as ed, atomai_amd.engine as eng
    ed.L.call = call; eng.L.call = call
    return recs


def bench_rvae(steps=10, warmup=3, B=512, emit=True, ab=True):
    """configs[3] on one GPU.  Rooflines are priced on the ALGORITHMIC FLOPs of SURVEY.md section 8-d — forward
    2*NL*HID^2 per pixel (139 GFLOP at bs 512), backward = dgrad + wgrad = 2x that (278), step = 3x (417) — whatever the
    backward kernel ISSUES (the recompute variant issues 3x forward; that extra work is not "achieved").  `ab`: the
    same step with the hidden activations recomputed in backward instead of saved by the forward (in-process A/B)."""
    import atomai_amd.nets.ed as ed
    rs = np.random.RandomState(0)
    X = rs.rand(B * 2, 64, 64).astype(np.float32)
    m = aoi.models.rVAE((64, 64), latent_dim=2, seed=0)
    m.dx_prior, m.kdict_["phi_prior"] = 0.1, 0.1
    m.compile_trainer((X, None), None, batch_size=B)
    xs = [torch.from_numpy(X[i * B:(i + 1) * B]).cuda() for i in range(2)]
    names = {"amx_rdecoder_fwd", "amx_rdecoder_bwd", "amx_rdecoder_fwd_save", "amx_rdecoder_bwd_saved"}
    recs = timed_calls(names)

    from atomai_amd.trainers.trainer import _EarlyScalar

    def step(i):                                      # the body of viBaseTrainer.train_epoch for one mini-batch
        m.optim.zero_grad()
        elbo = m.forward_compute_elbo(xs[i % 2])
        early = _EarlyScalar(elbo)
        (-elbo).backward()
        m.optim.step()
        return early.item()

    def run():
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize(); recs.clear()
        t0 = time.perf_counter()
        for i in range(steps):
            last = step(i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        tf = sum(e0.elapsed_time(e1) for n, e0, e1 in recs if "fwd" in n) / steps
        tb = sum(e0.elapsed_time(e1) for n, e0, e1 in recs if "bwd" in n) / steps
        return dt, tf, tb, last
    saved_default = ed.RDEC_SAVE[0]
    dt, tf, tb, last = run()
    rows = B * 64 * 64
    fl_fwd = rows * 2 * 2 * 128 * 128.0
    tfl = lambda fl, ms: round(fl / (ms * 1e-3) / 1e12, 2)          # noqa: E731
    out = {"metric": "rVAE training patches/sec (64x64, bs=512, latent_dim=2)", "value": round(B / dt, 1),
           "unit": "patches/s", "ms_per_step": round(dt * 1e3, 3), "n_gpus": 1, "dtype": "f32", "elbo": last,
           "backward_variant": "saved activations" if saved_default else "recompute",
           "flops_note": "algorithmic (SURVEY 8-d): fwd 139 GFLOP, bwd 278, step 417 at bs 512",
           "roofline": {"bound": "mfma", "kernel": "rdecoder_bwd_kernel<128,64,2>",
                        "achieved": tfl(2 * fl_fwd, tb), "peak": PEAK, "unit": "TFLOP/s",
                        "frac": round(tfl(2 * fl_fwd, tb) / PEAK, 4), "ms": round(tb, 3)},
           "roofline_fwd": {"kernel": "rdecoder_fwd_kernel<128,64>", "achieved": tfl(fl_fwd, tf),
                            "frac": round(tfl(fl_fwd, tf) / PEAK, 4), "ms": round(tf, 3)},
           "roofline_decoder_pair": {"achieved": tfl(3 * fl_fwd, tf + tb), "frac": round(tfl(3 * fl_fwd, tf + tb) / PEAK, 4),
                                     "ms": round(tf + tb, 3)},
           "step_frac_of_mfma_f32_peak": round(tfl(3 * fl_fwd, dt * 1e3) / PEAK, 4)}
    if ab and not os.environ.get("AMX_RVAE_NO_AB"):
        ed.RDEC_SAVE[0] = not saved_default
        try:
            dt2, tf2, tb2, _ = run()
        finally:
            ed.RDEC_SAVE[0] = saved_default
        out["ab_other_variant"] = {"backward_variant": "recompute" if saved_default else "saved activations",
                                   "ms_per_step": round(dt2 * 1e3, 3), "fwd_ms": round(tf2, 3), "bwd_ms": round(tb2, 3),
                                   "patches_per_s": round(B / dt2, 1)}
    if emit:
        print(json.dumps(out), flush=True)
    return out


def bench_jrvae(steps=10, warmup=4, reps=5, B=512, emit=True):
    """jrVAE((64, 64), latent_dim=2, discrete_dim=[10]) training step at bs 512 next to the rVAE step of configs[3], in ONE
    process and interleaved: rounds of `steps` steps of (rvae, jrvae on the default one-launch latent path, jrvae on the
    step-by-step path), each round closed by a device synchronise; the median of the rounds is reported.  The
    step-by-step path is selected the way a user would: an instance-level ``reparameterize_discrete``."""
    from atomai_amd.trainers.trainer import _EarlyScalar
    rs = np.random.RandomState(0)
    X = rs.rand(B * 2, 64, 64).astype(np.float32)
    xs = [torch.from_numpy(X[i * B:(i + 1) * B]).cuda() for i in range(2)]
    rv = aoi.models.rVAE((64, 64), latent_dim=2, seed=0)
    jr = aoi.models.jrVAE((64, 64), latent_dim=2, discrete_dim=[10], seed=0)
    for m in (rv, jr):
        m.dx_prior, m.kdict_["phi_prior"] = 0.1, 0.1
        m.compile_trainer((X, None), None, batch_size=B)
    stock = type(jr).reparameterize_discrete

    def step(m, i):                                   # the body of viBaseTrainer.train_epoch for one mini-batch
        m.optim.zero_grad()
        elbo = m.forward_compute_elbo(xs[i % 2])
        early = _EarlyScalar(elbo)
        (-elbo).backward()
        m.optim.step()
        return early.item()

    def select(name):
        jr.__dict__.pop("reparameterize_discrete", None)
        if name == "jrvae_step_by_step":
            jr.reparameterize_discrete = stock
        assert jr._default_sampling() == (name != "jrvae_step_by_step")
        return rv if name == "rvae" else jr
    variants = ["rvae", "jrvae_default", "jrvae_step_by_step"]
    for name in variants:
        m = select(name)
        for i in range(warmup):
            step(m, i)
    times, last = {name: [] for name in variants}, {}
    for _ in range(reps):
        for name in variants:
            m = select(name)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(steps):
                last[name] = step(m, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    select("jrvae_default")
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = {"metric": "jrVAE training step (64x64, bs=512, latent_dim=2, discrete_dim=[10])", "unit": "ms",
           "value": round(med["jrvae_default"], 3), "higher_is_better": False, "n_gpus": 1, "dtype": "f32",
           "patches_per_s": round(B / med["jrvae_default"] * 1e3, 1),
           "rvae_ms_per_step_same_process": round(med["rvae"], 3),
           "jrvae_minus_rvae_ms": round(med["jrvae_default"] - med["rvae"], 3),
           "ab_latent_path": {"one_launch_ms": round(med["jrvae_default"], 3),
                              "step_by_step_ms": round(med["jrvae_step_by_step"], 3)},
           "rounds_ms": {name: [round(t, 3) for t in ts] for name, ts in times.items()},
           "elbo": {name: round(v, 3) for name, v in last.items()},
           "note": f"medians of {reps} interleaved rounds of {steps} steps after {warmup} warm-up steps per variant"}
    if emit:
        print(json.dumps(out), flush=True)
    return out


def bench_predict(frames=256, hw=1024, emit=True):
    """configs[2] on a bounded stack: dilnet nb_classes=1 predict over `frames` 1024x1024 frames."""
    torch.manual_seed(1)
    net, _ = aoi.nets.init_fcnn_model("dilnet", 1)
    rs = np.random.RandomState(0)
    stack = rs.rand(frames, hw, hw).astype(np.float32)
    p = aoi.predictors.SegPredictor(net, use_gpu=True, nb_classes=1, downsampling=2, verbose=False)
    p.run(stack[:min(frames, 16)], compute_coords=False)     # warm-up with a full chunk: the pinned staging buffers get their final size
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = p.run(stack, compute_coords=False)
    dt = time.perf_counter() - t0
    x = torch.from_numpy(stack[:8, None]).cuda()
    from atomai_amd.nets.fcnn import predict_proba
    net.eval()
    for _ in range(2): predict_proba(net, x)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    for _ in range(5): predict_proba(net, x)
    torch.cuda.synchronize(); dk = (time.perf_counter() - t1) / 5 / 8
    res = {"metric": "dilnet predict frames/sec (1024x1024, nb_classes=1), end-to-end incl. H2D/D2H",
           "value": round(frames / dt, 2), "unit": "frames/s", "frames": frames,
           "device_only_ms_per_frame": round(dk * 1e3, 3),
           "device_tflops": round(91.62e9 / dk / 1e12, 2), "device_frac_of_mfma_peak": round(91.62e9 / dk / 1e12 / PEAK, 4),
           "out_shape": list(out.shape)}
    if emit:
        print(json.dumps(res), flush=True)
    return res


def bench_predict_full(frames=4096, hw=1024, emit=True):
    """BASELINE.json configs[2] at its FULL size: dilnet nb_classes=1, model.predict over a 4096-frame 1024x1024 stack
    (17.2 GB in, 17.2 GB out, through pinned staging buffers; compute_coords=False).  The stack is filled block by
    block from 64 random frames with a per-block gain (so global min / max live in different blocks); reported:
    end-to-end seconds / frames/s of the whole call and the steady rate (4096-frame call minus a 256-frame call)."""
    torch.manual_seed(1)
    net, _ = aoi.nets.init_fcnn_model("dilnet", 1)
    rs = np.random.RandomState(0)
    base = torch.from_numpy(rs.rand(64, hw, hw).astype(np.float32))
    t0 = time.perf_counter()
    stack = np.empty((frames, hw, hw), dtype=np.float32)
    st = torch.from_numpy(stack)
    for i in range(0, frames, 64):
        m = min(64, frames - i)
        torch.mul(base[:m], 0.5 + (i // 64) / 128.0, out=st[i:i + m])
    t_gen = time.perf_counter() - t0
    p = aoi.predictors.SegPredictor(net, use_gpu=True, nb_classes=1, downsampling=2, verbose=False)
    p.run(stack[:16], compute_coords=False)                   # warm-up with a full chunk (pinned staging buffers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.run(stack[:256], compute_coords=False)
    t256 = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = p.run(stack, compute_coords=False)
    dt = time.perf_counter() - t0
    chk = float(out[::257].mean())
    # Parity of the timed call's OUTPUT (outside the timed region): 8 frames spread over the stack — first, last, and both
    # sides of chunk borders (16-frame chunks, 3 in flight, collected by a worker thread) — against the oracle's eval
    # graph (oracle.seg_oracle.predict_probs: stock torch ops, fp64, on the device) on the same globally normalised input
    # (utils/preproc.py:torch_format_image: (x - min) / ptp over the WHOLE stack, numpy float32 arithmetic).
    from oracle import seg_oracle as so
    idx = sorted({i for i in (0, 15, 16, frames // 2 - 1, frames // 2, frames - 17, frames - 16, frames - 1) if 0 <= i < frames})
    mn, mx = (float(v) for v in torch.aminmax(st))
    sub = (stack[idx] - np.float32(mn)) / np.float32(mx - mn)
    sd64 = so.cast({k: v.detach().cpu() for k, v in net.state_dict().items()}, torch.float64)
    sd64 = {k: v.cuda() for k, v in sd64.items()}
    ref = so.predict_probs("dilnet", sd64, torch.from_numpy(sub[:, None]).double().cuda(), 1).cpu().numpy()
    got = out[idx].astype(np.float64)
    parity = float(np.abs(got - ref).max() / np.abs(ref).max())
    del out, sd64
    x = torch.from_numpy(stack[:16, None]).cuda()            # device-only rate of the network itself (16-frame chunk)
    from atomai_amd.nets.fcnn import predict_proba
    net.eval()
    for _ in range(2): predict_proba(net, x)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    for _ in range(5): predict_proba(net, x)
    torch.cuda.synchronize(); dk = (time.perf_counter() - t1) / 5 / 16
    res = {"metric": "dilnet predict over the full 4096-frame 1024x1024 stack (BASELINE configs[2]), end-to-end incl. "
                     "host min/max, H2D, D2H and the copy into the returned array",
           "value": round(frames / dt, 2), "unit": "frames/s", "frames": frames, "seconds": round(dt, 3),
           "steady_frames_per_s": round((frames - 256) / (dt - t256), 2) if frames > 256 else None,
           "first_256_frames_s": round(t256, 3), "stack_GB": round(stack.nbytes / 1e9, 2),
           "host_fill_s": round(t_gen, 2), "out_shape": [frames, hw, hw, 1], "out_mean_sample": round(chk, 6),
           "parity_max_rel": float(f"{parity:.3g}"), "parity_frames": idx,
           "parity_note": "max |out - oracle| / max |oracle| over the listed frames of the timed call's output; oracle = "
                          "seg_oracle.predict_probs in fp64 on the device, outside the timed region",
           "device_only_ms_per_frame": round(dk * 1e3, 3), "device_tflops": round(91.62e9 / dk / 1e12, 2),
           "device_frac_of_mfma_peak": round(91.62e9 / dk / 1e12 / PEAK, 4)}
    if emit:
        print(json.dumps(res), flush=True)
    return res


def bench_dkl(N=16384, D=2, emit=True):
    """configs[4]: RBF covariance on N=16384 embedded points — HBM-write bound (4*N^2 bytes)."""
    from atomai_amd.nets.gp import kernel_matrix, kernel_matvec, convFeatureExtractor
    rs = np.random.RandomState(0)
    Z = torch.from_numpy(rs.uniform(-1, 1, (N, D)).astype(np.float32)).cuda()
    ls = torch.full((D,), float(np.log(2.0)), device="cuda")
    s2 = float(np.log(2.0))
    res = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        z, l = Z.to(dt), ls.to(dt)
        for _ in range(3): K = kernel_matrix(z, z, l, s2, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): K = kernel_matrix(z, z, l, s2, 0)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        byt = N * N * K.element_size() + N * D * K.element_size()
        res[name] = {"ms": round(ms, 4), "GBps": round(byt / ms / 1e6, 1), "frac_of_8TBps": round(byt / ms / 1e6 / 8000, 4)}
        del K
    v = torch.randn(N, 1, device="cuda")
    for _ in range(2): kernel_matvec(Z, Z, ls, s2, v, 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): kernel_matvec(Z, Z, ls, s2, v, 0)
    e1.record(); torch.cuda.synchronize()
    res["matvec_f32_ms"] = round(e0.elapsed_time(e1) / 5, 4)
    if D == 2:
        fe = convFeatureExtractor(256, 2).cuda().eval()
        P = torch.randn(N, 256, device="cuda")
        with torch.no_grad():
            for _ in range(2): fe(P)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(5): fe(P)
            torch.cuda.synchronize()
        res["conv_extractor_16384x16x16_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
    if D == 2:
        # SURVEY section 8-d asks for the embedding dimensions 2 AND 8: D = 8 through the same harness (fp32 / fp64
        # builder + matrix-free product only)
        d8 = bench_dkl(N, 8, emit=False)["detail"]
        res["D8"] = {k: d8[k] for k in ("f32", "f64", "matvec_f32_ms")}
    out = {"metric": f"DKL RBF covariance build, N={N}, D={D}", "value": res["f32"]["ms"], "unit": "ms",
           "higher_is_better": False,
           "roofline": {"bound": "hbm", "achieved": res["f32"]["GBps"], "peak": 8000, "unit": "GB/s",
                        "frac": res["f32"]["frac_of_8TBps"], "traffic": None}, "detail": res}
    if emit:
        print(json.dumps(out), flush=True)
    return out


def bench_dkl_fit(N=16384, patch=16, steps=3, warmup=1, precisions=("single", "double"), emit=True,
                  modes=("kissgp", "exact")):
    """configs[4] END TO END (VERDICT r05 missing #1 / #3): one `dklGPR` training cycle — `dklGPTrainer.train_step`, the unit
    of /root/reference/atomai/trainers/gptrainer.py:126-137 — at N = 16384 flattened 16 x 16 patches with the convolutional
    feature extractor, embedding dimension 2, RBF kernel, for both GP layers of nets/gp.py:
      kissgp (default; the reference's GridInterpolationKernel model, grid 50 x 50): phases = extractor forward, ski_gram
        (weights + W^T W / W^T r, csrc/ski.hip), k_build (K_UU on the 2500 grid nodes), grid_solve / grid_bwd (the dense
        m x m algebra: LU, solves, GEMMs — LIBRARY calls through torch), k_bwd (covariance backward on the grid),
        ski_gram_bwd, extractor backward + glue, Adam;
      exact (dense N x N GP): extractor forward, covariance build, potrf, solve + log-determinant, potri, covariance
        backward, extractor backward + glue, Adam — its O(N^3) library calls dominate.
    Phases by HIP events on the launch stream (`nets.gp.PHASES`); `library_frac` = share of the step in torch.linalg / GEMM."""
    import atomai_amd.nets.gp as gp
    from atomai_amd.nets.gp import convFeatureExtractor
    rs = np.random.RandomState(0)
    X = rs.rand(N, patch * patch).astype(np.float32)
    y = (X.reshape(N, patch, patch)[:, 4:12, 4:12].mean((1, 2)) + 0.05 * rs.randn(N)).astype(np.float32)
    out = {}
    for mode in modes:
      out[mode] = {}
      for prec in precisions:
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        mem0 = torch.cuda.memory_allocated()          # (tensors of earlier bench legs may still be resident: report the delta)
        m = aoi.models.dklGPR(patch * patch, embedim=2, precision=prec, seed=1, gp=mode)
        m.compile_trainer(X, y, training_cycles=1, feature_extractor=convFeatureExtractor)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        per_step, phases = [], {}
        nst = steps if mode == "exact" else max(steps, 10)
        for it in range(warmup + nst):
            gp.PHASES = {} if it >= warmup else None
            e = [ev() for _ in range(5)]
            e[0].record()
            m.optimizer.zero_grad()
            loss = -m.gp_model.mll()
            e[1].record()
            loss.backward()
            e[2].record()
            m.optimizer.step()
            e[3].record()
            lv = loss.item()
            e[4].record(); torch.cuda.synchronize()
            if it >= warmup:
                per_step.append(e[0].elapsed_time(e[4]))
                ph = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in gp.PHASES.items()}
                ph["forward_total"] = e[0].elapsed_time(e[1])
                ph["backward_total"] = e[1].elapsed_time(e[2])
                ph["adam"] = e[2].elapsed_time(e[3])
                for k, v in ph.items():
                    phases.setdefault(k, []).append(v)
            gp.PHASES = None
        med = lambda v: float(np.median(v))
        ph = {k: round(med(v), 3) for k, v in phases.items()}
        step = med(per_step)
        if mode == "exact":
            ph["extractor_bwd_and_glue"] = round(ph["backward_total"] - ph.get("potri", 0.0) - ph.get("k_bwd", 0.0), 3)
            lib = ph.get("potrf", 0.0) + ph.get("potri", 0.0) + ph.get("solve_logdet", 0.0)
        else:
            bw_k = sum(v for k, v in ph.items() if k in ("grid_bwd", "k_bwd", "ski_gram_bwd")) + 0.5 * ph.get("k_build", 0.0)
            ph["extractor_bwd_and_glue"] = round(ph["backward_total"] - bw_k, 3)
            lib = ph.get("grid_solve", 0.0) + ph.get("grid_bwd", 0.0)
        rec = {"ms_per_fit_step": round(step, 2), "phases_ms": ph, "library_ms": round(lib, 2),
               "library_frac": round(lib / step, 4), "optimizer": type(m.optimizer).__name__,
               "peak_mem_GB": round((torch.cuda.max_memory_allocated() - mem0) / 1e9, 2), "loss": round(lv, 6)}
        if mode == "exact":
            with torch.no_grad():
                gpm = m.gp_model
                Z = gpm.embed(gpm.train_inputs[0])
                K = gp.kernel_matrix(Z, Z, gpm.lengthscale[0], float(gpm.outputscale[0]), 0, float(gpm.noise[0, 0]))
                Ki = torch.cholesky_inverse(torch.linalg.cholesky(K))
                asym = float((Ki - Ki.T).abs().max() / Ki.abs().max())
                del K, Ki
            rec.update({"potrf_tflops": round(N ** 3 / 3 / (ph["potrf"] * 1e-3) / 1e12, 2) if ph.get("potrf") else None,
                        "potri_tflops": round(2 * N ** 3 / 3 / (ph["potri"] * 1e-3) / 1e12, 2) if ph.get("potri") else None,
                        "kinv_rel_asymmetry": float(f"{asym:.2e}")})
        else:
            rec["grid_nodes"] = m.gp_model.grid.m
            # the same model state evaluated by the dense exact GP: how far the two layers' objectives are apart
            with torch.no_grad():
                gpm = m.gp_model
                Z = gpm.embed(gpm.train_inputs[0])
                a = gp._SkiMLLFn.apply(Z, gpm.train_targets, gpm.lengthscale, gpm.outputscale, gpm.noise[:, 0],
                                       gpm.mean_constant[:, 0], 0, gpm.grid)
                b = gp._ExactMLLFn.apply(Z, gpm.train_targets[0], gpm.lengthscale[0], gpm.outputscale[0], gpm.noise[0, 0],
                                         gpm.mean_constant[0, 0], 0)
                rec["mll_kissgp_vs_exact"] = [round(float(a), 6), round(float(b), 6)]
        out[mode][prec] = rec
        del m
    first = out[modes[0]][precisions[0]]
    res = {"metric": f"dklGPR fit step ({modes[0]} GP layer, conv extractor, N={N}, {patch}x{patch} patches, embedim 2)",
           "value": first["ms_per_fit_step"], "unit": "ms", "higher_is_better": False, "dtype": precisions[0],
           "note": "kissgp = the reference's GridInterpolationKernel model (grid 50 x 50) with its marginal likelihood evaluated "
                   "exactly through m x m grid algebra (gpytorch: CG / Lanczos estimators); exact = dense N x N GP, whose potrf + "
                   "potri + solve are rocSOLVER / rocBLAS through torch.  library_frac = share of the step inside torch.linalg / "
                   "GEMM calls; the HIP kernels of this build are ski_gram(_bwd), k_build, k_bwd, the extractor and Adam.",
           "detail": out}
    if emit:
        print(json.dumps(res), flush=True)
    return res


def _conv_flops(name, a):
    """Executed MFMA-conv FLOPs of one C-ABI call (stored/padded channel counts, as launched)."""
    if name == "amx_conv2d_fwd":
        return 2.0 * (a[3] + a[7]) * a[19] * a[20] * a[16] * a[17] * a[18]
    if name == "amx_conv2d_fwd_act":
        return 2.0 * (a[4] + a[9]) * a[21] * a[22] * a[18] * a[19] * a[20]
    if name == "amx_conv2d_dgrad":
        return 2.0 * a[1] * (a[5] + a[7]) * a[11] * a[8] * a[9] * a[10]
    if name == "amx_conv2d_dgrad_fused":
        return 2.0 * a[6] * (a[9] + a[11]) * a[15] * a[12] * a[13] * a[14]
    if name == "amx_conv2d_dgrad_fused_bsum":
        return 2.0 * a[6] * a[9] * a[13] * a[10] * a[11] * a[12]
    if name == "amx_conv2d_wgrad_fused":
        return 2.0 * (a[3] + a[7]) * a[20] * a[21] * a[17] * a[18] * a[19]
    if name == "amx_conv2d_wgrad_act":
        return 2.0 * (a[4] + a[9]) * a[22] * a[23] * a[19] * a[20] * a[21]
    return 0.0


def bench_segfamily(models=("SegResNet", "ResHedNet", "dilnet"), hw=512, bs=32, steps=10, warmup=4, emit=True):
    """Training throughput of the other Segmentor families (default widths) at the headline shape."""
    import atomai_amd.engine as eng
    res = {}
    for model in models:
        rs = np.random.RandomState(0)
        ncls = 1 if model == "dilnet" else 3
        X = rs.rand(2 * bs, hw, hw).astype(np.float32)
        y = rs.randint(0, 3, (2 * bs, hw, hw)) if ncls > 1 else (rs.rand(2 * bs, hw, hw) > 0.5).astype(np.float32)
        m = aoi.models.Segmentor(model, nb_classes=ncls, seed=1)
        m.compile_trainer((X, y, X[:bs], y[:bs]), training_cycles=steps + warmup, batch_size=bs,
                          plot_training_history=False)
        flops, orig = [0.0], L.call

        def call(name, *a):
            flops[0] += _conv_flops(name, a)
            return orig(name, *a)
        for i in range(warmup):
            m.train_step(m.X_train[i % 2], m.y_train[i % 2])
        L.call = eng.L.call = call
        m.train_step(m.X_train[0], m.y_train[0])
        L.call = eng.L.call = orig
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(steps):
            last = m.train_step(m.X_train[i % 2], m.y_train[i % 2])[0]
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
        res[model] = {"images_per_s": round(bs / dt, 1), "ms_per_step": round(dt * 1e3, 2), "loss": round(last, 4),
                      "conv_TFLOP_per_step_as_launched": round(flops[0] / 1e12, 3),
                      "step_TFLOPs": round(flops[0] / dt / 1e12, 1), "frac_of_mfma_peak": round(flops[0] / dt / 1e12 / PEAK, 3)}
        del m
        torch.cuda.empty_cache()
    out = {"metric": f"training images/sec, {hw}x{hw}, bs={bs}, default-width families", "unit": "images/s",
           "value": res.get("SegResNet", {}).get("images_per_s"), "detail": res}
    if emit:
        print(json.dumps(out), flush=True)
    return out


def bench_locate(frames=32, hw=1024, C=1, emit=True):
    """Locator on `frames` probability maps of hw x hw (the post-processing of configs[2]): HBM-bound integer
    work; algorithmic bytes = the probabilities read once (4*C bytes per pixel)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import locator_oracle as lo
    from atomai_amd.predictors.locator import locate_device
    rs = np.random.RandomState(0)
    base = lo.synthetic_maps(rs, 2, hw, hw, C, n_blobs=2500, noise=0.3)
    x = torch.from_numpy(np.concatenate([base] * (frames // 2))).cuda()
    recs = timed_calls({"amx_locate_label", "amx_locate_emit"})
    import atomai_amd.predictors.locator as lm
    lm.L.call = L.call
    for _ in range(2):
        d = locate_device(x, 0.5, 5)
    torch.cuda.synchronize(); recs.clear()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        d = locate_device(x, 0.5, 5)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    t_label = sum(e0.elapsed_time(e1) for n, e0, e1 in recs if n == "amx_locate_label") / reps
    t_emit = sum(e0.elapsed_time(e1) for n, e0, e1 in recs if n == "amx_locate_emit") / reps
    t0 = time.perf_counter()
    ref = lo.locate(base.copy(), 0.5, 5)
    cpu_dt = (time.perf_counter() - t0) / 2
    same = all(np.array_equal(d[i], ref[i]) for i in range(2))
    nbytes = frames * hw * hw * C * 4
    gbps = nbytes / ((t_label + t_emit) * 1e-3) / 1e9
    out = {"metric": f"Locator frames/sec ({hw}x{hw}, {C}-channel maps)", "value": round(frames / dt, 1),
           "unit": "frames/s", "n_gpus": 1, "dtype": "i32", "ms_per_frame_device": round((t_label + t_emit) / frames, 4),
           "ms_label": round(t_label, 3), "ms_emit": round(t_emit, 3), "ms_end_to_end": round(dt * 1e3, 3),
           "centres_per_frame": int(np.mean([len(v) for v in d.values()])), "matches_oracle": bool(same),
           "roofline": {"bound": "hbm", "achieved": round(gbps, 1), "peak": 8000, "unit": "GB/s",
                        "frac": round(gbps / 8000, 4), "traffic": None},
           "cpu_baseline": {"value": round(1 / cpu_dt, 2), "unit": "frames/s", "cores": 1, "kind": "port",
                            "sample": "2 frames through oracle/locator_oracle.py (scipy.ndimage)"}}
    if emit:
        print(json.dumps(out), flush=True)
    return out


def bench_losses(hw=512, bs=32, steps=10, warmup=4, reps=3, emit=True):
    """select_loss('dice' | 'focal') against the 'ce' step at the headline shape (U-Net, bs x hw x hw, fp32), interleaved in
    one process: variants ce3 (nb_classes 3, the yardstick), dice3 (fused head + dice), dice3_general (AMX_FUSE_PX_LOSS=0
    for that step: px -> dice kernels on logits -> px backward), bce1 / focal1 / dice1 (nb_classes 1).  `reps` rounds of
    `steps` steps per variant, median of the rounds; then one event-timed step per variant for the head / loss launches
    (their times and the bandwidth of the passes over the last activation, npix * Cs * 4 bytes read each)."""
    import atomai_amd.engine as eng
    import atomai_amd.trainers.trainer as tr
    rs = np.random.RandomState(0)
    X = rs.rand(bs, hw, hw).astype(np.float32)
    y3 = rs.randint(0, 3, (bs, hw, hw))
    y1 = (rs.rand(bs, hw, hw) < 0.03).astype(np.float32)             # a few percent of the pixels are atoms
    variants = [("ce3", 3, "ce", True), ("dice3", 3, "dice", True), ("dice3_general", 3, "dice", False),
                ("bce1", 1, "ce", True), ("focal1", 1, "focal", True), ("dice1", 1, "dice", True)]
    models = {}
    for name, ncls, loss, fused in variants:
        m = aoi.models.Segmentor(nb_classes=ncls, seed=1)
        yy = y3 if ncls == 3 else y1
        m.compile_trainer((X, yy, X, yy), loss=loss, training_cycles=1, batch_size=bs, plot_training_history=False)
        models[name] = m

    def step(name, fused):
        m = models[name]
        tr.FUSE_LOSS = eng.FUSE_PX_LOSS = fused
        try:
            return m.train_step(m.X_train[0], m.y_train[0])[0]
        finally:
            tr.FUSE_LOSS = eng.FUSE_PX_LOSS = True
    for name, _, _, fused in variants:
        for _ in range(warmup):
            step(name, fused)
    times = {name: [] for name, *_ in variants}
    for _ in range(reps):
        for name, _, _, fused in variants:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                last = step(name, fused)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    names = {"amx_px_ce_train", "amx_px_dice_sums", "amx_px_dice_train", "amx_dice_finalize", "amx_reduce_rows_chunked",
             "amx_px_bce_sum", "amx_px_focal_train",
             "amx_px_fwd", "amx_px_bwd", "amx_dice_sums", "amx_dice_bwd", "amx_focal_from_bce", "amx_mul_scalars",
             "amx_scale_unless_one_multi", "amx_ce_fwd_bwd", "amx_bce_fwd_bwd"}
    recs = timed_calls(names)
    import atomai_amd.losses_metrics.losses as lm
    lm.L.call = L.call
    act_bytes = bs * hw * hw * 16 * 4
    res = {}
    for name, ncls, loss, fused in variants:
        recs.clear()
        step(name, fused)
        torch.cuda.synchronize()
        launches = {}
        for n, e0, e1 in recs:
            launches[n] = round(launches.get(n, 0.0) + e0.elapsed_time(e1), 4)
        r = {"ms_per_step": round(float(np.median(times[name])), 3), "rounds_ms": [round(t, 3) for t in times[name]],
             "images_per_s": round(bs / float(np.median(times[name])) * 1e3, 1), "loss_path_launches_ms": launches}
        for k in ("amx_px_ce_train", "amx_px_dice_sums", "amx_px_dice_train", "amx_px_bce_sum", "amx_px_focal_train"):
            if k in launches:                       # train kernels also write dxn (as many bytes again)
                r[k + "_GBps"] = round(act_bytes * (1 if k.endswith("sum") or k.endswith("sums") else 2) / launches[k] / 1e6, 1)
        res[name] = r
    out = {"metric": f"dice / focal training steps vs the 'ce' step, U-Net {hw}x{hw}, bs={bs}", "unit": "ms",
           "value": res["dice3"]["ms_per_step"], "higher_is_better": False,
           "last_activation_MB": round(act_bytes / 1e6, 1), "detail": res}
    if emit:
        print(json.dumps(out), flush=True)
    return out


class _TorchSignalED(torch.nn.Module):
    """The SignalED stack (atomai/nets/ed.py:20-228, no down / upsampling) from stock torch.nn modules: the outside
    yardstick of bench_imspec on the same GPU."""

    def __init__(self, in_dim, out_dim, latent_dim, nl_e=3, nl_d=4, nf_e=64, nf_d=64):
        super().__init__()
        nn = torch.nn

        def pick(dim):
            return (nn.Conv2d, nn.BatchNorm2d) if len(dim) == 2 else (nn.Conv1d, nn.BatchNorm1d)

        def layer(dim, cin, cout, dil=1):
            conv, bn = pick(dim)
            return nn.Sequential(conv(cin, cout, 3, padding=dil, dilation=dil), nn.LeakyReLU(0.1), bn(cout))
        self.enc = nn.Sequential(*[layer(in_dim, 1 if i == 0 else nf_e, nf_e) for i in range(nl_e)])
        self.fc_e = nn.Linear(nf_e * int(np.prod(in_dim)), latent_dim)
        self.fc_d = nn.Linear(latent_dim, nf_d * int(np.prod(out_dim)))
        self.shape = (nf_d, *out_dim)
        self.dil = nn.ModuleList([layer(out_dim, nf_d, nf_d, d + 1) for d in range(nl_d)])
        self.conv = layer(out_dim, nf_d, 1)
        self.out = pick(out_dim)[0](1, 1, 1)

    def forward(self, x):
        z = self.fc_e(self.enc(x).flatten(1))
        h = self.fc_d(z).reshape(-1, *self.shape)
        tot = 0
        for blk in self.dil:                       # DilatedBlock: the sum of every sub-layer output
            for m in blk:
                h = m(h)
                tot = tot + h
        return self.out(self.conv(tot))


def bench_imspec(reps=3, iters=20, steps=10, warmup=4, emit=True):
    """ImSpec (im2spec).  (a) interleaved in-process A/B of amx_conv1d_fwd against the only in-tree baseline, the H = 1
    embedding through amx_conv2d_fwd (three taps in the middle row of a zero 3x3 weight), at (N, L, Cin -> Cout, dil) =
    (64, 64, 64 -> 64, 1) and (256, 1024, 64 -> 64, 4): min of `reps` rounds of `iters` launches, us per launch.
    (b) a whole training step of the default im2spec (16, 16) -> (64,), bs 64, and (16, 16) -> (1024,), bs 256, next to
    the same stack from stock torch.nn modules (_TorchSignalED, torch.optim.Adam, nn.MSELoss) on the same GPU: median of
    `reps` rounds of `steps` steps, ms per step."""
    dev = "cuda"
    res = {"conv1d_fwd_vs_h1_embedding_us": {}, "train_step_ms": {}}
    lib = L.load()
    for N, Ln, C, dil in ((64, 64, 64, 1), (256, 1024, 64, 4)):
        x = torch.randn(N, Ln, C, device=dev)
        w = torch.randn(C, C, 3, device=dev) / (3 * C) ** 0.5
        b = torch.randn(C, device=dev)
        w2 = torch.zeros(C, C, 3, 3, device=dev)
        w2[:, :, 1, :] = w
        sp = L.stream_ptr(x)
        p1 = torch.empty(lib.amx_pack_weights1d_size(C, C, 3), device=dev)
        L.call("amx_pack_weights1d", L.ptr(w), L.ptr(p1), C, C, C, 3, 0, sp)
        p2 = torch.empty(lib.amx_pack_weights_size(C, C, 0, 9, 0), device=dev)
        L.call("amx_pack_weights", L.ptr(w2), L.ptr(p2), C, C, C, 0, 0, 9, 0, sp)
        y1, y2 = torch.empty(N, Ln, C, device=dev), torch.empty(N, 1, Ln, C, device=dev)

        def run1():
            L.call("amx_conv1d_fwd", L.ptr(x), None, None, 1.0, C, L.ptr(p1), L.ptr(b), L.ptr(y1), None, N, Ln, C, 3, dil,
                   0.1, 0, 0, sp)

        def run2():
            L.call("amx_conv2d_fwd", L.ptr(x), None, None, C, None, None, None, 0, L.ptr(p2), L.ptr(b), None, L.ptr(y2), C,
                   None, 0, None, N, 1, Ln, C, 9, dil, 0.1, sp)
        for f in (run1, run2):
            for _ in range(3):
                f()
        t = {"conv1d": [], "h1_embedding": []}
        for _ in range(reps):
            for name, f in (("conv1d", run1), ("h1_embedding", run2)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) / iters * 1e3)
        diff = float((y1 - y2.view(N, Ln, C)).abs().max())
        res["conv1d_fwd_vs_h1_embedding_us"][f"{N}x{Ln}x{C}_dil{dil}"] = {
            "conv1d": round(min(t["conv1d"]), 2), "h1_embedding": round(min(t["h1_embedding"]), 2),
            "rounds": {k: [round(v, 2) for v in vs] for k, vs in t.items()}, "max_abs_diff": diff}
    rs = np.random.RandomState(0)
    for out_len, bs in ((64, 64), (1024, 256)):
        X = rs.rand(bs, 1, 16, 16).astype(np.float32)
        Y = rs.rand(bs, 1, out_len).astype(np.float32)
        m = aoi.models.ImSpec((16, 16), (out_len,), latent_dim=10, seed=1)
        m.compile_trainer((X, Y, X, Y), loss="mse", training_cycles=1, batch_size=bs, plot_training_history=False)
        torch.manual_seed(1)
        ref = _TorchSignalED((16, 16), (out_len,), 10).to(dev)
        opt, crit = torch.optim.Adam(ref.parameters(), lr=1e-3), torch.nn.MSELoss()
        xt, yt = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)

        def ours():
            return m.train_step(m.X_train[0], m.y_train[0])[0]

        def stock():
            ref.train()
            opt.zero_grad()
            loss = crit(ref(xt), yt)
            loss.backward()
            opt.step()
            return loss.item()
        for f in (ours, stock):
            for _ in range(warmup):
                f()
        t = {"atomai_amd": [], "torch_nn": []}
        for _ in range(reps):
            for name, f in (("atomai_amd", ours), ("torch_nn", stock)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(steps):
                    f()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / steps * 1e3)
        res["train_step_ms"][f"16x16_to_{out_len}_bs{bs}"] = {
            k: {"median": round(float(np.median(v)), 3), "rounds": [round(u, 3) for u in v]} for k, v in t.items()}
    first = res["train_step_ms"]["16x16_to_64_bs64"]
    out = {"metric": "ImSpec im2spec (16, 16) -> (64,) training step, bs=64", "unit": "ms",
           "value": first["atomai_amd"]["median"], "higher_is_better": False, "detail": res}
    if emit:
        print(json.dumps(out), flush=True)
    return out


def bench_denoiser(hw=256, bs=32, steps=100, warmup=10, reps=5, fused_head=True, emit=True):
    """DenoisingAutoencoder training step (default architecture [8, 16, 32, 64] / [64, 32, 16, 8], bs x hw x hw, fp32, MSE):
    steps per second, and the fused 1x1-head + MSE tail (amx_px_mse_train) against the three-launch tail (amx_px_fwd ->
    amx_mse_fwd_bwd -> amx_px_bwd), interleaved in ONE process on ONE model: warm-up of both paths, then an A/A pass (the
    fused step against itself: `reps` rounds of `steps` steps per label, device-synchronised around each window) whose
    largest difference between the two labels' rounds is the run-to-run spread, then the A/B pass in the same form.
    ``fused_head=False`` (command line: --unfused-head) makes the three-launch tail the headline and skips the A/B."""
    import atomai_amd.engine as eng
    import atomai_amd.trainers.trainer as tr
    rs = np.random.RandomState(0)
    clean = rs.rand(bs, 1, hw, hw).astype(np.float32)
    noisy = (clean + 0.1 * rs.randn(bs, 1, hw, hw)).astype(np.float32)
    m = aoi.models.DenoisingAutoencoder(seed=1)
    m.compile_trainer(aoi.utils.preprocess_denoiser_data(noisy, clean, noisy, clean), loss="mse", training_cycles=1,
                      batch_size=bs, plot_training_history=False)
    kinds = []
    orig = type(m.net).forward_loss

    def spy(self, *a, **k):
        r = orig(self, *a, **k)
        kinds.append(r[0])
        return r
    type(m.net).forward_loss = spy

    mse_default = eng.FUSE_PX_MSE

    def step(fused):
        tr.FUSE_LOSS = eng.FUSE_PX_LOSS = eng.FUSE_PX_MSE = fused
        try:
            return m.train_step(m.X_train[0], m.y_train[0])[0]
        finally:
            tr.FUSE_LOSS = eng.FUSE_PX_LOSS = True
            eng.FUSE_PX_MSE = mse_default

    def rounds(labels):
        t = {name: [] for name, _ in labels}
        for _ in range(reps):
            for name, fused in labels:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(steps):
                    step(fused)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / steps * 1e3)
        return t
    try:
        for fused in (True, False):
            for _ in range(warmup):
                step(fused)
        assert kinds == ["loss"] * warmup, kinds               # the fused node ran; the unfused step never asks for it
        lines = []
        if not fused_head:
            t = rounds([("unfused", False)])
            aa = ab = None
        else:
            aa = rounds([("fused_a", True), ("fused_b", True)])
            ab = rounds([("fused", True), ("unfused", False)])
            t = ab
        for tt in (aa, ab) if fused_head else (t,):
            for name, v in tt.items():
                lines.append(f"{name:<10} step ms {[f'{u:.3f}' for u in v]}  median {np.median(v):.3f}  min {min(v):.3f}")
    finally:
        type(m.net).forward_loss = orig
    head = "fused" if fused_head else "unfused"
    ms = float(np.median(t[head]))
    out = {"metric": f"DenoisingAutoencoder training step, default architecture, {hw}x{hw}, bs={bs}, {head} head",
           "unit": "steps/s", "value": round(1e3 / ms, 2), "higher_is_better": True, "ms_per_step": round(ms, 3),
           "detail": {k: [round(u, 3) for u in v] for k, v in t.items()}}
    if fused_head:
        spread = max(abs(a - b) for a, b in zip(aa["fused_a"], aa["fused_b"]))
        spread = max(spread, max(aa["fused_a"]) - min(aa["fused_a"]), max(aa["fused_b"]) - min(aa["fused_b"]))
        out.update({"aa_spread_ms": round(spread, 3), "aa": {k: [round(u, 3) for u in v] for k, v in aa.items()},
                    "unfused_ms_per_step": round(float(np.median(ab["unfused"])), 3),
                    "fused_minus_unfused_ms": round(ms - float(np.median(ab["unfused"])), 3)})
        lines.append(f"A/A spread {spread:.3f} ms; fused {ms:.3f} ms, unfused {np.median(ab['unfused']):.3f} ms per step")
    out["log"] = [f"# python tools/bench_extra.py denoiser{'' if fused_head else ' --unfused-head'} - default architecture, "
                  f"bs {bs} {hw}^2, interleaved in one process, {reps} x {steps} steps per label"] + lines
    if emit:
        print("\n".join(out["log"]))
        print(json.dumps(out), flush=True)
    return out


def _refine_frames(rs, frames, hw, spacing, sigma):
    """Synthetic frames with a jittered square lattice of Gaussian atoms, their true centres, and atom masks."""
    grid = np.arange(spacing, hw - spacing + 1, spacing, dtype=np.float64)
    r = 3 * int(np.ceil(sigma)) + 1
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = (yy[r - 2:r + 3, r - 2:r + 3] ** 2 + xx[r - 2:r + 3, r - 2:r + 3] ** 2 <= 5).astype(np.int64)
    imgs = np.full((frames, hw, hw), 0.1)
    masks = np.zeros((frames, hw, hw), dtype=np.int64)
    centres = []
    for f in range(frames):
        cr = (grid[:, None] + rs.uniform(-1.5, 1.5, (len(grid), len(grid)))).ravel()
        cc = (grid[None, :] + rs.uniform(-1.5, 1.5, (len(grid), len(grid)))).ravel()
        for a, b in zip(cr, cc):
            ia, ib = int(round(a)), int(round(b))
            imgs[f, ia - r:ia + r + 1, ib - r:ib + r + 1] += rs.uniform(0.6, 1.0) * np.exp(
                -((yy + ia - a) ** 2 + (xx + ib - b) ** 2) / (2 * sigma ** 2))
            masks[f, ia - 2:ia + 3, ib - 2:ib + 3] |= disc
        centres.append(np.stack((cr, cc), 1))
    imgs += 0.02 * rs.randn(frames, hw, hw)
    return imgs.astype(np.float32), centres, masks


def bench_refine(frames=4, hw=1024, spacing=16, d=4, sigma=1.6, cycles=300, sample=200, reps=5, emit=True):
    """Gaussian peak refinement on `frames` synthetic hw x hw frames that carry a lattice of (hw / spacing - 1)^2 Gaussian
    atoms each: (a) amx_peak_refine alone on the true centres displaced by up to 0.7 px (event-timed), (b)
    SegPredictor.run(refine=True, d) end to end with a default U-Net trained for `cycles` steps on crops of the same
    frames, next to the same run with refine=False, and (c) the yardstick: the reference's host loop, one
    scipy.optimize.curve_fit per atom (atomai/utils/coords.py:208-228), over a sample of the atoms of (a)."""
    from scipy import optimize
    from atomai_amd.predictors import SegPredictor
    from atomai_amd.predictors.locator import refine_device
    from atomai_amd.utils import gaussian_2d
    rs = np.random.RandomState(0)
    imgs, centres, masks = _refine_frames(rs, frames, hw, spacing, sigma)
    start = [c + rs.uniform(-0.7, 0.7, c.shape) for c in centres]
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    fr = torch.from_numpy(imgs).to(dev)
    xy = torch.from_numpy(np.concatenate(start)).to(dev)
    meta = np.zeros((len(xy), 2), dtype=np.int32)
    meta[:, 0] = np.repeat(np.arange(frames), [len(c) for c in start])
    meta = torch.from_numpy(meta).to(dev)
    n = len(xy)
    recs = timed_calls({"amx_peak_refine"}) if dev == "cuda" else []
    for _ in range(2):
        out, status = refine_device(fr, xy, meta, d, return_status=True)
    recs.clear()
    t0 = time.perf_counter()
    for _ in range(reps):
        out, status = refine_device(fr, xy, meta, d, return_status=True)
    if dev == "cuda":
        torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    ms = [e0.elapsed_time(e1) for _, e0, e1 in recs] or [wall * 1e3]
    out, status = out.cpu().numpy(), status.cpu().numpy()
    truth = np.concatenate(centres)
    err0, err1 = np.abs(xy.cpu().numpy() - truth).max(1), np.abs(out - truth).max(1)
    # (c) the host yardstick on a sample of the same atoms; everything it reads is on the host before the clock starts
    pick = rs.permutation(n)[:sample]
    grid = tuple(np.indices((2 * d, 2 * d)))
    starts_h, frame_h = xy.cpu().numpy(), meta.cpu().numpy()[:, 0]
    host = starts_h[pick].copy()                             # an atom whose fit fails or strays keeps its start
    t0 = time.perf_counter()
    for k, i in enumerate(pick):
        corner = np.rint(starts_h[i]).astype(np.int64) - d   # half to even, as the kernel rounds
        window = imgs[frame_h[i], corner[0]:corner[0] + 2 * d, corner[1]:corner[1] + 2 * d]
        guess = np.array([window[d, d], d, d, 1.0, 1.0, 0.0, 0.0])
        try:
            fit = optimize.curve_fit(gaussian_2d, grid, window.ravel(), p0=guess)[0]
        except RuntimeError:                                 # scipy: no convergence within maxfev
            continue
        if np.hypot(fit[1] - d, fit[2] - d) < 3:
            host[k] = fit[1:3] + corner
    host_dt = (time.perf_counter() - t0) / len(pick)
    # (b) end to end
    m = aoi.models.Segmentor(nb_classes=1, seed=1)
    crop = min(256, hw)
    rs2 = np.random.RandomState(1)
    idx = [(f % frames, *rs2.randint(0, hw - crop + 1, 2)) for f in range(16)]
    X = np.stack([imgs[f, i:i + crop, j:j + crop] for f, i, j in idx])[:, None]
    Y = np.stack([masks[f, i:i + crop, j:j + crop] for f, i, j in idx])[:, None].astype(np.float32)
    m.fit(X, Y, X[:8], Y[:8], training_cycles=cycles, batch_size=8, plot_training_history=False, print_loss=10 ** 9)
    e2e = {}
    for refine in (False, True):
        p = SegPredictor(m.net, refine=refine, use_gpu=True, d=d, nb_classes=1, verbose=False)
        p.run(imgs)
        t0 = time.perf_counter()
        for _ in range(reps):
            dec, co = p.run(imgs)
        e2e[refine] = ((time.perf_counter() - t0) / reps, co)
    found = sum(len(v) for v in e2e[True][1].values())
    moved = sum(int((e2e[True][1][i][:, :2] != e2e[False][1][i][:, :2]).any(1).sum()) for i in e2e[True][1])
    res = {"metric": f"amx_peak_refine atoms/sec ({frames} frames of {hw}x{hw}, {n} atoms, d={d})",
           "value": round(n / (float(np.median(ms)) * 1e-3), 1), "unit": "atoms/s", "n_gpus": 1, "dtype": "fp64",
           "ms_kernel": [round(v, 3) for v in ms], "ms_call_wall": round(wall * 1e3, 3),
           "status_counts": np.bincount(status, minlength=5).tolist(),
           "max_abs_error_vs_truth_px": {"start": round(float(err0.max()), 3),
                                          "refined_median": round(float(np.median(err1)), 4),
                                          "refined_max": round(float(err1.max()), 3)},
           "max_abs_diff_vs_host_loop_px": float(np.abs(host - out[pick]).max()),
           "end_to_end": {"atoms_found": found, "atoms_moved_by_fit": moved, "train_cycles": cycles,
                          "s_per_run_refine": round(e2e[True][0], 4), "s_per_run_plain": round(e2e[False][0], 4),
                          "atoms_per_s": round(found / e2e[True][0], 1),
                          "frames_per_s": round(frames / e2e[True][0], 2)},
           "cpu_baseline": {"value": round(1 / host_dt, 1), "unit": "atoms/s", "cores": 1, "kind": "reference loop",
                            "sample": f"{len(pick)} atoms through scipy.optimize.curve_fit, same run"}}
    res["log"] = [f"# python tools/bench_extra.py refine - {frames} frames of {hw}^2, {n} atoms, d = {d}",
                  f"amx_peak_refine alone        {res['value']:>14.1f} atoms/s  (kernel ms {res['ms_kernel']}, status counts "
                  f"fitted / patch / gate / no convergence / bad row {res['status_counts']})",
                  f"SegPredictor.run(refine=True){res['end_to_end']['atoms_per_s']:>14.1f} atoms/s  ({found} atoms found, {moved} "
                  f"moved; {e2e[True][0]:.4f} s per run against {e2e[False][0]:.4f} s with refine=False)",
                  f"host loop of curve_fit       {res['cpu_baseline']['value']:>14.1f} atoms/s  ({len(pick)} atoms of the same "
                  f"table; largest |device - host| {res['max_abs_diff_vs_host_loop_px']:.2e} px)"]
    if emit:
        print("\n".join(res["log"]))
        print(json.dumps(res), flush=True)
    return res


def _planted_stack(frames, per_frame, r, C, classes, noise):
    """Frames that carry ``classes`` planted prototypes + noise at frames * per_frame window centres: (images,
    coordinates per frame, planted class of every window)."""
    rs = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(per_frame)))
    H = (side + 2) * r
    proto = rs.uniform(0.1, 0.9, (classes, r, r, C)).astype(np.float32)
    imgs = rs.uniform(0, 0.05, (frames, H, H, C)).astype(np.float32)
    coords, planted = {}, []
    for b in range(frames):
        rows = []
        for n in range(per_frame):
            i, j = r + r * (n // side), r + r * (n % side)
            k = int(rs.integers(classes))
            imgs[b, i - r // 2:i - r // 2 + r, j - r // 2:j - r // 2 + r] = \
                proto[k] + noise * rs.standard_normal((r, r, C), dtype=np.float32)
            rows.append((i, j, 0.0))
            planted.append(k)
        coords[b] = np.array(rows, dtype=np.float64)
    planted = np.array(planted)
    return imgs, coords, planted


def bench_stat(frames=20, per_frame=1000, r=32, C=3, classes=10, noise=0.05, n_pca=4, em_iters=20, emit=True):
    """stat.imlocal on a synthetic stack of frames * per_frame windows of r x r x C (D = r r C) cut from frames that carry
    `classes` planted prototypes + noise: gmm(n_components=classes) and pca(n_pca) end to end, the EM pass kernel alone
    (event-timed; GB/s against the N D 4 bytes of the stack, which one pass must read at least once), and — if
    scikit-learn imports here — the reference-equivalent GaussianMixture(...).fit_predict on the same array in the same
    run."""
    imgs, coords, planted = _planted_stack(frames, per_frame, r, C, classes, noise)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    from atomai_amd.stat import _gmm
    import warnings
    _gmm.pass_timings = []
    try:
        s = aoi.stat.imlocal(imgs, coords, r, 0)
        N, D = s.d0, s.d1 * s.d2 * s.d3
        t0 = time.perf_counter()
        X = s._device_stack()
        if dev == "cuda":
            torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
        s.gmm(2)                                          # warm-up: library load, allocator, first launches
        _gmm.pass_timings.clear()
        t0 = time.perf_counter()
        cla, cl_all, cf = s.gmm(classes)
        t_gmm = time.perf_counter() - t0
        runs = list(_gmm.pass_timings)
        s.pca(1)
        t0 = time.perf_counter()
        comp, proj, _ = s.pca(n_pca)
        t_pca = time.perf_counter() - t0
        # the pass alone: a fit that is not allowed to stop, so that the median is over em_iters EM passes
        _gmm.pass_timings.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", _gmm.ConvergenceWarning)
            _gmm.fit_gmm(X, classes, "diag", 1, tol=0.0, max_iter=em_iters)
        if dev == "cuda":
            torch.cuda.synchronize()
        ms = {kind: [e0.elapsed_time(e1) for k, K, e0, e1 in _gmm.pass_timings if k == kind and K == classes]
              for kind in ("em", "lloyd")}
    finally:
        _gmm.pass_timings = None

    def purity(labels):
        return float(sum(np.bincount(planted[labels == c]).max() for c in np.unique(labels)) / len(labels))
    ours = cf[:, 2].astype(np.int64)
    n_run = {kind: sum(1 for k, K, _, _ in runs if k == kind and K == classes) for kind in ("em", "lloyd")}
    n_run["other"] = len(runs) - n_run["em"] - n_run["lloyd"]
    gb = N * D * 4 / 1e9
    med = {k: (float(np.median(v)) if v else None) for k, v in ms.items()}
    res = {"metric": f"stat.imlocal.gmm EM pass ({N} windows of {r}x{r}x{C}, D={D}, K={classes})",
           "value": None if med["em"] is None else round(med["em"], 3), "unit": "ms/pass", "n_gpus": 1, "dtype": "fp32 in, fp64 E step",
           "gb_per_s_vs_stack_bytes": None if med["em"] is None else round(gb / (med["em"] * 1e-3), 1),
           "stack_mb": round(gb * 1e3, 1), "em_passes": n_run["em"], "lloyd_passes": n_run["lloyd"],
           "em_passes_timed": len(ms["em"]),
           "ms_lloyd_pass": None if med["lloyd"] is None else round(med["lloyd"], 3), "other_passes": n_run["other"],
           "s_upload": round(t_up, 3), "s_gmm_end_to_end": round(t_gmm, 3), "s_pca_end_to_end": round(t_pca, 3),
           "purity_vs_planted": round(purity(ours), 4), "classes_found": int(ours.max())}
    log = [f"# python tools/bench_extra.py stat - {N} windows of {r}x{r}x{C} (D = {D}), {classes} planted classes, noise {noise}",
           f"upload of the fp32 stack ({res['stack_mb']} MB)      {t_up:8.3f} s",
           f"imlocal.gmm({classes}) end to end          {t_gmm:8.3f} s  ({res['lloyd_passes']} Lloyd + {res['em_passes']} EM passes "
           f"+ {res['other_passes']} seeding / label passes; purity against the planted classes {res['purity_vs_planted']})",
           f"imlocal.pca({n_pca}) end to end           {t_pca:8.3f} s"]
    if med["em"] is not None:
        log.append(f"amx_gmm_pass, EM (soft, K = {classes})   {med['em']:8.3f} ms/pass = {res['gb_per_s_vs_stack_bytes']} GB/s "
                   f"against N D 4 bytes (median of {len(ms['em'])} passes of a fit with tol = 0); Lloyd (hard) "
                   f"{med['lloyd']:.3f} ms/pass")
    try:
        from sklearn.mixture import GaussianMixture
    except ImportError:
        GaussianMixture = None
    if GaussianMixture is None:
        res["cpu_baseline"] = None
        log.append("scikit-learn does not import here: device figures alone")
    else:
        X = s.imgstack.reshape(N, D)
        t0 = time.perf_counter()
        clf = GaussianMixture(n_components=classes, covariance_type="diag", random_state=1)
        ref = clf.fit_predict(X)
        t_ref = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(t_ref, 3), "unit": "s", "kind": "sklearn GaussianMixture.fit_predict, same array, "
                               "same run", "n_iter": int(clf.n_iter_), "purity_vs_planted": round(purity(ref), 4),
                               "threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or None}
        log.append(f"sklearn GaussianMixture({classes}, 'diag').fit_predict on the host, same array: {t_ref:8.3f} s "
                   f"({clf.n_iter_} EM iterations, purity {res['cpu_baseline']['purity_vs_planted']})")
    res["log"] = log
    if emit:
        print("\n".join(log))
        print(json.dumps(res), flush=True)
    return res


def bench_knn(frames=64, per_frame=4000, nn=6, r=3, hw=512, reps=20, emit=True):
    """Nearest-neighbour analysis of a Locator dictionary: get_nn_distances and get_intensities end to end (host tables
    in, host arrays out), amx_knn alone (device events), and the reference's per-frame cKDTree loop where scipy imports."""
    from atomai_amd.utils import _knn
    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(per_frame)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:per_frame]
    coords = {}
    for f in range(frames):
        xy = 7.0 * ij + 8.0 + rng.uniform(-0.8, 0.8, (per_frame, 2))
        coords[f] = np.concatenate((xy, np.zeros((per_frame, 1))), axis=1)
    assert max(t[:, :2].max() for t in coords.values()) < hw - 2
    imgs = rng.uniform(0, 1, (frames, hw, hw)).astype(np.float32)
    k, N = nn + 1, frames * per_frame

    def wall(fn, n=3):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), out
    aoi.utils.get_nn_distances({0: coords[0]}, nn)                                  # warm-up: library load, allocator
    t_nn, (dists, pairs) = wall(lambda: aoi.utils.get_nn_distances(coords, nn))
    t_int, ints = wall(lambda: aoi.utils.get_intensities(coords, imgs, r))
    flat = torch.from_numpy(np.concatenate([t[:, :2] for t in coords.values()])).cuda()
    offs = np.arange(frames + 1, dtype=np.int64) * per_frame

    def kernel_ms(pts, seg):
        """amx_knn alone: tables and outputs made beforehand, device events around the one launch."""
        tiles = _knn.tile_table(seg)
        seg_d, tiles_d = torch.from_numpy(seg).cuda(), torch.from_numpy(tiles).cuda()
        dist = torch.empty(len(pts), k, dtype=torch.float64, device="cuda")
        idx = torch.empty(len(pts), k, dtype=torch.int64, device="cuda")
        out = []
        for i in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.call("amx_knn", L.ptr(pts), len(pts), L.ptr(pts), len(pts), 2, L.ptr(seg_d), L.ptr(seg_d), len(seg) - 1,
                   L.ptr(tiles_d), len(tiles), k, float("inf"), L.ptr(dist), L.ptr(idx), L.stream_ptr(pts))
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                out.append(e0.elapsed_time(e1))
        return out
    ms = kernel_ms(flat, offs)
    med = float(np.median(ms))
    pairs_eval = frames * per_frame ** 2
    flops = 5.0 * pairs_eval                          # two differences, two squares, one addition per pair (dim 2), fp64
    mb_in, mb_out = N * 2 * 8 / 1e6, N * k * 16 / 1e6
    one = torch.from_numpy(coords[0][:, :2].copy()).cuda()
    med1 = float(np.median(kernel_ms(one, np.array([0, per_frame], dtype=np.int64))))
    res = {"metric": f"amx_knn, k = {k}, {frames} frames x {per_frame} atoms in one launch (brute force, fp64)",
           "value": round(med, 3), "unit": "ms", "n_gpus": 1, "dtype": "fp64", "reps": reps,
           "pair_evaluations": pairs_eval, "tflops_fp64_at_5_per_pair": round(flops / (med * 1e-3) / 1e12, 2),
           "mb_in": round(mb_in, 1), "mb_out": round(mb_out, 1), "ms_one_frame_alone": round(med1, 3),
           "s_get_nn_distances": round(t_nn, 4), "s_get_intensities": round(t_int, 4)}
    log = [f"# python tools/bench_extra.py knn - {frames} frames x {per_frame} jittered-lattice atoms (spacing 7), nn = {nn}, "
           f"r = {r}, frames {hw} x {hw} float32",
           f"get_nn_distances(nn={nn}), host dictionary in, host lists out   {t_nn:8.4f} s (median of 3; one launch for "
           f"all frames, {sum(len(d) for d in dists)} rows kept)",
           f"get_intensities(r={r}), host arrays in (upload of {imgs.nbytes / 1e6:.0f} MB included), host lists out "
           f"{t_int:8.4f} s (median of 3)",
           f"amx_knn alone (one launch, tables resident), k = {k}               {med:8.3f} ms (median of {reps}, device events, "
           f"min {min(ms):.3f} max {max(ms):.3f})",
           f"   = {pairs_eval:.3e} pair evaluations (the search is O(n^2) per frame), {flops / (med * 1e-3) / 1e12:.2f} TFLOP/s fp64 "
           f"at 5 flops per pair; {mb_in:.1f} MB read once from HBM, {mb_out:.1f} MB written",
           f"amx_knn, one frame of {per_frame} atoms alone                      {med1:8.3f} ms (median of {reps})"]
    try:
        from scipy import spatial
    except ImportError:
        spatial = None
    if spatial is None:
        res["cpu_baseline"] = None
        log.append("scipy does not import here: the per-frame cKDTree loop was NOT measured")
    else:
        def ref_nn():
            out = []
            for t in coords.values():
                d, i = spatial.cKDTree(t[:, :2]).query(t[:, :2], k=k)
                out.append((d[:, 1:], t[i]))
            return out

        def ref_int():
            out = []
            for f, t in coords.items():
                img = imgs[f]
                out.append(np.array([np.mean(img[int(np.around(c[0])) - r // 2:int(np.around(c[0])) + r // 2 + 1,
                                                 int(np.around(c[1])) - r // 2:int(np.around(c[1])) + r // 2 + 1])
                                     for c in t]))
            return out
        t0 = time.perf_counter(); rn = ref_nn(); t_rn = time.perf_counter() - t0
        t0 = time.perf_counter(); ri = ref_int(); t_ri = time.perf_counter() - t0
        same = all(np.array_equal(a[1], b) for a, b in zip(rn, pairs))
        err = max(float(np.abs(a[0] - b).max()) for a, b in zip(rn, dists))
        res["cpu_baseline"] = {"s_ckdtree_loop": round(t_rn, 4), "s_intensity_loop": round(t_ri, 4), "same_neighbours": same,
                               "max_abs_distance_difference": err}
        log.append(f"host, same frames, same run: one scipy cKDTree per frame, query k = {k}        {t_rn:8.4f} s "
                   f"(neighbours identical: {same}, max |distance difference| {err:.1e})")
        log.append(f"host, same frames, same run: per-atom numpy window mean loop            {t_ri:8.4f} s")
    res["log"] = log
    if emit:
        print("\n".join(log))
        print(json.dumps(res), flush=True)
    return res


def bench_cluster(members=12, frames=64, per_frame=4000, sigma=0.15, eps=0.5, min_samples=10, reps=20, emit=True):
    """Density clustering of an ensemble's detections: every frame holds ``members`` jittered copies of one lattice of
    ``per_frame`` atoms.  The segmented DBSCAN alone (device table in, device labels out), the clustering of
    ensemble_locate end to end (host tables in, host means and variances out), and scikit-learn's DBSCAN frame by frame
    on the host where it imports, with the labels compared."""
    from atomai_amd.utils import _cluster
    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(per_frame)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:per_frame]
    stacks = []
    for f in range(frames):
        base = 7.0 * ij + 8.0 + rng.uniform(-0.8, 0.8, (per_frame, 2))
        stacks.append([np.concatenate((base + rng.normal(0.0, sigma, base.shape), np.zeros((per_frame, 1))), axis=1)
                       for _ in range(members)])
    n_seg = members * per_frame
    N = frames * n_seg
    offs = np.arange(frames + 1, dtype=np.int64) * n_seg

    def wall(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts, out
    flat = torch.from_numpy(np.concatenate([t[:, :2] for st in stacks for t in st])).cuda()
    _cluster.dbscan(flat[:n_seg].contiguous(), eps, min_samples)                    # warm-up: library load, allocator
    ts, (labels, core, rounds) = wall(lambda: _cluster.dbscan(flat, eps, min_samples, offs), reps)
    med = float(np.median(ts))
    ts1, _ = wall(lambda: _cluster.dbscan(flat[:n_seg].contiguous(), eps, min_samples), reps)
    t_e2e, (means, variances) = wall(lambda: aoi.utils.cluster_coord_frames(stacks, eps, min_samples), 3)
    t_e2e = float(np.median(t_e2e))
    labels = labels.cpu().numpy()
    res = {"metric": f"segmented DBSCAN, {frames} frames x {members} members x {per_frame} atoms in one pass (fp64, cell grid)",
           "value": round(med * 1e3, 3), "unit": "ms", "n_gpus": 1, "dtype": "fp64", "reps": reps, "points": N,
           "rounds": rounds, "clusters": int(sum(len(m) for m in means)), "noise_rows": int((labels < 0).sum()),
           "ms_one_frame_alone": round(float(np.median(ts1)) * 1e3, 3), "s_cluster_coord_frames": round(t_e2e, 4)}
    log = [f"# python tools/bench_extra.py cluster - {frames} frames x {members} members x {per_frame} jittered-lattice atoms "
           f"(spacing 7, sigma = {sigma} px), eps = {eps}, min_samples = {min_samples}: {N} rows",
           f"segmented DBSCAN alone (device table in, labels out, sorts and read-backs included)  {med * 1e3:9.3f} ms "
           f"(median of {reps}, wall clock around a synchronised call, min {min(ts) * 1e3:.3f} max {max(ts) * 1e3:.3f}); "
           f"{rounds} rounds of hooking",
           f"segmented DBSCAN, one frame of {n_seg} rows alone                                      "
           f"{float(np.median(ts1)) * 1e3:9.3f} ms (median of {reps})",
           f"cluster_coord_frames, host tables in, host means and variances out                     {t_e2e:9.4f} s "
           f"(median of 3; {res['clusters']} clusters kept, {res['noise_rows']} noise rows)"]
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    if DBSCAN is None:
        res["cpu_baseline"] = None
        log.append("scikit-learn does not import here: the per-frame DBSCAN on the host was NOT measured")
    else:
        t0 = time.perf_counter()
        ref_means, same = [], True
        for f, st in enumerate(stacks):                      # the host path of ensemble_locate before this kernel
            every = np.empty((0, 3))
            for t in st:
                every = np.append(every, t, axis=0)
            lab = DBSCAN(eps=eps, min_samples=min_samples).fit(every[:, :2]).labels_
            ref_means.append(np.array([np.mean(every[lab == c, :2], axis=0) for c in np.unique(lab)[1:]]))
            same = same and np.array_equal(lab, labels[offs[f]:offs[f + 1]])
        t_ref = time.perf_counter() - t0
        err = max(float(np.abs(a - b).max()) for a, b in zip(ref_means, means) if len(a))
        res["cpu_baseline"] = {"s_sklearn_loop": round(t_ref, 4), "same_labels": bool(same), "max_abs_mean_difference": err}
        log.append(f"host, same tables, same run: np.append + sklearn DBSCAN + per-label means, per frame  {t_ref:9.4f} s "
                   f"(labels identical: {same}, max |mean difference| {err:.1e})")
    res["log"] = log
    if emit:
        print("\n".join(log))
        print(json.dumps(res), flush=True)
    return res


def bench_nmf(hw=512, k=4, iters=1000, reps=20, emit=True):
    """NMF on the device at the reference's own SlidingFFTNMF setting: a ``hw`` x ``hw`` image gives 841 windows of 64 x 64
    and 4096 features each.  ``fit_nmf`` for ``iters`` iterations (tol = 0, init='random') against scikit-learn on the
    host where it imports, the two half-steps' product kernels alone (device events; achieved bytes/s of X), the FFT
    front end alone, and ``analyze_image`` end to end."""
    import tempfile
    from atomai_amd.stat import _nmf
    from atomai_amd.stat.fft_nmf import SlidingFFTNMF
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[:hw, :hw]
    img = (np.where(xx < hw // 2, np.sin(2 * np.pi * xx / 6.0) * np.sin(2 * np.pi * yy / 6.0), np.sin(2 * np.pi * (xx + yy) / 9.0))
           + np.where(yy < hw // 3, np.sin(2 * np.pi * yy / 4.0), 0.0) + 0.2 * rng.normal(size=(hw, hw)))

    def wall(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts, out
    s = SlidingFFTNMF(components=k)
    norm = s._normalised(img)
    s._features(norm, s.windows_shape)                                   # warm-up: library load, allocator
    t_fft, X = wall(lambda: s._features(norm, s.windows_shape), reps)
    n, d = X.shape
    _nmf.fit_nmf(X, k, init="random", random_state=42, tol=0, max_iter=3)
    t_fit, res = wall(lambda: _nmf.fit_nmf(X, k, init="random", random_state=42, tol=0, max_iter=iters), 3)
    t_fit = float(np.median(t_fit))
    X32 = X.to(torch.float32)
    halves = {}
    for tag, Xd in (("float64", X), ("float32", X32)):
        W, Ht = res["W"].clone(), res["H"].T.contiguous()
        hw_, hh = _nmf._Half(Xd, k, 0, W), _nmf._Half(Xd, k, 1, Ht)
        for name, half, F in (("W", hw_, Ht), ("Ht", hh, W)):
            ev = []
            for _ in range(reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.call("amx_nmf_xf", L.ptr(Xd), int(Xd.dtype == torch.float64), n, d, half.trans, L.ptr(F), k, L.ptr(half.P),
                       L.stream_ptr(Xd))
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            ms = float(np.median([a.elapsed_time(b) for a, b in ev[3:]]))
            halves[f"{tag}_{name}"] = {"ms": round(ms, 4), "splits": half.S,
                                       "GBps_of_X": round(n * d * Xd.element_size() / ms / 1e6, 1)}
    with tempfile.TemporaryDirectory() as tmp:
        t_all, (comp, ab) = wall(lambda: SlidingFFTNMF(components=k).analyze_image(img, os.path.join(tmp, "b")), 3)
    t_all = float(np.median(t_all))
    fft_ms = float(np.median(t_fft)) * 1e3
    res_d = {"metric": f"fit_nmf, {n} x {d} float64, k = {k}, init='random', {iters} iterations (tol = 0)",
             "value": round(t_fit, 4), "unit": "s", "n_gpus": 1, "dtype": "fp64", "ms_per_iteration": round(t_fit / iters * 1e3, 4),
             "xf_kernels": halves, "ms_fft_front_end": round(fft_ms, 3), "s_analyze_image": round(t_all, 4),
             "analyze_image_shapes": [list(comp.shape), list(ab.shape)]}
    log = [f"# python tools/bench_extra.py nmf - {hw} x {hw} image, windows {s.window_size_x} x {s.window_size_y}, step "
           f"{s.window_step_x}: {n} windows x {d} features, k = {k}",
           f"fit_nmf, float64 X, init='random', {iters} iterations (tol = 0), one read-back per iteration   {t_fit:9.4f} s "
           f"(median of 3, wall clock; {t_fit / iters * 1e3:.4f} ms per iteration = 2 half-steps)"]
    for key, v in halves.items():
        log.append(f"amx_nmf_xf alone, {key:<11s} ({v['splits']:2d} splits)   {v['ms']:8.4f} ms (median of {reps}, device events) = "
                   f"{v['GBps_of_X']:8.1f} GB/s of X")
    log += [f"amx_fftwin, {n} windows read in place from the image                                   {fft_ms:9.3f} ms "
            f"(median of {reps}, wall clock, tables and read-back of the flag included)",
            f"SlidingFFTNMF.analyze_image end to end (to convergence at tol = 1e-4, .npy files written)      {t_all:9.4f} s "
            f"(median of 3)"]
    try:
        from sklearn.decomposition import NMF
    except ImportError:
        NMF = None
    if NMF is None:
        res_d["cpu_baseline"] = None
        log.append("scikit-learn does not import here: NMF on the host was NOT measured")
    else:
        import warnings
        Xh = X.cpu().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            m = NMF(k, init="random", random_state=42, tol=0, max_iter=iters, solver="cd")
            Wh = m.fit_transform(Xh)
            t_ref = time.perf_counter() - t0
        err = max(float(np.abs(res["W"].cpu().numpy() - Wh).max() / np.abs(Wh).max()),
                  float(np.abs(res["H"].cpu().numpy() - m.components_).max() / np.abs(m.components_).max()))
        res_d["cpu_baseline"] = {"s_sklearn": round(t_ref, 4), "n_iter": int(m.n_iter_), "max_rel_difference": err}
        log.append(f"host, same matrix, same run: sklearn NMF(solver='cd'), {m.n_iter_} iterations                       "
                   f"{t_ref:9.4f} s (max difference over max value of W, H: {err:.1e})")
    res_d["log"] = log
    if emit:
        print("\n".join(log))
        print(json.dumps(res_d), flush=True)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "profiles", "nmf_bench.log"), "w") as f:
            f.write("\n".join(log) + "\n")
    return res_d


def bench_ica(frames=20, per_frame=1000, r=32, C=3, classes=10, noise=0.05, k=10, reps=20, emit=True):
    """FastICA on the device at the stat benchmark's own stack (frames * per_frame windows of r x r x C, planted classes),
    k components, random_state = 1: ``fit_ica`` end to end (wall clock around a synchronise), its split into Gram + eigh,
    projection and iterations (device events), the step + reduce pair alone (device events; bytes of X1 per second), the
    same iteration written as torch fp64 operations on the device, interleaved with the fused pair and with a second
    series of the fused pair (the A/A spread), and -- where scikit-learn imports -- FastICA on the host on the same matrix."""
    import warnings
    from atomai_amd.stat import _ica
    from atomai_amd.stat.nmf import _stack_matrix
    imgs, coords, _ = _planted_stack(frames, per_frame, r, C, classes, noise)
    X = torch.from_numpy(_stack_matrix(aoi.stat.imlocal(imgs, coords, r, 0))).cuda()
    n, d = X.shape

    def events(fn, n_rep):
        """Median and the individual times (ms) of ``n_rep`` runs of fn between device events, 3 warm-up runs dropped."""
        ev = []
        for _ in range(n_rep + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev[3:]]
        return float(np.median(ms)), ms

    def fit():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return _ica.fit_ica(X, k, random_state=1)
    fit()                                                                # warm-up: library load, allocator, BLAS, eigh
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fit()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t_fit = float(np.median(ts))
    ms_white, _ = events(lambda: _ica._whitening(X, k), reps)
    mean, K, u, sigma = _ica._whitening(X, k)
    ms_proj, _ = events(lambda: _ica.project(X, mean, K, np.sqrt(n)), reps)
    X1 = _ica.project(X, mean, K, np.sqrt(n))
    W = _ica.sym_decorrelation(torch.from_numpy(np.random.RandomState(1).normal(size=(k, k))).cuda())
    step = _ica._Step(X1, 0, 1.0)

    def fused_iteration():
        W1 = _ica.sym_decorrelation(step.run(W))
        return ((W1 * W).sum(1).abs() - 1.0).abs().max()

    def torch_step():
        g = torch.tanh(W @ X1)
        return g @ X1.T / n - (1.0 - g * g).mean(1)[:, None] * W

    def torch_iteration():
        W1 = _ica.sym_decorrelation(torch_step())
        return ((W1 * W).sum(1).abs() - 1.0).abs().max()
    ms_iter, _ = events(lambda: float(fused_iteration()), reps)           # with the read-back of lim, as in the fit
    ms_iter_torch, _ = events(lambda: float(torch_iteration()), reps)
    ab = {"fused_a": [], "torch": [], "fused_b": []}                     # interleaved: fused, torch, fused, ...
    for rep in range(reps + 3):
        for tag, fn in (("fused_a", lambda: step.run(W)), ("torch", torch_step), ("fused_b", lambda: step.run(W))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ab[tag].append((e0, e1))
    torch.cuda.synchronize()
    ab = {tag: float(np.median([a.elapsed_time(b) for a, b in ev[3:]])) * 1e3 for tag, ev in ab.items()}     # us
    us_fused = 0.5 * (ab["fused_a"] + ab["fused_b"])
    spread = abs(ab["fused_a"] - ab["fused_b"])
    diff = float((step.run(W) - torch_step()).abs().max())
    res_d = {"metric": f"fit_ica, {n} x {d} float32 stack, k = {k}, logcosh, random_state = 1, tol = 1e-4",
             "value": round(t_fit, 4), "unit": "s", "n_gpus": 1, "dtype": "fp64", "n_iter": res["n_iter"],
             "converged": res["converged"], "ms_gram_eigh": round(ms_white, 3), "ms_projection": round(ms_proj, 3),
             "ms_one_iteration": round(ms_iter, 4), "ms_one_iteration_torch_step": round(ms_iter_torch, 4),
             "us_step_reduce_fused": round(us_fused, 2),
             "us_step_torch_ops": round(ab["torch"], 2), "us_fused_a_a_spread": round(spread, 2),
             "GBps_of_X1": round(k * n * 8 / us_fused / 1e3, 1), "blocks": step.G, "fused_vs_torch_max_abs": diff}
    log = [f"# python tools/bench_extra.py ica - {n} windows x {d} features (float32 stack), k = {k}, logcosh, "
           f"random_state = 1, one run",
           f"fit_ica end to end, {res['n_iter']} iterations, converged {res['converged']}            {t_fit:9.4f} s "
           f"(median of {reps}, wall clock around a synchronise)",
           f"  Gram matrix over chunks + eigh + sign rule (whitening)                 {ms_white:9.3f} ms (median of {reps}, device events)",
           f"  projection X1 = sqrt(n) K (X - mean)^T (amx_ica_project)               {ms_proj:9.3f} ms (median of {reps}, device events)",
           f"  one iteration: step, reduce, decorrelation (eigh), lim read back       {ms_iter:9.4f} ms (median of {reps}, device events)",
           f"  the same iteration with the step written as torch fp64 operations     {ms_iter_torch:9.4f} ms (median of {reps}, device events)",
           f"step + reduce alone (amx_ica_step, amx_ica_reduce; {step.G} workgroups)       {us_fused:9.2f} us (median of {reps}, "
           f"device events, mean of the two interleaved series) = {res_d['GBps_of_X1']} GB/s of X1",
           f"the same step as torch fp64 operations, interleaved in the same run      {ab['torch']:9.2f} us; A/A spread of the "
           f"fused pair {spread:.2f} us; results agree within {diff:.1e} (max abs)"]
    try:
        from sklearn.decomposition import FastICA
    except ImportError:
        FastICA = None
    if FastICA is None:
        res_d["cpu_baseline"] = None
        log.append("scikit-learn does not import here: FastICA on the host was NOT measured")
    else:
        Xh = X.cpu().numpy().astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            m = FastICA(k, random_state=1)
            Sh = m.fit_transform(Xh)
            t_ref = time.perf_counter() - t0
        err = max(float(np.abs(res["sources"].cpu().numpy() - Sh).max() / np.abs(Sh).max()),
                  float(np.abs(res["components"].cpu().numpy() - m.components_).max() / np.abs(m.components_).max()))
        res_d["cpu_baseline"] = {"s_sklearn": round(t_ref, 4), "n_iter": int(m.n_iter_), "max_rel_difference": err}
        log.append(f"host, same matrix (as float64), same run: sklearn FastICA, {m.n_iter_} iterations      {t_ref:9.4f} s "
                   f"(one run; max difference over max value of sources, components: {err:.1e})")
    res_d["log"] = log
    if emit:
        print("\n".join(log))
        print(json.dumps(res_d), flush=True)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "profiles", "ica_bench.log"), "w") as f:
            f.write("\n".join(log) + "\n")
    return res_d


if __name__ == "__main__":
    what = sys.argv[1:] or ["rvae", "predict"]
    unfused_head = "--unfused-head" in what            # denoiser: time the three-launch tail instead of the fused head
    what = [w for w in what if w != "--unfused-head"]
    os.makedirs("gpurun_out", exist_ok=True)
    res = {}
    for w in what:
        if w == "denoiser":
            res[w] = bench_denoiser(fused_head=not unfused_head)
            continue
        res[w] = {"rvae": bench_rvae, "jrvae": bench_jrvae, "predict": bench_predict, "dkl": bench_dkl, "dklfit": bench_dkl_fit, "locate": bench_locate, "refine": bench_refine, "stat": bench_stat, "knn": bench_knn, "cluster": bench_cluster, "nmf": bench_nmf, "ica": bench_ica, "segfamily": bench_segfamily, "losses": bench_losses, "imspec": bench_imspec,
                  "predict4096": bench_predict_full}[w]()
    json.dump(res, open("gpurun_out/bench_extra.json", "w"), indent=1)
