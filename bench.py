"""Headline benchmark: per-channel int8 QDQ of a 4096 x 4096 bf16 weight on MI355X.

  python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run)
                  [--dump-outputs DIR]                 (the last timed step's output, sampled rows, as .npy)

One "step" = one pass of the hot path over one weight: sbq_quant_perchannel_forward
(bf16 in -> bf16 out, per-channel symmetric int8, scales from the minmax observer), called
through the C ABI with caller-allocated buffers that are already resident in HBM.  To keep
the number an HBM number, the steps rotate over 12 distinct input/output pairs (805 MB,
larger than the 256 MiB Infinity Cache); the cache-resident rate is reported separately.
Multi-GPU is weak scaling with no data-path collective: each rank quantizes its own
weights; the observer statistic all-reduce (RCCL) is timed beside it.

Prints ONE JSON line on rank 0 (contract: see the round prompt / DESIGN.md section 6).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = COLS = 4096
NBUF = 12
DUMP_ROWS = 2048  # --dump-outputs: half of the output's rows (32 MiB as float32; all of them would be 64 MiB)
QMIN, QMAX = -128, 127
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
BYTES_PER_ELEM = 4  # algorithmic: 2 B read + 2 B written (bf16 -> bf16), SURVEY.md 8(d)


def ctypes_stream(s):
    import ctypes

    return ctypes.c_void_p(s.cuda_stream)


def make_weight(seed):
    """randn * logspace(-2, 1) row scales, bf16."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(ROWS, COLS, generator=g) * torch.logspace(-2, 1, ROWS).unsqueeze(1)
    return w.bfloat16()


def sample_clocks(index):
    """current engine / memory clock of GPU `index` from the amdgpu sysfs tables (the entry marked '*'); best effort"""
    import glob

    out = {}
    cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device/pp_dpm_sclk"))
    if index < len(cards):
        base = os.path.dirname(cards[index])
        for key, name in (("sclk_mhz", "pp_dpm_sclk"), ("mclk_mhz", "pp_dpm_mclk")):
            try:
                with open(os.path.join(base, name)) as f:
                    for ln in f:
                        if ln.strip().endswith("*"):
                            out[key] = int("".join(ch for ch in ln.split(":")[1] if ch.isdigit()))
            except (OSError, ValueError, IndexError):
                pass
    return out


def self_launch(n):
    """Re-run this command line under `python -m torch.distributed.run --nnodes=1 --nproc-per-node n` on a free
    local port; returns the launcher's exit code (rank 0 prints the JSON line to the inherited stdout)."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this stack
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--reference", default=os.environ.get("SBQ_REFERENCE"),
                    help="checkout of megvii-research/Sparsebit: the CPU baseline is then the REAL reference's Quantizer "
                         "(tools/reference_cpu_baseline.py, kind 'reference'); without one, oracle/torch_port.py (kind 'port')")
    ap.add_argument("--quick", action="store_true",
                    help="headline + multi-GPU plumbing only: no config legs, no CPU baseline (tests/test_gpu_bench_n2.py)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR/qdq_output.npy (rank 0): %d of its %d output rows, "
                         "a fixed seeded sample, as float32" % (DUMP_ROWS, ROWS))
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` started like the N = 1 command: become the launcher the contract describes
        # (one process per GPU under torch.distributed.run, rendezvous on 127.0.0.1) and hand its exit code back
        sys.exit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d: launch with torch.distributed.run --nproc-per-node %d" % (
        world, args.gpus, args.gpus)
    assert torch.cuda.is_available(), "bench.py measures the HIP path: it needs an MI355X"
    # SBQ_BENCH_DEBUG_SINGLE_GPU=1: rehearse the N > 1 control flow on a one-GPU box (every rank on
    # cuda:0, gloo instead of RCCL).  Never set by the driver; numbers from such a run mean nothing.
    debug_one_gpu = os.environ.get("SBQ_BENCH_DEBUG_SINGLE_GPU") == "1"
    dev_index = 0 if debug_one_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)

    import torch.distributed as dist

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if debug_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI

    from sparsebit_amd import dist as sbq_dist
    from sparsebit_amd import lib as L
    from sparsebit_amd import ops
    from sparsebit_amd.common import Backend
    from sparsebit_amd.config import quantizer_config
    from sparsebit_amd.quantizers import build_quantizer

    lib = L.load()  # raises if libsbq.so / a symbol is missing: no fallback

    # ---- data: NBUF distinct weights per rank, resident in HBM ---------------------------
    host = make_weight(1000 * rank)
    xs = [host.to(dev)]
    for i in range(1, NBUF):
        xs.append(torch.roll(xs[0], shifts=i, dims=1).contiguous())  # same row statistics, distinct buffers
    ys = [torch.empty_like(x) for x in xs]

    # ---- calibration through the product API (minmax observer -> scale / zero_point) ------
    q = build_quantizer(quantizer_config("per-channel-symmetric", 8, observer="MINMAX"))
    q.set_backend(Backend.VIRTUAL)
    q.update_observer(xs[0])
    scale, zp = q.calc_qparams()
    scale = scale.reshape(-1).contiguous()
    zp = zp.reshape(-1).contiguous()

    stream = torch.cuda.current_stream(dev)
    st = L.stream_ptr(dev)
    xp = [L.ptr(x) for x in xs]
    yp = [L.ptr(y) for y in ys]
    sp, zpp = L.ptr(scale), L.ptr(zp)
    fwd = lib.sbq_quant_perchannel_forward

    def step(i):
        j = i % NBUF
        rc = fwd(xp[j], L.BF16, yp[j], L.BF16, None, L.Q_NONE, sp, zpp, 1, ROWS, COLS, QMIN, QMAX, 0, st)
        if rc:
            L.check(rc)

    flag = torch.zeros(1, device=dev)

    def sync_all():
        """barrier + synchronize.  Over RCCL the barrier is what dist.barrier() is underneath -- a
        one-element all-reduce, which cannot complete before every rank has enqueued it -- issued
        stream-ordered behind the launches, so the closing bracket costs one tiny collective and one
        host wait instead of two host round trips."""
        if world > 1:
            if debug_one_gpu:
                torch.cuda.synchronize(dev)
                dist.barrier()
            else:
                dist.all_reduce(flag)
        torch.cuda.synchronize(dev)

    # ---- parity gates inside the benchmark (rank 0): the timed kernel == oracle ----------
    # q_int bit-exact, dq_f32 within 1e-6 relative (0 ulp expected), bf16 output == RNE(ref), observer (min, max)
    # and (scale, zp) bit-exact -- bench_configs.headline_gates; BEFORE the timed region so that a wrong kernel
    # is never timed.
    import bench_configs as BC

    ctx = BC.Ctx(dev, lib, L, ops, stream, host, xs, ys, scale, zp)
    parity = None
    gates = None
    if rank == 0:
        gates = BC.headline_gates(ctx)
        parity = gates["all"]
        assert parity, "timed kernel does not match the oracle: %r" % (gates,)
    # --dump-outputs: the sampled rows of the last timed step's output are gathered on the device right after the timed
    # region (the legs after it write into the same output buffers) and written to disk once the kernel windows are done
    dump = None
    if args.dump_outputs and rank == 0:
        rows = torch.randperm(ROWS, generator=torch.Generator().manual_seed(0))[:DUMP_ROWS].sort().values
        dump = (rows.to(dev), torch.empty(DUMP_ROWS, COLS, dtype=torch.bfloat16, device=dev))

    # ---- timed region ------------------------------------------------------------------------
    # K direct C-ABI launches on the current stream.  (Replaying the same launches from a
    # hipGraph was measured 1.1-1.4 us per kernel SLOWER on this stack -- 14.9-15.3 vs
    # 13.7-13.9 us -- so the plain in-order stream is the fast path, and the host loop keeps
    # ahead of a ~13 us kernel.)
    # Everything that could stall the host or idle the GPU goes BEFORE the warm-up: event
    # creation (lazy on first record), a garbage collection, then no more allocation.
    import gc

    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    step(0)
    e1.record(stream)
    sync_all()
    e0.elapsed_time(e1)
    gc.collect()
    gc.disable()
    # Untimed pre-warm-up: ~0.25 s of the same launches so that the GPU has left its idle
    # power state before the W warm-up steps (W x 14 us alone is shorter than the DVFS ramp:
    # launches right after an idle period measured 7-8 % slower than steady state, and K = 500
    # steps are only 7 ms, so the clock state at entry decides the result).
    # Adaptive: windows of 1024 launches until two consecutive windows agree within 1 % (at
    # least 0.25 s, at most 3 s) -- a box that was idle for minutes needs longer than a warm one.
    t_pre = time.perf_counter()
    prev, i, stable = None, 0, 0
    windows = []  # us per launch of every 1024-launch window
    w0 = torch.cuda.Event(enable_timing=True)
    w1 = torch.cuda.Event(enable_timing=True)

    def window(during=None):
        """1024 launches between two events -> us per launch; `during` runs on the host while they execute"""
        nonlocal i
        w0.record(stream)
        for _ in range(1024):
            step(i)
            i += 1
        w1.record(stream)
        if during is not None:
            during()
        torch.cuda.synchronize(dev)
        return w0.elapsed_time(w1) * 1e3 / 1024

    # the same criterion on every box: three consecutive windows within 0.5 % of each other (at least 0.25 s, at
    # most 3 s of launches)
    while True:
        cur = window()
        stable = stable + 1 if prev is not None and abs(cur - prev) <= 0.005 * cur else 0
        prev = cur
        windows.append(cur)
        spent = time.perf_counter() - t_pre
        if (spent >= 0.25 and stable >= 3) or spent >= 3.0:
            break
    prewarm_s = time.perf_counter() - t_pre
    for i in range(args.warmup):
        step(i)
    sync_all()  # barrier + synchronize; the GPU idles only for this instant before the timed region
    # (nothing but the K launches between the two brackets: an event record is a packet of its own in front of the first
    # kernel and another one the closing synchronize has to wait for -- at K = 20 those are whole per-cents of the region)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    sync_all()
    t1 = time.perf_counter()
    if dump is not None:
        torch.index_select(ys[(args.steps - 1) % NBUF], 0, dump[0], out=dump[1])
    wall = t1 - t0
    kern_us_timed = wall * 1e6 / args.steps  # the timed region itself: launch + synchronisation latency included
    # The kernel's duration for the roofline: NOT the K timed launches alone (K = 20 is a 0.25 ms sample) but windows
    # of 1024 launches on both sides of the timed region -- the last four of the pre-warm-up and eight right after it --
    # median, with min and max beside it.  The engine / memory clocks are sampled while the first of them runs.
    clocks = {}
    post = [window(during=lambda: clocks.update(sample_clocks(dev_index)))]
    post += [window() for _ in range(7)]
    gc.enable()
    if dump is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "qdq_output.npy"), dump[1].cpu().float().numpy())
    around = sorted(windows[-4:] + post)
    kern_us = 0.5 * (around[(len(around) - 1) // 2] + around[len(around) // 2])  # median
    if world > 1:
        t = torch.tensor([wall, kern_us_timed, kern_us], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, kern_us_timed, kern_us = t.tolist()

    n_elem = ROWS * COLS
    value = world * args.steps * n_elem / wall
    achieved = n_elem * BYTES_PER_ELEM / (kern_us * 1e-6) / 1e9

    # ---- secondary measurements (outside the timed region) -------------------------------------
    def timed(fn, iters):
        for i in range(10):
            fn(i)
        torch.cuda.synchronize(dev)
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for i in range(iters):
            fn(i)
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / iters

    def pmc_extra(kernel_key):
        """counter summary of a kernel from the committed profile (None when there is none)"""
        try:
            with open(os.path.join(ROOT, "profiles", "pmc_latest.json")) as f:
                return json.load(f).get("valu", {}).get(kernel_key)
        except (OSError, ValueError):
            return None

    extras = {}
    warm_us = timed(lambda i: step(0), 200)
    extras["cache_resident_us"] = round(warm_us, 3)
    extras["cache_resident_GBps"] = round(n_elem * BYTES_PER_ELEM / warm_us / 1e3, 1)
    y32 = torch.empty(ROWS, COLS, dtype=torch.float32, device=dev)

    def step_f32(i):
        fwd(xp[i % NBUF], L.BF16, L.ptr(y32), L.F32, None, L.Q_NONE, sp, zpp, 1, ROWS, COLS, QMIN, QMAX, 0, st)

    f32_us = timed(step_f32, 100)
    extras["bf16_to_fp32_us"] = round(f32_us, 3)
    extras["bf16_to_fp32_GBps"] = round(n_elem * 6 / f32_us / 1e3, 1)
    mn_o = torch.empty(ROWS, dtype=torch.float32, device=dev)
    mx_o = torch.empty(ROWS, dtype=torch.float32, device=dev)
    ws = torch.empty(max(lib.sbq_stats_workspace_bytes(1, ROWS, COLS), 16), dtype=torch.uint8, device=dev)

    def step_stats(i):
        lib.sbq_channel_stats(xp[i % NBUF], L.BF16, 1, ROWS, COLS, L.ptr(mn_o), L.ptr(mx_o), None, L.ptr(ws),
                              ws.numel(), st)

    obs_us = timed(step_stats, 100)
    extras["minmax_observer_us"] = round(obs_us, 3)
    extras["minmax_observer_GBps"] = round(n_elem * 2 / obs_us / 1e3, 1)

    # multi-tensor launch: 6 of the weights per kernel (two alternating groups of 6 pairs, each
    # 403 MB > Infinity Cache), same arithmetic, reported per weight
    half = NBUF // 2
    groups = []
    for gi in range(2):
        sl = slice(gi * half, (gi + 1) * half)
        groups.append(ops.BatchedFakeQuant(xs[sl], [scale] * half, [zp] * half, QMIN, QMAX, 0, torch.bfloat16,
                                           outs=ys[sl]))
    bat_us = timed(lambda i: groups[i % 2](), 60) / half
    extras["batched_%d_weights_per_launch_us_per_weight" % half] = round(bat_us, 3)
    extras["batched_GBps"] = round(n_elem * BYTES_PER_ELEM / bat_us / 1e3, 1)
    extras["batched_frac_of_peak"] = round(n_elem * BYTES_PER_ELEM / bat_us / 1e3 / HBM_PEAK_GBS, 4)

    # model-wide launch: every conv / fc weight of a ResNet-50 (BASELINE configs 1, 2, 5; synthetic
    # fp32 masters, 4-bit per channel) one launch per layer vs ONE grid for all of them
    rshapes = []
    inp = 64
    for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            rshapes += [(width, inp, 1, 1), (width, width, 3, 3), (width * 4, width, 1, 1)]
            if b == 0:
                rshapes.append((width * 4, inp, 1, 1))
            inp = width * 4
    rshapes.append((1000, 2048))
    gw = torch.Generator().manual_seed(5)
    rentries = []
    for shp in rshapes:
        w_ = torch.randn(shp, generator=gw).to(dev)
        mn_, mx_, _ = ops.channel_stats(w_, 0, True)
        s_, z_ = ops.qparams_from_minmax(mn_, mx_, -8, 7, True)
        rentries.append((w_, s_, z_, -8, 7))
    gq = ops.GroupFakeQuant(rentries)
    r_elem = sum(e[0].numel() for e in rentries)
    grp_us = timed(lambda i: gq(), 60)

    def per_layer(i):
        for (w_, s_, z_, lo, hi) in rentries:
            ops.fake_quant(w_, s_, z_, lo, hi, 0)

    lay_us = timed(per_layer, 10)
    extras["resnet50_%d_weights_one_launch_us" % len(rentries)] = round(grp_us, 2)
    extras["resnet50_weights_one_launch_GBps"] = round(r_elem * 8 / grp_us / 1e3, 1)
    extras["resnet50_weights_launch_per_layer_us"] = round(lay_us, 1)

    # the same single-weight launches issued alternately on two HIP streams (independent
    # quantizers of different layers may overlap: one kernel's tail hides the next one's ramp)
    s2 = torch.cuda.Stream(device=dev)
    st2 = ctypes_stream(s2)
    s2.wait_stream(stream)

    def step_two_streams(i):
        j = i % NBUF
        fwd(xp[j], L.BF16, yp[j], L.BF16, None, L.Q_NONE, sp, zpp, 1, ROWS, COLS, QMIN, QMAX, 0, st2 if i & 1 else st)

    for i in range(20):
        step_two_streams(i)
    torch.cuda.synchronize(dev)
    t_a = time.perf_counter()
    for i in range(400):
        step_two_streams(i)
    torch.cuda.synchronize(dev)
    two_us = (time.perf_counter() - t_a) * 1e6 / 400
    extras["two_streams_us_per_weight"] = round(two_us, 3)
    extras["two_streams_GBps"] = round(n_elem * BYTES_PER_ELEM / two_us / 1e3, 1)

    # observer statistic exchange (BASELINE: "observer all-reduce scaling"), timed at every N:
    #   minmax      ONE MAX all-reduce of [max, -min, nan flags] for C = 4096           (64 KB)
    #   MSE         + ONE SUM of the fp64 [C, 80] squared-error table                   (2.6 MB)
    #   percentile  ONE SUM of the int64 [1, 2, 2048] histogram per radix pass          (32 KB, x 3 passes)
    mn, mx, _ = ops.channel_stats(xs[0], 0, True)
    sse_t = torch.zeros(ROWS, L.MSE_CANDIDATES, dtype=torch.float64, device=dev)
    hist_t = torch.zeros(1, 2, L.RADIX_BINS, dtype=torch.int64, device=dev)
    with sbq_dist.sharded_calibration():
        ar_us = timed(lambda i: sbq_dist.allreduce_minmax(mn, mx), 50) if world > 1 else 0.0
        ar_mse_us = timed(lambda i: sbq_dist.allreduce_sum_(sse_t), 50) if world > 1 else 0.0
        ar_hist_us = timed(lambda i: sbq_dist.allreduce_sum_(hist_t), 50) if world > 1 else 0.0
    ar_bytes = (4 * 4 * ROWS, sse_t.numel() * 8, hist_t.numel() * 8)
    if world == 1 and not args.quick:
        # N = 1: the same three collectives on a ONE-rank RCCL communicator (tools/rccl_ws1.py, in a subprocess with a
        # timeout: a hung rendezvous must not take the benchmark with it) -- the launch + RCCL-kernel floor that the
        # xGMI hops of N > 1 add to, and the first time RCCL itself runs under sparsebit_amd.dist
        import subprocess

        ws1 = {"ran": False}
        try:
            env = dict(os.environ)
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_ws1.py")], env=env, capture_output=True,
                               text=True, timeout=240)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode == 0 and lines:
                ws1 = json.loads(lines[-1])
                ws1["ran"] = True
                lat = ws1["latency"]
                ar_us, ar_mse_us, ar_hist_us = (lat["minmax_pack_allreduce_unpack_us"], lat["mse_sum_us"],
                                                lat["percentile_hist_sum_us"])
                ar_bytes = (lat["minmax_bytes"], lat["mse_sum_bytes"], lat["percentile_hist_sum_bytes"])
            else:
                ws1["error"] = (r.stderr or r.stdout)[-400:]
        except Exception as e:  # noqa: BLE001  (timeout, missing RCCL: the headline line must still print)
            ws1["error"] = repr(e)[:400]
        extras["rccl_world_size_1"] = ws1
    measured = world > 1 or ar_us > 0.0
    extras["observer_allreduce_us"] = round(ar_us, 2)
    extras["observer_allreduce_bytes"] = ar_bytes[0] if measured else 0
    extras["observer_allreduce_mse_sum_us"] = round(ar_mse_us, 2)
    extras["observer_allreduce_mse_sum_bytes"] = ar_bytes[1] if measured else 0
    extras["observer_allreduce_percentile_hist_sum_us"] = round(ar_hist_us, 2)
    extras["observer_allreduce_percentile_hist_sum_bytes"] = ar_bytes[2] if measured else 0
    extras["observer_allreduce_what"] = (
        "RCCL all-reduce over %d rank(s): MAX of the packed [max, -min, nan flags] fp32 buffer for C = 4096 incl. the pack / "
        "unpack kernels; SUM of the fp64 [C, 80] squared-error table; SUM of one int64 [1, 2, 2048] histogram" % world)

    # ---- config 3 across ranks: DeiT-small's percentile calibration with the batches SHARDED over the GPUs ----------
    # every rank holds its own 4 batches of 64 x 197 x 384 (bf16) for each of 12 activation quantizers (one per block);
    # the 12 observers' windowed selections advance in lock step (sparsebit_amd.dist.run_lockstep): sample SUM ->
    # identical windows -> ONE sweep of the rank's batches -> count SUM -> placement.  Timed per model (all 12
    # quantizers), collectives and bytes counted; gate: rank 0 gathers every rank's batches of quantizer 0 and runs
    # the single-process engine on the union.
    if world > 1 and not args.quick or (world > 1 and os.environ.get("SBQ_BENCH_SHARDED_LEG") == "1"):
        from sparsebit_amd import select

        gq = torch.Generator().manual_seed(77 + rank)
        n_q = 12
        acts = []
        for qi in range(n_q):
            bs = []
            for _ in range(4):
                a_ = torch.randn(64, 197, 384, generator=gq) * (1.0 + 0.1 * qi)
                bs.append(a_.bfloat16().to(dev).reshape(-1))
            acts.append(bs)

        def sharded_model():
            gens = [select.windowed_steps(acts[qi], ops.HipWindowBackend(torch.bfloat16), dev, percentile_alpha=1e-3)
                    for qi in range(n_q)]
            return sbq_dist.run_lockstep(gens)

        with sbq_dist.sharded_calibration():
            res = sharded_model()
            sync_all()
            sbq_dist.reset_stats()
            t_a = time.perf_counter()
            reps = 5
            for _ in range(reps):
                res = sharded_model()
            sync_all()
            shard_us = (time.perf_counter() - t_a) * 1e6 / reps
            stats = dict(sbq_dist.stats)
        # gate on quantizer 0: the union of all ranks' batches through the single-process engine
        mine0 = torch.cat(acts[0])
        gathered = [torch.empty_like(mine0) for _ in range(world)]
        dist.all_gather(gathered, mine0)
        ok_sh = None
        if rank == 0:
            mn_u, mx_u = ops.percentile_select([g_.reshape(1, -1) for g_ in gathered], 1e-3, 0, False)
            ok_sh = bool(float(res[0][0]) == float(mn_u) and float(res[0][1]) == float(mx_u))
        t = torch.tensor([shard_us], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        extras["sharded_percentile_calibration"] = {
            "what": "12 per-tensor percentile observers (alpha 1e-3), 4 batches of 64x197x384 bf16 per rank and observer, "
                    "batches sharded over %d ranks, windowed selection in lock step" % world,
            "us_per_model": round(float(t.item()), 1),
            "collectives_per_model": stats["collectives"] // reps,
            "bytes_per_model": stats["bytes"] // reps,
            "host_reads_per_model": stats["host_reads"] // reps,
            "elements_per_rank": n_q * 4 * 64 * 197 * 384,
            "parity": ok_sh,
            "gate": "(min, max) of observer 0 == the single-process engine on the all-gathered union, bit-exact",
        }
        del acts, gathered

    # ---- the rest of the hot path at the headline size (library calls through ops.py; events over a loop) -----
    def timed_op(fn, iters=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(dev)
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / iters

    st4 = torch.empty(4, ROWS, dtype=torch.float32, device=dev)
    st4p = [L.ptr(st4[k]) for k in range(4)]
    wsp, wsn = L.ptr(ws), ws.numel()

    def step_fused(i):
        j = i % NBUF
        lib.sbq_observe_quant_perchannel_forward(xp[j], L.BF16, yp[j], L.BF16, st4p[0], st4p[1], st4p[2], st4p[3],
                                                 ROWS, COLS, QMIN, QMAX, 1, wsp, wsn, st)

    fus_us = timed(step_fused, 100)
    extras["fused_observe_qdq_us"] = round(fus_us, 3)
    # the same call on ONE buffer pair (64 MB: stays in the Infinity Cache), as tools/observe_bench.py times it
    extras["fused_observe_qdq_cache_resident_us"] = round(timed(lambda i: step_fused(0), 100), 3)
    extras["fused_observe_qdq_GBps"] = round(n_elem * BYTES_PER_ELEM / fus_us / 1e3, 1)
    n_half = n_elem // 2 + 1
    extras["mask_threshold_kth_value_us"] = round(timed_op(lambda: ops.kth_value(xs[0], n_half, True)), 2)
    extras["percentile_per_tensor_us"] = round(timed_op(lambda: ops.percentile_select([xs[0]], 1e-3, 0, False)), 2)
    extras["percentile_per_channel_us"] = round(timed_op(lambda: ops.percentile_rows(xs[0], 1e-3)), 2)
    q_mse = build_quantizer(quantizer_config("per-channel-symmetric", 8, observer="MSE"))
    q_mse.set_backend(Backend.VIRTUAL)

    def step_mse():
        q_mse.update_observer(xs[0])
        q_mse.calc_qparams()

    extras["mse_observer_per_channel_us"] = round(timed_op(step_mse, 10), 1)
    # vector-ALU rate of the MSE kernel, from the committed counter pass (tools/rocprof_bench.sh)
    extras["mse_kernel_valu"] = pmc_extra("mse_partial_kernel")  # SQ_INSTS_VALU of the committed counter pass

    # ---- BASELINE configs 1-5: every leg with its own time, algorithmic bytes, roofline fraction and an oracle
    #      gate computed in this run (bench_configs.py).  Rank 0 only: the oracle legs are host work.
    if rank == 0:
        extras["headline_gates"] = gates
    if rank == 0 and not args.quick:
        extras["configs"] = {
            "config1_resnet18_minmax_trt": BC.config1_resnet18_minmax(ctx),
            "config2_mse_per_channel": BC.config2_mse(ctx),
            "config3_percentile": BC.config3_percentile(ctx),
            "config4_gptq_4bit_g128": BC.config4_gptq(ctx),
            "config5_mask_lsq_4bit": BC.config5_mask_lsq(ctx),
        }
        extras["model_wide_calibration"] = BC.model_wide_calibration(ctx)
        if os.environ.get("SBQ_BENCH_SKIP_E2E") == "1":  # (tools/rocprof_bench.sh: ~10^5 torch / MIOpen dispatches nobody profiles)
            e2e = {"parity": True, "skipped": "SBQ_BENCH_SKIP_E2E=1"}
        else:
            try:  # (torch's / MIOpen's kernels run in this leg: whatever they do on a given box must not cost the headline line)
                e2e = BC.e2e_resnet20(ctx)
                extras["e2e_resnet20_b16_forward_eager_us"] = e2e["eager_us"]
                extras["e2e_resnet20_b16_forward_plan_us"] = e2e["plan_us"]
                extras["e2e_resnet20_b16_forward_graph_us"] = e2e["graph_us"]
            except Exception as exc:  # noqa: BLE001
                e2e = {"parity": None, "error": repr(exc)[:400]}
        extras["e2e_resnet20_b16_forward"] = e2e

        def _gates(d):
            for v in d.values():
                if isinstance(v, dict):
                    if "parity" in v and "us" in v:
                        yield v["parity"]
                    yield from _gates(v)  # (a leg may carry a nested leg of its own)

        extras["all_config_gates_pass"] = all(g for g in _gates(extras["configs"]) if g is not None) and all(
            g for g in _gates(extras["model_wide_calibration"]) if g is not None) and e2e["parity"] is not False

    # ---- CPU baseline: the reference's CPU fake-quant ops on this box's host cores -----------
    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and not args.quick:
        from oracle import torch_port

        # the reference would run with torch's default thread count (all cores); on a many-core
        # host that oversubscribes a 67 MB elementwise op, so also try fewer threads and keep
        # the BEST rate: the baseline should be the CPU path at its best on this box
        ncpu = os.cpu_count() or 1
        xcpu = host.float()
        s_cpu = scale.cpu().reshape(-1, 1)
        z_cpu = zp.cpu().reshape(-1, 1)
        # (round 6: the reported rate is the best MEDIAN of 5 over the thread counts -- best-of-20 swung 2.8 x between
        # boxes; the single best run stays beside it.  OMP_PROC_BIND / OMP_PLACES, when the launcher sets them, pin
        # torch's OpenMP threads; they cannot be changed once the runtime is up, so this process only reports them.)
        best, best_threads, reps = float("inf"), ncpu, 0
        best_single = float("inf")
        per_threads = {}
        t_begin = time.perf_counter()
        for threads in sorted({ncpu, min(ncpu, 64), min(ncpu, 32), min(ncpu, 16)}, reverse=True):
            torch.set_num_threads(threads)
            torch_port.ort_fake_quant_cpu(xcpu, s_cpu, z_cpu, QMIN, QMAX)  # warm-up
            dts = []
            for _ in range(5):
                a = time.perf_counter()
                out = torch_port.ort_fake_quant_cpu(xcpu, s_cpu, z_cpu, QMIN, QMAX)
                dts.append(time.perf_counter() - a)
                reps += 1
            med = sorted(dts)[len(dts) // 2]
            per_threads[threads] = round(med * 1e3, 2)
            best_single = min(best_single, min(dts))
            if med < best:
                best, best_threads = med, threads
            if time.perf_counter() - t_begin > 20.0:
                break
        torch.set_num_threads(best_threads)
        step(0)  # (the config legs above reuse the output buffers)
        torch.cuda.synchronize(dev)
        same = bool((out.bfloat16() == ys[0].cpu()).all())
        cpu_baseline = {
            "value": round(n_elem / best, 1),
            "unit": "elements/s",
            "cores": best_threads,
            "host_cores": ncpu,
            "kind": "port",
            "sample": "full 4096x4096 weight (fp32 upcast of the same bf16 data), best MEDIAN-of-5 over thread "
                      "counts {all,64,32,16} (%d runs) of the reference's CPU ops (quant_tensor.py:182-184) in torch, "
                      "%.1f ms" % (reps, best * 1e3),
            "median_ms_per_thread_count": per_threads,
            "value_best_single_run": round(n_elem / best_single, 1),
            "omp_proc_bind": os.environ.get("OMP_PROC_BIND"),
            "matches_gpu_output": same,
        }
        if args.reference and os.path.isdir(os.path.join(args.reference, "sparsebit")):
            # the REAL reference: build_quantizer(cfg) -> update_observer -> calc_qparams -> forward of its own CPU path,
            # GPUs hidden, in a subprocess (tools/reference_cpu_baseline.py); the port above stays beside it
            import subprocess
            import zlib

            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "reference_cpu_baseline.py"), "--reference",
                                    args.reference, "--seed", str(1000 * rank), "--budget-s", "20"], capture_output=True,
                                   text=True, timeout=300)
                ref = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                gpu_crc = zlib.crc32(ys[0].cpu().view(torch.int16).numpy().tobytes()) & 0xFFFFFFFF
                s_crc = zlib.crc32(scale.reshape(-1).float().cpu().numpy().tobytes()) & 0xFFFFFFFF
                port = cpu_baseline
                cpu_baseline = {
                    "value": ref["value"], "unit": "elements/s", "cores": ref["cores"], "host_cores": ref["host_cores"],
                    "kind": "reference",
                    "sample": "full 4096x4096 weight (fp32 upcast of the same bf16 data) through the reference's own "
                              "build_quantizer(cfg) -> update_observer -> calc_qparams -> Quantizer.forward (%s), GPUs hidden, best "
                              "of %d forwards over thread counts {all,64,32,16}, %.1f ms; calibration %.1f ms"
                              % (ref["quantizer"], ref["runs"], ref["forward_ms"], ref["calibration_ms"]),
                    "matches_gpu_output": bool(ref["out_bf16_crc32"] == gpu_crc),
                    "scale_matches_gpu": bool(ref["scale_crc32"] == s_crc),
                    "port_value": port["value"], "port_cores": port["cores"],
                }
            except Exception as e:  # noqa: BLE001
                cpu_baseline["reference_error"] = repr(e)[:300]
        # the other CPU legs of BASELINE.md 3, same host, the thread count that was best for the QDQ, one timed run
        # each after a warm-up on a quarter of the data (bounded: the MSE observer is 80 passes over its input)
        torch.set_num_threads(best_threads)
        legs = {}

        def once(fn, *a):
            t_ = time.perf_counter()
            fn(*a)
            return (time.perf_counter() - t_) * 1e3

        quarter = xcpu[: ROWS // 4]
        part16 = xcpu[: ROWS // 16]
        torch_port.minmax_qparams_cpu(quarter, QMIN, QMAX)
        legs["minmax_per_channel_ms"] = round(once(torch_port.minmax_qparams_cpu, xcpu, QMIN, QMAX), 2)
        torch_port.percentile_minmax_cpu(quarter, 1e-3)
        legs["percentile_per_tensor_ms"] = round(once(torch_port.percentile_minmax_cpu, xcpu, 1e-3), 2)
        torch_port.l1_mask_cpu(quarter, 0.5)
        legs["l1_mask_ms"] = round(once(torch_port.l1_mask_cpu, xcpu, 0.5), 2)
        legs["mse_per_tensor_256_rows_ms"] = round(once(torch_port.mse_qparams_cpu, part16, QMIN, QMAX), 2)
        # config 2 is per channel: the same 80-candidate search with one scale per row (the reference's CPU path
        # mis-broadcasts there; the port follows the CUDA kernel's row indexing), best of 3
        torch_port.mse_qparams_perchannel_cpu(part16[:32], QMIN, QMAX)
        legs["mse_per_channel_256_rows_ms"] = round(min(once(torch_port.mse_qparams_perchannel_cpu, part16, QMIN, QMAX)
                                                         for _ in range(3)), 2)
        legs["threads"] = best_threads
        legs["what"] = ("torch ports (oracle/torch_port.py) of observers/minmax.py:14-25, percentile.py:16-46, "
                        "sparse/sparsers/l1norm.py:18-26 on the full 4096x4096 fp32 weight and mse.py:28-63 (80 candidates), per "
                        "tensor and per channel, on 256 rows of it (1/16: the full tensor is seconds to minutes on the "
                        "host); GPU times of the same steps on the full tensor are in extras / extras.configs")
        cpu_baseline["other_legs"] = legs

    # HBM traffic per launch from the PMC passes (tools/rocprof_bench.sh -> tools/pmc_summary.py
    # writes profiles/pmc_latest.json on the GPU box; the counters need their own profiled
    # runs, so they cannot be collected inside this un-profiled timing run)
    traffic = None
    traffic_source = None
    # which kernel served the timed call: the resident schedule needs a 256-CU part and knob 3 at its default
    # (csrc/sbq_qdq_resident.hip: try_resident); anything else is the pipelined kernel
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    resident = cus * 2 * 16 >= ROWS * COLS // 2048 > cus * 2 * 4 // 2
    n_slabs = ROWS * COLS // 2048
    res_u = 16 if n_slabs > cus * 2 * 8 else (8 if n_slabs > cus * 2 * 4 else 4)
    kernel_name = ("sbq::qdq_resident_kernel<BF16, BF16, 0, %d>" % res_u
                   if resident else "sbq::qdq_pack_kernel<BF16, BF16, ...> (pipelined)")
    pmc_path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    if os.path.exists(pmc_path):
        try:
            with open(pmc_path) as f:
                pmc = json.load(f)
            prof_kernel = str(pmc.get("kernel"))
            if prof_kernel.replace("sbq::", "") == kernel_name.replace("sbq::", ""):
                traffic = pmc.get("qdq_bf16_bf16_traffic_bytes_per_launch")
                traffic_source = ("committed profile profiles/pmc_latest.json (tag %s: two separate rocprofv3 --pmc passes, "
                                  "FETCH_SIZE and WRITE_SIZE, of this same command; kernel %s), not measured in this run"
                                  % (pmc.get("tag"), prof_kernel))
            else:
                traffic_source = ("none: the committed profile describes %s, this run dispatched %s" % (prof_kernel, kernel_name))
        except (OSError, ValueError):
            traffic = None

    # the same fraction from the COMMITTED rocprofv3 --kernel-trace --stats summary (profiles/pmc_latest.json:
    # rocprof_kernel_avg_ns of this kernel on the box that profile was taken on): reproducible from profiles/ alone
    frac_rocprof = rocprof_avg_us = None
    try:
        with open(pmc_path) as f:
            pmc_ = json.load(f)
        if str(pmc_.get("kernel")).replace("sbq::", "") == kernel_name.replace("sbq::", "") and pmc_.get("rocprof_kernel_avg_ns"):
            rocprof_avg_us = float(pmc_["rocprof_kernel_avg_ns"]) / 1e3
            frac_rocprof = round(n_elem * BYTES_PER_ELEM / rocprof_avg_us / 1e3 / HBM_PEAK_GBS, 4)
    except (OSError, ValueError):
        pass

    if rank == 0:
        # what a reader of the DRIVER's record must be able to verify sits in `config` / `roofline` (the driver's parse
        # keeps those; `extras` is dropped and its tail truncated): gates, the N = 1 RCCL floor, the worst leg
        verify = {}
        hg = extras.get("headline_gates") or {}
        if hg:
            verify["headline_gates_all"] = bool(hg.get("all"))
            verify["headline_gate_rows_checked"] = hg.get("rows_checked")
        if "all_config_gates_pass" in extras:
            verify["all_config_gates_pass"] = bool(extras["all_config_gates_pass"])
        ws1_ = extras.get("rccl_world_size_1") or {}
        if ws1_.get("ran"):
            lat_ = ws1_.get("latency", {})
            verify["rccl_n1_allreduce_us"] = {"minmax_MAX_pack_unpack": lat_.get("minmax_pack_allreduce_unpack_us"),
                                              "mse_fp64_SUM": lat_.get("mse_sum_us"),
                                              "percentile_int64_SUM": lat_.get("percentile_hist_sum_us")}
        elif world > 1:
            verify["rccl_allreduce_us"] = {"minmax_MAX_pack_unpack": extras.get("observer_allreduce_us"),
                                           "mse_fp64_SUM": extras.get("observer_allreduce_mse_sum_us"),
                                           "percentile_int64_SUM": extras.get("observer_allreduce_percentile_hist_sum_us")}
        worst = None

        def _legs(d, path):
            for k_, v_ in d.items():
                if isinstance(v_, dict):
                    if "us" in v_ and "frac" in v_ and v_.get("bound", "hbm") == "hbm":
                        yield (path + k_, v_["frac"], v_["us"])
                    yield from _legs(v_, path + k_ + ".")

        for src in ("configs", "model_wide_calibration"):
            for name_, frac_, us_ in _legs(extras.get(src) or {}, src + "."):
                if worst is None or frac_ < worst[1]:
                    worst = (name_, frac_, us_)
        if worst is not None:
            verify["worst_hbm_leg"] = {"name": worst[0], "frac": worst[1], "us": worst[2]}
        line = {
            "metric": "per-channel int8 QDQ throughput, 4096x4096 bf16 weight",
            "value": value,
            "unit": "elements/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": wall * 1e3 / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",  # arithmetic type of the path (bf16 storage in and out)
            "data": "synthetic",
            "config": {
                "workload": "per-channel symmetric int8 QDQ of one 4096x4096 bf16 weight per step (bf16 out), "
                            "minmax-observer scales, %d rotating HBM-resident buffer pairs (%d MB) per GPU"
                            % (NBUF, NBUF * 2 * n_elem * 2 // 2 ** 20),
                "elements_per_step_per_gpu": n_elem,
                "parallelism": "replicated weights, %d rank(s), no data-path collective" % world,
                "verify": verify,
            },
            "roofline": {
                "bound": "hbm",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "frac_of_measured_copy_ceiling": round(achieved / 6290.0, 4),  # MI355X_MICROARCH.md: float4 copy 6.29 TB/s
                "traffic": traffic,
                "traffic_source": traffic_source,
                "kernel": kernel_name,
                "kernel_avg_us": round(kern_us, 3),
                "kernel_avg_us_what": "median of %d windows of 1024 launches each (HIP events on the launch stream) around the "
                                      "timed region: the last 4 of the pre-warm-up and 8 right after it" % len(around),
                "kernel_avg_us_windows_min": round(around[0], 3),
                "kernel_avg_us_windows_max": round(around[-1], 3),
                "frac_1024_window_median": round(achieved / HBM_PEAK_GBS, 4),
                "frac_rocprof": frac_rocprof,
                "rocprof_kernel_avg_us": None if rocprof_avg_us is None else round(rocprof_avg_us, 3),
                "frac_rocprof_what": "algorithmic bytes / the committed rocprofv3 --kernel-trace --stats average of this kernel "
                                     "(profiles/pmc_latest.json, taken on the builder's box) / 8 TB/s; `frac` is the same bytes "
                                     "over this run's own HIP-event windows",
                "frac_windows_min": round(n_elem * BYTES_PER_ELEM / around[-1] / 1e3 / HBM_PEAK_GBS, 4),
                "frac_windows_max": round(n_elem * BYTES_PER_ELEM / around[0] / 1e3 / HBM_PEAK_GBS, 4),
                # the wall clock of the timed region per step (launch / synchronisation latency shared by the K steps
                # included): what `value` is computed from
                "us_per_step_wall": round(kern_us_timed, 3),
                "frac_wall": round(n_elem * BYTES_PER_ELEM / (wall * 1e6 / args.steps) / 1e3 / HBM_PEAK_GBS, 4),
                "windows_measured": len(windows) + len(post),
                "prewarm_s": round(prewarm_s, 3),
                "clocks_during_windows": clocks or None,
                "algorithmic_bytes_per_launch": n_elem * BYTES_PER_ELEM,
            },
            "cpu_baseline": cpu_baseline,
            "parity_checked": parity,
            "extras": extras,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
