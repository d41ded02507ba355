#!/usr/bin/env python3
"""bench.py -- rays/s of the fused render hot path at BASELINE.json's configuration.

    python bench.py --gpus N --steps K --warmup W                 (driver contract; --precision fp32 | bf16x3, --workload c2 | c3,
                                                                   --dump-outputs DIR: the timed path's last outputs as .npy files)
    (N > 1: one rank per GPU, either launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` or --
     when WORLD_SIZE is not set -- by bench.py itself, which starts exactly that command as a child and relays rank 0's line)

Default workload (BASELINE configs[1], "c2"): one *step* = one fused forward pass (sample -> frame transform -> positional encoding ->
decoder -> composite) over one object's ray batch, 4096 rays x 64 samples (supnerf.nusc.vehicle.car.json hyper-parameters, im_sz 64,
synthetic nuScenes-like car, random-init decoder with the sigma bias of SURVEY 8d), inputs resident in HBM.  Every rank renders its own
object (objects are independent: weak scaling, no data-path collective); the only collective is the max-reduce of the elapsed time.
Rank 0 prints ONE JSON line.

`value` is measured in the REFERENCE's arithmetic: exact fp32 (v_mfma_f32_32x32x2_f32, bit for bit an fp32 fma chain), `--precision fp32`.
The library's default arithmetic, split-bf16 ("bf16x3": operands carried as bf16 hi + lo, three bf16 MFMAs per product, fp32 accumulate)
is wall-clocked by the SAME loop and reported beside it under `bf16x3` with its own parity numbers and roofline -- it is narrower
arithmetic than the reference's and therefore not the headline.

Reported beside `value` (never part of it):
  * `roofline` (forward kernel of the headline precision) and `roofline_bwd` (its backward kernel): algorithmic FLOPs (57.56 MFLOP/ray
    forward; the same again for the optimise-mode backward, dX only -- BASELINE.md section 4) / kernel time from device events on the
    launch stream, against the matching MFMA peak of MI355X_MICROARCH.md; `traffic` = HBM bytes per launch from the committed counter
    profile of the same kernel (profiles/, read at run time; null when no profile of this round exists);
  * `api`: the public functions end to end (`utils.render_rays_v2`: ray generation, target resize, depths, per-object layers, render),
    forward and forward + backward to codes and pose;
  * `optimise_loop`: one object through the fused loop / the API-structured loop; `c3_sharded`: BASELINE
    config 3, 64 objects sharded over the ranks through driver.optimize_objects_batched + the metric all_gather;
  * `training_step`: BASELINE config 5's per-GPU step (8 objects x 1024 rays x 64 samples, decoder + codes trained);
  * `cpu_baseline`: the CPU oracle (oracle/, a PyTorch restatement of the reference pinned by the reference's own outputs) on this host's
    cores over the whole 4096-ray workload, with the parity of both GPU precisions against it.

`--workload c3` makes BASELINE config 3 the timed thing: one step = one optimise iteration (forward + backward + depth render + AdamW)
over the rank's shard of 64 objects x 4096 rays x 64 samples; value = rays of the training forward per second over all ranks (strong
scaling: the 64 objects are fixed), the per-object metric rows are all-gathered at the end.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_RAY = 57.56e6          # forward, S = 64; optimise-mode backward (dX only): the same again
PEAK_TFLOPS = {"fp32": 157.3,    # MI355X_MICROARCH.md "Peak FP32 (matrix)": v_mfma_f32_32x32x2_f32
               "bf16x3": 2500.0}  # dense BF16 MFMA peak; the split-bf16 path issues 3 MFMAs per algorithmic product
ISSUE_FACTOR = {"fp32": 1.0, "bf16x3": 3.0}
DTYPE = {"fp32": "f32", "bf16x3": "bf16x3 = split 16-bit pieces (fp32 operands as hi + lo: fp16 pieces in the forward chain, bf16 pieces in the backward chain and the weight-gradient products; 3 MFMAs per product, fp32 accumulate)"}
FWD_KERNEL = {"fp32": "decoder_fwd16_kernel<1,4,true,false,false>", "bf16x3": "bf16_fwd_kernel<1,false,true>"}
BWD_KERNEL = {"fp32": "decoder_bwd16_kernel<1>", "bf16x3": "bf16_bwd16_kernel<1>"}
N_RAYS, N_SAMPLES, IM_SZ = 4096, 64, 64
C3_OBJECTS = 64


def log(msg):
    """progress on stderr (stdout carries the one JSON line)"""
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


_JSON_OUT = None


def claim_stdout():
    """stdout must carry exactly ONE line, the JSON; RCCL prints a version banner on fd 1 when the first communicator is made, and other
    libraries may chat there too.  So fd 1 is pointed at stderr for the whole run and the JSON line goes to a saved copy of the real stdout."""
    global _JSON_OUT
    if _JSON_OUT is None:
        sys.stdout.flush()
        _JSON_OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit(obj):
    out = _JSON_OUT if _JSON_OUT is not None else sys.stdout
    out.write(json.dumps(obj) + "\n")
    out.flush()


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: the arrays the timed path handed its caller in the last timed step, one DIR/<name>.npy each, float32 (whole
    arrays: the workloads' outputs are far below DUMP_MAX_BYTES).  The inputs are seeded, so two builds run with the same arguments can be
    compared array for array."""
    host = {k: v.detach().to(torch.float32).cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes of outputs exceed the {DUMP_MAX_BYTES}-byte limit")
    os.makedirs(dirname, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(dirname, k + ".npy"), a)
    log(f"outputs of the last timed step -> {dirname}: " + ", ".join(f"{k} {tuple(a.shape)}" for k, a in host.items()))


def self_launch(n_gpus):
    """`python bench.py --gpus N` without a launcher: start the N ranks the way the driver's multi-GPU command does
    (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...) as CHILD
    processes and relay rank 0's JSON line.  This process never initialises the GPU (no torch.cuda call has happened yet) and never
    execs: the children are fresh interpreters."""
    import socket
    import subprocess
    with socket.socket() as sk:                     # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] --gpus {n_gpus} without WORLD_SIZE: launching {' '.join(cmd)}", file=sys.stderr, flush=True)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, text=True)
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    if proc.returncode == 0 and not lines:
        print("[bench] the ranks exited cleanly but printed no JSON line", file=sys.stderr)
        return 1
    if lines:
        sys.stdout.write(lines[-1] + "\n")
        sys.stdout.flush()
    return proc.returncode


def profile_traffic(precision, which="fwd"):
    """HBM bytes per launch of the dominant kernel from the newest committed counter profile of this kernel (rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE in separate passes; FETCH_SIZE doubled, the gfx950 correction of MI355X_MICROARCH.md).  The counters cannot be collected from
    inside this process; the file is read at run time so the figure follows the profile, and its name is reported with it."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_{which}_pmc_{precision}.json")))
    if not files:
        return None, None
    try:
        c = json.load(open(files[-1]))["counters"]
        return c["FETCH_SIZE"]["per_dispatch_mean"] * 1024.0 * 2 + c["WRITE_SIZE"]["per_dispatch_mean"] * 1024.0, os.path.relpath(files[-1], ROOT)
    except (KeyError, ValueError, OSError):
        return None, None


def make_workload(dev, seed):
    """One synthetic object: rays of a 64x64 grid over its roi, shared stratified depths, codes, decoder weights."""
    import supnerf_amd as A
    from supnerf_amd import synthetic as O
    params = O.init_decoder_params(seed=0)
    model = A.CodeNeRF(shape_blocks=3, texture_blocks=1)
    model.load_state_dict(params)
    model = model.to(dev)
    ob = O.synthetic_object(seed)
    img, mask = O.synthetic_targets(seed, IM_SZ)
    gen = torch.Generator().manual_seed(seed)
    sc = (torch.randn(1, 256, generator=gen) * 0.3).to(dev)
    tc = (torch.randn(1, 256, generator=gen) * 0.3).to(dev)
    jit = torch.rand(N_SAMPLES, generator=gen)
    return dict(model=model, params=params, ob=ob, img=img, mask=mask, sc=sc, tc=tc, jit=jit)


class Clock:
    """The contract's timing: barrier + synchronize on both sides, MAX over ranks."""

    def __init__(self, dist, dev):
        self.dist, self.dev = dist, dev

    def barrier(self):
        torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
            torch.cuda.synchronize()

    def wall(self, fn, steps, warmup):
        for _ in range(warmup):
            fn()
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        self.last_local = time.perf_counter() - t0          # this rank's own time for its own launches (the per-rank record)
        self.barrier()
        dt = time.perf_counter() - t0
        if self.dist is not None:
            t = torch.tensor([dt], device=self.dev, dtype=torch.float64)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    def rank_records(self, rank, rays_per_s):
        """One record per rank, all-gathered over the communicator: evidence that N DISTINCT devices joined it (device index, PCI
        bus id, uuid) and what each of them rendered on its own clock."""
        idx = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        pr = torch.cuda.get_device_properties(idx)
        bus = "%04x:%02x:%02x" % tuple(int(getattr(pr, k, -1)) & 0xFFFF for k in ("pci_domain_id", "pci_bus_id", "pci_device_id"))
        rec = {"rank": rank, "device_index": idx, "pci_bus_id": bus, "uuid": str(getattr(pr, "uuid", "")), "name": pr.name,
               "rays_per_s": rays_per_s}
        if self.dist is None:
            return [rec]
        out = [None] * self.dist.get_world_size()
        self.dist.all_gather_object(out, rec)
        return sorted(out, key=lambda r: r["rank"])

    @staticmethod
    def events(fn, steps):
        """Average duration from device events on the launch stream (torch's current stream IS the stream the C ABI launches on)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps


def roofline(precision, kern_ms, which):
    achieved = N_RAYS * FLOP_PER_RAY / (kern_ms * 1e-3) / 1e12
    traffic, src = profile_traffic(precision, which)
    return {"bound": "mfma", "achieved": achieved, "peak": PEAK_TFLOPS[precision], "unit": "TFLOP/s", "frac": achieved / PEAK_TFLOPS[precision],
            "traffic": traffic, "traffic_unit": "bytes per launch", "traffic_source": src,
            "traffic_measured_in_run": False,      # (the counters come from the committed rocprofv3 --pmc profile named above, not from this run)
            "kernel": (FWD_KERNEL if which == "fwd" else BWD_KERNEL)[precision], "kernel_ms": kern_ms, "flop_per_launch": N_RAYS * FLOP_PER_RAY,
            "mfma_pipe_frac": ISSUE_FACTOR[precision] * achieved / PEAK_TFLOPS[precision],
            "note": "achieved = ALGORITHMIC flops (57.56 MFLOP/ray" + (", optimise-mode backward = dX only: the same count" if which == "bwd" else "")
                    + ") / kernel time from device events; bf16x3 issues 3x that on the bf16 MFMA pipe (mfma_pipe_frac)"}


def c3_leg(model, dev, rank, world, dist, clock, n_it, warm=True, warm_iters=2, outputs=None):
    """BASELINE config 3: 64 objects x 4096 x 64, object-sharded (driver.shard_slice), every rank optimises its slice in one launch per
    iteration, then ONE all_gather of the metric rows (the only collective).  Returns (seconds for n_it iterations [max over ranks], rows).
    ``outputs`` (optional dict) receives this rank's shape codes, texture codes and poses as optimize_objects_batched returned them."""
    from supnerf_amd import driver as D
    hp = D.load_hpams()
    hp["render_im_sz"] = IM_SZ
    mine = list(D.shard_slice(C3_OBJECTS, world, rank))
    objs = D.make_objects([200 + i for i in mine], IM_SZ)
    gl = torch.Generator().manual_seed(3)
    sc_all, tc_all = torch.randn(C3_OBJECTS, 256, generator=gl) * 0.3, torch.randn(C3_OBJECTS, 256, generator=gl) * 0.3
    sc_l, tc_l = sc_all[mine], tc_all[mine]
    if warm and warm_iters > 0 and objs:
        hp["optimize"]["num_opts"] = warm_iters
        D.optimize_objects_batched(model, dev, objs[:2], hp, sc_l[:2], tc_l[:2], mine[:2], reg_iters=-1)
    hp["optimize"]["num_opts"] = n_it
    clock.barrier()
    t0 = time.perf_counter()
    if objs:
        # reg_iters = -1: EVERY timed iteration is a full optimisation iteration (forward + backward + depth render + AdamW).  The loop's
        # first reg_iters + 1 iterations are render-only in the reference (src/optimizer_nuscenes.py:684-689,768-769) and since round 4 skip
        # the backward whose gradients the reference clears unread -- with the default reg_iters = 3 half of an 8-iteration leg would be cheap
        m, sc_o, tc_o, pose_o = D.optimize_objects_batched(model, dev, objs, hp, sc_l, tc_l, mine, reg_iters=-1)
        local = m.reshape(len(objs), -1)
        if outputs is not None:
            outputs.update(shape_codes=sc_o, texture_codes=tc_o, poses=pose_o)
    else:
        local = torch.zeros(0, n_it * 4, device=dev)
    rows = D.gather_metric_rows(local.to(dev), torch.tensor(mine, device=dev, dtype=torch.float32), C3_OBJECTS)
    clock.barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, rows, len(mine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--headline-only", action="store_true",
                    help="only the headline launches (no other legs): the form profiled for profiles/*_bench_kernel_stats.csv, so the "
                         "per-kernel average there is the headline kernel alone")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3"],
                    help="decoder GEMM arithmetic of the headline `value` (default: the reference's fp32; the other mode is wall-clocked by the "
                         "same loop and reported beside it)")
    ap.add_argument("--workload", default="c2", choices=["c2", "c3"],
                    help="c2: fused forward of one object per GPU (BASELINE configs[1], weak scaling); c3: the optimise iteration over 64 objects "
                         "sharded across the GPUs (BASELINE configs[2], strong scaling)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32; rank 0): "
                         "c2 -> rgb, depth, acc of the fused forward; c3 -> the all-gathered metric rows and rank 0's shape codes, texture "
                         "codes and poses")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))            # (before anything touches the GPU: the ranks are fresh child processes)
    claim_stdout()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         "(python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)")
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    # SNR_BENCH_BACKEND=gloo: rehearsal of the N > 1 branch on a box with fewer GPUs than ranks (ranks share the cards; the numbers mean nothing)
    backend = os.environ.get("SNR_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or os.environ.get("SNR_BENCH_FORCE_DIST"):      # (FORCE_DIST: exercise the RCCL set-up with a single rank)
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)     # RCCL over xGMI
        else:
            dist.init_process_group(backend)
    clock = Clock(dist, dev)

    import supnerf_amd as A
    from supnerf_amd import ops, utils as U
    w = make_workload(dev, seed=100 + rank)
    model, ob = w["model"], w["ob"]
    prec, other = args.precision, ("bf16x3" if args.precision == "fp32" else "fp32")

    if args.workload == "c3":
        model.precision = prec
        n_it = args.steps
        c3_out = {}
        dt, rows, n_mine = c3_leg(model, dev, rank, world, dist, clock, n_it, warm_iters=args.warmup, outputs=c3_out)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, dict(metric_rows=rows, **c3_out))
        res = {"metric": "rays/sec, optimise iteration (fwd + bwd + depth render + AdamW) over 64 objects x 4096 rays x 64 samples, object-sharded",
               "value": C3_OBJECTS * N_RAYS * n_it / dt, "unit": "rays/s", "n_gpus": world, "steps": n_it, "warmup": args.warmup, "ms_per_step": dt / n_it * 1e3,
               "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": DTYPE[prec], "data": "synthetic",
               "config": {"workload": "BASELINE configs[2]: 64 synthetic nuScenes-like cars, 4096 rays x 64 samples each, contiguous object shards "
                                      "(driver.shard_slice), one launch per iteration and rank, one all_gather of the metric rows at the end",
                          "objects": C3_OBJECTS, "objects_this_rank": n_mine, "precision": prec},
               "object_iterations_per_s": C3_OBJECTS * n_it / dt, "metric_rows_finite": bool(torch.isfinite(rows).all())}
        if rank == 0:
            emit(res)
        if dist is not None:
            dist.barrier(); dist.destroy_process_group()
        return

    # ---- device-resident inputs of the hot path (ray generation is outside the path's timed region: it is part of the
    # caller-side glue and costs microseconds; the `api` leg times it)
    with torch.no_grad():
        rays_o, viewdir = U.get_rays(ob["K"], ob["cam_pose"].to(dev), ob["roi"], uv_steps=[IM_SZ, IM_SZ])
        near, far = U._sphere_bounds(ob["cam_pose"], ob["obj_diag"])
        z = U._shared_depths(near, far, N_SAMPLES, dev, jitter=w["jit"])
        lat = model.latent_terms(w["sc"], w["tc"])
    packed = model.packed_weights()
    div = torch.full((1,), float(ob["obj_diag"]), device=dev)
    frame = U._frame(False, False, True)
    cfgs = {p: ops.RenderCfg(N_SAMPLES, ops.Z_SHARED, N_RAYS, 3, 1, frame=frame, precision=p) for p in ("fp32", "bf16x3")}
    for c in cfgs.values():      # like model.fused_render: the latent terms also folded into the next layers' biases (bf16x3 uses them)
        c.latent_bias = model.latent_biases(lat)
    assert rays_o.shape[0] == N_RAYS
    outs = {}

    def step(p):
        outs[p] = ops.render_fwd(rays_o, viewdir, z, div, None, lat, packed, cfgs[p])

    log(f"headline: {args.steps} fused forwards, {prec}")
    # ---- headline: the contract's wall clock around EXACTLY --steps launches, in the reference's arithmetic unless asked otherwise
    elapsed = clock.wall(lambda: step(prec), args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        rgb, depth, acc = outs[prec][:3]
        dump_outputs(args.dump_outputs, dict(rgb=rgb, depth=depth, acc=acc))
    value = world * N_RAYS * args.steps / elapsed
    ranks = clock.rank_records(rank, N_RAYS * args.steps / clock.last_local)
    kern_ms = clock.events(lambda: step(prec), args.steps)
    result = {
        "metric": "rays/sec at 4096 rays x 64 samples (fused render forward)",
        "value": value, "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE[prec], "data": "synthetic",
        "config": {"workload": "supnerf.nusc.vehicle.car.json decoder (shape_blocks 3, texture_blocks 1, W 256), 1 object per GPU, "
                               "4096 rays x 64 samples, family-A render (render_rays_v2 tail)", "precision": prec,
                   "rays": N_RAYS, "samples": N_SAMPLES, "objects_per_gpu": 1, "sharding": "objects across ranks, no data-path collective"},
        "roofline": roofline(prec, kern_ms, "fwd"),
        "ranks": ranks, "distinct_devices": len({(r["pci_bus_id"], r["uuid"]) for r in ranks}),
    }
    if args.headline_only:
        if rank == 0:
            emit(result)
        if dist is not None:
            dist.barrier(); dist.destroy_process_group()
        return

    log(f"same loop, {other}")
    # ---- the other arithmetic, wall-clocked by the same loop
    o_elapsed = clock.wall(lambda: step(other), args.steps, args.warmup)
    o_kern_ms = clock.events(lambda: step(other), args.steps)
    result[other] = {"value": world * N_RAYS * args.steps / o_elapsed, "unit": "rays/s", "ms_per_step": o_elapsed / args.steps * 1e3,
                     "steps": args.steps, "dtype": DTYPE[other], "roofline": roofline(other, o_kern_ms, "fwd"),
                     "note": "same launches, same loop and clock as `value`; " + ("the library's default arithmetic (model.precision = 'auto')"
                                                                                 if other == "bf16x3" else "the reference's arithmetic")}

    log("backward kernels")
    # ---- backward kernels alone (optimise mode: gradients wrt latent terms, ray origins and directions), device events
    def bwd_ms(p):
        fw = ops.render_fwd(rays_o, viewdir, z, div, None, lat, packed, cfgs[p], save_for_bwd=True)
        d_rgb, d_depth, d_acc = torch.rand_like(fw[0]), torch.zeros_like(fw[1]), torch.rand_like(fw[2])
        fn = lambda: ops.render_bwd(rays_o, viewdir, z, div, None, lat, packed, cfgs[p], fw[3], fw[4], fw[5], d_rgb, d_depth, d_acc)
        for _ in range(5):
            fn()
        n = max(20, args.steps // 4)
        # the launch is followed by the 2-step reduction of the latent partials; the kernel dominates (>97 %)
        return clock.events(fn, n)
    result["roofline_bwd"] = roofline(prec, bwd_ms(prec), "bwd")
    result[other]["roofline_bwd"] = roofline(other, bwd_ms(other), "bwd")
    for r in (result["roofline_bwd"], result[other]["roofline_bwd"]):
        r["kernel_ms_includes"] = "backward kernel + the reduction of the per-tile latent-gradient partials (one timed call of ops.render_bwd)"

    extra = {}
    log("public API legs")
    # ---- the public API end to end: what a caller of the reference's render_rays_v2 pays per call
    def api_leg(p):
        model.precision = p
        sc_g, tc_g = w["sc"].clone().requires_grad_(), w["tc"].clone().requires_grad_()
        pose_g = ob["cam_pose"].to(dev).requires_grad_()

        def fwd():
            with torch.no_grad():
                return U.render_rays_v2(model, dev, w["img"], w["mask"], pose_g, ob["obj_diag"], ob["K"], ob["roi"], N_SAMPLES, sc_g, tc_g, 1, 0, im_sz=IM_SZ)

        def fwd_bwd():
            out = U.render_rays_v2(model, dev, w["img"], w["mask"], pose_g, ob["obj_diag"], ob["K"], ob["roi"], N_SAMPLES, sc_g, tc_g, 1, 0, im_sz=IM_SZ)
            loss, _ = ops.LossTail.apply(out[0], out[2], out[3], out[4], 0.1, N_RAYS)
            sc_g.grad = tc_g.grad = pose_g.grad = None
            loss.sum().backward()
        # family B: NeRFRenderer.render_rays (src/renderer.py:117-166; its defaults ARE 4096 rays x 64 samples) -- box bounds, per-ray
        # depths and the in-kernel jitter in the fused launch's prologue
        rend = A.NeRFRenderer(n_samples=N_SAMPLES, white_bkgd=True)

        def b_fwd():
            with torch.no_grad():
                return rend.render_rays(model, dev, w["img"], w["mask"], pose_g, ob["wlh"], ob["K"], ob["roi"], sc_g, tc_g, im_sz=IM_SZ)

        def b_fwd_bwd():
            out = rend.render_rays(model, dev, w["img"], w["mask"], pose_g, ob["wlh"], ob["K"], ob["roi"], sc_g, tc_g, im_sz=IM_SZ)
            loss, _ = ops.LossTail.apply(out[0], out[2], out[3], out[4], 0.1, N_RAYS)
            sc_g.grad = tc_g.grad = pose_g.grad = None
            loss.sum().backward()
        n = max(20, args.steps // 4)
        # (30 untimed calls first: a process's first few dozen launches of a new kind run with cold code objects, BLAS heuristics and clocks --
        # tools/_diag/api_warm.py: the first batch of 20 calls costs 4 ms per call, every later one 0.57)
        t_f = clock.wall(fwd, n, 30)
        t_fb = clock.wall(fwd_bwd, n, 30)
        t_bf = clock.wall(b_fwd, n, 30)
        t_bfb = clock.wall(b_fwd_bwd, n, 30)
        return {"render_rays_v2_fwd_rays_per_s": world * N_RAYS * n / t_f, "render_rays_v2_fwd_ms": t_f / n * 1e3,
                "render_rays_v2_fwd_bwd_rays_per_s": world * N_RAYS * n / t_fb, "render_rays_v2_fwd_bwd_ms": t_fb / n * 1e3,
                "nerf_renderer_render_rays_fwd_rays_per_s": world * N_RAYS * n / t_bf, "nerf_renderer_render_rays_fwd_ms": t_bf / n * 1e3,
                "nerf_renderer_render_rays_fwd_bwd_rays_per_s": world * N_RAYS * n / t_bfb, "nerf_renderer_render_rays_fwd_bwd_ms": t_bfb / n * 1e3,
                "calls": n}
    extra["api"] = {p: api_leg(p) for p in (prec, other)}
    extra["api"]["note"] = ("utils.render_rays_v2 / NeRFRenderer.render_rays with the reference's signatures, every call: ray generation from the pose, "
                            "(cached) target resize, depths (family A: one shared vector; family B: box bounds + per-ray stratified depths + jitter inside "
                            "the fused launch), per-object latent layers, fused render; fwd_bwd adds the loss tail and the backward to both codes and the "
                            "camera pose (family B: also through the box bounds)")

    log("family B fused kernels (box bounds in the prologue)")
    # ---- family B at the kernel level: the same launches as the headline with SNR_Z_BOX sampling (slab test, per-ray depths, Philox
    # jitter, metric z, white background), device events; roofline like the headline's (same FLOPs per ray)
    def box_leg(p):
        from supnerf_amd import renderer as R
        _, half, zs = R._box_constants(ob["wlh"], 1, dev)
        cfg_b = ops.RenderCfg(N_SAMPLES, ops.Z_BOX, N_RAYS, 3, 1, frame=U._frame(False, False, False), white_bkgd=True, metric_z=True,
                              precision=p, box_half=half)
        cfg_b.latent_bias = cfgs[p].latent_bias
        ro_raw = rays_o.contiguous()
        f = lambda: ops.render_fwd(ro_raw, viewdir, None, None, zs, lat, packed, cfg_b)
        for _ in range(5):
            f()
        n = max(20, args.steps // 4)
        ms_f = clock.events(f, n)
        fw = ops.render_fwd(ro_raw, viewdir, None, None, zs, lat, packed, cfg_b, save_for_bwd=True)
        d_rgb, d_depth, d_acc = torch.rand_like(fw[0]), torch.rand_like(fw[1]), torch.rand_like(fw[2])
        b = lambda: ops.render_bwd(ro_raw, viewdir, None, None, zs, lat, packed, cfg_b, fw[3], fw[4], fw[5], d_rgb, d_depth, d_acc)
        for _ in range(5):
            b()
        ms_b = clock.events(b, n)
        hit_frac = float((fw[2] < 0.999).float().mean())
        return {"fwd_kernel_ms": ms_f, "fwd_rays_per_s": N_RAYS / (ms_f * 1e-3), "fwd_frac_of_peak": N_RAYS * FLOP_PER_RAY / (ms_f * 1e-3) / 1e12 / PEAK_TFLOPS[p],
                "bwd_kernel_ms": ms_b, "bwd_frac_of_peak": N_RAYS * FLOP_PER_RAY / (ms_b * 1e-3) / 1e12 / PEAK_TFLOPS[p],
                "rays_with_opacity": hit_frac}
    extra["family_b_fused"] = {p: box_leg(p) for p in (prec, other)}
    extra["family_b_fused"]["note"] = ("ops.render_fwd / render_bwd with z_mode SNR_Z_BOX at 4096 x 64: the slab test, hit / miss bounds, per-ray stratified depths, "
                                       "in-kernel Philox jitter (torch.rand_like's stream) and metric depth run in the prologue of the same kernels as the headline; "
                                       "the backward also returns the gradient through the box bounds")
    model.precision = "auto"

    log("one-object optimise loops")
    # ---- the optimise loop (f1): one object
    from supnerf_amd import driver as D
    loop = {}
    if rank == 0 and world == 1:      # (single-GPU runs only: at N > 1 the c3 leg below is the loop measurement)
        hp = D.load_hpams()
        hp["render_im_sz"] = IM_SZ
        objs = D.make_objects([200], IM_SZ)
        gl = torch.Generator().manual_seed(3)
        sc_l, tc_l = torch.randn(1, 256, generator=gl) * 0.3, torch.randn(1, 256, generator=gl) * 0.3
        n_it1 = 50                                   # the reference runs 100 iterations per object: amortise the set-up alike
        hp["optimize"]["num_opts"] = n_it1

        def timed(fn):
            fn(); torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            return time.perf_counter() - t0
        for p, name in (("fp32", "fp32"), (("fp32", "bf16x3"), "fp32_forward_bf16x3_backward"), ("auto", "auto")):
            model.precision = p
            t_f = timed(lambda: D.optimize_object(model, dev, objs[0], hp, sc_l, tc_l, seed=0, reg_iters=-1))
            loop[f"fused_eager_{name}"] = {"ms_per_iteration": t_f / n_it1 * 1e3, "object_iterations_per_s": n_it1 / t_f}
        t_a = timed(lambda: D.optimize_object_api(model, dev, objs[0], hp, sc_l, tc_l, seed=0, reg_iters=-1))
        loop.update({"api_structured_auto": {"ms_per_iteration": t_a / n_it1 * 1e3, "object_iterations_per_s": n_it1 / t_a},
                     "iterations": n_it1, "rays_per_object": N_RAYS,
                     "note": "iteration = forward + backward (codes, pose) + 64-pixel depth render + metric row + AdamW at 4096 x 64 (reg_iters = -1: no render-only iterations in the timed loop); fused_eager = driver.optimize_object "
                             "(~20 launches per iteration, no graph; fp32_forward_bf16x3_backward: precision = ('fp32', 'bf16x3'), the reference's forward values bit for bit with the gradient on the split-bf16 kernel); api_structured = the same loop on the public functions, call for call like the reference; "
                             "set-up included everywhere"})
    extra["optimise_loop"] = loop

    log("config 3: 64 objects sharded")
    # ---- BASELINE config 3 through the driver: 64 objects sharded over the ranks, one all_gather at the end; the library's default
    # arithmetic, then the reference's
    n_it3 = 8
    for p3, key in (("auto", "c3_sharded"), ("fp32", "c3_sharded_fp32"), (("fp32", "bf16x3"), "c3_sharded_fp32_forward_bf16x3_backward")):
        model.precision = p3
        dt3, rows3, n_mine = c3_leg(model, dev, rank, world, dist, clock, n_it3 if p3 == "auto" else 4)
        it3 = n_it3 if p3 == "auto" else 4
        extra[key] = {"objects": C3_OBJECTS, "objects_this_rank": n_mine, "iterations": it3, "seconds": dt3,
                      "ms_per_iteration": dt3 / it3 * 1e3, "object_iterations_per_s": C3_OBJECTS * it3 / dt3,
                      "rays_per_s_fwd_bwd_plus_depth_render": C3_OBJECTS * it3 * N_RAYS / dt3,
                      "precision": "auto (bf16x3)" if p3 == "auto" else ("fp32" if p3 == "fp32" else "fp32 forward (the reference's values) + bf16x3 backward"), "metric_rows_finite": bool(torch.isfinite(rows3).all()),
                      "note": "strong scaling of BASELINE configs[2]: the 64 objects are fixed, each rank optimises its contiguous slice in one launch per "
                              "iteration; includes the per-object host set-up and the final all_gather of the metric rows (RCCL)"}
    model.precision = "auto"

    log("training step")
    # ---- BASELINE config 5's per-GPU step: decoder + codes trained (weak scaling across ranks; the gradient bucket is all-reduced), in the
    # reference's arithmetic (exact fp32 chains and weight-gradient products) and in split-bf16
    from supnerf_amd import trainer as T
    Bt, nt = 8, 1024
    gt = torch.Generator().manual_seed(rank)
    batch = dict(code_idx=torch.arange(Bt), xyz=torch.rand(Bt, nt, N_SAMPLES, 3, generator=gt) - 0.5,
                 viewdir=torch.nn.functional.normalize(torch.randn(Bt, nt, 1, 3, generator=gt), dim=-1).repeat(1, 1, N_SAMPLES, 1),
                 z_vals=torch.sort(torch.rand(Bt, N_SAMPLES, generator=gt) * 4 + 9, dim=-1)[0], rgb_tgt=torch.rand(Bt, nt, 3, generator=gt),
                 occ_pixels=(torch.randint(0, 3, (Bt, nt, 1), generator=gt) - 1).float())
    batch = {k: v.to(dev) for k, v in batch.items()}
    hp_t = dict(lr_schedule=[dict(lr=1e-4, interval=40000), dict(lr=1e-4, interval=40000)])
    extra["training_step"] = {}
    DTYPE_T = dict(DTYPE, auto=DTYPE["bf16x3"] + " -- what 'auto' trains in", fp32_fwd="f32 forward chain (exact) + split backward chain and weight-gradient products")
    for p_t in ("auto", "fp32", "fp32_fwd"):
        m_t = A.CodeNeRF(3, 1); m_t.load_state_dict(w["params"]); m_t = m_t.to(dev); m_t.train_decoder_weights = True
        m_t.precision = ("fp32", "bf16x3", "bf16x3") if p_t == "fp32_fwd" else p_t
        codes = T.CodeTables(64, 256, seed=1).to(dev)
        bucket = T.GradBucket(list(m_t.parameters()) + list(codes.parameters()), row_sparse=list(codes.parameters()))
        opt_t = T.make_optimizer(m_t, codes, hp_t)
        n_t = 10
        t_t = clock.wall(lambda: T.train_step(m_t, codes, opt_t, bucket, batch, 0.1), n_t, 3)
        extra["training_step"][p_t] = {"ms_per_step": t_t / n_t * 1e3, "rays_per_s": world * Bt * nt * n_t / t_t, "objects_per_gpu": Bt, "rays_per_object": nt,
                                       "samples": N_SAMPLES, "steps": n_t, "dtype": DTYPE_T[p_t], "model_precision": m_t.precision}
        del m_t, codes, bucket, opt_t
    extra["training_step"]["note"] = ("trainer.train_step: forward + backward incl. every decoder weight gradient + one all-reduce of the flat gradient bucket + AdamW (one launch); "
                                      "`auto` = the library default in training mode = the split kernels throughout (fp16 pieces in the forward chain: a 60-step run ends where the "
                                      "reference's own fp32 arithmetic ends -- the forward chain's arithmetic decides that, and two fp16 pieces carry 22 bits); `fp32` = exact fp32 throughout, the "
                                      "reference's arithmetic product for product; `fp32_fwd` = the exact-fp32 forward chain with the split backward chain and products "
                                      "(tests/test_driver_gpu.py::test_training_outcome_fp32_and_bf16x3_track_the_oracle has the evidence)")
    del batch

    log("HBM-bound kernels")
    # ---- the HBM-bound stand-alone kernels (encode with PE output, composite, scene composite): achieved GB/s
    hbm = {}
    if rank == 0 and world == 1:
        Bh = 64
        ro_h, vd_h = rays_o.repeat(Bh, 1), viewdir.repeat(Bh, 1)
        z_h = z[None].repeat(Bh, 1).contiguous()
        div_h = div.repeat(Bh)
        cfg_h = ops.RenderCfg(N_SAMPLES, ops.Z_PER_OBJECT, N_RAYS, 3, 1, frame=frame)
        P_h = Bh * N_RAYS * N_SAMPLES

        def timed_ev(fn, n=10):
            for _ in range(2):
                fn()
            return clock.events(fn, n) * 1e-3
        t_enc = timed_ev(lambda: ops.encode(ro_h, vd_h, z_h, div_h, None, cfg_h, want_pe=True))
        enc_bytes = P_h * (12 + 12 + 4 + 63 * 4) + Bh * N_RAYS * (24 + 27 * 4)          # xyz, viewdir, z, PE(xyz) per point; rays in, PE(dir) out
        # three input sets used in turn (3 x 268 MB): with one set, launches back to back re-read part of it from the 256 MB Infinity Cache
        # and the figure lands above what HBM can deliver
        sets = [(torch.rand(Bh * N_RAYS, N_SAMPLES, device=dev), torch.rand(Bh * N_RAYS, N_SAMPLES, 3, device=dev)) for _ in range(3)]
        turn = [0]

        def cmp_once():
            sg_, rg_ = sets[turn[0] % 3]
            turn[0] += 1
            return ops.composite_fwd(sg_, rg_, z_h, ops.Z_PER_OBJECT, False, N_RAYS)
        t_cmp = timed_ev(cmp_once, n=12)
        sig_h, rgb_h = sets[0]
        del sets
        cmp_bytes = P_h * 16 + Bh * N_RAYS * 20
        # scene composite (vis_scene): 131072 pixels x 3 objects x 64 samples, depth merge + composite
        P_s, n_s = 131072, 3 * N_SAMPLES
        # per object and pixel: near + (far - near) * (k + u_k) / S, the stratified depths of sample_from_rays (src/utils.py:159-164); the three
        # objects' depth ranges (4 m each, near in [2, 10) m) overlap for most pixels
        strat = (torch.arange(N_SAMPLES, device=dev) + torch.rand(P_s, 3, N_SAMPLES, device=dev)) / N_SAMPLES
        z_s = (torch.rand(P_s, 3, 1, device=dev) * 8 + 2 + strat * 4).view(P_s, n_s)
        del strat
        sig_s, rgb_s = torch.rand(P_s, n_s, device=dev), torch.rand(P_s, n_s, 3, device=dev)
        t_scn = timed_ev(lambda: ops.scene_composite(sig_s, rgb_s, z_s, True, run_length=N_SAMPLES))      # as scene.py calls it
        scn_bytes = P_s * n_s * 20 + P_s * 20
        del z_s, sig_s, rgb_s, sig_h, rgb_h
        mk = lambda b, t: {"GB_per_s": b / t / 1e9, "ms": t * 1e3, "bytes": b, "frac_of_8TBps": b / t / 8e12}
        hbm = {"encode": mk(enc_bytes, t_enc), "composite_fwd": mk(cmp_bytes, t_cmp), "scene_composite": dict(mk(scn_bytes, t_scn), shape=f"{P_s} pixels x 3 objects x {N_SAMPLES} samples"),
               "shape": f"{Bh} objects x {N_RAYS} rays x {N_SAMPLES} samples"}
    extra["hbm_bound_kernels"] = hbm
    result["extra"] = extra

    log("CPU baseline + parity")
    # ---- CPU baseline + parity (rank 0, N = 1 only): the oracle is the checker and the baseline, never the product
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import supnerf_oracle as O
        # the box's CPU share for one GPU is 16 cores whatever os.cpu_count() says; more threads only thrash
        cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
        torch.set_num_threads(cores)
        ro_c, vd_c, z_c = rays_o.cpu(), viewdir.cpu(), z.cpu()
        sc_c, tc_c = w["sc"].cpu(), w["tc"].cpu()

        def cpu_pass():
            with torch.no_grad():
                xyz, vd = O.points_on_rays(ro_c, vd_c, z_c)
                xyz = xyz / ob["obj_diag"]
                xyz, vd = O.object_frame_transforms(xyz, vd, False, False, True)
                sig, rgb = O.decoder_forward(w["params"], xyz, vd, sc_c, tc_c)
                return O.volume_rendering2(sig, rgb, z_c)
        ref = cpu_pass()
        times = []
        t_start = time.perf_counter()
        while len(times) < 3 or (time.perf_counter() - t_start < 12 and len(times) < 20):
            t0 = time.perf_counter(); ref = cpu_pass(); times.append(time.perf_counter() - t0)
        result["cpu_baseline"] = {"value": N_RAYS / float(np.median(times)), "unit": "rays/s", "cores": torch.get_num_threads(), "kind": "port",
                                  "sample": f"the whole workload: 4096 rays x 64 samples, forward, oracle/supnerf_oracle.py (PyTorch {torch.__version__} CPU), "
                                            f"median of {len(times)} passes ({sum(times):.1f} s of CPU work)"}
        tgt_c, occ_c = w["img"].reshape(-1, 3), w["mask"].reshape(-1, 1)
        fg = occ_c.clone(); fg[occ_c < 0] = 0
        ps = lambda rgb: float(-10 * torch.log10(((rgb - tgt_c) ** 2 * fg).sum() / (fg.sum() + 1e-9)))

        def parity(p):
            rgb_g, depth_g, acc_g = [t.cpu() for t in outs[p][:3]]
            return {"psnr_delta_db": abs(ps(rgb_g) - ps(ref[0])), "depth_l1_mean_m": float((depth_g - ref[1]).abs().mean()),
                    "rgb_max_abs": float((rgb_g - ref[0]).abs().max()), "acc_max_abs": float((acc_g - ref[2]).abs().max()), "rays": N_RAYS,
                    "bound": "north_star: PSNR delta <= 0.01 dB, depth L1 <= 1e-4"}
        result["parity"] = parity(prec)
        result[other]["parity"] = parity(other)
    if rank == 0:
        emit(result)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
