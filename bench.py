#!/usr/bin/env python3
"""bench.py -- images/sec extract+match (1600x1200, n4096) on MI355X.

One "step" = one pass of the hot path over one synthetic query image:
  sfd2_extract (ResSegNetV2 conv stack -> heat map -> NMS -> top-4096 -> descriptors)
  + sfd2_match_batch of its 4096 descriptors against K=50 resident database sets
    (the Aachen netvlad-50 unit of BASELINE.json configs[2]).
Inputs (images, database descriptors) are resident in HBM before the timed region.
Multi-GPU: one process per GPU, images sharded, no collective on the data path
("scaling": "weak"); torch.distributed is used for the barrier and the max-over-ranks time only.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus N ...            (no launcher: bench.py starts one worker per GPU itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

`value` is the fastest mode whose tests assert BASELINE.json north_star's tolerance (descriptors within 1e-3 of the fp32
reference): precision 'f16c', compensated fp16 -- fp16 MFMA operands plus one block-scaled MFMA per 32 channels that adds the
two first-order rounding terms (fp6 x fp6 records on conv2a / conv3a / conv3b, option fp6_acts, the default; fp8 elsewhere;
tests/test_gpu_f16c.py asserts 1e-3 at every BASELINE geometry; measured <= 6.2e-4 as shipped -- conv3b without its correction chunks where the load-time self-check finds the room: profiles/r06g_f16c_parity_measured.txt).  Other modes of the same workload, same bracket, in the same line with --full: `approx_f16` (plain fp16, descriptors within
3e-3: OUTSIDE the tolerance, reported for reference only), `strict_f32` (fp32 on the f32-input MFMA: descriptors within
2e-5, key-point list equal up to near-ties), `strict_f16x3` (three hi / lo fp16 passes, same tolerances as f32) and
`strict_kp_f16x3d` (f16x3's backbone and detector branch -- its key points bit for bit -- with the descriptor branch in plain fp16:
descriptors within 1e-3, i.e. north_star's contract as written: key-point list equal up to near-ties AND descriptors within 1e-3).
Tolerances are asserted by tests/, not here.

A plain run does what `value` needs and nothing else: it sets up, warms up (the ~1 s pre-heat, the W steps and the untimed
three-step pre-pass that `value` has always been measured behind), times the K steps, writes --dump-outputs and prints the
line.  --full adds every leg that takes a run of its own: the per-kernel breakdown and the roofline (with its single-stream
leg), `sustained`, the other BASELINE configs, the other precisions, the files -> stores `pipeline` and the CPU baseline.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W, TOPK, K_DB, N_DB = 1200, 1600, 4096, 50, 4096
PEAK_TFLOPS_F16 = 2500.0   # MI355X dense fp16/bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def pmc_traffic(kernel_label):
    """HBM-side bytes per launch of a kernel family from the committed PMC profile
    (profiles/pmc_traffic.json: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same
    bench command, read side doubled as MI355X_MICROARCH.md prescribes for gfx950)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            e = json.load(f).get(kernel_label)
            return e["bytes_per_launch"] if e else None
    except Exception:
        return None


def _cpu_info():
    """(model string, physical cores, logical cpus usable by this process) from /proc/cpuinfo."""
    model, cores = "unknown", set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name") and model == "unknown":
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    phys = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
    except OSError:
        pass
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    physical = min(len(cores), logical) if cores else logical
    return model, physical, logical


def _cpu_quota():
    """CPUs' worth of time the container's cgroup allows (cpu.max), or None: on a box with a quota every thread count above it is throttled -- the GPU boxes
    of this pool: 2 x 64 cores visible, cpu.max = 1600000 100000 = 16 CPUs (tools/diag/cpu_quota_probe.py, profiles/r06e_cpu_quota_probe.json)."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        return None if q == "max" else float(q) / float(p)
    except (OSError, ValueError):
        return None


def cpu_baseline(sd, n_match_sample=10):
    """The reference's CPU path, timed on this host beside the GPU number (warm-up 2,
    median of >= 5, core count and CPU model stated).  Two CPU implementations of the same unit (one 1600x1200
    top-4096 extract + 50 NNM matches of 4096 x 4096 x 128):
    oracle/torch_twin.py -- stock torch ops (oneDNN convolutions), i.e. the arithmetic the reference itself runs, on the
    thread count that is fastest on this host.  Written here from SURVEY section 8a; the reference's own files cannot travel."""
    import torch
    from oracle import torch_twin as tt
    from sfd2_amd import synth
    model, physical, logical = _cpu_info()
    twin = tt.Twin(sd)
    # oneDNN does not scale to every core of a big host on these shapes (measured on the 2 x 64-core EPYC 9575F box:
    # 128 threads 8.5 s per image, fewer threads faster): probe a few thread counts on a 640x480 image, keep the best
    probe = synth.make_image(480, 640, 5)
    best_t, best_s = physical, None
    for nt in sorted({min(physical, n) for n in (8, 16, 32, 64, 128, physical)}):
        torch.set_num_threads(nt)
        tt.extract(twin, probe, conf_th=0.001, topK=1024)
        t0 = time.perf_counter()
        tt.extract(twin, probe, conf_th=0.001, topK=1024)
        dt = time.perf_counter() - t0
        if best_s is None or dt < best_s:
            best_t, best_s = nt, dt
    torch.set_num_threads(best_t)
    img = synth.make_image(H, W, 5)
    t_ext = []
    pred = None
    for it in range(2 + 5):
        t0 = time.perf_counter()
        pred = tt.extract(twin, img, conf_th=0.001, topK=TOPK)
        if it >= 2:
            t_ext.append(time.perf_counter() - t0)
    d0 = pred["descriptors"].astype(np.float32)
    dbs = [synth.make_descriptors(N_DB, seed=100 + i) for i in range(n_match_sample)]
    t_m = []
    for it in range(2 + 5):
        t0 = time.perf_counter()
        for d1 in dbs:
            tt.nnm(d0, d1)
        if it >= 2:
            t_m.append((time.perf_counter() - t0) * (K_DB / n_match_sample))
    te, tm = float(np.median(t_ext)), float(np.median(t_m))
    torch_entry = {"value": round(1.0 / (te + tm), 5), "extract_s": round(te, 3), "match50_s": round(tm, 3),
                   "threads": best_t, "warmup": 2, "median_of": 5}
    # BASELINE.md section 4 asks for all physical cores: the same unit at that thread count beside the probed-best one
    all_cores = None
    if physical != best_t:
        torch.set_num_threads(physical)
        ta, tma = [], []
        for it in range(1 + 3):
            t0 = time.perf_counter()
            tt.extract(twin, img, conf_th=0.001, topK=TOPK)
            t1 = time.perf_counter()
            for d1 in dbs[:5]:
                tt.nnm(d0, d1)
            t2 = time.perf_counter()
            if it >= 1:
                ta.append(t1 - t0)
                tma.append((t2 - t1) * (K_DB / 5))
        tea, tmaa = float(np.median(ta)), float(np.median(tma))
        all_cores = {"value": round(1.0 / (tea + tmaa), 5), "unit": "images/sec", "threads": physical, "extract_s": round(tea, 3), "match50_s": round(tmaa, 3),
                     "warmup": 1, "median_of": 3}
        torch.set_num_threads(best_t)
    # (the C oracle -- the naive OpenMP loop nest the parity tests check against -- was timed here too until round 3: 4-6x slower than the
    #  twin, a single unwarmed sample; it is a checker, not a baseline, and is no longer in the line)
    return {"value": torch_entry["value"], "unit": "images/sec", "cores": best_t, "kind": "port", "model": model, "host_physical_cores": physical, "logical_cpus": logical,
            "threads": best_t, "median_of": 5, "warmup": 2, "all_cores": all_cores,
            "container_cpu_quota_cpus": _cpu_quota(),      # (the probe's best thread count follows this, not the host's core count)
            "sample": f"1 image {W}x{H} top-{TOPK} extract + {n_match_sample} of {K_DB} NNM matches 4096x4096x128 scaled x{K_DB // n_match_sample}; "
                      f"torch-CPU twin (stock torch ops, oneDNN convolutions; {best_t} threads = best of a probe over 8..{physical}): "
                      f"extract {te:.2f}s + match {tm:.2f}s",
            "implementations": {"torch": torch_entry}}


def spawn_workers(n, argv):
    """`python bench.py --gpus N` without a launcher: start one worker process per GPU (LOCAL_RANK = GPU index,
    rendezvous on 127.0.0.1), forward rank 0's JSON line.  Refuses when fewer than N GPUs are visible."""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n:
        raise SystemExit(f"--gpus {n} requested but {have} GPU(s) visible; refusing to report a smaller n_gpus")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SFD2_BENCH_WORKER="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0 = procs[0].communicate()[0].decode()
    rcs = [p.wait() for p in procs]
    sys.stdout.write(out0)
    sys.stdout.flush()
    if any(rcs):
        raise SystemExit(f"worker exit codes {rcs}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true", help="also run the legs beyond `value` (per-kernel breakdown and roofline, single-stream, "
                    "sustained, other configs, other precisions, pipeline, CPU baseline); --no-cpu-baseline, --no-strict, --no-pipeline, "
                    "--no-configs and --sustain 0 leave some out again")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--extract-only", action="store_true", help="configs[1]: extract without matching")
    ap.add_argument("--dump-layers", action="store_true", help="per-layer device times to stderr (needs --full)")
    ap.add_argument("--streams", type=int, default=2, help="contexts (HIP streams) per GPU processing different images concurrently "
                    "(default 2: the kernels of one image leave CUs idle -- tile tails, the small selection kernels, the row-marching "
                    "ResBlocks -- that a second image's kernels fill: +17 %% images/sec on one MI355X; 3 measures no better)")
    ap.add_argument("--no-profile", action="store_true", help="experiment: no per-launch events in the timed region")
    ap.add_argument("--branches", action="store_true", help="experiment: detector-head branch on a side stream (option 'branches')")
    ap.add_argument("--no-graphs", action="store_true", help="headline leg with eager launches instead of the per-context hipGraph cache")
    ap.add_argument("--graphs", action="store_true", help="(default since round 2; kept for old command lines) sfd2_extract_match with the per-context hipGraph cache (configs[4]); "
                                                          "per-kernel events are not available then")
    ap.add_argument("--no-strict", action="store_true", help="skip the strict-f32 leg")
    ap.add_argument("--strict-graphs", action="store_true", help="the parity legs (strict_f32, strict_f16x3, strict_kp_f16x3d, approx) in the headline's launch mode "
                                                                 "(sfd2_extract_match, one hipGraph replay per image) instead of eager launches")
    ap.add_argument("--no-pipeline", action="store_true", help="skip the files -> feature store -> match store leg (the `pipeline` object: tools/pipeline_bench.py "
                    "on a reduced workload, N = 1 only)")
    ap.add_argument("--no-configs", action="store_true", help="skip the short legs of the other BASELINE configs (the 'configs' object)")
    ap.add_argument("--sustain", type=float, default=2.0, help="seconds of the extra untimed-by-contract sustained leg (0 = off)")
    ap.add_argument("--lib", default=None, help="kernel A/B runs: another build of libsfd2hip.so (sfd2_amd/build.py build_lib(out=...))")
    ap.add_argument("--precision", default="f16c", choices=["f16c", "f16"], help="mode of the headline legs (default f16c: the "
                    "tolerance-conformant throughput mode; f16 = the 3e-3 approximation, for kernel A/Bs of that path)")
    ap.add_argument("--fp6-acts", type=int, default=1, help="f16c option fp6_acts (0: fp8 correction records everywhere, the round-3 arithmetic)")
    ap.add_argument("--comp-det", type=int, default=0, help="f16c option comp_det (1: the detector branch's 3x3 layers compensated)")
    ap.add_argument("--comp-heads", type=int, default=0, help="f16c option comp_heads (1: the head branches' 3x3 layers compensated as well)")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="sfd2_set_option on every context (A/B switches, e.g. fuse_rb23=0)")
    ap.add_argument("--rb-inner", type=int, default=2, help="f16c option rb_inner (2: the tensors inside the ResBlocks plain fp16, the shipped default; "
                    "1: only the grouped conv's output; 0: both compensated, descriptors <= 3.5e-4)")
    ap.add_argument("--comp-rb", type=int, default=1, help="f16c option comp_rb (0: ResBlocks on the fused fp16 kernel; descriptors ~7e-4)")
    ap.add_argument("--mix", action="store_true", help="every fifth query image in portrait orientation (SURVEY C2: the Aachen query set "
                    "is ~80 %% landscape / 20 %% portrait); the hipGraph cache then holds two geometries per stream")
    ap.add_argument("--size", default=None, help="WxH of the synthetic query images (default 1600x1200, the size the metric "
                                                 "is quoted on; e.g. 1024x1024 for BASELINE configs[3])")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step returned "
                    "(keypoints, scores, descriptors; matches, match_scores unless --extract-only) as DIR/<name>.npy, float32 / float64, "
                    "~5 MB; rank 0 only.  Inputs are seeded: two builds run with the same arguments can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_layers and not args.full:
        ap.error("--dump-layers needs --full (per-kernel figures are part of the full run)")
    global H, W
    if args.size:
        W, H = (int(v) for v in args.size.lower().split("x"))

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_workers(args.gpus, sys.argv[1:])
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: refusing to report an n_gpus that was not requested")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or os.environ.get("SFD2_BENCH_FORCE_DIST"):   # the second form lets a 1-GPU box exercise the N>1 code path
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from sfd2_amd import _lib, synth
    if args.lib:
        _lib.use_library(args.lib)
    # one process per GPU: the rank's threads (the pipeline leg's decoders / writers, torch's pools) stay on the socket its GPU hangs off
    from sfd2_amd.sharding import pin_to_gpu_socket
    placement = pin_to_gpu_socket(local_rank, local_world=world) if world > 1 else {"pinned": False, "why": "one rank: not pinned", "cpus": []}
    from sfd2_amd.model import ResSegNetV2

    sd = synth.make_state_dict(0)
    # ---- resident inputs: a few distinct query images per rank + K database descriptor sets (fp16)
    n_img = 5 if args.mix else 4
    geo = [(W, H) if (args.mix and i == 4) else (H, W) for i in range(n_img)]          # (rows, cols) of image i
    imgs = [torch.from_numpy(synth.make_image(geo[i][0], geo[i][1], 100 + rank * n_img + i)).to(dev) for i in range(n_img)]
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    db = []
    for _ in range(K_DB):
        d = torch.randn(N_DB, 128, generator=g)
        db.append((d / d.norm(dim=1, keepdim=True)).to(torch.float16).to(dev).contiguous())
    dbs = (_lib.DescSet * K_DB)(*[_lib.DescSet(d.data_ptr(), N_DB, _lib.DT_F16, _lib.LAYOUT_ND, 1) for d in db])
    mconf = _lib.MatchConf(_lib.MATCH_HLOC, 1, 0.0, 0.0, _lib.SIM_F16)   # NNM (hloc/match_features.py:21-28)

    use_graphs = not args.no_graphs
    class Lane:   # one context = one HIP stream, its packed weights, workspace and output buffers
        def __init__(self):
            self.model = ResSegNetV2(outdim=128, require_stability=True, precision=args.precision).eval()
            self.model.load_state_dict(sd)
            self.model.cuda(local_rank)
            self.ctx = self.model.context
            self.kpts = torch.empty((TOPK, 2), dtype=torch.float32, device=dev)
            self.scores = torch.empty((TOPK,), dtype=torch.float32, device=dev)
            self.desc = torch.empty((TOPK, 128), dtype=torch.float32, device=dev)
            self.matches = torch.empty((K_DB, TOPK), dtype=torch.int64, device=dev)
            self.mscores = torch.empty((K_DB, TOPK), dtype=torch.float32, device=dev)
            self.q = _lib.DescSet(self.desc.data_ptr(), TOPK, _lib.DT_F32, _lib.LAYOUT_ND, 1)
            self.n_out = ctypes.c_int(0)
            if use_graphs:
                self.ctx.set_option("graphs", 1)
            if args.precision == "f16c" and not args.comp_rb:
                self.ctx.set_option("comp_rb", 0)
            if args.precision == "f16c" and args.rb_inner != 2:
                self.ctx.set_option("rb_inner", args.rb_inner)
            if args.precision == "f16c" and args.comp_heads:
                self.ctx.set_option("comp_heads", 1)
            if args.precision == "f16c" and args.comp_det:
                self.ctx.set_option("comp_det", 1)
            if args.precision == "f16c" and not args.fp6_acts:
                self.ctx.set_option("fp6_acts", 0)
            if args.branches:
                self.ctx.set_option("branches", 1)
            for kv in args.opt:
                k, _, v = kv.partition("=")
                self.ctx.set_option(k, int(v))

    lanes = [Lane() for _ in range(max(1, args.streams))]
    ctx = lanes[0].ctx
    lib = ctx.lib
    matches = lanes[0].matches
    torch.cuda.synchronize()

    def step(i, only=None, eager=False):
        ln = lanes[i % len(lanes)] if only is None else only
        if use_graphs and not eager:
            _lib.check(lib.sfd2_extract_match(ln.ctx.h, imgs[i % n_img].data_ptr(), geo[i % n_img][0], geo[i % n_img][1], 0.001, TOPK, 0, ln.kpts.data_ptr(),
                                              ln.scores.data_ptr(), ln.desc.data_ptr(), dbs, 0 if args.extract_only else K_DB, 128,
                                              ctypes.byref(mconf), ln.matches.data_ptr(), ln.mscores.data_ptr()))
            return
        _lib.check(lib.sfd2_extract(ln.ctx.h, imgs[i % n_img].data_ptr(), 1, geo[i % n_img][0], geo[i % n_img][1], 0.001, TOPK, _lib.FLAG_ASYNC,
                                    ln.kpts.data_ptr(), ln.scores.data_ptr(), ln.desc.data_ptr(), 1, TOPK, ctypes.byref(ln.n_out)))
        if not args.extract_only:
            _lib.check(lib.sfd2_match_batch(ln.ctx.h, ctypes.byref(ln.q), dbs, K_DB, 128, ctypes.byref(mconf),
                                            ln.matches.data_ptr(), ln.mscores.data_ptr(), 1, _lib.FLAG_ASYNC))

    def sync_all():
        for ln in lanes:
            ln.ctx.sync()

    def dump_outputs(i):
        """--dump-outputs: the arrays step(i) left in its lane's buffers, cut to the key-point count of that extraction (the later legs
        reuse the buffers, so this runs right after the timed region)."""
        ln = lanes[i % len(lanes)]
        n = ctypes.c_int(0)
        _lib.check(lib.sfd2_extract_count(ln.ctx.h, ctypes.byref(n)))
        k = max(0, min(n.value, TOPK))
        outs = {"keypoints": ln.kpts[:k], "scores": ln.scores[:k], "descriptors": ln.desc[:k]}
        if not args.extract_only:
            outs["matches"] = ln.matches[:, :k].to(torch.float64)      # (-1 = no match; exact in float64)
            outs["match_scores"] = ln.mscores[:, :k]
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, t in outs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), t.cpu().numpy())

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # untimed pre-heat (~1 s: clocks, allocator, lazily created kernels), then the W warm-up steps
    t_heat = time.perf_counter()
    while time.perf_counter() - t_heat < 1.0:
        for i in range(8):
            step(i)
        sync_all()
    for i in range(max(args.warmup, len(lanes))):
        step(i)
    sync_all()
    n_kp = ctypes.c_int(0)
    _lib.check(lib.sfd2_extract_count(ctx.h, ctypes.byref(n_kp)))
    if n_kp.value != TOPK and not os.environ.get("SFD2_BENCH_ALLOW_FEW"):   # (timing ablations produce garbage images)
        raise SystemExit(f"synthetic image yielded {n_kp.value} < {TOPK} key points; the match leg assumes {TOPK}")

    def fam_key(kernel):
        # conv2a / conv3a / conv3b of the compensated mode are instantiations of one kernel template (conv3_kernels.hip): with option "c3b_plain" conv3a
        # is "<comp,plain out>" and conv3b "<comp out>" (no correction chunks) -- one family, as in every earlier round's line
        return "conv3x3_pp<comp>" if kernel.startswith("conv3x3_pp<comp") else kernel

    def dominant_family(rows):
        fam = {}
        for r in rows:
            f = fam.setdefault(fam_key(r["kernel"]), {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0, "layers": [], "issued_flops": 0.0})
            # matrix time of a unit relative to the plain fp16 unit's two 32-cycle MFMAs: + one scaled MFMA (fp6 x fp6: 33.5 cycles, fp8: 66) where the
            # instantiation has correction chunks (profiles/r04_mfma_probe.txt)
            k = r["kernel"]
            cf = 1.0 if (not k.startswith("conv3x3_pp<comp") or k == "conv3x3_pp<comp out>") else (64.0 + (33.5 if args.fp6_acts else 66.0)) / 64.0
            f["issued_flops"] += r["flops"] * r["launches"] * cf
            f["ms"] += r["ms_total"]
            f["flops"] += r["flops"] * r["launches"]
            f["bytes"] += r["bytes"] * r["launches"]
            f["launches"] += r["launches"]
            f["layers"].append(r["name"])
        return fam

    # untimed pre-pass with every launch bracketed: per-kernel breakdown (reported with --full) + which family dominates.  Every run
    # makes it: `value` has always been measured behind it, and without it the hipGraph headline measured ~2 % faster on one MI355X
    ctx.set_profiling(8)
    for i in range(3):
        step(0, lanes[0], eager=True)
    breakdown_rows = ctx.layer_timings()
    fam_all = dominant_family(breakdown_rows)
    dom_name = max(fam_all.items(), key=lambda kv: kv[1]["ms"])[0]
    dom_filter = "conv3x3_pp<comp" if dom_name == "conv3x3_pp<comp>" else dom_name      # (substring filter of sfd2_set_profile_filter)

    # timed region: HIP events only around the dominant kernel's launches (an event pair costs
    # ~2-4 us of stream time; bracketing all ~35 launches would slow the step by ~10 %)
    ctx.set_profiling(0 if (args.no_profile or use_graphs) else 2 * args.steps + 2, dom_filter)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    sync_all()
    barrier()
    dt = time.perf_counter() - t0
    layers = ctx.layer_timings()
    ctx.set_profiling(0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.steps - 1)

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        if dist is not None:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def all_ranks(x):
        """x of every rank, in rank order (the max is what `value` uses; min / max side by side show an imbalance at once)."""
        t = torch.zeros(world, dtype=torch.float64, device=dev)
        t[rank] = x
        if dist is not None:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    dt_ranks = all_ranks(dt)
    dt = max_over_ranks(dt)
    n_matched = int((matches >= 0).sum().item()) if not args.extract_only else 0

    # With more than one stream per GPU the launches of different images share the CUs, so the event-timed duration of a
    # launch in the region above is not its own (it stretches by whatever ran beside it).  The roofline of the dominant
    # kernel therefore comes from a second timed leg of this same run: the same K steps, the same bracketing, on ONE
    # stream; the concurrent region's figures are reported next to it.
    single = None
    layers_concurrent = None
    if args.full and (len(lanes) > 1 or use_graphs) and not args.no_profile:
        layers_concurrent = layers
        ctx.set_profiling(2 * args.steps + 2, dom_filter)
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(i, lanes[0], eager=True)
        lanes[0].ctx.sync()
        barrier()
        d1 = max_over_ranks(time.perf_counter() - t0)
        layers = ctx.layer_timings()
        ctx.set_profiling(0)
        single = {"value": round(args.steps * world / d1, 3), "unit": "images/sec", "ms_per_step": round(d1 / args.steps * 1e3, 4),
                  "steps": args.steps, "streams_per_gpu": 1, "launches": "eager, HIP events around the dominant kernel"}

    # extra leg (not `value`): the same steps for ~args.sustain seconds without any per-launch events, to show the
    # K-step number is not a boost-clock artefact
    sustained = None
    if args.full and args.sustain > 0:
        n_s = max(args.steps, int(args.sustain / max(dt / args.steps, 1e-6)))
        barrier()
        t0 = time.perf_counter()
        for i in range(n_s):
            step(i)
        sync_all()
        barrier()
        ds = max_over_ranks(time.perf_counter() - t0)
        sustained = {"steps": n_s, "seconds": round(ds, 3), "value": round(n_s * world / ds, 3), "unit": "images/sec"}

    # The other BASELINE configs on this GPU, same bracket, short legs: SURVEY C2's query mix (every fifth image portrait:
    # two geometries per hipGraph cache), configs[3]'s geometry (RobotCar 1024x1024, netvlad-20) and configs[4]'s (Extended CMU 1024x768,
    # netvlad-10, per-GPU hipGraph capture) -- each on the headline's lanes (two streams, hipGraph replay per image).
    def config_leg(label, geos, k_db, n_steps, seed0):
        ims = [torch.from_numpy(synth.make_image(gh, gw, seed0 + rank * 16 + i)).to(dev) for i, (gh, gw) in enumerate(geos)]

        def cstep(i):
            ln = lanes[i % len(lanes)]
            j = i % len(ims)
            if use_graphs:
                _lib.check(lib.sfd2_extract_match(ln.ctx.h, ims[j].data_ptr(), geos[j][0], geos[j][1], 0.001, TOPK, 0, ln.kpts.data_ptr(),
                                                  ln.scores.data_ptr(), ln.desc.data_ptr(), dbs, k_db, 128, ctypes.byref(mconf),
                                                  ln.matches.data_ptr(), ln.mscores.data_ptr()))
            else:
                _lib.check(lib.sfd2_extract(ln.ctx.h, ims[j].data_ptr(), 1, geos[j][0], geos[j][1], 0.001, TOPK, _lib.FLAG_ASYNC,
                                            ln.kpts.data_ptr(), ln.scores.data_ptr(), ln.desc.data_ptr(), 1, TOPK, ctypes.byref(ln.n_out)))
                _lib.check(lib.sfd2_match_batch(ln.ctx.h, ctypes.byref(ln.q), dbs, k_db, 128, ctypes.byref(mconf),
                                                ln.matches.data_ptr(), ln.mscores.data_ptr(), 1, _lib.FLAG_ASYNC))
        # every (lane, image) pair is seen twice before the clock starts: the first sight sizes the workspace, the second captures
        n_pairs = len(lanes) * len(ims)
        for i in range(3 * n_pairs + 4):
            cstep(i)
        sync_all()
        barrier()
        t0 = time.perf_counter()
        for i in range(n_steps):
            cstep(i)
        sync_all()
        barrier()
        d = max_over_ranks(time.perf_counter() - t0)
        return {"workload": label, "value": round(n_steps * world / d, 3), "unit": "images/sec", "ms_per_step": round(d / n_steps * 1e3, 4),
                "steps": n_steps, "db_sets_per_query": k_db, "max_keypoints": TOPK,
                "images": sorted({f"{gw}x{gh}" for gh, gw in geos}), "streams_per_gpu": len(lanes),
                "launch": "hipGraph replay per image" if use_graphs else "eager", "dtype": args.precision}

    configs_obj = None
    if args.full and not args.no_configs and not args.extract_only and not args.size and not args.mix:
        n_c = max(20, min(args.steps, 60))
        configs_obj = {
            "aachen_mix_80_20": config_leg("SURVEY C2: aachen_v1.1 queries, every fifth image portrait (1200x1600), K = 50 (BASELINE configs[2])",
                                           [(1200, 1600)] * 4 + [(1600, 1200)], K_DB, n_c, 300),
            "robotcar_1024x1024_k20": config_leg("BASELINE configs[3] geometry: 1024x1024 queries, netvlad-20", [(1024, 1024)] * 4, 20, n_c, 400),
            "ecmu_1024x768_k10": config_leg("BASELINE configs[4] geometry: 1024x768 queries, netvlad-10, hipGraph replay", [(768, 1024)] * 4, 10, n_c, 500),
            # every database image of configs[2] has this size: height not a multiple of 8 (score map resized, no fused post kernel) nor of 4 (no
            # space-to-depth conv2b); extract only -- database images are not queries
            "aachen_db_1600x1063": config_leg("aachen_v1.1 database images 1600x1063 (odd geometry: heat-map resize path), extract only", [(1063, 1600)] * 4, 0, n_c, 600),
        }
    # what the compensated mode's range status saw over everything above (the headline's steps; with --full the legs as well; include/sfd2_hip.h
    # "Range management"): nothing may have saturated
    range_seen = None
    if args.precision == "f16c":
        sts = [ln.ctx.range_status() for ln in lanes]
        range_seen = {"saturated": sorted({t for s in sts for t in s["saturated"]}), "low": sorted({t for s in sts for t in s["low"]}),
                      "fallbacks": sum(s["fallbacks"] for s in sts),
                      "stored_max": {k: round(max(s["tensors"][k]["max_stored"] for s in sts), 3) for k in sts[0]["tensors"]}}

    # strict parity mode, same workload, same bracket (precision 'f32'; the matcher is unchanged: its fp16 GEMM already
    # meets the 1e-3 similarity tolerance)
    # parity modes, same workload, same bracket: precision 'f32' (exact fp32 on the f32-input MFMA) and 'f16x3' (the same
    # buffers and layer sequence with the convolutions on the fp16 matrix path in three passes); the matcher is unchanged:
    # its fp16 GEMM already meets the 1e-3 similarity tolerance
    def parity_leg(mode, headline_launch=False):
        for ln in lanes:
            ln.ctx.set_precision(mode)
        n_st = max(4, min(args.steps, 10))
        replay = use_graphs and (args.strict_graphs or headline_launch)
        if headline_launch:
            n_st = max(n_st, min(args.steps, 40))

        def sstep(i):
            if replay:      # the headline's launch mode (one hipGraph replay per image) for this precision too
                return step(i)
            sl = lanes[i % len(lanes)]
            _lib.check(lib.sfd2_extract(sl.ctx.h, imgs[i % n_img].data_ptr(), 1, geo[i % n_img][0], geo[i % n_img][1], 0.001, TOPK, _lib.FLAG_ASYNC,
                                        sl.kpts.data_ptr(), sl.scores.data_ptr(), sl.desc.data_ptr(), 1, TOPK, ctypes.byref(sl.n_out)))
            if not args.extract_only:
                _lib.check(lib.sfd2_match_batch(sl.ctx.h, ctypes.byref(sl.q), dbs, K_DB, 128, ctypes.byref(mconf),
                                                sl.matches.data_ptr(), sl.mscores.data_ptr(), 1, _lib.FLAG_ASYNC))
        for i in range((4 if replay else 2) * max(len(lanes), n_img)):      # (a geometry is captured the second time a context sees it)
            sstep(i)
        sync_all()
        barrier()
        t0 = time.perf_counter()
        for i in range(n_st):
            sstep(i)
        sync_all()
        barrier()
        dst = max_over_ranks(time.perf_counter() - t0)
        for ln in lanes:
            ln.ctx.set_precision(args.precision)
        par = {"f32": "descriptors <= 2e-5, ordered key-point list equal up to near-ties (tests/test_gpu_parity.py::test_strict_*)",
               "f16x3": "descriptors <= 2e-5, ordered key-point list equal up to near-ties (tests/test_gpu_baseline_configs.py::test_f16x3_*)",
               "f16x3d": "key points and scores bit-identical to f16x3's (ordered list equal to the reference's up to near-ties), descriptors <= 1e-3 "
                         "(descriptor branch in plain fp16: tests/test_gpu_x3_desc16.py)",
               "f16": "OUTSIDE north_star's tolerance: descriptors <= 3e-3 (measured 1.8e-3), key-point set IoU >= 0.93 (tests/test_gpu_parity.py)",
               "f16c": "descriptors <= 1e-3 asserted (measured <= 6.2e-4), key-point set IoU >= 0.985 (tests/test_gpu_f16c.py)"}[mode]
        return {"value": round(n_st * world / dst, 3), "unit": "images/sec", "ms_per_step": round(dst / n_st * 1e3, 3),
                "steps": n_st, "dtype": mode, "streams_per_gpu": len(lanes),
                "launch": "hipGraph replay per image (sfd2_extract_match)" if replay else "eager", "parity": par}

    strict = strict_x3 = strict_kp = approx = north_star_strict = None
    if args.full and not args.no_strict:
        strict = parity_leg("f32")
        strict_x3 = parity_leg("f16x3")
        strict_kp = parity_leg("f16x3d")
        # north_star read to the letter -- the reference's ordered key-point list (up to fp32 near-ties) AND descriptors within 1e-3 -- in the HEADLINE's
        # launch mode (the same lanes, one hipGraph replay per image): what `value` would be if list-level parity were demanded of it
        north_star_strict = parity_leg("f16x3d", headline_launch=True)
        north_star_strict["contract"] = ("north_star as written: key-point list = the fp32 reference's up to near-ties (bit-identical to f16x3's), descriptors <= 1e-3; "
                                         "`value` (f16c) meets the descriptor tolerance and the key-point SET (IoU >= 0.985, rank order asserted statistically)")
        approx = parity_leg("f16" if args.precision == "f16c" else "f16c")

    if rank == 0:
        # the headline line: what the set-up and the timed region give
        out = {
            "metric": "images/sec extract" + ("" if args.extract_only else "+match") + f" ({W}x{H}, n4096)",
            "value": round(args.steps * world / dt, 3), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": ("aachen_v1.1 day query, extract-only (BASELINE configs[1])" if args.extract_only else
                                    "aachen_v1.1 query extract + NNM match vs netvlad-50 resident db sets (BASELINE configs[2])"),
                       "image": f"{W}x{H}" + (" (every fifth image portrait)" if args.mix else ""), "max_keypoints": TOPK, "db_sets_per_query": 0 if args.extract_only else K_DB,
                       "db_keypoints": N_DB, "weights": "synthetic seeded ResSegNetV2 (checkpoint not shipped)",
                       "parallelism": f"images sharded over {world} GPU(s), no collective", "streams_per_gpu": len(lanes),
                       "launch": "hipGraph replay per image (sfd2_extract_match)" if use_graphs else "eager"},
            "mutual_matches_last_step": n_matched,
            "parity": ({"mode": "f16c: compensated fp16 (fp16 MFMA + one block-scaled MFMA of the rounding residuals per 32 channels -- "
                                + ("fp6 x fp6 on conv2a / conv3a / conv3b (option fp6_acts), fp8 elsewhere" if args.fp6_acts else "fp8 operands") + " -- fp32 accumulate)"
                                + (f"; backbone compensated, tensors inside the ResBlocks per option rb_inner = {args.rb_inner}" if args.comp_rb else "; option comp_rb = 0 (ResBlocks plain fp16)"),
                        "descriptors_max_abs": "<= 1e-3 asserted = north_star's tolerance (measured "
                                               + (("<= 6.2e-4 as shipped (option c3b_plain on where the self-check allows: margin_selfcheck.c3b_plain; 4.9e-4 with it off)", "<= 3.8e-4", "<= 3.5e-4")[2 - max(0, min(2, args.rb_inner))] if args.comp_rb else "<= 8.5e-4") + " at 480x640 .. 2048x1536)",
                        "keypoint_set_iou": ">= 0.985 asserted (measured 0.992 - 1.0)" if args.comp_rb else ">= 0.97 asserted (measured 0.991 - 0.996)",
                        "keypoint_order": "asserted among the points whose stability class did not flip: Spearman >= 0.999, rank shift <= n / 32 (measured <= 90 of 4096); the ordered LIST of the reference is `north_star_strict`'s contract",
                        "selection_given_heat_map": "bit-exact", "asserted_in": "tests/test_gpu_f16c.py",
                        "measured_in": "profiles/r06g_f16c_parity_measured.txt"} if args.precision == "f16c" else
                       {"mode": "f16 throughput (OUTSIDE north_star's 1e-3)", "descriptors_max_abs": "<= 3e-3 (measured 1.8e-3)", "keypoint_set_iou": ">= 0.93",
                        "selection_given_heat_map": "bit-exact", "asserted_in": "tests/test_gpu_parity.py"}),
            "range_status": range_seen,
            "margin_selfcheck": (lanes[0].ctx.margin_status() if args.precision == "f16c" else None),
            "per_rank": {"ms_per_step": [round(d / args.steps * 1e3, 4) for d in dt_ranks], "min": round(min(dt_ranks) / args.steps * 1e3, 4),
                         "max": round(max(dt_ranks) / args.steps * 1e3, 4), "cpu_placement_rank0": {k: placement[k] for k in ("pinned", "why")}},
        }
    if rank == 0 and args.full:
        # dominant kernel family = largest summed device time
        fam = dominant_family(layers)
        if not fam:
            print(json.dumps({"value": round(args.steps * world / dt, 3), "n_gpus": world, "ms_per_step": round(dt / args.steps * 1e3, 4),
                              "sustained": sustained, "strict_f32": strict,
                              "note": "no per-launch events (--no-profile)", "graphs": bool(use_graphs)}), flush=True)
            if dist is not None:
                dist.barrier()
                dist.destroy_process_group()
            return
        dom_name, dom = max(fam.items(), key=lambda kv: kv[1]["ms"])
        is_gemm = dom["flops"] > 0
        if is_gemm:
            achieved = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
            roof = {"bound": "mfma", "kernel": dom_name, "layers": dom["layers"], "achieved": round(achieved, 2),
                    "peak": PEAK_TFLOPS_F16, "unit": "TFLOP/s", "frac": round(achieved / PEAK_TFLOPS_F16, 4),
                    "avg_launch_ms": round(dom["ms"] / max(1, dom["launches"]), 5), "launches": dom["launches"],
                    "traffic": pmc_traffic(dom_name),
                    "traffic_source": "profiles/pmc_traffic.json (committed rocprofv3 --pmc passes of this command; not re-measured in this run)"}
            # matrix time of a compensated 32-channel unit relative to the plain one's two v_mfma_f32_32x32x16_f16 (2 x 32 cycles), measured
            # (profiles/r04_mfma_probe.txt): + one v_mfma_scale_f32_32x32x64_f8f6f4 of 66 cycles with fp8 operands, 33.5 with fp6 on both sides
            # (option fp6_acts, the default for this family's three layers)
            corr_factor = dom["issued_flops"] / dom["flops"]
            if "comp" in dom_name:
                roof["note"] = ("achieved / frac count ALGORITHMIC FLOPs (2 * MAC of the layer) against the fp16 peak; an instantiation with correction chunks also "
                                "issues one correction MFMA (32x32x64, " + ("fp6 x fp6: 33.5" if args.fp6_acts else "fp8: 66") + " cycles) per two 32x32x16 (2 x 32 cycles); "
                                f"over this family's launches that is {corr_factor:.2f}x the matrix time of plain fp16 layers: 'frac_of_issued_peak' = frac * {corr_factor:.2f}")
                roof["frac_of_issued_peak"] = round(corr_factor * achieved / PEAK_TFLOPS_F16, 4)
                roof["instantiations"] = sorted({r["kernel"] + ": " + r["name"] for r in layers if fam_key(r["kernel"]) == dom_name})
            # what this part sustains on v_mfma_f32_32x32x16_f16 alone (tools/probe/mfma_peak.hip, profiles/r04_mfma_probe.txt): one MFMA per 32.2-32.9
            # cycles and SIMD in every configuration; the clock the part holds depends on the operands' switching activity -- 2.39 GHz on zeros
            # (2.49 PFLOP/s), 1.73 GHz on post-ReLU-like activations (1.77), 1.65 GHz on uniform +-0.5 (1.68).  A POWER ceiling, not an issue limit:
            # context for `frac`, which stays against the nominal peak.  (Round 3 quoted 1.11 PFLOP/s from an issue-limited probe: retracted.)
            issued = corr_factor * achieved
            roof["mfma_only_probe"] = {"zeros": 2490.0, "relu_like": 1765.0, "uniform": 1680.0, "unit": "TFLOP/s",
                                       "source": "profiles/r04_mfma_probe.txt (not re-measured in this run)",
                                       "issued_frac_of_relu_like": round(issued / 1765.0, 4),
                                       "note": "issued-FLOP rate of this kernel (correction MFMAs counted at fp16-equivalent time) / the MFMA-only rate on relu-like data"}
            roof["power"] = {"cap_w": 1400, "socket_w_during_this_loop": "1372-1399", "sclk_ghz": "1.97-2.09",
                             "source": "profiles/r04s_power_during_bench.txt (rocm-smi sampled during the headline loop; not re-measured in this run)",
                             "note": "the part runs this workload at its power cap: time follows the work issued (MFMAs, VALU, bytes) more than its overlap"}
            if single is not None:
                roof["measured_in"] = ("single-stream timed leg of this run (same K steps and bracketing, one stream per GPU, eager "
                                       "launches: see 'single_stream').  The headline region replays one hipGraph per image on "
                                       f"{len(lanes)} stream(s) per GPU: no per-launch events inside a graph, and with two streams a launch's "
                                       "duration includes its neighbour's work ('concurrent' = the eager two-stream figure when --no-graphs)")
                famc = dominant_family(layers_concurrent or [])
                if dom_name in famc and famc[dom_name]["ms"] > 0:
                    ac = famc[dom_name]["flops"] / (famc[dom_name]["ms"] * 1e-3) / 1e12
                    roof["concurrent"] = {"achieved": round(ac, 2), "frac": round(ac / PEAK_TFLOPS_F16, 4),
                                          "avg_launch_ms": round(famc[dom_name]["ms"] / max(1, famc[dom_name]["launches"]), 5),
                                          "launches": famc[dom_name]["launches"]}
        else:
            achieved = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9
            roof = {"bound": "hbm", "kernel": dom_name, "layers": dom["layers"], "achieved": round(achieved, 2),
                    "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(achieved / PEAK_HBM_GBS, 4),
                    "avg_launch_ms": round(dom["ms"] / max(1, dom["launches"]), 5), "launches": dom["launches"],
                    "traffic": pmc_traffic(dom_name)}
        total_ms = sum(r["ms_total"] / max(1, r["launches"]) for r in breakdown_rows) * 1.0
        if args.dump_layers:
            for r in breakdown_rows:
                ms = r["ms_total"] / max(1, r["launches"])
                tf = r["flops"] / (ms * 1e-3) / 1e12 if ms > 0 else 0
                gb = r["bytes"] / (ms * 1e-3) / 1e9 if ms > 0 else 0
                print(f"{r['name']:16s} {r['kernel']:34s} {ms*1e3:9.1f} us  {r['flops']/1e9:8.2f} GF {tf:8.1f} TF/s  "
                      f"{r['bytes']/1e6:8.1f} MB {gb:8.0f} GB/s", file=sys.stderr)
        breakdown = {k: round(v["ms"] / 3, 4) for k, v in sorted(fam_all.items(), key=lambda kv: -kv[1]["ms"])}
        out.update({
            "roofline": roof, "kernel_ms_per_step": breakdown, "device_ms_per_step": round(total_ms, 4),
            "single_stream": single, "sustained": sustained, "configs": configs_obj,
            "strict_f32": strict, "strict_f16x3": strict_x3, "strict_kp_f16x3d": strict_kp, "north_star_strict": north_star_strict,
            ("approx_f16" if args.precision == "f16c" else "f16c"): approx,
        })
        if world == 1 and not args.no_pipeline and not args.extract_only and not args.size and args.precision == "f16c":
            # not `value`: what the reference-shaped DRIVERS reach from JPEG files and stores (host decode, PCIe, float64 stores included)
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location("pipeline_bench", os.path.join(ROOT, "tools", "pipeline_bench.py"))
                pb = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(pb)
                lanes.clear()                      # the headline contexts' workspaces are not needed any more
                torch.cuda.empty_cache()
                out["pipeline"] = pb.run(pb.parse_args(["--queries", "160", "--db", "64", "--k", "50", "--workers", "16", "--precision", "f16c",
                                                        "--serial-images", "16", "--serial-pairs", "100"]))
                out["pipeline"]["note"] = ("extract_localization.main(num_workers=16) and match_features.main(grouped=True) on synthetic JPEG files, timed end to end "
                                           "(tools/pipeline_bench.py; DESIGN.md section 6); never part of `value`")
            except Exception as e:      # noqa: BLE001 -- the leg is informative: a failure must not cost the line
                out["pipeline"] = {"error": repr(e)}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(sd)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
