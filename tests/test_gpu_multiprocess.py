"""The N > 1 code paths, executed on ONE MI355X: no 8-GPU node has been available to any round, so what
can be run is run here -- bench.py's distributed bracket (NCCL init, barrier, MAX all-reduce) on a world of one, bench.py
as torch.distributed.run launches it, and the sharded drivers with the REAL extractor and matcher in two processes that
share the device (rendezvous over gloo: the data path has no collective, extract_localization.py:240,
hloc/match_features.py:90)."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
         "--no-strict", "--sustain", "0"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_bench_distributed_bracket_on_one_gpu():
    """SFD2_BENCH_FORCE_DIST=1: the N > 1 branch of bench.py (init_process_group('nccl'), dist.barrier around the timed
    region, all_reduce(MAX) of the elapsed time) with WORLD_SIZE = 1."""
    env = dict(os.environ, SFD2_BENCH_FORCE_DIST="1", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(BENCH + ["--full"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = _one_json_line(r.stdout.decode())
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["dtype"] == "f16c" and "roofline" in d
    # every rank's own time beside the max-over-ranks the value uses (VERDICT r5 #5c): one entry per rank, through the all-reduce of the N > 1 branch
    pr = d["per_rank"]
    assert len(pr["ms_per_step"]) == 1 and pr["min"] == pr["max"] == pr["ms_per_step"][0] and abs(pr["max"] - d["ms_per_step"]) < 1e-3
    assert d["margin_selfcheck"]["c3b_plain"] in (True, False) and "north_star_strict" in d


def test_bench_under_torch_distributed_run():
    """Exactly the driver's launch line for N > 1, with N = 1."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port())] + BENCH[1:]
    r = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = _one_json_line(r.stdout.decode())
    assert d["n_gpus"] == 1 and d["value"] > 0


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs: the last timed step's arrays as .npy (float32 / float64, at most 64 MB), the same bits from two runs with the same
    arguments -- also when the number of steps, and so the last step's lane and image, is odd."""
    import numpy as np
    cmd = BENCH + ["--no-pipeline", "--no-configs", "--steps", "5"]     # (a later --steps overrides BENCH's)
    got = []
    for run in ("a", "b"):
        r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / run)], env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        d = _one_json_line(r.stdout.decode())
        assert d["steps"] == 5 and d["ms_per_step"] > 0
        got.append({n: np.load(tmp_path / run / (n + ".npy")) for n in ("keypoints", "scores", "descriptors", "matches", "match_scores")})
    a, b = got
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["keypoints"].shape == (4096, 2) and a["descriptors"].shape == (4096, 128) and a["matches"].shape == (50, 4096)
    for n in a:
        assert a[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(a[n], b[n]), n
    assert np.allclose(np.linalg.norm(a["descriptors"], axis=1), 1.0, atol=1e-3)
    assert (a["matches"] >= 0).any() and np.array_equal(a["matches"], np.round(a["matches"]))


def test_bench_plain_run_is_the_headline_alone():
    """Without --full the line carries the headline and what the timed region itself gave; no leg that needs a run of its own."""
    r = subprocess.run(BENCH, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = _one_json_line(r.stdout.decode())
    assert d["metric"] == "images/sec extract+match (1600x1200, n4096)" and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert d["dtype"] == "f16c" and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert "range_status" in d and d["margin_selfcheck"]["c3b_plain"] in (True, False)
    for k in ("roofline", "kernel_ms_per_step", "single_stream", "sustained", "configs", "strict_f32", "north_star_strict", "approx_f16",
              "pipeline", "cpu_baseline"):
        assert k not in d, k


def test_bench_refuses_unrequested_world():
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run(BENCH, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b"refusing" in r.stderr


WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %r)
    import numpy as np
    import torch.distributed as dist
    from sfd2_amd import extract_localization as el, match_features as mf, synth
    from sfd2_amd.feature_io import open_store
    rank, world = int(os.environ["RANK"]), 2
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%%s" %% os.environ["PORT"], rank=rank, world_size=world)
    out = os.environ["OUT"]
    sd = synth.make_state_dict(0)
    images = [{"name": "db/img%%02d.jpg" %% i, "image": synth.make_image(96, 128, 40 + i), "original_size": (128, 96)} for i in range(5)]
    conf = dict(el.confs["ressegnetv2-20220810-wapv2-sd2mfsf-uspg-0001-n4096-r1600"])
    conf["model"] = dict(conf["model"], max_keypoints=150)
    # the real HIP extractor: each process creates its own context (one per process, as on N GPUs) on device 0
    path = el.main(conf, images, out, state_dict=sd, precision="f16c", world=world, rank=rank, barrier=dist.barrier)
    dist.barrier()
    pairs = ["db/img00.jpg db/img01.jpg", "db/img02.jpg db/img03.jpg", "db/img04.jpg db/img00.jpg", "db/img01.jpg db/img00.jpg"]
    mpath = mf.main(mf.confs["NNM"], pairs, conf["output"], out, world=world, rank=rank, barrier=dist.barrier)
    dist.barrier()
    if rank == 0:
        solo = os.path.join(out, "solo")
        p1 = el.main(conf, images, solo, state_dict=sd, precision="f16c")
        m1 = mf.main(mf.confs["NNM"], pairs, conf["output"], solo)
        for got, want in ((path, p1), (mpath, m1)):
            a, b = open_store(got, "r"), open_store(want, "r")
            assert list(a.keys()) == list(b.keys()) and len(list(a.keys())) > 0
            for k in a.keys():
                for ds in b[k].keys():
                    x, y = np.asarray(a[k][ds].__array__()), np.asarray(b[k][ds].__array__())
                    assert x.dtype == y.dtype and np.array_equal(x, y), (k, ds)   # same kernels, same inputs: bit-identical
        assert len(list(open_store(mpath, "r").keys())) == 3
        print("GPU_DRIVERS_OK")
    dist.barrier()
    dist.destroy_process_group()
""") % ROOT


def test_sharded_drivers_two_processes_one_device(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), PORT=str(port), OUT=str(tmp_path / "out"))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "GPU_DRIVERS_OK" in outs[0]


def test_reference_shaped_command_lines_single_and_torchrun(tmp_path):
    """`python -m sfd2_amd.extract_localization --image_dir .. --export_dir .. --conf ..` and `python -m sfd2_amd.match_features --export_dir .. --features ..
    --pairs .. --conf NNM` -- the reference scripts' own arguments (extract_localization.py:281-291, hloc/match_features.py:129-142) -- alone and as two
    ranks under torch.distributed.run sharing the one GPU: the same stores either way, and --exhaustive writes its pairs file."""
    pytest.importorskip("PIL")
    import numpy as np
    import torch
    from PIL import Image
    from sfd2_amd import synth, feature_io as fio
    root = tmp_path / "images"
    (root / "db").mkdir(parents=True)
    (root / "query").mkdir(parents=True)
    for i in range(7):
        u8 = (synth.make_image(96 + 8 * (i % 3), 128, 700 + i).transpose(1, 2, 0) * 255).astype(np.uint8)
        Image.fromarray(u8).save(root / ("query" if i < 2 else "db") / f"im{i}.png")
    ck = tmp_path / "ck.pth"
    torch.save({"model": {k: torch.from_numpy(v) for k, v in synth.make_state_dict(0).items()}}, ck)
    conf = "ressegnetv2-20220810-wapv2-sd2mfsf-uspg-0001-n2000-r1024"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    def run(cmd):
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stdout.decode()
    tr = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1"]
    ex = ["-m", "sfd2_amd.extract_localization", "--image_dir", str(root), "--conf", conf, "--weights", str(ck), "--precision", "f16c", "--num_workers", "2"]
    out1, out2 = tmp_path / "one", tmp_path / "two"
    p1 = run([sys.executable] + ex + ["--export_dir", str(out1)]).strip().splitlines()[-1]
    run(tr + ["--master-port", str(_free_port())] + ex + ["--export_dir", str(out2)])
    feats = "feats-" + conf
    def same(a, b):
        x, y = fio.open_store(str(a), "r"), fio.open_store(str(b), "r")
        assert list(x.keys()) == list(y.keys()) and len(list(x.keys())) > 0
        for k in x.keys():
            for d in x[k].keys():
                u, v = np.asarray(x[k][d].__array__()), np.asarray(y[k][d].__array__())
                assert u.dtype == v.dtype and np.array_equal(u, v), (k, d)
        return list(x.keys())
    names = same(os.path.join(out1, feats + ".h5"), os.path.join(out2, feats + ".h5"))
    assert len(names) == 7 and os.path.basename(p1).startswith(feats)
    pairs = tmp_path / "pairs-q.txt"
    pairs.write_text("\n".join(f"query/im{q}.png db/im{d}.png" for q in range(2) for d in range(2, 7)))
    mt = ["-m", "sfd2_amd.match_features", "--features", feats, "--conf", "NNM"]
    run([sys.executable] + mt + ["--export_dir", str(out1), "--pairs", str(pairs)])
    run(tr + ["--master-port", str(_free_port())] + mt + ["--export_dir", str(out2), "--pairs", str(pairs)])
    mname = f"{feats}-NNM-pairs-q.h5"
    got = same(os.path.join(out1, mname), os.path.join(out2, mname))
    assert len(got) == 10
    ex_pairs = tmp_path / "pairs-all.txt"
    run([sys.executable] + mt + ["--export_dir", str(out1), "--pairs", str(ex_pairs), "--exhaustive"])
    assert len(ex_pairs.read_text().split("\n")) == 7 * 6 // 2
