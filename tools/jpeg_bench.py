#!/usr/bin/env python3
"""The device JPEG decoder against PIL: host CPU per image, device time per image, and files -> features images/s.

    python tools/jpeg_bench.py [--size 1600x1200 --quality 90 --files 64 --workers 2,16 --stage host,device,extract]

  host     read + parse + destuff (sfd2_jpeg_parse / sfd2_jpeg_prepare) per file, against PIL's decode + convert("RGB"); CPU only
  device   synchronous sfd2_jpeg_decode of one prepared file, timed with events around --reps calls (upload included; the kernel sum is
           what a rocprofv3 --kernel-trace run reports)
  extract  extract_localization.main, f16c, two lanes, over --files JPEGs, decoder "hip" and "pil" interleaved per worker count
Prints one JSON line.  Weights are synth.make_state_dict; the files are synthetic photographs (tools/pipeline_bench.write_images).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--workers", default="2,16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--stage", default="host,device,extract")
    args = ap.parse_args()
    W, H = (int(x) for x in args.size.split("x"))
    stages = set(args.stage.split(","))
    from tools.pipeline_bench import write_images
    tmp = tempfile.mkdtemp(prefix="jpeg_bench_")
    out = {"size": args.size, "quality": args.quality}
    try:
        write_images(tmp, args.files, 0, H, W, quality=args.quality)
        files = sorted(os.path.join(tmp, "query", f) for f in os.listdir(os.path.join(tmp, "query")))
        out["file_bytes"] = int(np.mean([os.path.getsize(f) for f in files]))
        if "host" in stages:
            from PIL import Image
            from sfd2_amd import jpeg
            buf = np.empty(jpeg.reserve_bytes(max(os.path.getsize(f) for f in files)), dtype=np.uint8)
            t0 = time.perf_counter()
            for f in files:
                b, info = jpeg.read_prepared(f, lambda n: buf[:n])
                assert b is not None
            out["host_ms_hip"] = 1e3 * (time.perf_counter() - t0) / len(files)
            t0 = time.perf_counter()
            for f in files:
                with Image.open(f) as im:
                    np.asarray(im.convert("RGB"))
            out["host_ms_pil"] = 1e3 * (time.perf_counter() - t0) / len(files)
        if "device" in stages or "extract" in stages:
            import torch
            from sfd2_amd import _lib, jpeg
        if "device" in stages:
            ctx = _lib.Context(0)
            data = open(files[0], "rb").read()
            img = jpeg.decode(ctx, data)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.reps):
                jpeg.decode(ctx, data, out=img)
            b.record()
            b.synchronize()
            out["device_ms_per_image_sync"] = (time.perf_counter() - t0) * 1e3 / args.reps
            ctx.close()
        if "extract" in stages:
            from sfd2_amd import extract_localization as el
            from sfd2_amd import synth
            sd = synth.make_state_dict(0)
            model, ext = el.get_model("ressegnetv2", state_dict=sd, use_stability=True, precision="f16c")
            name, conf = next(iter(el.confs.items()))
            ds = el.ImageDataset(os.path.join(tmp, "query"), conf["preprocessing"])
            el.main(conf, ds, os.path.join(tmp, "warm"), model_and_extractor=(model, ext), num_workers=2, lanes=2, decoder="hip")
            el.main(conf, ds, os.path.join(tmp, "warm2"), model_and_extractor=(model, ext), num_workers=2, lanes=2, decoder="pil")
            for w in [int(x) for x in args.workers.split(",")]:
                for dec in ("pil", "hip"):
                    rep = {}
                    d = os.path.join(tmp, f"out_{dec}_{w}")
                    t0 = time.perf_counter()
                    el.main(conf, ds, d, model_and_extractor=(model, ext), num_workers=w, lanes=2, decoder=dec, report=rep)
                    out[f"images_per_s_{dec}_w{w}"] = len(files) / (time.perf_counter() - t0)
                    out[f"report_{dec}_w{w}"] = rep
                    shutil.rmtree(d, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
