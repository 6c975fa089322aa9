"""The VLAD stages (sfd2_amd.vlad) at the scale of a retrieval database, on one MI355X, against the same work in torch on the CPU.

  aggregate   assignment + aggregation + intra-normalisation of 1 000 images x 4 096 descriptors at K = 64 and at K = 256
  kmeans      Lloyd iterations on 2^20 rows, K = 64, 20 iterations

Per case the median of --reps wall-clock runs after one warm-up (the calls synchronise before they return): with the rows already on
the device, and with the rows uploaded from pageable host memory by the call -- the difference is the upload.  From the library's
own event pairs (sfd2_set_profiling) the device time of the launches alone, and for the assignment the achieved share of the HBM
bandwidth, whose floor is reading the rows once (the call reads them twice: the finite check, then the assignment).  The CPU side is
matmul, argmax and index_add_ at --threads threads, image blocks of 100 so that the n x K score matrix stays small.

    python tools/vlad_bench.py [--reps 3] [--threads 16] [--out profiles/vlad_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X: 8 TB/s


def timed(fn, reps):
    """(median ms, all ms, last result) of fn() after one warm-up."""
    out, times = None, []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if rep:
            times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), times, out


def scope_ms(ctx, fn, name):
    """Device milliseconds of the launches of one call, from the library's event pairs around scope `name`."""
    ctx.set_profiling(4)
    fn()
    rows = [r for r in ctx.layer_timings() if r["name"] == name]
    ctx.set_profiling(0)
    return float(sum(r["ms_total"] for r in rows)), int(sum(r["launches"] for r in rows))


def make_rows(torch, n, n_centres, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(n_centres, 128, generator=g), dim=1)
    x = centres[torch.randint(0, n_centres, (n,), generator=g)] + noise * torch.randn(n, 128, generator=g)
    return torch.nn.functional.normalize(x, dim=1).contiguous(), centres.contiguous()


def host_aggregate(torch, x, per_image, c, block=100):
    """matmul, argmax, index_add_ and the intra-normalisation, `block` images at a time."""
    k, h = len(c), 0.5 * (c * c).sum(1)
    out = []
    for i0 in range(0, len(x) // per_image, block):
        xb = x[i0 * per_image:(i0 + block) * per_image]
        n_img = len(xb) // per_image
        a = torch.argmax(xb @ c.T - h[None, :], dim=1)
        slot = torch.arange(n_img).repeat_interleave(per_image) * k + a
        v = torch.zeros(n_img * k, 128).index_add_(0, slot, xb - c[a]).double()
        v = v / v.norm(dim=1, keepdim=True).clamp_min(1e-300)
        v = v.reshape(n_img, k * 128)
        out.append((v / v.norm(dim=1, keepdim=True).clamp_min(1e-300)).float())
    return torch.cat(out, 0)


def host_kmeans(torch, x, c, iters):
    k = len(c)
    c = c.clone()
    for _ in range(iters):
        a = torch.argmax(x @ c.T - 0.5 * (c * c).sum(1)[None, :], dim=1)
        s = torch.zeros(k, 128, dtype=torch.float64).index_add_(0, a, x.double())
        n = torch.bincount(a, minlength=k)
        live = n > 0
        c[live] = (s[live] / n[live, None]).float()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--per_image", type=int, default=4096)
    ap.add_argument("--kmeans_rows", type=int, default=1 << 20)
    ap.add_argument("--kmeans_iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vlad_bench.json"))
    args = ap.parse_args()
    import torch
    from sfd2_amd import _lib, vlad
    torch.set_num_threads(args.threads)
    ctx = _lib.default_context(0)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": args.threads, "reps": args.reps, "hbm_peak_gb_s": HBM_PEAK_GBS, "aggregate": []}

    n = args.images * args.per_image
    x, _ = make_rows(torch, n, 256, 1)
    xn = x.numpy()
    xd = x.cuda()
    offsets = np.arange(args.images + 1, dtype=np.int64) * args.per_image
    row_gb = n * 512 / 1e9
    for k in (64, 256):
        c = x[torch.randperm(n, generator=torch.Generator().manual_seed(k))[:k]].clone()
        for _ in range(3):                                             # a few Lloyd steps on a sample: centroids like a vocabulary's
            c = host_kmeans(torch, x[:1 << 18], c, 1)
        cn, cd = c.numpy(), c.cuda()
        ms_res, all_res, out_res = timed(lambda: vlad.aggregate(xd, offsets, cd), args.reps)
        ms_up, all_up, out_up = timed(lambda: vlad.aggregate(xn, offsets, cn), args.reps)
        ms_assign, all_assign, (a_dev, _) = timed(lambda: vlad.assign(xd, cd), args.reps)
        k_agg, _ = scope_ms(ctx, lambda: vlad.aggregate(xd, offsets, cd), "vlad_aggregate")
        k_asg, _ = scope_ms(ctx, lambda: vlad.assign(xd, cd), "vlad_assign")
        ms_host, all_host, out_host = timed(lambda: host_aggregate(torch, x, args.per_image, c), args.reps)
        a_host = torch.argmax(x[:1 << 18] @ c.T - 0.5 * (c * c).sum(1)[None, :], dim=1).numpy()
        res["aggregate"].append({
            "images": args.images, "descriptors_per_image": args.per_image, "k": k, "row_gigabytes": row_gb,
            "device_ms_inputs_resident": ms_res, "device_ms_inputs_resident_all": all_res,
            "device_ms_with_uploads": ms_up, "device_ms_with_uploads_all": all_up, "upload_ms": ms_up - ms_res,
            "device_ms_launches_only": k_agg,
            "assign_ms_inputs_resident": ms_assign, "assign_ms_inputs_resident_all": all_assign, "assign_ms_launches_only": k_asg,
            "assign_gb_s_rows_once": row_gb / (k_asg * 1e-3), "assign_share_of_hbm_peak": row_gb / (k_asg * 1e-3) / HBM_PEAK_GBS,
            "assign_tflops": 2.0 * n * k * 128 / (k_asg * 1e-3) / 1e12,
            "host_ms_torch": ms_host, "host_ms_torch_all": all_host, "host_over_device_resident": ms_host / ms_res,
            "host_over_device_with_uploads": ms_host / ms_up,
            "resident_equals_uploaded": bool(out_res.tobytes() == out_up.tobytes()),
            "assignments_equal_to_host_share": float((a_dev[:1 << 18] == a_host).mean()),
            "max_abs_difference_to_host": float(np.abs(out_res - out_host.numpy()).max())})
        print(json.dumps(res["aggregate"][-1]), flush=True)
    del xd, x, xn

    n, k = args.kmeans_rows, 64
    x, _ = make_rows(torch, n, 256, 2, noise=0.2)                      # clusters that overlap: the iterations do not run out of rows to move
    xn, xd = x.numpy(), x.cuda()
    start = xn[np.random.RandomState(0).permutation(n)[:k]].copy()
    ms_res, all_res, (c_res, counts, moved) = timed(lambda: vlad.kmeans_from(xd, start, args.kmeans_iters), args.reps)
    ms_up, all_up, (c_up, _, _) = timed(lambda: vlad.kmeans_from(xn, start, args.kmeans_iters), args.reps)
    k_ms, _ = scope_ms(ctx, lambda: vlad.kmeans_from(xd, start, args.kmeans_iters), "vlad_kmeans")
    ms_host, all_host, c_host = timed(lambda: host_kmeans(torch, x, torch.from_numpy(start), len(moved)), args.reps)
    res["kmeans"] = {
        "rows": n, "k": k, "max_iters": args.kmeans_iters, "iters_run": len(moved), "moved": [int(m) for m in moved],
        "device_ms_inputs_resident": ms_res, "device_ms_inputs_resident_all": all_res, "device_ms_with_uploads": ms_up,
        "device_ms_with_uploads_all": all_up, "upload_ms": ms_up - ms_res, "device_ms_launches_only": k_ms,
        "device_ms_per_iteration_launches_only": k_ms / len(moved),
        "host_ms_torch_same_iterations": ms_host, "host_ms_torch_all": all_host, "host_over_device_resident": ms_host / ms_res,
        "host_over_device_with_uploads": ms_host / ms_up, "resident_equals_uploaded": bool(c_res.tobytes() == c_up.tobytes()),
        "counts_sum": int(counts.sum()), "max_abs_difference_to_host": float(np.abs(c_res - c_host.numpy()).max())}
    print(json.dumps(res["kmeans"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
