"""probabilit_amd.inspection on one sampled node against the route it replaces, at the same size:

    summary(node), quantile(node, [0.1, 0.5, 0.9]), histogram(node, bins=100)     on the device
    pbh_hbm_copy of the node's bytes                                            the HBM yardstick
    node.samples_ (the download) + numpy / scipy on the host                    the existing route

Device figures are times between two HIP events on the launching stream (torch.cuda.Event on the
current stream) after warm-up calls, over several repetitions; they span the calls' own host
synchronisations (select reads 1 KB back per pass).  The host route is wall time, once.  Per
kernel the JSON also gives the bytes it reads and that as a fraction of the measured copy rate.

    python tools/bench_summary.py [--n 100000000] [--reps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import probabilit_amd  # noqa: E402,F401
from probabilit_amd import _lib, device, inspection, native  # noqa: E402
from probabilit_amd.modeling import Distribution  # noqa: E402


def timed(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    device.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps_ms": [round(m, 4) for m in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/summary/bench_summary.json")
    a = ap.parse_args()
    import torch

    n = a.n
    node = Distribution("norm", loc=1.0, scale=2.0)
    node.sample_device(n, random_state=0)
    x = node.samples_device
    nbytes = 8 * n
    res = {"rows": n, "bytes": nbytes, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(device.device()), "timer": "HIP events on the launching stream",
           "cases": {}}
    cases = res["cases"]

    dst = device.empty(n)
    lib = _lib.load()
    copies = {}
    for variant in range(5):
        copies[variant] = timed(lambda: _lib.check(lib.pbh_hbm_copy(x.data_ptr(), dst.data_ptr(), nbytes, variant,
                                                                    device.stream())), a.reps, a.warmup)
    best = min(copies, key=lambda v: copies[v]["median_ms"])
    copy_ms = copies[best]["median_ms"]
    # a copy moves 2 bytes per byte of the vector; one read pass of a summary kernel moves 1
    copy_rate = 2 * nbytes / (copy_ms * 1e-3)
    cases["pbh_hbm_copy"] = dict(copies[best], variant=best, bytes_moved=2 * nbytes,
                                 tb_per_s=round(copy_rate / 1e12, 3))
    del dst

    def kernel_case(name, fn, read_passes):
        r = timed(fn, a.reps, a.warmup)
        r["read_passes"] = read_passes
        r["bytes_read"] = read_passes * nbytes
        rate = r["bytes_read"] / (r["median_ms"] * 1e-3)
        r["tb_per_s"] = round(rate / 1e12, 3)
        r["fraction_of_copy_rate"] = round(rate / copy_rate, 3)
        cases[name] = r
        print(name, json.dumps({k: r[k] for k in ("median_ms", "tb_per_s", "fraction_of_copy_rate")}), flush=True)

    ranks = [n // 10, n // 2, (9 * n) // 10]
    kernel_case("native.moments", lambda: native.moments(x), 2)
    kernel_case("native.select_ranks_3", lambda: native.select_ranks(x, ranks), 4)
    kernel_case("native.histogram_100", lambda: native.histogram(x, 100, (-7.0, 9.0)), 1)
    for name, fn in (("summary", lambda: inspection.summary(node)),
                     ("quantile_3", lambda: inspection.quantile(node, [0.1, 0.5, 0.9])),
                     ("histogram_100", lambda: inspection.histogram(node, bins=100))):
        cases[name] = timed(fn, a.reps, a.warmup)
        print(name, cases[name]["median_ms"], "ms", flush=True)
    assert node.__dict__.get("_host") is None

    # the existing route, once: the download through the pinned ring, then numpy / scipy
    import scipy.stats

    device.synchronize()
    t0 = time.perf_counter()
    host = node.samples_
    t1 = time.perf_counter()
    stats = [np.mean(host), np.std(host), np.min(host), np.max(host), scipy.stats.skew(host), scipy.stats.kurtosis(host)]
    t2 = time.perf_counter()
    qs = np.quantile(host, [0.1, 0.5, 0.9])
    t3 = time.perf_counter()
    hist = np.histogram(host, bins=100)
    t4 = time.perf_counter()
    cases["host_route"] = {"download_ms": round((t1 - t0) * 1e3, 1), "numpy_moments_ms": round((t2 - t1) * 1e3, 1),
                           "numpy_quantile_3_ms": round((t3 - t2) * 1e3, 1),
                           "numpy_histogram_100_ms": round((t4 - t3) * 1e3, 1),
                           "total_ms": round((t4 - t0) * 1e3, 1), "timer": "wall clock, one run"}
    print("host_route", json.dumps(cases["host_route"]), flush=True)
    del stats, qs, hist

    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
